"""Create and destroy contexts that use every mode; VRAM in use after n and 2n iterations (a leak grows linearly).
python tools/leak_probe.py [n]"""
import json
import os
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phylo_amd import _ffi, model as M          # noqa: E402
from phylo_amd import train as T                # noqa: E402
from phylo_amd.datasets import load_dataset     # noqa: E402

g = load_dataset("primate_data")["genome"][:, :200]
N, S, _ = g.shape
Q = M.get_Q(M.init_y_q())
pi = M.get_stationary_probs(np.zeros(4) + 0.25)
lam = np.full(N - 1, 10.0)
# 66 taxa: more rank events than one 64-bit word has bits (the reverse pass's hand-off state, the VI step's buffers)
N2, S2 = 66, 64
codes2 = np.random.default_rng(66).integers(0, 5, size=(N2, S2))
g2 = np.stack([(codes2 == b) | (codes2 == 4) for b in range(4)], axis=-1).astype(np.float64)


def used():
    out = subprocess.run(["rocm-smi", "--showmeminfo", "vram", "--json"], capture_output=True, text=True).stdout
    d = json.loads(out)
    return int(d[list(d.keys())[0]]["VRAM Total Used Memory (B)"]) / 2 ** 20


def cycle(i):
    with _ffi.Context(256 + 4 * (i % 8), N, S) as c:
        c.set_leaves(g)
        c.set_model(Q, pi, lam, lam)
        c.sweep(i)
        c.sweep(i, _ffi.FLAGS_DEFAULT | _ffi.ONE_LAUNCH)
        c.sweep(i, _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)
        c.sweep_backward()
        c.sweep(i, _ffi.FLAGS_DEFAULT | _ffi.TWISTING | _ffi.KEEP_GRAPH, 2)
        c.sweep_backward()
        c.sweep_batch_async([1, 2, 3, 4])
        c.sweep_fetch()
        c.sweep_batch_async([1, 2, 3, 4], _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH)   # the batched graph and its reverse pass
        c.sweep_backward_batch(4)
        c.rell(np.full((40 + i % 8, 300), 0.25), 64, i)     # the bootstrap's own slab (logs, counts, replicate scores)
        c.rell_multiscale(np.full((40 + i % 8, 300), 0.25), (150, 300, 420), 64, i, want_reps=i % 2 == 1)   # ... and the multiscale one's
        child = np.array([[j - 1 + N if j else 0, j + 1] for j in range(N - 1)], dtype=np.int32)   # a caterpillar, 30 .. 37 times
        n = 30 + i % 8
        c.trees_grad(np.tile(child, (n, 1, 1)), np.full((n, N - 1, 2), 0.1), want_curv=True)   # the gradient's own slab and node stores
        c.trees_nni(np.tile(child, (n, 1, 1)), np.full((n, N - 1, 2), 0.1))   # the NNI neighbourhood's own slab and node stores
        c.trees_grad_rates(np.tile(child, (n, 1, 1)), np.full((n, N - 1, 2), 0.1), np.linspace(0.0, 2.0, 2 + i % 4), np.full(2 + i % 4, 0.25),
                           want_curv=True, want_params=True)   # ... and the mixture gradient's: a slab that grows with the categories
        c.trees_nni_rates(np.tile(child, (n, 1, 1)), np.full((n, N - 1, 2), 0.1), np.linspace(0.0, 2.0, 2 + i % 4), np.full(2 + i % 4, 0.25))
                                                            # ... and the mixture neighbourhood's, with its own pair of events
        c.trees_grad_model(np.tile(child, (n, 1, 1)), np.full((n, N - 1, 2), 0.1), np.linspace(-1.0, 1.0, (1 + i % 16) * 16).reshape(-1, 4, 4),
                           want_grad=True)                  # ... and the model gradient's: a slab that grows with the directions
        c.trees_ancestral(np.tile(child, (n, 1, 1)), np.full((n, N - 1, 2), 0.1), want_pmax=i % 2 == 1)
                                                            # ... and the ancestral posteriors': staged outputs that grow with what is asked for
        c.trees_ancestral_rates(np.tile(child, (n, 1, 1)), np.full((n, N - 1, 2), 0.1), np.linspace(0.0, 2.0, 2 + i % 4), np.full(2 + i % 4, 0.25),
                                want_catpost=i % 2 == 1, want_siterate=i % 4 < 2)
                                                            # ... and the same under a mixture: node stores and staging that grow with the categories
    v = T.Variables(N2, np.log(10.0), False)            # a context of 66 taxa that trains: two steps, so two passes on one context
    tr = T.Trainer(g2, 32 + 4 * (i % 8), v, T.make_optimizer('Adam', 0.01), S2)
    try:
        tr.step(np.arange(S2), seed=i)
        tr.step(np.arange(S2), seed=i + 1)
    finally:
        tr.close()


n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
marks = [used()]
for rep in range(3):
    for i in range(n):
        cycle(i)
    marks.append(used())
print("VRAM MiB in use: start %.0f, after %d / %d / %d cycles: %.0f / %.0f / %.0f" % (marks[0], n, 2 * n, 3 * n, marks[1], marks[2], marks[3]))
