#!/usr/bin/env python3
"""How many phase-1 steps the clade tables of the merge's site-pattern form leave (phylo_amd/csrc/phylo_site_patterns.h) -- no GPU:
the C oracle's sweeps replayed through the root tables' leaf BITSETS (probe_child_types.py's replay with bitsets in the place of
leaf counts), every merge that is not leaf x leaf classed by the distinct columns U_Z of the alignment restricted to the clade it
creates.  Run by tools/clade_steps.sh:
    python tests/probe_clade_steps.py [--dataset primate_data] [--K 2048] [--seeds 0 1 2]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import c_oracle as CO                          # noqa: E402
from oracle import cpu_ref as O                            # noqa: E402
from phylo_amd.datasets import load_dataset                # noqa: E402


def merged_clades(g, Q, pi, lam, K, seed):
    """([R][K] bitset of the clade every merge creates, [R][K] whether the merge is leaf x leaf) of one sweep"""
    N = g.shape[0]
    out = CO.sweep(g, Q, pi, lam, lam, K, seed)
    record = np.tile(1 << np.arange(N, dtype=np.int64), (K, 1))
    ar = np.arange(K)
    clade = np.zeros((N - 1, K), dtype=np.int64)
    cherry = np.zeros((N - 1, K), dtype=bool)
    for r in range(N - 1):
        if r > 0:
            record = record[out['ancestors'][r - 1]]
        coalesced, remaining, _ = O.extend_partial_state(K, N - r, seed, r)
        assert np.array_equal(coalesced, out['merges'][r])
        a, b = record[ar, coalesced[:, 0]], record[ar, coalesced[:, 1]]
        clade[r] = a | b
        cherry[r] = ((a & (a - 1)) == 0) & ((b & (b - 1)) == 0)
        record = np.concatenate([record[ar[:, None], remaining], clade[r][:, None]], axis=1)
    return clade, cherry


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--dataset', default='primate_data')
    p.add_argument('--K', type=int, default=2048)
    p.add_argument('--seeds', type=int, nargs='+', default=[0, 1, 2])
    a = p.parse_args()
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    codes = np.where(g.sum(axis=2) == 4, 4, g.argmax(axis=2)).astype(np.uint8)
    U = len({codes[:, s].tobytes() for s in range(S)})
    Q, pi, lam = O.get_Q(O.init_y_q()), np.full((1, 4), 0.25), np.full(N - 1, 10.0)
    both = [merged_clades(g, Q, pi, lam, a.K, s) for s in a.seeds]
    clade = np.concatenate([c for c, _ in both], axis=1)
    cherry = np.concatenate([c for _, c in both], axis=1)
    uz = {}
    for Z in np.unique(clade[~cherry]):
        rows = codes[[i for i in range(N) if int(Z) >> i & 1]]
        uz[int(Z)] = len({rows[:, s].tobytes() for s in range(S)})
    steps = np.zeros(clade.shape, dtype=np.int64)
    for Z, u in uz.items():
        steps[(clade == Z) & ~cherry] = -(-u // 64)
    nU = -(-U // 64)
    n = int((~cherry).sum())
    print("%s %d x %d, U = %d, GTR-init, K = %d, seeds %s" % (a.dataset, N, S, U, a.K, a.seeds))
    print("merges that are not leaf x leaf: %d of %d (%.1f %%); distinct clades among them: %d" % (n, cherry.size, 100.0 * n / cherry.size, len(uz)))
    print("phase-1 steps ceil(U_Z / 64): mean %.2f against %d" % (steps[~cherry].mean(), nU))
    print("| phase-1 steps | " + " | ".join(str(k) for k in range(1, nU + 1)) + " |")
    print("| merges | " + " | ".join(str(int((steps == k).sum())) for k in range(1, nU + 1)) + " |")
    print("| rank event | " + " | ".join(str(r + 1) for r in range(1, N - 1)) + " |")
    print("| mean steps | " + " | ".join("%.2f" % steps[r][~cherry[r]].mean() if (~cherry[r]).any() else "-" for r in range(1, N - 1)) + " |")


if __name__ == "__main__":
    main()
