#!/usr/bin/env python
"""Time phylo_rell (the RELL bootstrap over a scored tree set) at a shipped dataset's shape and report device
and wall time, units/s (a unit = one multiply-add of the T x S by S x B product) and the share of the fp64 peak; beside it the
wall time of the same product in NumPy, `x @ counts.T`, on the threads the process may use -- the yardstick.

    python tools/rell_probe.py --dataset hohna_data --trees 4096 --reps 1000 --out profiles/rell_probe.jsonl

The site factors are those of phylo_trees_loglik on random trees.  The call is timed whole `--runs` times after a warm-up (wall,
and perf.sweep_ms from hipEvents: the kernels, without the upload of the factors and the copies back); medians with the
quartiles.  A few replicates at both ends are checked bit for bit against the host loop (phylo_debug_rell_host).  Appends one
JSON line to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from phylo_amd import _ffi, model                          # noqa: E402
from phylo_amd.datasets import load_dataset                # noqa: E402

FP64_PEAK = 78.6e12                                        # flop/s: 256 CUs x 4 SIMDs x 16 multiply-adds per cycle x 2 x 2.4 GHz


def random_rows(n, rng):
    roots = list(rng.permutation(n))
    child = []
    for i in range(n - 1):
        a = roots.pop(rng.integers(0, len(roots)))
        b = roots.pop(rng.integers(0, len(roots)))
        child.append((a, b))
        roots.append(n + i)
    return np.array(child, dtype=np.int32).reshape(n - 1, 2), rng.exponential(0.1, (n - 1, 2))


def quartiles(x):
    q1, q2, q3 = np.percentile(np.asarray(x, dtype=np.float64), [25, 50, 75])
    return {'median': float(q2), 'q1': float(q1), 'q3': float(q3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--dataset', default='hohna_data')
    ap.add_argument('--trees', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=1000, help='bootstrap replicates B')
    ap.add_argument('--runs', type=int, default=7, help='timed calls')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--numpy_runs', type=int, default=3, help='timed x @ counts.T products (0: skip the yardstick)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args(argv)
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    rng = np.random.default_rng(a.seed)
    rows = [random_rows(N, rng) for _ in range(a.trees)]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    T, B = a.trees, a.reps
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(model.get_Q(model.init_y_q()), np.full(4, 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0))
        ll, sites = ctx.trees_loglik(child, blen, want_sites=True)
        full = ctx.rell(sites, B, a.seed, want_reps=True, want_counts=True, want_logs=True)      # warm-up, and the arrays to compare
        wall, dev, wall_reps = [], [], []
        for _ in range(a.runs):
            t0 = time.perf_counter()
            out = ctx.rell(sites, B, a.seed)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(out['stats']['sweep_ms'])
            t0 = time.perf_counter()
            ctx.rell(sites, B, a.seed, want_reps=True)
            wall_reps.append((time.perf_counter() - t0) * 1e3)
        stats = out['stats']
    k = min(4, B)
    same = True
    for b0 in sorted({0, B - k}):
        host = _ffi.debug_rell_host(sites, b0, k, a.seed)
        same = same and bool(np.array_equal(host['rep_loglik'].view(np.uint64),
                                            np.ascontiguousarray(full['rep_loglik'][:, b0:b0 + k]).view(np.uint64)))
        same = same and bool(np.array_equal(host['counts'], full['counts'][b0:b0 + k]))
    same = same and bool(np.array_equal(full['best'], np.argmax(full['rep_loglik'], axis=0))) and int(full['wins'].sum()) == B
    w, d, wr = quartiles(wall), quartiles(dev), quartiles(wall_reps)
    units = float(T) * S * B
    rec = {'probe': 'rell', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': T, 'B': B, 'runs': a.runs,
           'wall_ms': w, 'wall_with_rep_matrix_ms': wr, 'device_ms': d, 'launches': stats['n_launches'], 'units': units,
           'units_per_s_device': units / (d['median'] * 1e-3), 'units_per_s_wall': units / (w['median'] * 1e-3),
           'share_of_fp64_peak_device': 2.0 * units / (d['median'] * 1e-3) / FP64_PEAK, 'bit_equal_host_loop': same}
    if a.numpy_runs > 0:
        x, cnt = full['site_loglik'], full['counts'].astype(np.float64)
        ref = x @ cnt.T                                      # warm-up; BLAS adds in its own order: close, not the contract's bits
        t_np = []
        for _ in range(a.numpy_runs):
            t0 = time.perf_counter()
            ref = x @ cnt.T
            t_np.append((time.perf_counter() - t0) * 1e3)
        try:
            cpus = len(os.sched_getaffinity(0))
        except AttributeError:
            cpus = os.cpu_count()
        q = quartiles(t_np)
        rec.update(numpy_matmul_wall_ms=q, numpy_threads_env=os.environ.get('OMP_NUM_THREADS'), cpus_available=cpus,
                   numpy_max_rel_diff=float(np.max(np.abs(ref - full['rep_loglik']) / np.abs(ref))),
                   ratio_numpy_over_device=q['median'] / d['median'], ratio_numpy_over_wall=q['median'] / w['median'],
                   ratio_numpy_over_wall_with_rep_matrix=q['median'] / wr['median'])
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
