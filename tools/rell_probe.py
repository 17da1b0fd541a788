#!/usr/bin/env python
"""Time phylo_rell (the RELL bootstrap over a scored tree set) at a shipped dataset's shape and report device
and wall time, units/s (a unit = one multiply-add of the T x S by S x B product) and the share of the fp64 peak; beside it the
wall time of the same product in NumPy, `x @ counts.T`, on the threads the process may use -- the yardstick.

    python tools/rell_probe.py --dataset hohna_data --trees 4096 --reps 1000 --out profiles/rell_probe.jsonl

The site factors are those of phylo_trees_loglik on random trees.  The call is timed whole `--runs` times after a warm-up (wall,
and perf.sweep_ms from hipEvents: the kernels, without the upload of the factors and the copies back); medians with the
quartiles.  A few replicates at both ends are checked bit for bit against the host loop (phylo_debug_rell_host).  Appends one
JSON line to --out.

    python tools/rell_probe.py --multiscale --dataset hohna_data --trees 4096 --reps 1000 --out profiles/rell_probe.jsonl

times phylo_rell_multiscale at the scales of --scales against one phylo_rell call per scale."""
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


def multiscale(a, ctx, sites, N, S):
    """--multiscale: phylo_rell_multiscale at the scales of --scales against the parent's path to the same replicates, K calls of
    phylo_rell at the same B (which can only draw S sites: nearly the same multiply-adds, not the same samples).  Interleaved, one
    warm-up each; medians with quartiles of --runs."""
    from phylo_amd import treetests
    T, B = a.trees, a.reps
    sc = treetests.au_scales(S, a.scales)
    K = len(sc['draws'])
    ms = ctx.rell_multiscale(sites, sc['draws'], B, a.seed)                 # warm-ups
    ctx.rell(sites, B, a.seed)
    dev, wall, dev_plain, wall_plain = [], [], [], []
    for _ in range(a.runs):
        t0 = time.perf_counter()
        ms = ctx.rell_multiscale(sites, sc['draws'], B, a.seed)
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(ms['stats']['sweep_ms'])
        t0 = time.perf_counter()
        d = 0.0
        for k in range(K):
            d += ctx.rell(sites, B, a.seed + k)['stats']['sweep_ms']
        wall_plain.append((time.perf_counter() - t0) * 1e3)
        dev_plain.append(d)
    # a few replicates at both ends of the first and the last scale against the host loop, through the instance that stores nothing
    full = ctx.rell_multiscale(sites, sc['draws'], B, a.seed, want_best=True)
    n = min(4, B)
    same = bool(np.array_equal(full['wins'], ms['wins'])) and bool((full['wins'].sum(axis=1) == B).all())
    for k in sorted({0, K - 1}):
        for b0 in sorted({0, B - n}):
            host = _ffi.debug_rell_multiscale_host(sites, sc['draws'], k, b0, n, a.seed, want_counts=False, want_reps=False)
            same = same and bool(np.array_equal(host['best'], full['best'][k, b0:b0 + n]))
    same = same and bool(np.array_equal(np.stack([np.bincount(r, minlength=T) for r in full['best']]), full['wins']))
    fit = treetests.au_test(ms['wins'], sc['sigma2'], B)
    order = np.argsort(-ctx.rell(sites, 1, a.seed)['obs'])[:5]              # the five best trees by observed score
    d, w, dp, wp = quartiles(dev), quartiles(wall), quartiles(dev_plain), quartiles(wall_plain)
    units = float(T) * S * B * float(np.sum(sc['draws'])) / S               # multiply-adds that carry a draw: T B sum_k n_k
    sp, tiles = (S + 3) // 4 * 4, (T + 63) // 64
    rec = {'probe': 'rell_multiscale', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': T, 'B': B, 'K': K, 'runs': a.runs,
           'r': sc['r'].tolist(), 'draws': sc['draws'].tolist(), 'device_ms': d, 'wall_ms': w, 'launches': ms['stats']['n_launches'],
           'plain_calls_device_ms': dp, 'plain_calls_wall_ms': wp, 'ratio_plain_over_multiscale_device': dp['median'] / d['median'],
           'ratio_plain_over_multiscale_wall': wp['median'] / w['median'], 'units_T_S_K_B': ms['stats']['units'],
           'units_per_s_device': ms['stats']['units'] / (d['median'] * 1e-3), 'drawn_units': units,
           'columns_per_chunk': min((256 << 20) // (sp * 2 + tiles * 12 + 4), 1 << 20, K * B),
           'columns_per_chunk_limit': min((256 << 20) // (sp * 2 + tiles * 12 + 4), 1 << 20),
           'bit_equal_host_loop': same,
           'au_of_best_trees': [{'tree': int(t), 'p_au': float(fit['p_au'][t]), 'se_au': float(fit['se_au'][t]) if fit['au_ok'][t] else None, 'rss': float(fit['rss'][t]),
                                 'df': int(fit['df'][t]), 'au_ok': bool(fit['au_ok'][t]), 'bp': float(fit['bp'][int(np.argmin(np.abs(sc['sigma2'] - 1)))][t])}
                                for t in order]}
    return rec, same


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--dataset', default='hohna_data')
    ap.add_argument('--trees', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=1000, help='bootstrap replicates B')
    ap.add_argument('--runs', type=int, default=7, help='timed calls')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--numpy_runs', type=int, default=3, help='timed x @ counts.T products (0: skip the yardstick)')
    ap.add_argument('--out', default=None)
    ap.add_argument('--multiscale', action='store_true',
                    help='time phylo_rell_multiscale (the AU test\'s resampling) against one phylo_rell call per scale instead')
    ap.add_argument('--scales', default='default', help="with --multiscale: 'default' (r = 0.5 .. 1.4) or r1,r2,...")
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
        if a.multiscale:
            rec, same = multiscale(a, ctx, sites, N, S)
            line = json.dumps(rec)
            print(line)
            if a.out:
                os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
                with open(a.out, 'a') as f:
                    f.write(line + '\n')
            return 0 if same else 1
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
