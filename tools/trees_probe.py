#!/usr/bin/env python
"""Time phylo_trees_loglik against a loop over phylo_tree_loglik on the same random trees of a shipped dataset, check that the
two agree bit for bit, and report units/s.

    python tools/trees_probe.py --dataset hohna_data --trees 4096 --reps 7 --out profiles/trees_probe.jsonl

The batched call is timed whole (wall, and perf.sweep_ms from hipEvents) `reps` times; the loop is timed over `--loop_trees` of
the trees (all of them by default) `loop_reps` times.  Medians with the quartiles.  Appends one JSON line to --out.

    python tools/trees_probe.py --dataset hohna_data --trees 4096 --rates 4 --reps 7 --out profiles/trees_probe.jsonl

--rates C times phylo_trees_loglik_rates under C discrete Gamma categories (--alpha) instead, against C
plain phylo_trees_loglik calls on the scaled trees in the same run: device and wall times of both, their ratios, and whether
cat_lik carries the plain calls' site factors bit for bit.

    python tools/trees_probe.py --dataset hohna_data --trees 4096 --grad --reps 7 --out profiles/trees_probe.jsonl

--grad times phylo_trees_grad, with and without curvature, against the plain phylo_trees_loglik on the
same trees in the same run: device and wall times, their ratios, the 4 (N-1) + 1 plain calls a central-difference gradient would
cost, and whether loglik carries the plain call's bits.

    python tools/trees_probe.py --dataset hohna_data --trees 4096 --grad --rates 4 --reps 7 --out profiles/trees_probe.jsonl

--grad --rates C times phylo_trees_grad_rates under C discrete Gamma categories: the gradient alone,
with curvature, and with curvature and the rate and weight sums, against C calls of phylo_trees_grad (with curvature) on the
scaled trees, interleaved in the same run; the number of chunks, and whether loglik carries phylo_trees_loglik_rates' bits.

    python tools/trees_probe.py --dataset hohna_data --trees 4096 --nni --reps 7 --out profiles/trees_probe.jsonl

--nni times phylo_trees_nni against phylo_trees_loglik on the explicitly built NNI neighbours of the first
--explicit_trees trees (and phylo_trees_nni on those trees alone), the plain call and phylo_trees_grad with and without
curvature, interleaved in the same run: device and wall times, their ratios, whether loglik carries the plain call's bits, and
the worst relative difference of loglik + delta to the explicit neighbour's log-likelihood.

    python tools/trees_probe.py --dataset hohna_data --trees 4096 --nni --rates 4 --reps 7 --out profiles/trees_probe.jsonl

--nni --rates C times phylo_trees_nni_rates under C discrete Gamma categories against C calls of
phylo_trees_nni on the scaled trees and, for the first --explicit_trees trees, against phylo_trees_loglik_rates on their explicitly
built neighbours, interleaved in the same run: device and wall times, their ratios, the number of chunks, whether loglik carries
phylo_trees_loglik_rates' bits, and the worst relative difference of loglik + delta to the explicit neighbour's log-likelihood.

    python tools/trees_probe.py --dataset hohna_data --trees 4096 --model --dirs 12 --reps 7 --out profiles/trees_probe.jsonl

--model times phylo_trees_grad_model along --dirs P directions of the row-softmax Q (and with P = 1)
against phylo_trees_grad without curvature, phylo_trees_loglik, and the central-difference yardstick it replaces -- 2 P pairs of
set_model and phylo_trees_loglik --, interleaved in the same run: device and wall times, their ratios, the number of chunks, and
whether loglik and grad carry the siblings' bits.

    python tools/trees_probe.py --dataset hohna_data --trees 4096 --ancestral --reps 7 --out profiles/trees_probe.jsonl

--ancestral times phylo_trees_ancestral with states only and with post (the latter on the first
--post_trees trees: its output is 32 bytes per node-site, on the device and on the host) against phylo_trees_grad without
curvature on the same trees, interleaved in the same run: device and wall times, their ratios, the bytes each form writes, the
number of chunks, and whether loglik carries phylo_trees_grad's bits.

    python tools/trees_probe.py --dataset hohna_data --trees 4096 --ancestral --rates 4 --reps 7 --out profiles/trees_probe.jsonl

--ancestral --rates C times phylo_trees_ancestral_rates under C discrete Gamma categories -- states only,
the site rates only (catpost and siterate), and with post on the first --post_trees trees -- against phylo_trees_grad_rates
without curvature and against C calls of phylo_trees_ancestral (states only) on the scaled trees, interleaved in the same run:
device and wall times, their ratios, the number of chunks, and whether loglik and catpost carry phylo_trees_loglik_rates' bits."""
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


def rates_probe(a):
    """the rates call against C plain calls on the scaled trees: same trees, same context, same run"""
    from phylo_amd import rates as R
    jc = a.jc.lower() == 'true'
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    rng = np.random.default_rng(a.seed)
    rows = [random_rows(N, rng) for _ in range(a.trees)]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    rates, weights = R.rate_model(a.alpha, a.rates)
    C = rates.size
    scaled = [rates[c] * blen for c in range(C)]             # (outside the timed region: the caller of C plain calls holds them)
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, np.full(4, 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=jc)
        ll, cats = ctx.trees_loglik_rates(child, blen, rates, weights, want_cats=True)     # warm-up, and the factors to compare
        same = True
        for c in range(C):
            _, f = ctx.trees_loglik(child, scaled[c], want_sites=True)                     # warm-up of the plain call too
            same = same and bool(np.array_equal(f.view(np.uint64), np.ascontiguousarray(cats[:, c]).view(np.uint64)))
        del cats
        wall, dev, pwall, pdev = [], [], [], []
        for _ in range(a.reps):                              # interleaved: both see the same machine
            t0 = time.perf_counter()
            ll = ctx.trees_loglik_rates(child, blen, rates, weights)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(ctx.last_trees_stats['sweep_ms'])
            stats = dict(ctx.last_trees_stats)
            t0 = time.perf_counter()
            d = 0.0
            for c in range(C):
                ctx.trees_loglik(child, scaled[c])
                d += ctx.last_trees_stats['sweep_ms']
            pwall.append((time.perf_counter() - t0) * 1e3)
            pdev.append(d)
    w, d, pw, pd = quartiles(wall), quartiles(dev), quartiles(pwall), quartiles(pdev)
    rec = {'probe': 'trees_loglik_rates', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': a.trees, 'jc': jc, 'reps': a.reps,
           'C': int(C), 'alpha': a.alpha, 'rates': rates.tolist(),
           'rates_wall_ms': w, 'rates_device_ms': d, 'plain_x_C_wall_ms': pw, 'plain_x_C_device_ms': pd,
           'device_ratio_rates_over_plain_x_C': d['median'] / pd['median'], 'wall_ratio_rates_over_plain_x_C': w['median'] / pw['median'],
           'launches': stats['n_launches'], 'units': stats['units'], 'units_per_s_device': stats['units'] / (d['median'] * 1e-3),
           'cat_lik_bit_equal': same, 'finite': bool(np.isfinite(ll).all())}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0 if same else 1


def model_probe(a):
    """phylo_trees_grad_model along P directions (and along one) against phylo_trees_grad, the plain call and the 2 P
    set_model + phylo_trees_loglik pairs of a central difference: same trees, same context, same run"""
    from phylo_amd import modelfit
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    rng = np.random.default_rng(a.seed)
    rows = [random_rows(N, rng) for _ in range(a.trees)]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    y_q = model.init_y_q()
    Q, pi, lam = model.get_Q(y_q), np.full(4, 0.25), np.full(N - 1, 10.0)
    P = a.dirs
    dirs = np.concatenate([modelfit.q_directions(y_q), rng.normal(size=(4, 4, 4))])[:P]
    h = 1e-6
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam, lam)
        ll = ctx.trees_loglik(child, blen)                   # warm-up of all
        lg, grad = ctx.trees_grad(child, blen)
        lm, dth, mgrad, dpr = ctx.trees_grad_model(child, blen, dirs, want_grad=True)
        ctx.trees_grad_model(child, blen, dirs[:1], want_grad=True)
        same = bool(np.array_equal(ll.view(np.uint64), lm.view(np.uint64)) and np.array_equal(grad.view(np.uint64), mgrad.view(np.uint64)))
        t = {k: ([], []) for k in ('model', 'model1', 'model_only', 'grad', 'plain', 'fd')}

        def timed(key, fn):
            t0 = time.perf_counter()
            dev = fn()
            t[key][0].append((time.perf_counter() - t0) * 1e3)
            t[key][1].append(dev)

        def one(fn):
            fn()
            return ctx.last_trees_stats['sweep_ms']

        def central():
            dev, fd = 0.0, np.empty((a.trees, P))
            for p in range(P):
                pair = []
                for sgn in (1.0, -1.0):
                    ctx.set_model(Q + sgn * h * dirs[p], pi, lam, lam)
                    pair.append(ctx.trees_loglik(child, blen))
                    dev += ctx.last_trees_stats['sweep_ms']
                fd[:, p] = (pair[0] - pair[1]) / (2 * h)
            ctx.set_model(Q, pi, lam, lam)
            central.fd = fd
            return dev

        for _ in range(a.reps):                              # interleaved: all see the same machine
            timed('model', lambda: one(lambda: ctx.trees_grad_model(child, blen, dirs, want_grad=True)))
            stats = dict(ctx.last_trees_stats)
            timed('model1', lambda: one(lambda: ctx.trees_grad_model(child, blen, dirs[:1], want_grad=True)))
            timed('model_only', lambda: one(lambda: ctx.trees_grad_model(child, blen, dirs, want_prior=False)))
            timed('grad', lambda: one(lambda: ctx.trees_grad(child, blen)))
            timed('plain', lambda: one(lambda: ctx.trees_loglik(child, blen)))
            timed('fd', central)
    q = {k: (quartiles(v[0]), quartiles(v[1])) for k, v in t.items()}
    fd_off = float(np.max(np.abs(central.fd - dth) / (1.0 + np.abs(dth))))
    rec = {'probe': 'trees_grad_model', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': a.trees, 'reps': a.reps, 'P': int(P),
           'model_wall_ms': q['model'][0], 'model_device_ms': q['model'][1], 'model_P1_wall_ms': q['model1'][0], 'model_P1_device_ms': q['model1'][1],
           'model_without_grad_device_ms': q['model_only'][1],
           'grad_wall_ms': q['grad'][0], 'grad_device_ms': q['grad'][1], 'plain_wall_ms': q['plain'][0], 'plain_device_ms': q['plain'][1],
           'central_2P_wall_ms': q['fd'][0], 'central_2P_device_ms': q['fd'][1],
           'device_ratio_model_over_grad': q['model'][1]['median'] / q['grad'][1]['median'],
           'device_ratio_model_P1_over_grad': q['model1'][1]['median'] / q['grad'][1]['median'],
           'device_ratio_model_over_plain': q['model'][1]['median'] / q['plain'][1]['median'],
           'device_ratio_model_over_central_2P': q['model'][1]['median'] / q['fd'][1]['median'],
           'wall_ratio_model_over_grad': q['model'][0]['median'] / q['grad'][0]['median'],
           'wall_ratio_model_over_central_2P': q['model'][0]['median'] / q['fd'][0]['median'],
           'launches': stats['n_launches'], 'chunks': stats['n_launches'] // 8, 'units': stats['units'],
           'units_per_s_device': stats['units'] / (q['model'][1]['median'] * 1e-3),
           'central_difference_off': fd_off, 'loglik_and_grad_bit_equal': same, 'finite': bool(np.isfinite(dth).all() and np.isfinite(dpr).all())}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0 if same else 1


def grad_probe(a):
    """phylo_trees_grad, with and without curvature, against the plain call: same trees, same context, same run"""
    jc = a.jc.lower() == 'true'
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    rng = np.random.default_rng(a.seed)
    rows = [random_rows(N, rng) for _ in range(a.trees)]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, np.full(4, 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=jc)
        ll = ctx.trees_loglik(child, blen)                   # warm-up of all three
        lg, grad = ctx.trees_grad(child, blen)
        lc, grad2, curv = ctx.trees_grad(child, blen, want_curv=True)
        same = bool(np.array_equal(ll.view(np.uint64), lg.view(np.uint64)) and np.array_equal(ll.view(np.uint64), lc.view(np.uint64))
                    and np.array_equal(grad.view(np.uint64), grad2.view(np.uint64)))
        t = {k: ([], []) for k in ('plain', 'grad', 'curv')}
        for _ in range(a.reps):                              # interleaved: all three see the same machine
            for k, call in (('plain', lambda: ctx.trees_loglik(child, blen)), ('grad', lambda: ctx.trees_grad(child, blen)),
                            ('curv', lambda: ctx.trees_grad(child, blen, want_curv=True))):
                t0 = time.perf_counter()
                call()
                t[k][0].append((time.perf_counter() - t0) * 1e3)
                t[k][1].append(ctx.last_trees_stats['sweep_ms'])
            stats = dict(ctx.last_trees_stats)
    q = {k: (quartiles(v[0]), quartiles(v[1])) for k, v in t.items()}
    n_fd = 4 * (N - 1) + 1
    rec = {'probe': 'trees_grad', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': a.trees, 'jc': jc, 'reps': a.reps,
           'plain_wall_ms': q['plain'][0], 'plain_device_ms': q['plain'][1], 'grad_wall_ms': q['grad'][0], 'grad_device_ms': q['grad'][1],
           'curv_wall_ms': q['curv'][0], 'curv_device_ms': q['curv'][1],
           'device_ratio_grad_over_plain': q['grad'][1]['median'] / q['plain'][1]['median'],
           'device_ratio_curv_over_plain': q['curv'][1]['median'] / q['plain'][1]['median'],
           'wall_ratio_grad_over_plain': q['grad'][0]['median'] / q['plain'][0]['median'],
           'wall_ratio_curv_over_plain': q['curv'][0]['median'] / q['plain'][0]['median'],
           'central_difference_calls': n_fd, 'central_difference_device_ms': n_fd * q['plain'][1]['median'],
           'launches': stats['n_launches'], 'units': stats['units'], 'units_per_s_device_grad': stats['units'] / (q['grad'][1]['median'] * 1e-3),
           'loglik_and_grad_bit_equal': same, 'finite': bool(np.isfinite(grad).all() and np.isfinite(curv).all())}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0 if same else 1


def grad_rates_probe(a):
    """phylo_trees_grad_rates against C calls of phylo_trees_grad on the scaled trees: same trees, same context, same run"""
    from phylo_amd import rates as R
    jc = a.jc.lower() == 'true'
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    rng = np.random.default_rng(a.seed)
    rows = [random_rows(N, rng) for _ in range(a.trees)]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    rates, weights = R.rate_model(a.alpha, a.rates)
    C = rates.size
    scaled = [rates[c] * blen for c in range(C)]             # (outside the timed region: the caller of C plain calls holds them)
    forms = {'grad': {}, 'curv': dict(want_curv=True), 'all': dict(want_curv=True, want_params=True)}
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, np.full(4, 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=jc)
        ll = ctx.trees_loglik_rates(child, blen, rates, weights)                           # warm-up of every form
        outs = {k: ctx.trees_grad_rates(child, blen, rates, weights, **kw) for k, kw in forms.items()}
        per_chunk = 6 if ctx.last_trees_stats['n_launches'] % 6 == 0 else 5
        chunks = ctx.last_trees_stats['n_launches'] // per_chunk
        for c in range(C):
            ctx.trees_grad(child, scaled[c], want_curv=True)
        same = all(bool(np.array_equal(o[0].view(np.uint64), ll.view(np.uint64)) and
                        np.array_equal(o[1].view(np.uint64), outs['grad'][1].view(np.uint64))) for o in outs.values())
        t = {k: ([], []) for k in list(forms) + ['plain_x_C']}
        for _ in range(a.reps):                              # interleaved: all see the same machine
            for k, kw in forms.items():
                t0 = time.perf_counter()
                ctx.trees_grad_rates(child, blen, rates, weights, **kw)
                t[k][0].append((time.perf_counter() - t0) * 1e3)
                t[k][1].append(ctx.last_trees_stats['sweep_ms'])
                stats = dict(ctx.last_trees_stats)
            t0 = time.perf_counter()
            d = 0.0
            for c in range(C):
                ctx.trees_grad(child, scaled[c], want_curv=True)
                d += ctx.last_trees_stats['sweep_ms']
            t['plain_x_C'][0].append((time.perf_counter() - t0) * 1e3)
            t['plain_x_C'][1].append(d)
    q = {k: (quartiles(v[0]), quartiles(v[1])) for k, v in t.items()}
    rec = {'probe': 'trees_grad_rates', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': a.trees, 'jc': jc, 'reps': a.reps,
           'C': int(C), 'alpha': a.alpha, 'chunks': int(chunks)}
    for k in t:
        rec[k + '_wall_ms'], rec[k + '_device_ms'] = q[k]
    for k in forms:
        rec['device_ratio_%s_over_plain_x_C' % k] = q[k][1]['median'] / q['plain_x_C'][1]['median']
        rec['wall_ratio_%s_over_plain_x_C' % k] = q[k][0]['median'] / q['plain_x_C'][0]['median']
    rec.update({'launches': stats['n_launches'], 'units': stats['units'],
                'units_per_s_device_curv': stats['units'] / (q['curv'][1]['median'] * 1e-3), 'loglik_and_grad_bit_equal': same,
                'finite': bool(all(np.isfinite(x).all() for x in outs['all']))})
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0 if same else 1


def nni_probe(a):
    """phylo_trees_nni against phylo_trees_loglik on the explicitly built neighbours of the same trees, and against
    phylo_trees_grad: same trees, same context, same run.  The neighbours of the first --explicit_trees trees are built as rows
    (phylo_amd.treesearch.apply_nni, outside the timed region: 2 (N-2) or 2 (N-1) trees each) and compared per tree of the set."""
    from phylo_amd.treesearch import apply_nni, nni_moves
    jc = a.jc.lower() == 'true'
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    rng = np.random.default_rng(a.seed)
    rows = [random_rows(N, rng) for _ in range(a.trees)]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    n_x = min(a.explicit_trees, a.trees) if a.explicit_trees > 0 else a.trees
    at, cs, bs = [], [], []
    for t in range(n_x):
        for mv in nni_moves(child[t]):
            c2, b2 = apply_nni(child[t], blen[t], *mv)
            at.append((t,) + mv)
            cs.append(c2)
            bs.append(b2)
    xc, xb, at = np.array(cs), np.array(bs), np.array(at)
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, np.full(4, 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=jc)
        ll = ctx.trees_loglik(child, blen)                   # warm-up of every call
        ln, delta = ctx.trees_nni(child, blen)
        ctx.trees_nni(child[:n_x], blen[:n_x])
        ctx.trees_grad(child, blen)
        ctx.trees_grad(child, blen, want_curv=True)
        lx = ctx.trees_loglik(xc, xb)
        same = bool(np.array_equal(ll.view(np.uint64), ln.view(np.uint64)))
        with np.errstate(invalid='ignore'):
            diff = np.abs((ll[at[:, 0]] + delta[at[:, 0], at[:, 1], at[:, 2]]) - lx) / np.abs(lx)
        worst = float(np.nanmax(diff))
        calls = (('plain', lambda: ctx.trees_loglik(child, blen)), ('nni', lambda: ctx.trees_nni(child, blen)),
                 ('nni_subset', lambda: ctx.trees_nni(child[:n_x], blen[:n_x])), ('explicit_subset', lambda: ctx.trees_loglik(xc, xb)),
                 ('grad', lambda: ctx.trees_grad(child, blen)), ('curv', lambda: ctx.trees_grad(child, blen, want_curv=True)))
        t = {k: ([], []) for k, _ in calls}
        stats = {}
        for _ in range(a.reps):                              # interleaved: every call sees the same machine
            for k, call in calls:
                t0 = time.perf_counter()
                call()
                t[k][0].append((time.perf_counter() - t0) * 1e3)
                t[k][1].append(ctx.last_trees_stats['sweep_ms'])
                stats[k] = dict(ctx.last_trees_stats)
    q = {k: (quartiles(v[0]), quartiles(v[1])) for k, v in t.items()}
    rec = {'probe': 'trees_nni', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': a.trees, 'jc': jc, 'reps': a.reps,
           'explicit_trees': int(n_x), 'neighbours': int(xc.shape[0])}
    for k in t:
        rec[k + '_wall_ms'], rec[k + '_device_ms'] = q[k]
    rec.update({'device_ratio_nni_over_plain': q['nni'][1]['median'] / q['plain'][1]['median'],
                'device_ratio_nni_over_grad': q['nni'][1]['median'] / q['grad'][1]['median'],
                'device_ratio_nni_over_curv': q['nni'][1]['median'] / q['curv'][1]['median'],
                'device_ratio_explicit_over_nni_same_trees': q['explicit_subset'][1]['median'] / q['nni_subset'][1]['median'],
                'wall_ratio_explicit_over_nni_same_trees': q['explicit_subset'][0]['median'] / q['nni_subset'][0]['median'],
                'launches': stats['nni']['n_launches'], 'units': stats['nni']['units'],
                'units_per_s_device_nni': stats['nni']['units'] / (q['nni'][1]['median'] * 1e-3),
                'loglik_bit_equal': same, 'worst_relative_difference_to_explicit': worst,
                'finite': bool(np.isfinite(delta[at[:, 0], at[:, 1], at[:, 2]]).all())})
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0 if same and worst < 1e-9 else 1


def nni_rates_probe(a):
    """phylo_trees_nni_rates against C calls of phylo_trees_nni on the scaled trees and against phylo_trees_loglik_rates on the
    explicitly built neighbours of the first --explicit_trees trees: same trees, same context, same run"""
    from phylo_amd import rates as R
    from phylo_amd.treesearch import apply_nni, nni_moves
    jc = a.jc.lower() == 'true'
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    rng = np.random.default_rng(a.seed)
    rows = [random_rows(N, rng) for _ in range(a.trees)]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    rates, weights = R.rate_model(a.alpha, a.rates)
    C = rates.size
    scaled = [rates[c] * blen for c in range(C)]             # (outside the timed region: the caller of C plain calls holds them)
    n_x = min(a.explicit_trees, a.trees) if a.explicit_trees > 0 else a.trees
    at, cs, bs = [], [], []
    for t in range(n_x):
        for mv in nni_moves(child[t]):
            c2, b2 = apply_nni(child[t], blen[t], *mv)
            at.append((t,) + mv)
            cs.append(c2)
            bs.append(b2)
    xc, xb, at = np.array(cs), np.array(bs), np.array(at)
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, np.full(4, 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=jc)
        ll = ctx.trees_loglik_rates(child, blen, rates, weights)          # warm-up of every call
        ln, delta = ctx.trees_nni_rates(child, blen, rates, weights)
        per_chunk = 5 if ctx.last_trees_stats['n_launches'] % 5 == 0 else 4
        chunks = ctx.last_trees_stats['n_launches'] // per_chunk
        ctx.trees_nni_rates(child[:n_x], blen[:n_x], rates, weights)
        for c in range(C):
            ctx.trees_nni(child, scaled[c])
        lx = ctx.trees_loglik_rates(xc, xb, rates, weights)
        same = bool(np.array_equal(ll.view(np.uint64), ln.view(np.uint64)))
        with np.errstate(invalid='ignore'):
            diff = np.abs((ll[at[:, 0]] + delta[at[:, 0], at[:, 1], at[:, 2]]) - lx) / np.abs(lx)
        worst = float(np.nanmax(diff))

        def plain_x_C():
            d = 0.0
            for c in range(C):
                ctx.trees_nni(child, scaled[c])
                d += ctx.last_trees_stats['sweep_ms']
            ctx.last_trees_stats['sweep_ms'] = d

        calls = (('nni_rates', lambda: ctx.trees_nni_rates(child, blen, rates, weights)), ('plain_x_C', plain_x_C),
                 ('nni_rates_subset', lambda: ctx.trees_nni_rates(child[:n_x], blen[:n_x], rates, weights)),
                 ('explicit_subset', lambda: ctx.trees_loglik_rates(xc, xb, rates, weights)))
        t = {k: ([], []) for k, _ in calls}
        stats = {}
        for _ in range(a.reps):                              # interleaved: every call sees the same machine
            for k, call in calls:
                t0 = time.perf_counter()
                call()
                t[k][0].append((time.perf_counter() - t0) * 1e3)
                t[k][1].append(ctx.last_trees_stats['sweep_ms'])
                stats[k] = dict(ctx.last_trees_stats)
    q = {k: (quartiles(v[0]), quartiles(v[1])) for k, v in t.items()}
    rec = {'probe': 'trees_nni_rates', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': a.trees, 'jc': jc, 'reps': a.reps,
           'C': int(C), 'alpha': a.alpha, 'chunks': int(chunks), 'explicit_trees': int(n_x), 'neighbours': int(xc.shape[0])}
    for k in t:
        rec[k + '_wall_ms'], rec[k + '_device_ms'] = q[k]
    rec.update({'device_ratio_nni_rates_over_plain_x_C': q['nni_rates'][1]['median'] / q['plain_x_C'][1]['median'],
                'wall_ratio_nni_rates_over_plain_x_C': q['nni_rates'][0]['median'] / q['plain_x_C'][0]['median'],
                'device_ratio_explicit_over_nni_rates_same_trees': q['explicit_subset'][1]['median'] / q['nni_rates_subset'][1]['median'],
                'wall_ratio_explicit_over_nni_rates_same_trees': q['explicit_subset'][0]['median'] / q['nni_rates_subset'][0]['median'],
                'launches': stats['nni_rates']['n_launches'], 'units': stats['nni_rates']['units'],
                'units_per_s_device_nni_rates': stats['nni_rates']['units'] / (q['nni_rates'][1]['median'] * 1e-3),
                'loglik_bit_equal': same, 'worst_relative_difference_to_explicit': worst,
                'finite': bool(np.isfinite(delta[at[:, 0], at[:, 1], at[:, 2]]).all())})
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0 if same and worst < 1e-9 else 1


def ancestral_probe(a):
    """phylo_trees_ancestral with states only and with post against phylo_trees_grad without curvature: same trees, same context,
    same run"""
    jc = a.jc.lower() == 'true'
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    rng = np.random.default_rng(a.seed)
    rows = [random_rows(N, rng) for _ in range(a.trees)]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    n_post = min(a.post_trees, a.trees) if a.post_trees > 0 else a.trees
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    u64 = lambda x: np.ascontiguousarray(x).view(np.uint64)
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, np.full(4, 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=jc)
        lg, grad = ctx.trees_grad(child, blen)               # warm-up of all three
        ls, state = ctx.trees_ancestral(child, blen, want_post=False, want_state=True)
        lp, post, state_p = ctx.trees_ancestral(child[:n_post], blen[:n_post])
        same = bool(np.array_equal(u64(lg), u64(ls)) and np.array_equal(u64(lg[:n_post]), u64(lp)) and np.array_equal(state[:n_post], state_p))
        nostate = int((state == _ffi.ANC_NOSTATE).sum())
        del post, state_p
        calls = (('grad', lambda: ctx.trees_grad(child, blen)),
                 ('state', lambda: ctx.trees_ancestral(child, blen, want_post=False, want_state=True)),
                 ('post', lambda: ctx.trees_ancestral(child[:n_post], blen[:n_post], want_post=True, want_state=False)))
        t = {k: ([], []) for k, _ in calls}
        stats = {}
        for _ in range(a.reps):                              # interleaved: all three see the same machine
            for k, call in calls:
                t0 = time.perf_counter()
                call()
                t[k][0].append((time.perf_counter() - t0) * 1e3)
                t[k][1].append(ctx.last_trees_stats['sweep_ms'])
                stats[k] = dict(ctx.last_trees_stats)
    q = {k: (quartiles(v[0]), quartiles(v[1])) for k, v in t.items()}
    per = 4 if ((g == 0) | (g == 1)).all() and (g.sum(axis=2) >= 1).all() else 3
    rec = {'probe': 'trees_ancestral', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': a.trees, 'post_trees': int(n_post), 'jc': jc,
           'reps': a.reps, 'grad_wall_ms': q['grad'][0], 'grad_device_ms': q['grad'][1], 'state_wall_ms': q['state'][0],
           'state_device_ms': q['state'][1], 'post_wall_ms': q['post'][0], 'post_device_ms': q['post'][1],
           'device_ratio_state_over_grad': q['state'][1]['median'] / q['grad'][1]['median'],
           'wall_ratio_state_over_grad': q['state'][0]['median'] / q['grad'][0]['median'],
           'state_bytes_written': float(a.trees) * (N - 1) * S, 'post_bytes_written': float(n_post) * (N - 1) * S * 32,
           'post_device_GB_per_s': float(n_post) * (N - 1) * S * 32 / (q['post'][1]['median'] * 1e-3) / 1e9,
           'state_launches': stats['state']['n_launches'], 'state_chunks': stats['state']['n_launches'] // per,
           'post_launches': stats['post']['n_launches'], 'post_chunks': stats['post']['n_launches'] // per,
           'units': stats['state']['units'], 'units_per_s_device_state': stats['state']['units'] / (q['state'][1]['median'] * 1e-3),
           'units_per_s_device_grad': stats['grad']['units'] / (q['grad'][1]['median'] * 1e-3),
           'sites_without_state': nostate, 'loglik_bit_equal': same}
    line = json.dumps(rec)
    print(line)
    print("loglik bit for bit phylo_trees_grad's: %s" % same)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0 if same else 1


def ancestral_rates_probe(a):
    """phylo_trees_ancestral_rates under C discrete Gamma categories -- states only, the site rates only (catpost and siterate),
    and with post (on the first post_trees trees) -- against phylo_trees_grad_rates without curvature and against C calls of
    phylo_trees_ancestral (states only) on the scaled trees: same trees, same context, same run"""
    from phylo_amd import rates as rates_mod
    jc = a.jc.lower() == 'true'
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    rng = np.random.default_rng(a.seed)
    rows = [random_rows(N, rng) for _ in range(a.trees)]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    n_post = min(a.post_trees, a.trees) if a.post_trees > 0 else a.trees
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    r, w = rates_mod.rate_model(a.alpha, a.rates)
    nc = r.size
    u64 = lambda x: np.ascontiguousarray(x).view(np.uint64)
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, np.full(4, 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=jc)
        calls = (('grad', lambda: ctx.trees_grad_rates(child, blen, r, w)),
                 ('plain', lambda: [ctx.trees_ancestral(child, rc * blen, want_post=False, want_state=True) for rc in r]),
                 ('state', lambda: ctx.trees_ancestral_rates(child, blen, r, w, want_post=False, want_state=True)),
                 ('rates', lambda: ctx.trees_ancestral_rates(child, blen, r, w, want_post=False, want_state=False, want_catpost=True,
                                                             want_siterate=True)),
                 ('post', lambda: ctx.trees_ancestral_rates(child[:n_post], blen[:n_post], r, w, want_post=True, want_state=False)))
        warm = {k: call() for k, call in calls}             # warm-up of all of them
        ls, sites, cats = ctx.trees_loglik_rates(child, blen, r, w, want_sites=True, want_cats=True)
        same = bool(np.array_equal(u64(warm['state'][0]), u64(ls)) and np.array_equal(u64(warm['grad'][0]), u64(ls)) and
                    np.array_equal(u64(warm['rates'][1]), u64((w[None, :, None] * cats) * (1.0 / sites)[:, None, :])))
        nostate = int((warm['state'][1] == _ffi.ANC_NOSTATE).sum())
        mean_rate = float(np.nanmean(warm['rates'][2]))
        del warm
        t = {k: ([], []) for k, _ in calls}
        stats = {}
        for _ in range(a.reps):                              # interleaved: all of them see the same machine
            for k, call in calls:
                dev = 0.0
                t0 = time.perf_counter()
                if k == 'plain':
                    for rc in r:
                        ctx.trees_ancestral(child, rc * blen, want_post=False, want_state=True)
                        dev += ctx.last_trees_stats['sweep_ms']
                else:
                    call()
                    dev = ctx.last_trees_stats['sweep_ms']
                t[k][0].append((time.perf_counter() - t0) * 1e3)
                t[k][1].append(dev)
                stats[k] = dict(ctx.last_trees_stats)
    q = {k: (quartiles(v[0]), quartiles(v[1])) for k, v in t.items()}
    per = 4 if ((g == 0) | (g == 1)).all() and (g.sum(axis=2) >= 1).all() else 3
    rec = {'probe': 'trees_ancestral_rates', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': a.trees, 'post_trees': int(n_post),
           'C': int(nc), 'alpha': a.alpha, 'jc': jc, 'reps': a.reps}
    for k in t:
        rec[k + '_wall_ms'], rec[k + '_device_ms'] = q[k]
    rec.update({'device_ratio_state_over_grad_rates': q['state'][1]['median'] / q['grad'][1]['median'],
                'device_ratio_state_over_C_plain_calls': q['state'][1]['median'] / q['plain'][1]['median'],
                'wall_ratio_state_over_C_plain_calls': q['state'][0]['median'] / q['plain'][0]['median'],
                'state_launches': stats['state']['n_launches'], 'state_chunks': stats['state']['n_launches'] // per,
                'post_launches': stats['post']['n_launches'], 'post_chunks': stats['post']['n_launches'] // per,
                'post_bytes_written': float(n_post) * (N - 1) * S * 32,
                'post_device_GB_per_s': float(n_post) * (N - 1) * S * 32 / (q['post'][1]['median'] * 1e-3) / 1e9,
                'units': stats['state']['units'], 'units_per_s_device_state': stats['state']['units'] / (q['state'][1]['median'] * 1e-3),
                'units_per_s_device_grad_rates': stats['grad']['units'] / (q['grad'][1]['median'] * 1e-3),
                'sites_without_state': nostate, 'mean_site_rate': mean_rate, 'bit_contracts_hold': same})
    line = json.dumps(rec)
    print(line)
    print("loglik bit for bit phylo_trees_loglik_rates', catpost its cat_lik and site_lik: %s" % same)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0 if same else 1


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--dataset', default='hohna_data')
    ap.add_argument('--trees', type=int, default=4096)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--loop_trees', type=int, default=0, help='trees the loop over tree_loglik takes (0: all)')
    ap.add_argument('--loop_reps', type=int, default=3)
    ap.add_argument('--jc', default='false')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('--out', default=None)
    ap.add_argument('--rates', type=int, default=0, help='C > 0: probe phylo_trees_loglik_rates under C Gamma categories')
    ap.add_argument('--alpha', type=float, default=0.5)
    ap.add_argument('--grad', action='store_true', help='probe phylo_trees_grad (with and without curvature) against the plain call')
    ap.add_argument('--nni', action='store_true', help='probe phylo_trees_nni against phylo_trees_loglik on the explicit neighbours, and phylo_trees_grad')
    ap.add_argument('--explicit_trees', type=int, default=512, help='with --nni: trees whose neighbours are built and scored explicitly (0: all)')
    ap.add_argument('--model', action='store_true', help='probe phylo_trees_grad_model against phylo_trees_grad, the plain call and central differences')
    ap.add_argument('--ancestral', action='store_true', help='probe phylo_trees_ancestral (states only, and with post) against phylo_trees_grad')
    ap.add_argument('--post_trees', type=int, default=512, help='with --ancestral: trees of the call that asks for post (0: all)')
    ap.add_argument('--dirs', type=int, default=12, help='with --model: directions of a call (1 .. 16)')
    a = ap.parse_args(argv)
    if a.ancestral and a.rates > 0:
        return ancestral_rates_probe(a)
    if a.ancestral:
        return ancestral_probe(a)
    if a.model:
        return model_probe(a)
    if a.nni and a.rates > 0:
        return nni_rates_probe(a)
    if a.nni:
        return nni_probe(a)
    if a.grad and a.rates > 0:
        return grad_rates_probe(a)
    if a.grad:
        return grad_probe(a)
    if a.rates > 0:
        return rates_probe(a)
    jc = a.jc.lower() == 'true'
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    rng = np.random.default_rng(a.seed)
    rows = [random_rows(N, rng) for _ in range(a.trees)]
    child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    Q = model.jc_Q() if jc else model.get_Q(model.init_y_q())
    pi = np.full(4, 0.25)
    n_loop = a.trees if a.loop_trees <= 0 else min(a.loop_trees, a.trees)
    nodes = []
    for c, b in rows[:n_loop]:
        left = np.full(2 * N - 1, -1, dtype=np.int32)
        right = left.copy()
        bl, br = np.zeros(2 * N - 1), np.zeros(2 * N - 1)
        left[N:], right[N:], bl[N:], br[N:] = c[:, 0], c[:, 1], b[:, 0], b[:, 1]
        nodes.append((left, right, bl, br))
    with _ffi.Context(4, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, np.full(N - 1, 10.0), np.full(N - 1, 10.0), jc69_closed_form=jc)
        ll = ctx.trees_loglik(child, blen)                   # warm-up: scratch, code objects
        wall, dev = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ll = ctx.trees_loglik(child, blen)
            wall.append((time.perf_counter() - t0) * 1e3)
            dev.append(ctx.last_trees_stats['sweep_ms'])
        stats = dict(ctx.last_trees_stats)
        ctx.tree_loglik(*nodes[0], 2 * N - 2, g, pi, want_root=False)
        loop = []
        for _ in range(a.loop_reps):
            t0 = time.perf_counter()
            one = np.array([ctx.tree_loglik(l, r, x, y, 2 * N - 2, g, pi, want_root=False)[0] for l, r, x, y in nodes])
            loop.append((time.perf_counter() - t0) * 1e3)
    same = bool(np.array_equal(one.view(np.uint64), ll[:n_loop].view(np.uint64)))
    w, d, lp = quartiles(wall), quartiles(dev), quartiles(loop)
    rec = {'probe': 'trees_loglik', 'dataset': a.dataset, 'N': int(N), 'S': int(S), 'trees': a.trees, 'jc': jc, 'reps': a.reps,
           'batched_wall_ms': w, 'batched_device_ms': d, 'launches': stats['n_launches'], 'units': stats['units'],
           'units_per_s_device': stats['units'] / (d['median'] * 1e-3), 'units_per_s_wall': stats['units'] / (w['median'] * 1e-3),
           'us_per_tree_wall': w['median'] * 1e3 / a.trees,
           'loop_trees': n_loop, 'loop_reps': a.loop_reps, 'loop_wall_ms': lp, 'loop_us_per_tree': lp['median'] * 1e3 / n_loop,
           'ratio_loop_over_batched_per_tree': (lp['median'] / n_loop) / (w['median'] / a.trees),
           'bit_equal': same, 'finite': bool(np.isfinite(ll).all())}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main())
