"""Timing of one VI training step (sweep with the graph kept + reverse pass + host update) and a short ELBO
trajectory.  python tools/train_probe.py [--K 2048] [--sites 898] [--steps 20] [--epochs 0]
--batched G: one batched step over G particle systems of K particles each (one batched sweep, one reverse pass) next to G serial
steps on the same model and seeds in the same process; medians of --steps steps after 3 warm-ups, appended to
profiles/train_batched_probe.jsonl.
--synthetic N S: a coded alignment (A, C, G, T, gap) of N taxa x S sites drawn here from numpy's default_rng(--synthetic-seed) instead of
a dataset -- the shipped data stops at 64 taxa (DS8), training does not (2 ... 512).  --out FILE appends the result line to FILE
(profiles/train_many_taxa_probe.jsonl is where recorded ones go)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from phylo_amd import train as T                    # noqa: E402
from phylo_amd.datasets import load_dataset         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--dataset', default='primate_data')
ap.add_argument('--K', type=int, default=2048)
ap.add_argument('--sites', type=int, default=0)
ap.add_argument('--steps', type=int, default=20)
ap.add_argument('--jcmodel', action='store_true')
ap.add_argument('--nested', action='store_true')
ap.add_argument('--phases', action='store_true')
ap.add_argument('--M', type=int, default=1)
ap.add_argument('--batched', type=int, default=0)
ap.add_argument('--synthetic', type=int, nargs=2, metavar=('N', 'S'), default=None)
ap.add_argument('--synthetic-seed', type=int, default=20260005)
ap.add_argument('--out', default='')
a = ap.parse_args()

if a.synthetic:
    codes = np.random.default_rng(a.synthetic_seed).integers(0, 5, size=tuple(a.synthetic))
    genome = np.stack([(codes == b) | (codes == 4) for b in range(4)], axis=-1).astype(np.float64)
    a.dataset = 'synthetic_%dx%d_seed%d' % (a.synthetic[0], a.synthetic[1], a.synthetic_seed)
else:
    genome = load_dataset(a.dataset)['genome']
N, S, _ = genome.shape
B = a.sites or S
if a.batched > 1:
    Gn = a.batched
    rng = np.random.default_rng(0)
    sites = np.sort(rng.permutation(S)[:B])                # one minibatch for every step: the leaves stay on the device
    res = {}
    for name, batched in (('serial', 1), ('batched', Gn)):
        # lr = 0: every step sees the same model, so the two runs time the same work on the same seeds
        tr = T.Trainer(genome, a.K, T.Variables(N, np.log(10.0), a.jcmodel), T.make_optimizer('GradientDescentOptimizer', 0.0), B,
                       batched=batched)
        fw, bw, wall = [], [], []
        for i in range(a.steps + 3):
            seeds = [i + (g << 32) for g in range(Gn)]
            t0 = time.perf_counter()
            if batched > 1:
                tr.step(sites, seeds[0], seeds[1:])
                f, b = tr.last['raw']['forward_ms'], tr.last['raw']['backward_ms']
            else:                                           # G sweep-and-reverse-pass pairs one after the other (what Trainer.step does)
                f = b = 0.0
                for sd in seeds:
                    tr.step(sites, sd)
                    f += tr.last['raw']['forward_ms']
                    b += tr.last['raw']['backward_ms']
            t1 = time.perf_counter()
            if i >= 3:
                fw.append(f); bw.append(b); wall.append((t1 - t0) * 1e3)
        res[name] = {'forward_ms': float(np.median(fw)), 'backward_ms': float(np.median(bw)), 'step_wall_ms': float(np.median(wall)),
                     'step_wall_ms_min': float(np.min(wall)), 'step_wall_ms_p25': float(np.percentile(wall, 25)),
                     'step_wall_ms_p75': float(np.percentile(wall, 75)), 'backward_lists': tr.last['raw']['backward_lists']}
        tr.close()
    line = {'dataset': a.dataset, 'K_per_system': a.K, 'G': Gn, 'N': N, 'sites': B, 'steps': a.steps, 'serial_G_steps': res['serial'],
            'batched_step': res['batched'], 'ratio_serial_over_batched': res['serial']['step_wall_ms'] / res['batched']['step_wall_ms']}
    print(json.dumps(line))
    out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'train_batched_probe.jsonl')
    with open(out, 'a') as fh:
        fh.write(json.dumps(line) + '\n')
    sys.exit(0)

v = T.Variables(N, np.log(10.0), a.jcmodel)
tr = T.Trainer(genome, a.K, v, T.make_optimizer('Adam', 0.01), B, nested=a.nested, M=a.M)
rng = np.random.default_rng(0)
fw, bw, wall, hostms, launches = [], [], [], [], []
phases = {}
if a.phases:                      # wall time of every host call of a step (Trainer.gradients, taken apart)
    orig = {}
    for name in ('set_model', 'sweep_async', 'sweep_fetch', 'sweep_backward', 'set_leaves'):
        fn = getattr(tr.ctx, name)
        def timed(*args, _fn=fn, _name=name, **kw):
            t = time.perf_counter()
            out = _fn(*args, **kw)
            phases.setdefault(_name, []).append((time.perf_counter() - t) * 1e3)
            return out
        setattr(tr.ctx, name, timed)
for i in range(a.steps + 3):
    sites = np.sort(rng.permutation(S)[:B])
    if i == 3:
        phases.clear()
    t0 = time.perf_counter()
    tr.step(sites, seed=i)
    t1 = time.perf_counter()
    if i >= 3:
        fw.append(tr.last['raw']['forward_ms'])
        bw.append(tr.last['raw']['backward_ms'])
        hostms.append(tr.last['raw'].get('backward_host_ms', 0.0))
        wall.append((t1 - t0) * 1e3)
        launches.append(tr.last['raw'].get('backward_launches', 0))
if a.phases:
    print(json.dumps({'host_call_ms': {k: float(np.mean(v)) for k, v in phases.items()}}))
line = {'dataset': a.dataset, 'nested': a.nested, 'M': a.M, 'K': a.K, 'N': N, 'sites': B, 'steps': a.steps,
        'forward_ms': float(np.mean(fw)), 'backward_ms': float(np.mean(bw)), 'backward_host_ms': float(np.mean(hostms)), 'step_wall_ms': float(np.mean(wall)),
        'step_wall_ms_min': float(np.min(wall)), 'last_logZ': tr.last['logZ'],
        'forward_ms_median': float(np.median(fw)), 'backward_ms_median': float(np.median(bw)), 'step_wall_ms_median': float(np.median(wall)),
        'step_wall_ms_p25': float(np.percentile(wall, 25)), 'step_wall_ms_p75': float(np.percentile(wall, 75)),
        'backward_launches': int(np.median(launches)), 'backward_lists': tr.last['raw'].get('backward_lists', '')}
print(json.dumps(line))
if a.out:
    with open(a.out, 'a') as fh:
        fh.write(json.dumps(line) + '\n')
tr.close()
