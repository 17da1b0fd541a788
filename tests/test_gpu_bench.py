"""bench.py on one GPU: a plain run times exactly --steps steps and carries no --full figures; --dump-outputs writes the
last timed step, which is the oracle's sweep of the last step's seed bit for bit."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from oracle import c_oracle as CO
from phylo_amd import model as M
from phylo_amd.datasets import load_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


# 12 steps: one launch set of 12 sweeps (the last step is its last group); --batch 5: two launch sets, then 2 single sweeps
@pytest.mark.parametrize("extra", [[], ['--batch', '5']], ids=["launch-sets", "remainder"])
def test_plain_run_dumps_the_last_step(extra):
    steps, K = 12, 64
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), '--gpus', '1', '--steps', str(steps), '--warmup', '2',
               '--n_particles', str(K), '--dump-outputs', tmp] + extra
        p = subprocess.run(cmd, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        line = json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith('{')][-1])
        dumped = {f[:-4]: np.load(os.path.join(tmp, f)) for f in os.listdir(tmp)}
    assert line['steps'] == steps and line['timed_region']['repeats'] == 1 and line['ms_per_step'] > 0
    assert not {'t_sweep_ms', 'roofline', 'delta_logZ_max', 'vi_step', 'cpu_baseline'} & set(line)
    g = load_dataset('primate_data')['genome']
    N = g.shape[0]
    lam = np.full(N - 1, 10.0)
    ref = CO.sweep(g, M.get_Q(M.init_y_q()), M.get_stationary_probs(np.zeros(4) + 0.25), lam, lam, K, steps - 1)
    assert set(dumped) == {'log_weights', 'log_likelihood', 'left_branches', 'right_branches', 'merges', 'ancestors', 'log_Z'}
    for name in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches', 'merges', 'ancestors'):
        assert dumped[name].dtype == np.float64
        assert np.array_equal(dumped[name].view(np.uint64), np.asarray(ref[name], dtype=np.float64).view(np.uint64)), name
    assert dumped['log_Z'][0] == ref['logZ'] == line['log_Z']
