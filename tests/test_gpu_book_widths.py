"""The bookkeeping at a wave per particle (pk_rank_book_packed<64>) against the C oracle, bit for bit: the strided key loop of more
than 63 Philox key blocks (257 taxa), batched groups at 64 lanes, both sides of the combined launch's limit, owner-held tables
with the cache of remote nodes on two ranks, and the twisted proposal's search.  tests/book_width_cases.py says what each case is
there for; tests/test_book_widths_cpu.py pins the plan facts the cases stand on.  No tolerances: the contract is bit equality."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import book_width_cases as BC
import many_taxa_cases as MC
from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FLOATS = ('log_weights', 'log_likelihood', 'left_branches', 'right_branches')
FORMS = {'default': _ffi.FLAGS_DEFAULT, 'eager': _ffi.FLAGS_DEFAULT | _ffi.EAGER_NODES, 'keep-graph': _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, ref, tag, keys=FLOATS):
    np.testing.assert_array_equal(got['ancestors'], ref['ancestors'], err_msg=tag)
    np.testing.assert_array_equal(got['merges'], ref['merges'], err_msg=tag)
    for key in keys:
        bad = np.argwhere(bits(got[key]) != bits(ref[key]))
        assert len(bad) == 0, "%s: %s: %d of %d differ, first at %s" % (tag, key, len(bad), got[key].size, tuple(bad[0]))
    assert bits(got['logZ']) == bits(ref['logZ']), "%s: log Z %r against %r" % (tag, got['logZ'], ref['logZ'])


def sweep_case(name, flags):
    """the case's sweep, cut into its groups: [{arrays of Kg particles, 'logZ'}]"""
    c = BC.CASES[name]
    g, Q, pi, lam_l, lam_r = BC.model(c["N"])
    G, Kg = c["G"], c["Kg"]
    with _ffi.Context(G * Kg, c["N"], BC.S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam_l, lam_r)
        if G == 1:
            out = ctx.sweep(c["seeds"][0], flags=flags)
            logz = [out['logZ']]
        else:
            ctx.sweep_batch_async(list(c["seeds"]), flags=flags)
            out = ctx.sweep_fetch()
            logz = ctx.sweep_fetch_logz(G)
    plan = _ffi.debug_sweep_plan(c["N"], G * Kg, BC.S, G=G, flags=flags & ~_ffi.FLAGS_DEFAULT)
    assert out['stats']['n_launches'] == sum(plan['launches'])
    return [dict({k: out[k][:, i * Kg:(i + 1) * Kg] for k in FLOATS + ('ancestors', 'merges')}, logZ=logz[i]) for i in range(G)]


@pytest.mark.parametrize("form", list(FORMS))
def test_key_block_loop_at_257_taxa(form):
    got, = sweep_case("key-loop", FORMS[form])
    same(got, BC.reference("key-loop")[0], "key-loop " + form)


@pytest.mark.parametrize("name", ["key-loop-batched", "n65", "n33-batched"])
def test_wave_per_particle_against_the_oracle(name):
    for i, (got, ref) in enumerate(zip(sweep_case(name, _ffi.FLAGS_DEFAULT), BC.reference(name))):
        same(got, ref, "%s group %d" % (name, i))


def run_world(extra_env):
    """tests/test_gpu_sharded.py::run_world for BC.SHARDED: every rank a process of its own on GPU 0, under its own time limit"""
    c = BC.SHARDED
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, PHYLO_RDZV_DIR=tmp, MASTER_PORT=str(29000 + os.getpid() % 2000), PHYLO_COMM='hostshm')
        env.update(extra_env)
        procs = []
        for r in range(c["world"]):
            out = os.path.join(tmp, "r%d.npz" % r)
            procs.append((out, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_shard_worker.py"), str(r), str(c["world"]),
                                                 str(c["K"]), c["dataset"], str(c["seed"]), '0', out, '1'],
                                                env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
        outs = []
        for out, p in procs:
            try:
                log, _ = p.communicate(timeout=240)
            except subprocess.TimeoutExpired:
                for _, q in procs:
                    q.kill()
                raise
            assert p.returncode == 0, log.decode()[-2000:]
            outs.append(dict(np.load(out)))
        return outs


@pytest.fixture(scope="module")
def sharded_reference():
    c = BC.SHARDED
    g = load_dataset(c["dataset"])['genome']
    assert g.shape[:2] == (c["N"], c["S"])
    lam = np.full(c["N"] - 1, 10.0)
    return CO.sweep(g, O.get_Q(O.init_y_q()), np.full((1, 4), 0.25), lam, lam, c["K"], c["seed"])


@pytest.mark.parametrize("cache", ['default', 'full'])
def test_owner_held_tables_and_remote_cache_at_64_lanes(cache, sharded_reference):
    """Both ranks equal the unsharded oracle sweep.  (The worker reports the left branch lengths only.)"""
    c, ref = BC.SHARDED, sharded_reference
    parts = run_world({'PHYLO_REMOTE_CACHE_CAP': '1'} if cache == 'full' else {})
    Kl = c["K"] // c["world"]
    for r, p in enumerate(parts):
        assert int(p['k0']) == r * Kl
        sl = slice(r * Kl, (r + 1) * Kl)
        want = dict({k: ref[k][:, sl] for k in FLOATS + ('ancestors', 'merges')}, logZ=ref['logZ'])
        same(dict(p, logZ=float(p['logZ'])), want, "rank %d, %s cache" % (r, cache), keys=('log_weights', 'log_likelihood', 'left_branches'))
    assert (parts[0]['ancestors'] >= Kl).any()               # some ancestor of a rank-0 particle lives on the other rank
    used, cap = [int(p['cache_used']) for p in parts], [int(p['cache_cap']) for p in parts]
    if cache == 'full':
        assert cap == [1] * c["world"] and max(used) > 1, (used, cap)      # more nodes wanted than slots: the rest is read in place
    else:
        assert min(cap) > 0 and max(used) > 0, (used, cap)


def test_twisted_search_by_one_wave():
    c = BC.TWISTED
    g = MC.coded_alignment(1000 + c["N"], c["N"], c["S"])
    Q, pi, lam_l, lam_r = MC.random_model(2000 + c["N"], c["N"])
    with _ffi.Context(c["K"], c["N"], c["S"]) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, pi, lam_l, lam_r)
        out = ctx.sweep(c["seed"], flags=_ffi.FLAGS_DEFAULT | _ffi.TWISTING, M=c["M"])
    ref = CO.sweep_twisted(g, Q, pi, lam_l, lam_r, c["K"], c["M"], c["seed"])
    same(out, ref, "twisted")
    assert any(len(np.unique(row)) > 1 for row in ref['ancestors']) and (ref['ancestors'] != np.arange(c["K"])).any()
