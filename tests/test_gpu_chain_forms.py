"""Whole batched sweeps in the chain form of a rank event (sweep_chain_form_of, phylo_sweep_plan.h) -- the scan
hands out ancestors and adopted particles, the bookkeeping reads its ancestor, the adopted nodes are written from the list by item
waves inside the bookkeeping's launch -- against the C oracle per group seed and against the same sweep with PHYLO_SCAN_ANCESTORS=0, which issues the launches the library had before.  Equal bits in every array a caller can
fetch and in log Z-hat; every comparison first asks the context which form ran (phylo_debug_sweep_chain_of).  tests/
test_sweepchain_cpu.py restates the rule, tests/test_gpu_scan_ancestors.py tests the scan's tail alone."""
import numpy as np
import pytest

import many_taxa_cases as MC
from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi

pytestmark = pytest.mark.gpu
ARRAYS = ('log_weights', 'log_likelihood', 'left_branches', 'right_branches', 'merges', 'ancestors')     # bench.py's DUMP_ARRAYS
SWITCH = {'0': False, '1': True}                        # PHYLO_SCAN_ANCESTORS -> did the chain form run
#         N   S    G   Kg    lanes per particle of the bookkeeping
SHAPES = [(5, 70, 3, 96, 16), (12, 130, 16, 512, 8), (20, 64, 2, 128, 32), (40, 40, 2, 64, 64)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, ref, tag):
    for key in ARRAYS:
        bad = np.argwhere(bits(got[key]) != bits(ref[key]))
        assert len(bad) == 0, "%s: %s: %d of %d differ, first at %s" % (tag, key, len(bad), got[key].size, tuple(bad[0]))
    np.testing.assert_array_equal(bits(np.asarray(got['logZ'], dtype=np.float64)), bits(np.asarray(ref['logZ'], dtype=np.float64)), err_msg=tag)


def run(monkeypatch, switch, g, model, K, seeds, flags=_ffi.FLAGS_DEFAULT, jc=False, expect='rule', env=()):
    """one batched sweep of a fresh context under PHYLO_SCAN_ANCESTORS = switch: the fetched arrays, 'logZ' [G]; the context's
    answer to "which form ran" is asserted here"""
    N, S = g.shape[:2]
    monkeypatch.setenv('PHYLO_SCAN_ANCESTORS', switch)
    for k, v in env:
        monkeypatch.setenv(k, v)
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(*model, jc69_closed_form=jc)
        out = sweep(ctx, seeds, flags)
        assert ctx.debug_sweep_chain() == (SWITCH[switch] if expect == 'rule' else expect), (switch, ctx.debug_sweep_chain())
    return out


def sweep(ctx, seeds, flags=_ffi.FLAGS_DEFAULT):
    if len(seeds) == 1:
        out = ctx.sweep(int(seeds[0]), flags=flags)
        out['logZ'] = np.array([out['logZ']])
        return out
    ctx.sweep_batch_async(list(seeds), flags=flags)
    out = ctx.sweep_fetch()
    out['logZ'] = ctx.sweep_fetch_logz(len(seeds))
    return out


def oracle(g, model, Kg, seeds, jc=False):
    """the C oracle's sweep of every group seed, side by side like a batched fetch"""
    parts = [CO.sweep(g, model[0], model[1], model[2], model[3], Kg, int(s), jc=jc) for s in seeds]
    out = {k: np.concatenate([p[k] for p in parts], axis=1) for k in ARRAYS}
    out['logZ'] = np.array([p['logZ'] for p in parts])
    return out, parts


@pytest.mark.parametrize("N,S,G,Kg,lanes", SHAPES)
def test_shapes_against_the_oracle_and_the_switch(monkeypatch, N, S, G, Kg, lanes):
    g, model = MC.coded_alignment(300 + N, N, S), MC.random_model(400 + N, N)
    seeds = [1000 * N + i for i in range(G)]
    plan = _ffi.debug_sweep_plan(N, G * Kg, S, G=G)
    assert plan['book_width'] == lanes and plan['mat_after_book'] and plan['use_rec']
    ref, _ = oracle(g, model, Kg, seeds)
    outs = {sw: run(monkeypatch, sw, g, model, G * Kg, seeds) for sw in SWITCH}
    for sw, out in outs.items():
        same(out, ref, "N=%d G=%d Kg=%d switch %s against the oracle" % (N, G, Kg, sw))
        assert out['stats']['n_launches'] == sum(plan['launches'])             # the count stays that of the stages
    assert (ref['ancestors'] != np.arange(G * Kg) % Kg).any()


def test_one_group_above_8192_particles(monkeypatch):
    """K > 8192 in one group: scanned by several workgroups under the default PHYLO_SCAN_MULTI_MIN (today's launches), by
    pp_resample_scan<1024> when the switch leaves it to one workgroup (the chain form, sixteen waves in the scan's tail)"""
    N, S, K = 5, 64, 8256
    g, model = MC.coded_alignment(31, N, S), MC.random_model(32, N)
    ref, _ = oracle(g, model, K, [77])
    same(run(monkeypatch, '1', g, model, K, [77], expect=False), ref, "one group, scan of several workgroups")
    for sw in SWITCH:
        out = run(monkeypatch, sw, g, model, K, [77], env=(('PHYLO_SCAN_MULTI_MIN', '16384'),))
        same(out, ref, "one group, one workgroup's scan, switch " + sw)


def test_many_adopted_nodes_all_gap_leaves(monkeypatch):
    """All-gap leaves under JC69: every weight of a rank event is equal, about 63 % of a group's particles are adopted, the list is
    many times the item waves of a group and the waves stride.  The node rows of every rank event through phylo_sweep_node equal
    the EAGER_NODES sweep's (adopted nodes: written by the item waves; the others: by phylo_sweep_node from their children)."""
    N, S, G, Kg = 6, 70, 2, 2048
    g = np.ones((N, S, 4))
    model = (O.jc_Q(), np.full((1, 4), 0.25), np.full(N - 1, 10.0), np.full(N - 1, 10.0))
    seeds = [5, 6]
    ref, _ = oracle(g, model, Kg, seeds, jc=True)
    adopted = [np.unique(ref['ancestors'][r, :Kg]) for r in range(N - 2)]
    assert 0.55 * Kg < len(adopted[0]) < 0.72 * Kg and all(len(a) > 100 for a in adopted)     # (equal weights at the first resampling)
    picks = []                                             # per rank event: adopted and not adopted particles of both groups
    for r in range(N - 1):
        ks = np.arange(0, G * Kg, 97) if r == N - 2 else np.concatenate([adopted[r][:24], np.setdiff1d(np.arange(Kg), adopted[r])[:8],
                                                                         Kg + np.arange(0, Kg, 131)])
        picks.append(ks)
    rows = {}
    for sw, flags in (('1', _ffi.FLAGS_DEFAULT), ('0', _ffi.FLAGS_DEFAULT | _ffi.EAGER_NODES)):
        monkeypatch.setenv('PHYLO_SCAN_ANCESTORS', sw)
        with _ffi.Context(G * Kg, N, S) as ctx:
            ctx.set_leaves(g)
            ctx.set_model(*model, jc69_closed_form=True)
            out = sweep(ctx, seeds, flags)
            assert ctx.debug_sweep_chain() == SWITCH[sw]
            same(out, ref, "all-gap, switch " + sw)
            rows[sw] = [np.stack([ctx.sweep_node(r, int(k)) for k in picks[r]]) for r in range(N - 1)]
    for r in range(N - 1):
        assert np.array_equal(bits(rows['1'][r]), bits(rows['0'][r])), "node rows of rank event %d" % r


def test_heavy_particle(monkeypatch):
    """Long rows make the weights of a rank event spread widely: nearly all of a group adopts one ancestor (a list of a few entries,
    hundreds of adopters storing the same flag)"""
    N, S, G, Kg = 6, 1500, 3, 256
    g, model = MC.coded_alignment(51, N, S), MC.random_model(52, N)
    seeds = [11, 12, 13]
    ref, parts = oracle(g, model, Kg, seeds)
    assert min(len(np.unique(p['ancestors'][r])) for p in parts for r in range(N - 2)) <= 4
    for sw in SWITCH:
        same(run(monkeypatch, sw, g, model, G * Kg, seeds), ref, "heavy particle, switch " + sw)


def test_one_context_swept_again_and_with_another_batch(monkeypatch, sw='1'):
    """the ancestors, lists and counts live with the context: a second sweep, then fewer and larger groups, then more and smaller
    ones must not see what the sweep before left (stale counts of groups no longer there, list tails)"""
    N, S, K = 7, 90, 768
    g, model = MC.coded_alignment(61, N, S), MC.random_model(62, N)
    monkeypatch.setenv('PHYLO_SCAN_ANCESTORS', sw)
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(*model)
        for G, s0 in ((6, 100), (6, 200), (3, 300), (12, 400), (6, 100)):
            seeds = [s0 + i for i in range(G)]
            out = sweep(ctx, seeds)
            assert ctx.debug_sweep_chain() == SWITCH[sw]
            same(out, oracle(g, model, K // G, seeds)[0], "G=%d seeds from %d, switch %s" % (G, s0, sw))


def test_kept_graph_gradients(monkeypatch):
    """a kept graph of one site tile stays lazy and takes the chain form: the reverse pass reads the adopted nodes and the marks the
    item waves left.  Gradient bits equal the switch-off run's."""
    N, S, G, Kg = 8, 100, 4, 128
    g, model = MC.coded_alignment(71, N, S), MC.random_model(72, N)
    seeds = [21, 22, 23, 24]
    flags = _ffi.FLAGS_DEFAULT | _ffi.KEEP_GRAPH
    assert _ffi.debug_sweep_chain(N, G * Kg, S, G=G, flags=_ffi.KEEP_GRAPH)['taken']
    grads = {}
    for sw in SWITCH:
        monkeypatch.setenv('PHYLO_SCAN_ANCESTORS', sw)
        with _ffi.Context(G * Kg, N, S) as ctx:
            ctx.set_leaves(g)
            ctx.set_model(*model)
            out = sweep(ctx, seeds, flags)
            assert ctx.debug_sweep_chain() == SWITCH[sw]
            grads[sw] = (out, ctx.sweep_backward_batch(G))
    same(grads['1'][0], grads['0'][0], "kept graph")
    for key in ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q'):
        assert np.array_equal(bits(grads['1'][1][key]), bits(grads['0'][1][key])), "kept graph: %s" % key
