"""The forward sweep's large-launch forms, bit for bit against the C oracle: the sorted prologue (pk_sweep_prologue_sorted), log Z
summed by a launch of its own (pk_logz_total, pk_logz_total_groups), the scan of a group by several workgroups with G > 1
(pp_scan_multi_*), grouped adopted nodes with G > 1 (pk_materialize_adopted_grouped), and 8 lanes per particle with a group
boundary inside a wave (pk_rank_book_packed<8>) -- the forms on the far side of the size thresholds of phylo_sweep_plan.h, which
the batched training step and every sweep of more than 16384 particles take.  tests/large_launch_cases.py says what each case is
the smallest shape for; tests/test_large_launch_cpu.py pins the plan bits the cases claim and that the oracle's sweeps are a
usable reference.  No tolerances: the contract is bit equality."""
import numpy as np
import pytest

import large_launch_cases as LC
from oracle import c_oracle as CO
from phylo_amd import _ffi

pytestmark = pytest.mark.gpu
EAGER = _ffi.FLAGS_DEFAULT | _ffi.EAGER_NODES
FLOATS = ('log_weights', 'log_likelihood', 'left_branches', 'right_branches')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def make_ctx(name):
    c = LC.CASES[name]
    g, Q, pi, lam_l, lam_r, jc, _ = LC.model(name)
    ctx = _ffi.Context(c["G"] * c["Kg"], c["N"], c["S"])
    ctx.set_leaves(g)
    ctx.set_model(Q, pi, lam_l, lam_r, jc69_closed_form=jc)
    return ctx


def run(ctx, name, flags=_ffi.FLAGS_DEFAULT):
    """(arrays, log Z-hat of every group) of the case's sweep"""
    G = LC.CASES[name]["G"]
    seeds = LC.model(name)[6]
    if G == 1:
        out = ctx.sweep(seeds[0], flags=flags)
        return out, np.array([out['logZ']])
    ctx.sweep_batch_async(seeds, flags=flags)
    out = ctx.sweep_fetch()
    return out, ctx.sweep_fetch_logz(G)


def first_difference(got, want):
    bad = np.argwhere(bits(got) != bits(want))
    return "%d of %d differ, first at %s: %r against %r" % (len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def same_as_oracle(out, logz, name, what):
    c = LC.CASES[name]
    Kg = c["Kg"]
    for i, ref in enumerate(LC.reference(name)):
        sl = slice(i * Kg, (i + 1) * Kg)
        tag = "%s %s group %d" % (name, what, i)
        np.testing.assert_array_equal(out['ancestors'][:, sl], ref['ancestors'], err_msg=tag)
        np.testing.assert_array_equal(out['merges'][:, sl], ref['merges'], err_msg=tag)
        for key in FLOATS:
            got = out[key][:, sl]
            assert np.array_equal(bits(got), bits(ref[key])), "%s: %s: %s" % (tag, key, first_difference(got, ref[key]))
        assert bits(logz[i]) == bits(ref['logZ']), "%s: log Z %r against %r" % (tag, logz[i], ref['logZ'])
    assert bits(out['logZ']) == bits(logz[0]), "%s %s: the fetched log Z is not group 0's" % (name, what)


def launches(name, flags=0):
    c = LC.CASES[name]
    return sum(_ffi.debug_sweep_plan(c["N"], c["G"] * c["Kg"], c["S"], G=c["G"], flags=flags,
                                     switches=('jc',) if c["jc"] else ())['launches'])


@pytest.mark.parametrize("name", LC.NAMES)
def test_large_launch_against_the_oracle(name):
    c = LC.CASES[name]
    N, K = c["N"], c["G"] * c["Kg"]
    with make_ctx(name) as ctx:
        out, logz = run(ctx, name)
        assert out['stats']['n_launches'] == launches(name)
        same_as_oracle(out, logz, name, "lazy")
        # the node the sweep did not store: nobody adopts a node of the last rank event, phylo_sweep_node has to write it
        node = ctx.sweep_node(N - 2, K - 1)
        want = LC.reference(name)[-1]['nodes'][N - 2, c["Kg"] - 1]
        assert np.array_equal(bits(node), bits(want)), "%s: node (%d, %d)" % (name, N - 2, K - 1)
        if c["eager"]:
            out, logz = run(ctx, name, EAGER)
            assert out['stats']['n_launches'] == launches(name, _ffi.EAGER_NODES)
            same_as_oracle(out, logz, name, "eager")
            assert np.array_equal(bits(ctx.sweep_node(N - 2, K - 1)), bits(want)), "%s: eager node" % name


def test_buffers_are_reused_across_group_counts():
    """The batch (G = 2, nine scan tiles per group, rows of R + 1 log-normalisers), one plain sweep of all K particles (G = 1,
    seventeen tiles, one row), the batch again on ONE context: the scan's scratch and the rows are the same allocations."""
    name = "sorted-ragged"
    c = LC.CASES[name]
    g, Q, pi, lam_l, lam_r, jc, _ = LC.model(name)
    K = c["G"] * c["Kg"]
    with make_ctx(name) as ctx:
        first, logz1 = run(ctx, name)
        same_as_oracle(first, logz1, name, "first batch")
        one = ctx.sweep(LC.SEED0)
        ref = CO.sweep(g, Q, pi, lam_l, lam_r, K, LC.SEED0, jc=jc)
        np.testing.assert_array_equal(one['ancestors'], ref['ancestors'])
        np.testing.assert_array_equal(one['merges'], ref['merges'])
        for key in FLOATS:
            assert np.array_equal(bits(one[key]), bits(ref[key])), "one sweep of %d: %s: %s" % (K, key, first_difference(one[key], ref[key]))
        assert bits(one['logZ']) == bits(ref['logZ'])
        again, logz2 = run(ctx, name)
    for key in FLOATS:
        assert np.array_equal(bits(again[key]), bits(first[key])), "second batch: %s: %s" % (key, first_difference(again[key], first[key]))
    np.testing.assert_array_equal(again['ancestors'], first['ancestors'])
    np.testing.assert_array_equal(again['merges'], first['merges'])
    assert np.array_equal(bits(logz2), bits(logz1)) and bits(again['logZ']) == bits(first['logZ'])
