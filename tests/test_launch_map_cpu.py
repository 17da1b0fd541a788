"""Which wave takes which item (phylo_amd/csrc/phylo_launch_map.h), through phylo_debug_launch_map, which runs the two functions the
driver and the kernels run: pk_launch_grid and pk_launch_item.  A launch of n items = (particle, tile) pairs at W waves per
workgroup; with the remap the 8 XCDs, to which workgroups are dealt round-robin, each own a contiguous range of items."""
import numpy as np
import pytest

from phylo_amd import _ffi


def lib_or_skip():
    try:
        return _ffi.load()
    except OSError as e:
        pytest.skip(str(e))


def check(n, W, xcd):
    grid, items = _ffi.debug_launch_map(n, W, xcd)
    assert items.shape == (grid, W)
    need = -(-n // W)
    if xcd:
        assert grid % 8 == 0 and need <= grid < need + 8, (n, W, grid)
    else:
        assert grid == need, (n, W, grid)
    flat = items.ravel()
    live = flat[flat < n]
    # every item exactly once, every other wave beyond the end (and no negative item)
    assert live.size == n and np.array_equal(np.sort(live), np.arange(n)), (n, W, xcd)
    assert (flat >= 0).all() and (flat[flat >= n] >= n).all()
    # the waves of a workgroup take consecutive items
    assert (np.diff(items, axis=1) == 1).all()
    if xcd:
        # XCD x gets workgroups x, x + 8, ...: their slots are the contiguous range [x grid/8, (x + 1) grid/8), in order
        per = grid // 8
        for x in range(8):
            slots = items[x::8, 0] // W
            assert np.array_equal(slots, np.arange(x * per, (x + 1) * per)), (n, W, x)
    else:
        assert np.array_equal(items[:, 0], np.arange(grid) * W)
    return grid, items


@pytest.mark.parametrize("W", [1, 2, 4])
@pytest.mark.parametrize("xcd", [False, True])
def test_every_item_once(W, xcd):
    lib_or_skip()
    for ntiles in (1, 3):
        for K in list(range(1, 301)) + [40960]:
            n = K * ntiles
            grid, items = check(n, W, xcd)
            if ntiles == 3 and K in (7, 100):
                # an item is (particle, tile) exactly as without the map: k = item / ntiles
                live = np.sort(items.ravel()[items.ravel() < n])
                assert np.array_equal(live // ntiles, np.repeat(np.arange(K), ntiles))


def test_particles_of_a_sweep_share_an_xcd():
    """The flagship's launch: 20 sweeps of 2 048 particles.  With the remap a sweep's particles lie on at most two XCDs (5 120 per
    XCD), dealt round-robin they lie on all eight."""
    lib_or_skip()
    G, Kg = 20, 2048
    for W in (1, 2, 4):
        grid, items = _ffi.debug_launch_map(G * Kg, W, True)
        xcd_of = np.empty(G * Kg, dtype=np.int64)
        for x in range(8):
            it = items[x::8].ravel()
            xcd_of[it[it < G * Kg]] = x
        assert max(len(set(xcd_of[g * Kg:(g + 1) * Kg])) for g in range(G)) <= 2
        grid0, items0 = _ffi.debug_launch_map(G * Kg, W, False)
        x0 = np.empty(G * Kg, dtype=np.int64)
        for x in range(8):
            x0[items0[x::8].ravel()] = x
        assert len(set(x0[:Kg])) == 8


def test_bad_arguments():
    lib_or_skip()
    for n, W in ((0, 1), (5, 3), (5, 0), (5, 8)):
        with pytest.raises(_ffi.PhyloError):
            _ffi.debug_launch_map(n, W, True)


def test_the_plan_decides():
    """launch_xcd / book_xcd come from the plan: only the record form (one rank, plain proposal, lazy nodes) takes them, the
    switch overrides inside it, and phylo_debug_sweep_plan's mask does not know them."""
    lib_or_skip()
    F = _ffi.FLAGS_DEFAULT
    assert _ffi.debug_sweep_plan(12, 40960, 898, G=20, flags=F)['use_rec']
    assert _ffi.debug_sweep_launch(12, 40960, 898, G=20, flags=F) == {'launch_xcd': True, 'book_xcd': True}      # the flagship
    assert _ffi.debug_sweep_launch(12, 40960, 898, G=20, flags=F, launch_xcd=2) == {'launch_xcd': True, 'book_xcd': False}
    assert _ffi.debug_sweep_launch(12, 40960, 898, G=20, flags=F, launch_xcd=3) == {'launch_xcd': False, 'book_xcd': True}
    # small launches (a single sweep: a latency chain) keep the plain deal unless the switch says otherwise
    assert _ffi.debug_sweep_launch(12, 2048, 898, flags=F) == {'launch_xcd': False, 'book_xcd': False}
    assert _ffi.debug_sweep_launch(12, 8192, 898, flags=F) == {'launch_xcd': False, 'book_xcd': False}
    assert _ffi.debug_sweep_launch(12, 8200, 898, flags=F) == {'launch_xcd': True, 'book_xcd': True}
    assert _ffi.debug_sweep_launch(12, 2048, 898, flags=F, launch_xcd=1) == {'launch_xcd': True, 'book_xcd': True}
    on = _ffi.debug_sweep_launch(12, 40960, 898, G=20, flags=F, launch_xcd=1)
    off = _ffi.debug_sweep_launch(12, 40960, 898, G=20, flags=F, launch_xcd=-1)
    assert on['launch_xcd'] and on['book_xcd'] and not off['launch_xcd'] and not off['book_xcd']
    # no record, no map: the twisted proposal, an eager sweep, a sharded one
    for kw in (dict(flags=F | _ffi.TWISTING), dict(flags=F | _ffi.EAGER_NODES), dict(world=2, K_local=64, transport=True, flags=F)):
        assert not _ffi.debug_sweep_plan(12, 128, 898, **kw)['use_rec']
        d = _ffi.debug_sweep_launch(12, 128, 898, launch_xcd=1, **kw)
        assert d == {'launch_xcd': False, 'book_xcd': False}, kw
