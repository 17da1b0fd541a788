"""How pk_rank_merge_nostore and the chain bookkeeping are launched (phylo_amd/csrc/phylo_launch_map.h; the plan's launch_xcd and
book_xcd): workgroup indices remapped so that an XCD owns a contiguous range of particles, on a grid rounded up to a multiple of 8
whose surplus waves leave at once.  It may not change a byte: every case runs under every W that ships (one wave per workgroup: two
and four measured no gain and left) x PHYLO_LAUNCH_XCD 0 / 1 on a fresh context and compares every fetched array and log Z-hat
as bytes against a context without the remap, and that one against the C oracle's sweep; the launch count stays.  The shapes are
the smallest at which a mapping can go wrong: particle counts below, at and off multiples of 8 (a rounded grid, surplus waves), one
to three steps of sites, three site tiles, the clade form at 12 taxa, batched groups.  No tolerances."""
import functools

import numpy as np
import pytest

import packed_codes_cases as PC
import site_patterns_cases as SP
from oracle import c_oracle as CO
from phylo_amd import _ffi
from test_gpu_clade_patterns import same_bytes
from test_gpu_packed_codes import PI, gtr, lam, same, uses_record

pytestmark = pytest.mark.gpu

WS = (1,)                                                  # waves per workgroup of the merge that the library ships
KS = (1, 7, 8, 9, 31, 33, 65, 100)
SHAPES = {"5x37": (5, 37, 20), "5x130": (5, 130, 90), "12x200": (12, 200, 120)}     # N, S, distinct columns


@functools.lru_cache(maxsize=None)
def alignment(name):
    N, S, U = SHAPES[name]
    g = PC.genome(SP.pool_codes(N, S, U, seed=N + S))
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def oracle(name, K, seed, tile=0):
    g = alignment(name)
    N = g.shape[0]
    if tile:
        CO.set_site_tile(tile)
    try:
        return CO.sweep(g, gtr(), PI, lam(N), lam(N), K, seed)
    finally:
        if tile:
            CO.set_site_tile(0)


def launch_env(monkeypatch, W, xcd):
    assert W == 1
    monkeypatch.setenv("PHYLO_LAUNCH_XCD", "1" if xcd else "0")


def one_sweep(g, K, seed, W, xcd, tile=0):
    """A fresh context under the current environment (the switches are read at creation); asserts what the plan launched"""
    N, S, _ = g.shape
    ctx = _ffi.Context(K, N, S)
    try:
        ctx.set_leaves(g)
        ctx.set_model(gtr(), PI, lam(N), lam(N))
        if tile:
            ctx.set_site_tile(tile)
        out = ctx.sweep(seed)
        assert ctx.debug_sweep_launch() == {"launch_xcd": xcd, "book_xcd": xcd}
        pat = ctx.debug_clade_patterns()[1]
    finally:
        ctx.close()
    return out, pat


def every_launch(monkeypatch, name, K, seed, tile=0, clade=None):
    g = alignment(name)
    N, S, _ = g.shape
    assert uses_record(N, K, S)
    launch_env(monkeypatch, 1, False)
    base, pat = one_sweep(g, K, seed, 1, False, tile)
    if clade is not None:
        assert pat == clade
    same(base, base['logZ'], oracle(name, K, seed, tile), "%s K=%d W=1" % (name, K))
    for W in WS:
        for xcd in (False, True):
            if W == 1 and not xcd:
                continue
            launch_env(monkeypatch, W, xcd)
            out, pat2 = one_sweep(g, K, seed, W, xcd, tile)
            what = "%s K=%d W=%d xcd=%d" % (name, K, W, xcd)
            assert pat2 == pat, what
            same_bytes(out, base, what)
            assert out['stats']['n_launches'] == base['stats']['n_launches'], what
            assert out['stats']['merge_launches'] == base['stats']['merge_launches'], what


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_pattern_and_clade_forms(monkeypatch, name, K):
    """The pattern form forced, so that every wave that is not leaf x leaf fills and walks the launch's LDS table; at 12 taxa and 5
    taxa alike the clade tables are taken (the bookkeeping carries the bitsets into the record)."""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    monkeypatch.delenv("PHYLO_CLADE_PATTERNS", raising=False)
    every_launch(monkeypatch, name, K, seed=3 + K, clade=True)


@pytest.mark.parametrize("K", (7, 33, 100))
@pytest.mark.parametrize("name", ("5x130", "12x200"))
def test_rows_forms(monkeypatch, name, K):
    """PHYLO_CLADE_PATTERNS=0 and the pattern form off: the row loops over packed codes, no dynamic LDS at all"""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "0")
    monkeypatch.setenv("PHYLO_CLADE_PATTERNS", "0")
    every_launch(monkeypatch, name, K, seed=11 + K, clade=False)


@pytest.mark.parametrize("K", (7, 9, 100))
def test_pattern_form_without_clade_tables(monkeypatch, K):
    """PHYLO_CLADE_PATTERNS=0 alone: phase 1 over the whole alignment's columns"""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    monkeypatch.setenv("PHYLO_CLADE_PATTERNS", "0")
    every_launch(monkeypatch, "5x130", K, seed=5 + K, clade=False)


@pytest.mark.parametrize("K", (1, 8, 33))
def test_three_site_tiles(monkeypatch, K):
    """A site tile of 64 on S = 130: an item is (particle, tile), 3 K items, tile values through pk_tile_epilogue"""
    monkeypatch.delenv("PHYLO_SITE_PATTERNS", raising=False)
    monkeypatch.delenv("PHYLO_CLADE_PATTERNS", raising=False)
    every_launch(monkeypatch, "5x130", K, seed=21 + K, tile=64)


@pytest.mark.parametrize("Kg", (7, 8, 32))
def test_batch_of_three_groups(monkeypatch, Kg):
    """G = 3 sweeps in one launch set (the chain form of a rank event: the bookkeeping's particle waves behind the item waves take
    the remap too): 21, 24 and 96 particles -- off every multiple of 8, the first multiple above, a larger one"""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    monkeypatch.delenv("PHYLO_CLADE_PATTERNS", raising=False)
    name, G, seeds = "12x200", 3, [31, 8, 5]
    g = alignment(name)
    N, S, _ = g.shape
    assert uses_record(N, G * Kg, S, G=G)
    res = {}
    for W in WS:
        for xcd in (False, True):
            launch_env(monkeypatch, W, xcd)
            ctx = _ffi.Context(G * Kg, N, S)
            try:
                ctx.set_leaves(g)
                ctx.set_model(gtr(), PI, lam(N), lam(N))
                ctx.sweep_batch_async(seeds)
                out = ctx.sweep_fetch()
                logz = ctx.sweep_fetch_logz(G)
                assert ctx.debug_sweep_launch() == {"launch_xcd": xcd, "book_xcd": xcd}
                chain = ctx.debug_sweep_chain()
            finally:
                ctx.close()
            res[W, xcd] = (out, logz, chain)
    base, logz0, chain0 = res[1, False]
    assert chain0 == _ffi.debug_sweep_chain(N, G * Kg, S, G=G, flags=_ffi.FLAGS_DEFAULT)['taken']
    for i, sd in enumerate(seeds):
        same(base, logz0[i], oracle(name, Kg, sd), "group %d" % i, slice(i * Kg, (i + 1) * Kg))
    for key, (out, logz, chain) in res.items():
        what = "batch Kg=%d W=%d xcd=%d" % ((Kg,) + key)
        same_bytes(out, base, what)
        assert np.array_equal(np.asarray(logz).view(np.uint8), np.asarray(logz0).view(np.uint8)), what
        assert chain == chain0 and out['stats']['n_launches'] == base['stats']['n_launches'], what
