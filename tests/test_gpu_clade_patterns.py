"""pk_rank_merge_nostore with the clade tables of its site-pattern form (phylo_amd/csrc/phylo_site_patterns.h: phase 1 computes one
site likelihood per distinct column of the MERGED CLADE, found from the leaf bitset the bookkeeping carries through the root
tables into the merge record).  Every case compares every fetched array and log Z-hat as bytes between two fresh contexts, one with
the form and one with PHYLO_CLADE_PATTERNS=0, and against the C oracle's sweep (ancestors, merges, the four float arrays, log
Z-hat), and asserts through the debug entry which form ran.  One rank, plain proposal, lazy nodes (use_rec).  No tolerances."""
import numpy as np
import pytest

import clade_patterns_cases as CP
import packed_codes_cases as PC
import site_patterns_cases as SP
from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset
from test_gpu_packed_codes import PI, gtr, lam, same, uses_record
from tests import site_product_cases as SC

pytestmark = pytest.mark.gpu


def same_bytes(a, b, what):
    assert sorted(a) == sorted(b), what
    for key in a:
        if key == 'stats':
            continue
        x, y = np.atleast_1d(np.ascontiguousarray(a[key])), np.atleast_1d(np.ascontiguousarray(b[key]))
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), "%s: %s" % (what, key)


def sweep(g, K, seed, taken, Q, rates, jc=False, eligible=None):
    """One sweep on a fresh context under the current environment; asserts the tables' state and whether the sweep's plan took them."""
    N, S, _ = g.shape
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, rates, rates, jc69_closed_form=jc)
        el, _, nbytes = ctx.debug_clade_patterns()
        assert el == (taken if eligible is None else eligible) and (nbytes > 0) == el
        out = ctx.sweep(seed)
        assert ctx.debug_clade_patterns()[1] == taken
    return out


def check(g, K, seed, what, monkeypatch, taken=True, Q=None, rates=None, jc=False):
    N, S, _ = g.shape
    assert uses_record(N, K, S), what
    Q = gtr() if Q is None else Q
    rates = lam(N) if rates is None else rates
    monkeypatch.delenv("PHYLO_CLADE_PATTERNS", raising=False)
    on = sweep(g, K, seed, taken, Q, rates, jc)
    monkeypatch.setenv("PHYLO_CLADE_PATTERNS", "0")
    off = sweep(g, K, seed, False, Q, rates, jc)
    monkeypatch.delenv("PHYLO_CLADE_PATTERNS")
    same_bytes(on, off, what)
    ref = CO.sweep(g, Q, PI, rates, rates, K, seed, jc=jc)
    same(on, on['logZ'], ref, what)
    return on


def primate():
    g = load_dataset('primate_data')['genome']
    assert g.shape[:2] == (12, 898)
    return g


def test_primate_single_sweep(monkeypatch):
    """The flagship's alignment as one sweep: bookkeeping and adopted nodes in one launch (pk_rank_book_mat), clades of 3 to 12 leaves."""
    assert _ffi.debug_sweep_plan(12, 128, 898, flags=_ffi.FLAGS_DEFAULT)['book_mat']
    check(primate(), 128, 4, "primate.p", monkeypatch)


def test_primate_batch_of_three(monkeypatch):
    """G = 3 groups of 64 in one launch set (the chain form of a rank event): on against off as bytes, every group against the oracle."""
    g, G, Kg, seeds = primate(), 3, 64, [31, 8, 5]
    N, S, _ = g.shape
    assert uses_record(N, G * Kg, S, G=G)
    assert _ffi.debug_sweep_chain(N, G * Kg, S, G=G, flags=_ffi.FLAGS_DEFAULT)['taken']
    Q = gtr()
    res = {}
    for sw in (None, "0"):
        if sw is None:
            monkeypatch.delenv("PHYLO_CLADE_PATTERNS", raising=False)
        else:
            monkeypatch.setenv("PHYLO_CLADE_PATTERNS", sw)
        with _ffi.Context(G * Kg, N, S) as ctx:
            ctx.set_leaves(g)
            ctx.set_model(Q, PI, lam(N), lam(N))
            ctx.sweep_batch_async(seeds)
            out = ctx.sweep_fetch()
            logz = ctx.sweep_fetch_logz(G)
            assert ctx.debug_clade_patterns()[:2] == (sw is None, sw is None)
        res[sw] = (out, logz)
    monkeypatch.delenv("PHYLO_CLADE_PATTERNS")
    same_bytes(res[None][0], res["0"][0], "batch")
    assert np.array_equal(np.asarray(res[None][1]).view(np.uint8), np.asarray(res["0"][1]).view(np.uint8))
    for i, sd in enumerate(seeds):
        ref = CO.sweep(g, Q, PI, lam(N), lam(N), Kg, sd)
        same(res[None][0], res[None][1][i], ref, "group %d" % i, slice(i * Kg, (i + 1) * Kg))


def test_quadruples_full_steps(monkeypatch):
    """4 taxa, all 256 quadruples of A/C/G/T and repeats: U_Z is exactly 64 for every triple and 256 for the whole clade -- full
    phase-1 steps, the pad entry behind a full step.  (The pattern form is forced: five walk steps are too few for the rule.)"""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    check(PC.genome(CP.quadruples()), 128, 6, "quadruples", monkeypatch)


def test_five_taxa_with_gaps(monkeypatch):
    """5 taxa, S = 130, gaps: classes of one to three steps, an odd last walk step."""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    codes = CP.gapped()
    sizes = {CP.classes(codes, Z)[1].size for Z in range(32) if bin(Z).count("1") >= 3}
    assert {-(-u // 64) for u in sizes} == {1, 2, 3}
    check(PC.genome(codes), 256, 2, "gapped", monkeypatch)


def test_three_taxa(monkeypatch):
    """The only merge that is not leaf x leaf builds the whole alignment."""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    check(PC.genome(SP.pool_codes(3, 200, 90, seed=5)), 64, 9, "three taxa", monkeypatch)


def test_redo_with_the_form_on(monkeypatch):
    """test_gpu_site_patterns.test_redo_from_phase_one's inputs (a table entry outside the positive normals: rates of 1e155 under the
    JC69 closed form give site likelihoods of exactly 0): phase 1 over the clade's block raises the flag and the wave recomputes in
    pk_rows_general."""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    N, S, K = 6, 200, 64
    g = SC.coded_leaves(N, S, seed=2)
    rates = np.full(N - 1, 1e155)
    ref = CO.sweep(g, O.jc_Q(), PI, rates, rates, K, 3, jc=True)
    assert np.isneginf(ref['log_likelihood'][1:]).any()
    check(g, K, 3, "zero table entries", monkeypatch, Q=O.jc_Q(), rates=rates, jc=True)


def test_off_above_the_caps(monkeypatch):
    """13 taxa (one above the bitset's cap) and an alignment of more than 512 distinct columns: no tables, the plan says so, and the
    sweeps are the oracle's."""
    g13 = PC.genome(SP.pool_codes(CP.MAX_TAXA + 1, 898, 300, seed=13))
    assert _ffi.debug_sweep_plan(13, 64, 898, flags=_ffi.FLAGS_DEFAULT)['use_rec']
    check(g13, 64, 5, "13 taxa", monkeypatch, taken=False)
    monkeypatch.setenv("PHYLO_CLADE_PATTERNS", "force")
    out = sweep(g13, 64, 5, False, gtr(), lam(13))
    same(out, out['logZ'], CO.sweep(g13, gtr(), PI, lam(13), lam(13), 64, 5), "13 taxa, forced")
    monkeypatch.delenv("PHYLO_CLADE_PATTERNS")
    check(PC.genome(SP.pool_codes(5, 898, 513, seed=513)), 64, 5, "U = 513", monkeypatch, taken=False)


def test_tables_follow_the_leaves(monkeypatch):
    """One context: leaves A, leaves B (another U: other tables), A again -- every sweep equals a fresh context's as bytes."""
    monkeypatch.delenv("PHYLO_CLADE_PATTERNS", raising=False)
    N, S, K = 5, 898, 64
    A = PC.genome(SP.pool_codes(N, S, 100, seed=1))
    B = PC.genome(SP.pool_codes(N, S, 300, seed=2))
    Q = gtr()
    fresh = {id(g): sweep(g, K, 12, True, Q, lam(N)) for g in (A, B)}
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_model(Q, PI, lam(N), lam(N))
        for g, what in ((A, "leaves A"), (B, "leaves B"), (A, "leaves A again")):
            ctx.set_leaves(g)
            assert ctx.debug_clade_patterns()[0], what
            out = ctx.sweep(12)
            assert ctx.debug_clade_patterns()[1], what
            same_bytes(out, fresh[id(g)], what)
    same(fresh[id(A)], fresh[id(A)]['logZ'], CO.sweep(A, Q, PI, lam(N), lam(N), K, 12), "leaves A")
