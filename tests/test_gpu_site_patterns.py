"""pk_rank_merge_nostore in its site-pattern form (phylo_amd/csrc/phylo_site_patterns.h: a merge with an uncoded child computes one
site likelihood per DISTINCT column of the alignment into a table in LDS and takes the product over all sites by looking the factors
up), bit for bit against the C oracle's sweep -- ancestors, merges, the four float arrays as uint64, log Z-hat -- at the edges of the
table, of the walk and of the tables' lifetime.  Every case is one rank, plain proposal, lazy nodes (use_rec), and asserts through
the debug entry that the form it means to test was taken.  No tolerances."""
import numpy as np
import pytest

import packed_codes_cases as PC
import site_patterns_cases as SP
from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset
from test_gpu_packed_codes import FLOATS, PI, bits, gtr, lam, same, uses_record
from tests import site_product_cases as SC

pytestmark = pytest.mark.gpu
N0, K0 = 5, 64


def check(g, K, seed, what, U, taken, Q=None, rates=None, jc=False):
    """test_gpu_packed_codes.check -- one sweep of alignment g on a fresh context against the oracle's -- and the context's facts: U
    distinct columns, the form taken or not.  Returns the sweep's outputs."""
    N, S, _ = g.shape
    assert uses_record(N, K, S), what
    Q = gtr() if Q is None else Q
    rates = lam(N) if rates is None else rates
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, rates, rates, jc69_closed_form=jc)
        assert ctx.debug_site_patterns() == (U, taken), what
        ref = CO.sweep(g, Q, PI, rates, rates, K, seed, jc=jc)
        out = ctx.sweep(seed)
        same(out, out['logZ'], ref, what)
    return out


@pytest.mark.parametrize("U", [1, 63, 64, 65, 512])
def test_table_edges(U, monkeypatch):
    """One entry; a step with one lane idle, a full step, a second step of one lane; the cap (eight full steps, the pad entry the
    table's last).  S = 898: fifteen steps of the walk, the last with two lanes."""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    check(PC.genome(SP.pool_codes(N0, 898, U, seed=U)), K0, 5, "U=%d" % U, U, True)


def test_one_column_over_the_cap_is_off(monkeypatch):
    g = PC.genome(SP.pool_codes(N0, 898, 513, seed=513))
    check(g, K0, 5, "U=513", 513, False)
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    check(g, K0, 5, "U=513 forced", 513, False)


def test_forced_where_every_column_is_distinct(monkeypatch):
    """U = S = 64: the rule would not take it (nothing to gain), force does; one step in both phases."""
    g = PC.genome(SP.pool_codes(N0, 64, 64, seed=64))
    check(g, K0, 5, "U=S=64", 64, False)
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    check(g, K0, 5, "U=S=64 forced", 64, True)


@pytest.mark.parametrize("S", [1, 2, 65, 127, 512, 513, 1024, 1025, 2048])
def test_walk_edges(S, monkeypatch):
    """A pool of S / 2 distinct columns (at most the cap): one lane, two; a second step of one lane, an odd last step; eight steps
    -- one half of the image's chunk -- and a ninth of one lane; a whole chunk, a second chunk of one lane, the full tile."""
    U = min(max(S // 2, 1), SP.CAP)
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    check(PC.genome(SP.pool_codes(N0, S, U, seed=S)), K0, 6, "S=%d" % S, U, True)


def test_two_tiles_are_off(monkeypatch):
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    check(PC.genome(SP.pool_codes(N0, 2049, 300, seed=2049)), K0, 6, "S=2049", 300, False)


def test_primate_by_the_rule_and_switched_off(monkeypatch):
    """primate.p, 12 x 898, U = 413: the flagship's row (seven phase-1 steps, the last with 29 lanes; fifteen steps of the walk, the
    last with two), taken by the rule with nothing set; the same sweep with PHYLO_SITE_PATTERNS=0 gives the same bytes."""
    g = load_dataset('primate_data')['genome']
    assert g.shape[:2] == (12, 898)
    on = check(g, 128, 4, "primate.p", 413, True)
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "0")
    off = check(g, 128, 4, "primate.p, switched off", 413, False)
    for key in FLOATS + ('ancestors', 'merges'):
        assert np.array_equal(np.ascontiguousarray(on[key]).view(np.uint8), np.ascontiguousarray(off[key]).view(np.uint8)), key
    assert bits(on['logZ']) == bits(off['logZ'])


def test_batched_groups(monkeypatch):
    """G = 3 groups of 64 in one launch set: every group against the oracle's sweep of its own seed."""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    N, S, G, Kg, U = N0, 129, 3, K0, 40
    assert uses_record(N, G * Kg, S, G=G)
    g = PC.genome(SP.pool_codes(N, S, U, seed=77))
    Q = gtr()
    seeds = [31, 8, 5]
    with _ffi.Context(G * Kg, N, S) as ctx:
        ctx.set_leaves(g)
        ctx.set_model(Q, PI, lam(N), lam(N))
        assert ctx.debug_site_patterns() == (U, True)
        ctx.sweep_batch_async(seeds)
        out = ctx.sweep_fetch()
        logz = ctx.sweep_fetch_logz(G)
    for i, sd in enumerate(seeds):
        ref = CO.sweep(g, Q, PI, lam(N), lam(N), Kg, sd)
        same(out, logz[i], ref, "group %d" % i, slice(i * Kg, (i + 1) * Kg))


def test_new_leaves_replace_the_tables():
    """Training on site minibatches: one context, by the rule alone -- leaves A (U = 100, taken), B (another U, taken), C (U over the
    cap: off), D (a row without a code: off, no tables), then A again.  Every sweep equals the oracle's for its leaves."""
    N, S, K = N0, 898, K0
    assert uses_record(N, K, S)
    A = PC.genome(SP.pool_codes(N, S, 100, seed=1))
    B = PC.genome(SP.pool_codes(N, S, 300, seed=2))
    Cc = PC.genome(SP.pool_codes(N, S, 600, seed=3))
    D = A.copy()
    D[3, 70] = [0.5, 0.5, 0.0, 0.0]
    Q = gtr()
    with _ffi.Context(K, N, S) as ctx:
        ctx.set_model(Q, PI, lam(N), lam(N))
        for g, what, facts in ((A, "leaves A", (100, True)), (B, "leaves B", (300, True)), (Cc, "leaves C", (600, False)),
                               (D, "leaves D", (0, False)), (A, "leaves A again", (100, True))):
            ctx.set_leaves(g)
            assert ctx.debug_site_patterns() == facts, what
            out = ctx.sweep(12)
            same(out, out['logZ'], CO.sweep(g, Q, PI, lam(N), lam(N), K, 12), what)


def test_all_gaps_many_adopted_internal_children():
    """The all-gap alignment (U = 1) at N = 8, K = 256: near-uniform weights, children spread over all earlier nodes -- merges of two
    internal children and adopted nodes in plenty -- every factor read from the table's one entry."""
    N, S, K = 8, 898, 256
    g = PC.genome(np.full((N, S), 4, dtype=np.uint8))
    check(g, K, 9, "all gaps", 1, True)


def test_redo_from_phase_one(monkeypatch):
    """A table entry outside the positive normal range (the inputs of test_gpu_site_product_edges' coded leaves at rates of 1e155
    under the JC69 closed form: the off-diagonal transition probabilities are exactly 0, so a leaf x internal site likelihood is 0
    wherever the codes disagree): phase 1 raises the flag and the wave recomputes in pk_rows_general.  Against the oracle alone,
    exactly."""
    monkeypatch.setenv("PHYLO_SITE_PATTERNS", "force")
    N, S, K = 6, 200, 64
    g = SC.coded_leaves(N, S, seed=2)
    codes = g.argmax(axis=2).astype(np.uint8)
    U = len({codes[:, s].tobytes() for s in range(S)})
    rates = np.full(N - 1, 1e155)
    ref = CO.sweep(g, O.jc_Q(), PI, rates, rates, K, 3, jc=True)
    assert np.isneginf(ref['log_likelihood'][1:]).any()    # a zero factor in a merge behind rank event 0: an uncoded child
    check(g, K, 3, "zero table entries", U, True, Q=O.jc_Q(), rates=rates, jc=True)
