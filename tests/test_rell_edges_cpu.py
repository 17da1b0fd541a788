"""The RELL edge cases without a GPU (tests/rell_edges_cases.py; DESIGN.md sections 12 and 12b): every case of
tests/test_gpu_rell_edges.py is held to what it claims to be -- the tile, panel, chunk and slice arithmetic read off the kernels'
constants, the winners, ties and zeros in exact rationals, the draw vectors and the shared count words from the restatement
(tests/rell_ref.py, tests/rell_ms_ref.py) alone -- and the library's host loops (phylo_debug_rell_host,
phylo_debug_rell_multiscale_host), the device file's full-array reference, are held to the rational replay and to the restated
counts on each case's sample."""
import numpy as np
import pytest

import rell_edges_cases as EC
import rell_ms_ref
import rell_ref
from phylo_amd import _ffi
from rell_edges_cases import CASES, DRAWS, PR_KP, PR_TB, PR_TT, SEED
from test_rell_cpu import bits


def bit(v):
    return int(bits(v).reshape(-1)[0])


def tiles(n, w):
    return -(-n // w)


# ---- every case: the sample is what it claims, and the host loop is the rational replay on it ---------------------------------
@pytest.mark.parametrize("name", EC.NAMES)
def test_sample_and_host_loop_against_rationals(name):
    case = CASES[name]
    T, S = case.shape
    trees, cols, pairs = EC.sample_trees(case), EC.sample_cols(case), EC.sample(case)
    for t0 in range(0, T, PR_TT):                          # the first and last real tree of every tree tile ...
        assert t0 in trees and min(t0 + PR_TT, T) - 1 in trees
    for k in range(case.K):                                # ... the first and last replicate of every scale ...
        assert k * case.B in cols and (k + 1) * case.B - 1 in cols
    if case.cols == 'tiles':                               # ... and of every column tile of every chunk
        for c0, n in EC.chunks(case):
            for b0 in range(0, n, PR_TB):
                assert c0 + b0 in cols and c0 + min(b0 + PR_TB, n) - 1 in cols
    assert {t for t, _ in pairs} == set(trees) and {c for _, c in pairs} == set(cols)      # thinning drops no tree and no column
    assert set(case.named) <= set(trees) and all((t, c) in pairs for t in case.named for c in cols)
    assert len(pairs) <= EC.CAP + len(case.named) * len(cols) + max(len(trees), len(cols))
    ref, rat = EC.host(name), EC.rational(name)
    assert ref['counts'].shape == (case.K, case.B, S) and ref['rep_loglik'].shape == (case.K, T, case.B) and ref['best'].shape == (case.K, case.B)
    for c, cnt in rat['counts'].items():
        k, b = divmod(c, case.B)
        np.testing.assert_array_equal(ref['counts'][k, b], cnt, err_msg="counts of column %d" % c)
        assert int(cnt.sum()) == (S if case.call == 'rell' else case.draws[k])
    for (t, c), v in rat['rl'].items():
        k, b = divmod(c, case.B)
        assert bit(ref['rep_loglik'][k, t, b]) == bit(v), "host loop against rationals: tree %d, column %d" % (t, c)
    for t, v in rat['obs'].items():
        assert bit(ref['obs'][t]) == bit(v), "the left-to-right sum against the rational chain of ones: tree %d" % t
    for k in range(case.K):
        ck = [c - k * case.B for c in cols if c // case.B == k]
        np.testing.assert_array_equal(ref['best'][k], rell_ref.first_argmax(ref['rep_loglik'][k]))
        np.testing.assert_array_equal(ref['best'][k][ck], rell_ms_ref.best_lex(ref['rep_loglik'][k][:, ck]))
    if case.winner is not None:                            # in rationals: the named row above every other sampled row
        for c in cols:
            others = [v for (t, cc), v in rat['rl'].items() if cc == c and t != case.winner]
            assert others and all(rat['rl'][case.winner, c] > v for v in others)
        assert (ref['best'] == case.winner).all()
    if case.tie is not None:                               # the two rows' scores bit-equal, and above every other sampled row's
        lo, hi = case.tie
        for c in cols:
            assert bit(rat['rl'][lo, c]) == bit(rat['rl'][hi, c])
            others = [v for (t, cc), v in rat['rl'].items() if cc == c and t not in case.tie]
            assert others and all(rat['rl'][lo, c] > v for v in others)
        assert (ref['best'] == lo).all()


def test_launch_counts_are_the_existing_suites():
    """the restated plan gives what tests/test_gpu_rell.py and tests/test_gpu_rell_multiscale.py assert: 6 and 3 + 3 chunks, 5 and
    2 + 3 chunks"""
    one, three = EC.Case('x', EC.f_a, 40), EC.Case('x', EC.f_a, 40, chunk=16)
    assert (EC.launches(one), len(EC.chunks(three)), EC.launches(three)) == (6, 3, 3 + 3 * 3)
    one, five = EC.Case('x', EC.f_a, 150, DRAWS), EC.Case('x', EC.f_a, 150, DRAWS, chunk=100)
    assert (EC.launches(one), len(EC.chunks(five)), EC.launches(five)) == (5, 5, 2 + 3 * 5)
    for name in EC.NAMES:
        if not CASES[name].chunk:
            assert len(EC.chunks(CASES[name])) == len(EC.chunks(CASES[name], scores=False)) == 1, name


# ---- A: columns on tile edges ---------------------------------------------------------------------------------------------------
def test_a_columns_on_tile_edges():
    assert EC.f_a().shape == (65, 37) and tiles(65, PR_TT) == 2 and 65 - PR_TT == 1 and tiles(37, PR_KP) == 2
    # phylo_rell: the row of ones is column B of the one chunk
    where = {B: (B // PR_TB, B % PR_TB, tiles(B + 1, PR_TB)) for B in (127, 128, 129, 256)}
    assert where == {127: (0, 127, 1), 128: (1, 0, 2), 129: (1, 1, 2), 256: (2, 0, 3)}     # (its tile, its lane, tiles)
    assert [CASES[n].B for n in EC.group('A1')] == [127, 128, 129, 256]
    # the multiscale call: column K B
    for name, KB, tile, lane in (('A2-ms-K3-B128', 384, 3, 0), ('A2-ms-K2-B64', 128, 1, 0), ('A2-ms-K1-B127', 127, 0, 127)):
        case = CASES[name]
        assert case.K * case.B == KB and (KB // PR_TB, KB % PR_TB) == (tile, lane) and EC.chunks(case) == [(0, KB)]
    assert 64 % PR_TB != 0 and 64 < PR_TB                 # K = 2, B = 64: the scale edge lies inside the one full tile
    # chunks
    assert EC.chunks(CASES['A3-rell-B300-chunk128']) == [(0, 128), (128, 128), (256, 44)]
    assert EC.chunks(CASES['A3-ms-B128-chunk128']) == [(0, 128), (128, 128), (256, 128)]              # every chunk one scale
    assert EC.chunks(CASES['A3-ms-B128-chunk64']) == [(64 * i, 64) for i in range(6)]                  # every scale edge a chunk edge
    assert {n: EC.launches(CASES[n]) for n in EC.group('A3', chunked=True)} == {'A3-rell-B300-chunk128': 12, 'A3-ms-B128-chunk128': 11,
                                                                                 'A3-ms-B128-chunk64': 20}
    for name in EC.group('A3', chunked=True):
        assert EC.launches(CASES[name]) == (3 if CASES[name].call == 'rell' else 2) + 3 * len(EC.chunks(CASES[name]))


# ---- B: many tree tiles -------------------------------------------------------------------------------------------------------------
def test_b_many_tree_tiles():
    assert tiles(1025, PR_TT) == 17 and 1025 - 16 * PR_TT == 1 and tiles(1025, 16) == 65 and tiles(257, PR_TT) == 5 and 257 - 4 * PR_TT == 1
    per = tiles(1025, 16)                                  # pr_best: slice = t // per
    assert (3 // per, 1000 // per, 3 // PR_TT, 1000 // PR_TT) == (0, 15, 0, 15)                        # distant tiles and slices
    assert (64 // per, 65 // per, 64 // PR_TT, 65 // PR_TT, 64 % PR_TT) == (0, 1, 1, 1, 0)             # adjacent slices, tile 1's first rows
    assert (63 // per, 64 // per, 63 // PR_TT, 64 // PR_TT) == (0, 0, 0, 1)                            # a tile edge inside slice 0
    for T in (1025, 257):
        f = EC.f_b(T)
        assert f.shape == (T, 37) and f.max() < np.exp(-1.0)
    assert EC.dominating_row(37).min() > np.exp(-1.0)
    for name in EC.group('B'):
        case = CASES[name]
        f, ref = case.f(), EC.host(name)
        assert (ref['rep_loglik'] < 0).all() and (ref['obs'] < 0).all()       # a padded row's +0.0 would win by value
        others = np.delete(np.arange(case.shape[0]), list(case.named))
        assert f[others].max() < np.exp(-1.0) and np.array_equal(f[others], EC.f_b(case.shape[0])[others])
        for t in case.named:
            np.testing.assert_array_equal(f[t], EC.dominating_row(37))
        if not case.named:                                  # as drawn: the best moves with the replicate, over several tiles
            assert len({int(t) // PR_TT for t in ref['best'].reshape(-1)}) > 2


# ---- C: long walks ----------------------------------------------------------------------------------------------------------------
def test_c_panel_arithmetic():
    assert 2048 % PR_KP == 0 and 2048 // PR_KP == 64 and not (63 * PR_KP + PR_KP < 2048) and 62 * PR_KP + PR_KP < 2048
    assert tiles(2051, PR_KP) == 65 and 2051 - 64 * PR_KP == 3 and 2051 % 4 == 3 and EC.count_stride(2051) == 2052
    assert max(EC.C_SWAP) < 2048 // PR_KP
    for name, S in (('C1-rell-S2048', 2048), ('C1-rell-S2051', 2051), ('C2-ms-S2051', 2051)):
        f = CASES[name].f()
        assert f.shape == (65, S) and (f[0] == 5e-324).any() and (f[0] == 1.0).any() and (f[0] > 1.0).any()
    assert CASES['C2-ms-S2051'].K * CASES['C2-ms-S2051'].B == 132


@pytest.mark.parametrize("name", EC.group('C'))
def test_c_the_sample_sees_a_misordered_panel(name):
    """every sampled chain, and every sampled tree's chain of ones, changes its bits when the panels C_SWAP change places"""
    case = CASES[name]
    x, rat = EC.host(name)['x'], EC.rational(name)
    every = np.concatenate(list(rat['counts'].values()))
    assert (every >= 3).any() and (every == 0).any()
    for (t, c), v in rat['rl'].items():
        cnt = rat['counts'][c]
        assert (cnt[:PR_KP] > 0).any() and (cnt[PR_KP * EC.C_SWAP[1]:][:PR_KP] > 0).any()
        w = rell_ref.chain(EC.swap_panels(cnt, *EC.C_SWAP), EC.swap_panels(x[t], *EC.C_SWAP))
        assert bit(w) != bit(v), "tree %d, column %d" % (t, c)
    for t, v in rat['obs'].items():
        assert bit(rell_ref.chain(np.ones(case.shape[1]), EC.swap_panels(x[t], *EC.C_SWAP))) != bit(v), "observed score of tree %d" % t


# ---- D: scores of exactly +0.0 --------------------------------------------------------------------------------------------------------
def test_d_zero_scores():
    for name in EC.group('D'):
        case, ref = CASES[name], EC.host(name)
        assert case.shape == (65, 37)
        assert (bits(ref['x'][64]) == 0).all() and (bits(ref['rep_loglik'][:, 64]) == 0).all() and bit(ref['obs'][64]) == 0    # +0.0, the bits
        if 'ones' in name:
            assert (bits(ref['rep_loglik']) == 0).all() and (bits(ref['obs']) == 0).all() and (ref['best'] == 0).all()
        elif 'wins' in name:
            assert (ref['rep_loglik'][:, :64] < 0).all() and (ref['best'] == 64).all()
        else:
            assert (ref['rep_loglik'][:, :64] > 0).all() and (ref['best'] != 64).all() and len(set(ref['best'].reshape(-1).tolist())) > 1
        for (t, c), v in EC.rational(name)['rl'].items():
            if t == 64:
                assert bit(v) == 0


# ---- E: draw vectors --------------------------------------------------------------------------------------------------------------------
def test_e_draw_vectors():
    for name in EC.group('E1'):
        case, ref = CASES[name], EC.host(name)
        assert case.shape == (5, 37) and case.B == 150
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert not np.array_equal(ref['counts'][i], ref['counts'][j])
        np.testing.assert_array_equal(ref['counts'].sum(axis=2), np.repeat(np.array(case.draws)[:, None], 150, axis=1))
    plain = _ffi.debug_rell_host(EC.f_e(), 0, 150, SEED)
    rep = EC.host('E1-ms-repeated')
    np.testing.assert_array_equal(rep['counts'][0], plain['counts'])           # scale 0 shares phylo_rell's stream
    np.testing.assert_array_equal(bits(rep['rep_loglik'][0]), bits(plain['rep_loglik']))
    np.testing.assert_array_equal(rep['counts'][0, 7], rell_ref.counts(37, 7, SEED))
    case = CASES['E2-ms-unsorted-chunk100']
    assert case.draws == (52, 18, 37) and EC.chunks(case) == [(0, 100), (100, 100), (200, 100), (300, 100), (400, 50)]
    spans = [(c0 // case.B, (c0 + n - 1) // case.B) for c0, n in EC.chunks(case)]
    assert spans == [(0, 0), (0, 1), (1, 1), (2, 2), (2, 2)]
    assert case.draws[spans[1][1]] < max(case.draws[spans[1][0]:spans[1][1] + 1])      # chunk 1: the last scale's draws are not the largest
    assert EC.launches(case) == 2 + 3 * 5


# ---- F: counts that share a word, far columns --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.group('F1'))
def test_f_counts_that_share_a_word(name):
    case, ref = CASES[name], EC.host(name)
    T, S = case.shape
    assert T == 5 and case.B == 20 and EC.count_stride(S) == 4            # the sites of a row lie in two 32-bit words, S = 2: in one
    for k, nd in enumerate(case.draws):
        for b in range(case.B):
            want = rell_ms_ref.counts(S, case.draws, k, b, SEED)
            assert int(want.sum()) == nd
            np.testing.assert_array_equal(ref['counts'][k, b], want)
            if S == 2:
                assert want.min() > 30000
            if nd == 65535:
                assert want[0] + want[1] > 30000 and want.max() > 65535 // S


def test_f_far_columns():
    case = CASES['F2-ms-B5000']
    assert case.K * case.B == 15000 and tiles(15001, PR_TB) == 118 and len(EC.chunks(case)) == 1 == len(EC.chunks(case, scores=False))
    assert EC.sample_cols(case) == [0, 4999, 5000, 9999, 10000, 14999]
