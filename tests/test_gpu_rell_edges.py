"""phylo_rell and phylo_rell_multiscale on the device where tests/test_gpu_rell.py and tests/test_gpu_rell_multiscale.py stop
(DESIGN.md sections 12 and 12b; the cases and why they are cases: tests/rell_edges_cases.py, held to their preconditions by
tests/test_rell_edges_cpu.py): column counts of 127, 128 and multiples of 128, chunks that end on tile and scale edges, 5 and 17
tree tiles with winners and ties across tiles and pr_best's slices, walks of 64 and 65 panels over factors that differ, real
rows that score exactly +0.0 beside padded rows, unsorted and repeated draw vectors, two counts above 30000 in one 32-bit word,
15000 columns.  Every array is held bit for bit to the library's host loop, the sample of every case to the exact-rational
chain and the restated counts; best and wins by the tie rule, through both instances of the multiscale product; launch counts
from the drivers' chunk plans.

Every test here needs Context.rell and Context.rell_multiscale: AttributeError without them."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import rell_edges_cases as EC
import rell_ms_ref
import test_gpu_rell as PLAIN
import test_gpu_rell_multiscale as MS
from phylo_amd import _ffi
from rell_edges_cases import CASES, SEED
from test_gpu_rell import bits

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


@pytest.fixture(scope="module")
def ctx():
    with _ffi.Context(4, 5, 10) as c:                    # the calls read no leaves: their S is their own
        yield c


def call(ctx, case):
    """the case on this context: the call with every output, and the call with the required ones alone"""
    if case.call == 'rell':
        return (ctx.rell(case.f(), case.B, SEED, want_reps=True, want_counts=True, want_logs=True), ctx.rell(case.f(), case.B, SEED))
    return (ctx.rell_multiscale(case.f(), case.draws, case.B, SEED, want_best=True, want_reps=True, want_counts=True),
            ctx.rell_multiscale(case.f(), case.draws, case.B, SEED, want_best=True))


def against_the_sample(name, rl_KxTxB, counts_KxBxS, best_KxB, obs):
    """the independent reference: scores and observed scores against exact rationals, counts against phylo_amd.rng, best by the
    loop restatement over the fetched columns"""
    case, rat = CASES[name], EC.rational(name)
    for c, cnt in rat['counts'].items():
        k, b = divmod(c, case.B)
        np.testing.assert_array_equal(counts_KxBxS[k, b], cnt, err_msg="counts of column %d against the restatement" % c)
    for (t, c), v in rat['rl'].items():
        k, b = divmod(c, case.B)
        assert bits(rl_KxTxB[k, t, b]) == bits(v), "score of tree %d, column %d against rationals" % (t, c)
    for t, v in rat['obs'].items():
        assert bits(obs[t]) == bits(v), "observed score of tree %d against rationals" % t
    for k in range(case.K):
        ck = [c - k * case.B for c in EC.sample_cols(case) if c // case.B == k]
        np.testing.assert_array_equal(best_KxB[k][ck], rell_ms_ref.best_lex(rl_KxTxB[k][:, ck]), err_msg="best of scale %d on the sample" % k)


def named_rows(case, rl_KxTxB, outs):
    """outs: (best [K][B], wins [K][T]) of every instance"""
    if case.winner is not None:
        for best, wins in outs:
            assert (best == case.winner).all() and (wins[:, case.winner] == case.B).all() and (wins.sum(axis=1) == case.B).all()
    if case.tie is not None:
        lo, hi = case.tie
        np.testing.assert_array_equal(bits(rl_KxTxB[:, lo]), bits(rl_KxTxB[:, hi]))
        for best, wins in outs:
            assert (best == lo).all() and (wins[:, lo] == case.B).all() and (wins[:, hi] == 0).all()


def run(ctx, name):
    """one case in this process (one chunk): every array against the host loop, the sample against the independent reference"""
    case, ref = CASES[name], EC.host(name)
    T, S = case.shape
    if case.call == 'rell':
        out, lean = call(ctx, case)
        PLAIN.check(out, {'counts': ref['counts'][0], 'x': ref['x'], 'rl': ref['rep_loglik'][0], 'obs': ref['obs']}, T, case.B, S)
        assert sorted(lean) == ['best', 'obs', 'stats', 'wins']
        np.testing.assert_array_equal(lean['best'], out['best'])
        np.testing.assert_array_equal(lean['wins'], out['wins'])
        np.testing.assert_array_equal(bits(lean['obs']), bits(out['obs']))
        out = {'rep_loglik': out['rep_loglik'][None], 'counts': out['counts'][None], 'best': out['best'][None], 'wins': out['wins'][None],
               'obs': out['obs'], 'stats': out['stats']}
        lean = {'best': lean['best'][None], 'wins': lean['wins'][None], 'stats': lean['stats']}
    else:
        out, lean = MS.check(ctx, case.f(), case.draws, case.B, SEED, ref)     # both instances; obs is phylo_rell's
        np.testing.assert_array_equal(bits(out['obs']), bits(ref['obs']), err_msg="observed scores")
    np.testing.assert_array_equal(out['best'], ref['best'], err_msg="best against the host loop")
    against_the_sample(name, out['rep_loglik'], out['counts'], out['best'], out['obs'])
    named_rows(case, out['rep_loglik'], [(out['best'], out['wins']), (lean['best'], lean['wins'])])
    assert len(EC.chunks(case)) == len(EC.chunks(case, scores=False)) == 1
    assert out['stats']['n_launches'] == lean['stats']['n_launches'] == EC.launches(case) == (6 if case.call == 'rell' else 5)
    return out, lean


# ---- A. column counts on tile edges ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.group('A1') + EC.group('A2'))
def test_a_columns_on_tile_edges(ctx, name):
    """the row of ones as the last lane of a column tile, alone in a tile of its own, the second of its tile; a scale edge inside
    one tile; two tree tiles (the second: one real row) and two panels"""
    run(ctx, name)


CHUNK_SCRIPT = r"""
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import rell_edges_cases as EC
from phylo_amd import _ffi
case = EC.CASES[sys.argv[2]]
with _ffi.Context(4, 5, 10) as ctx:
    if case.call == 'rell':
        out = ctx.rell(case.f(), case.B, EC.SEED, want_reps=True, want_counts=True, want_logs=True)
        lean = ctx.rell(case.f(), case.B, EC.SEED)
    else:
        out = ctx.rell_multiscale(case.f(), case.draws, case.B, EC.SEED, want_best=True, want_reps=True, want_counts=True)
        lean = ctx.rell_multiscale(case.f(), case.draws, case.B, EC.SEED, want_best=True)
    np.savez(sys.argv[1], launches=out['stats']['n_launches'], lean_launches=lean['stats']['n_launches'], lean_best=lean['best'],
             lean_wins=lean['wins'], lean_obs=lean['obs'], **{k: v for k, v in out.items() if k != 'stats'})
"""


def run_chunked(ctx, name):
    """PHYLO_RELL_CHUNK is read when the context is created: the case in a fresh process with its chunk, against this process's
    single chunk, the host loop and the sample (whose columns are the tile edges of every chunk)"""
    case, ref = CASES[name], EC.host(name)
    one, one_lean = call(ctx, case)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'chunked.npz')
        env = dict(os.environ, PHYLO_RELL_CHUNK=str(case.chunk))
        p = subprocess.run([sys.executable, '-c', CHUNK_SCRIPT % (ROOT, os.path.join(ROOT, 'tests')), path, name], env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert p.returncode == 0, p.stdout.decode()[-2000:]
        got = dict(np.load(path))
    n = len(EC.chunks(case))
    assert n > 1 and int(got['launches']) == int(got['lean_launches']) == EC.launches(case) == (3 if case.call == 'rell' else 2) + 3 * n
    assert one['stats']['n_launches'] == one_lean['stats']['n_launches'] == (6 if case.call == 'rell' else 5)
    for key in ('obs', 'rep_loglik') + (('site_loglik',) if case.call == 'rell' else ()):
        np.testing.assert_array_equal(bits(got[key]), bits(one[key]), err_msg=key)
    for key in ('counts', 'best', 'wins'):
        np.testing.assert_array_equal(got[key], one[key], err_msg=key)
    np.testing.assert_array_equal(got['lean_best'], one['best'])
    np.testing.assert_array_equal(got['lean_wins'], one['wins'])
    np.testing.assert_array_equal(bits(got['lean_obs']), bits(one['obs']))
    shape = (case.K,) + got['rep_loglik'].shape[-2:]
    rl, counts, best = got['rep_loglik'].reshape(shape), got['counts'].reshape(ref['counts'].shape), got['best'].reshape(ref['best'].shape)
    np.testing.assert_array_equal(bits(rl), bits(ref['rep_loglik']), err_msg="scores against the host loop")
    np.testing.assert_array_equal(counts, ref['counts'], err_msg="counts against the host loop")
    np.testing.assert_array_equal(best, ref['best'], err_msg="best against the host loop")
    np.testing.assert_array_equal(bits(got['obs']), bits(ref['obs']), err_msg="observed scores")
    np.testing.assert_array_equal(got['wins'].reshape(case.K, -1), MS.wins_of(best, case.shape[0]))
    against_the_sample(name, rl, counts, best, got['obs'])
    return got


@pytest.mark.parametrize("name", EC.group('A3', chunked=True))
def test_a_chunks_on_tile_and_scale_edges(ctx, name):
    """phylo_rell: 128 replicates and the row of ones, then 128, then 44; the multiscale call: every chunk exactly one scale, and
    every scale edge a chunk edge"""
    run_chunked(ctx, name)


# ---- B. many tree tiles ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.group('B'))
def test_b_many_tree_tiles(ctx, name):
    """17 tree tiles (5 at T = 257), the last with one real row; pr_best with 65 trees per slice; a winner in that one real row;
    identical dominating rows across distant tiles and slices, across a slice edge, across a tile edge: the lower index takes
    every replicate"""
    out, _ = run(ctx, name)
    assert out['best'].min() >= 0 and out['best'].max() < CASES[name].shape[0]


# ---- C. long walks with factors that differ ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.group('C'))
def test_c_long_walks(ctx, name):
    """64 panels exactly (no prefetch behind the last), 65 panels with a last one of 3 sites and one padded count: a panel
    dropped, repeated or out of place changes the sampled chains (tests/test_rell_edges_cpu.py asserts that it would)"""
    run(ctx, name)


# ---- D. scores of exactly +0.0 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.group('D'))
def test_d_zero_scores_beside_padded_rows(ctx, name):
    """every score +0.0: tree 0 wins, the padded rows of tile 1 leave by index; row 64 alone at +0.0 above negative scores: it
    wins, the one real row among 63 padded ones that hold its value; below positive scores: it never wins"""
    out, lean = run(ctx, name)
    assert (bits(out['rep_loglik'][:, 64]) == 0).all() and bits(out['obs'][64]) == 0
    for o in (out, lean):
        if 'ones' in name:
            assert (o['best'] == 0).all() and (o['wins'][:, 0] == CASES[name].B).all()
        elif 'loses' in name:
            assert (o['best'] != 64).all() and (o['wins'][:, 64] == 0).all()
    if 'ones' in name:
        assert (bits(out['rep_loglik']) == 0).all() and (bits(out['obs']) == 0).all()


# ---- E. draw vectors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.group('E1'))
def test_e_draw_vectors(ctx, name):
    """draws that are not ascending, and one draw count three times (the scale is counter word 1: three different samples)"""
    out, _ = run(ctx, name)
    for i, j in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(out['counts'][i], out['counts'][j])
    if 'repeated' in name:
        case = CASES[name]
        plain = ctx.rell(case.f(), case.B, SEED, want_reps=True, want_counts=True)       # scale 0 shares phylo_rell's stream
        np.testing.assert_array_equal(out['counts'][0], plain['counts'])
        np.testing.assert_array_equal(bits(out['rep_loglik'][0]), bits(plain['rep_loglik']))
        np.testing.assert_array_equal(out['best'][0], plain['best'])


def test_e_a_chunk_covers_the_largest_draw_count_of_its_scales(ctx):
    """chunks of 100 columns over draws (52, 18, 37): columns 100 .. 199 hold scale 0 (52 draws) and then scale 1 (18)"""
    run_chunked(ctx, 'E2-ms-unsorted-chunk100')


# ---- F. counts that share a word, far columns ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EC.group('F1'))
def test_f_counts_that_share_a_word(ctx, name):
    """65535 draws over 2, 3 and 4 sites: both halves of a 32-bit word above 30000 at S = 2, built by 65535 atomic adds a row"""
    case = CASES[name]
    out, _ = run(ctx, name)
    S = case.shape[1]
    for k, nd in enumerate(case.draws):
        assert (out['counts'][k].sum(axis=1) == nd).all()
        for b in range(case.B):
            np.testing.assert_array_equal(out['counts'][k, b], rell_ms_ref.counts(S, case.draws, k, b, SEED), err_msg="k=%d b=%d" % (k, b))
    if S == 2:
        assert out['counts'].min() > 30000


def test_f_far_columns(ctx):
    """15000 columns, 118 column tiles, one chunk"""
    out, _ = run(ctx, 'F2-ms-B5000')
    assert out['counts'].shape == (3, 5000, 37)
