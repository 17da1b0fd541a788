"""Cases of the RELL edge suites (tests/test_rell_edges_cpu.py, tests/test_gpu_rell_edges.py; DESIGN.md sections 12 and 12b):
phylo_rell and phylo_rell_multiscale where tests/test_gpu_rell.py and tests/test_gpu_rell_multiscale.py stop.  Read against the
kernels' constants (a workgroup's tile is PR_TT = 64 trees x PR_TB = 128 columns, a panel PR_KP = 32 sites, pr_best joins 16 tree
slices, prm_join walks the tree tiles):

  A  column counts on tile edges (the row of ones as the last lane of a tile, alone in a tile), chunks on tile and scale edges
  B  17 and 5 tree tiles, pr_best with 65 trees per slice, winners and ties across tiles, slices and the last tile's one real row
  C  64 and 65 panels with factors that differ, a last panel of 3 sites behind a padded count
  D  scores of exactly +0.0 beside the padded rows' +0.0
  E  draw vectors that are unsorted or repeat
  F  two counts above 30000 in one 32-bit word; 15000 columns in 118 column tiles

Every case is an input (cached, read-only), its call and the sample on which the exact-rational replay runs: the first and last
real tree of every tree tile x the first and last replicate of every column tile and of every scale, the rows a case names
added, thinned to about CAP chains.  The references: the library's host loops for the full arrays, rell_ref.chain on the sample.
Nothing here needs a GPU."""
import functools

import numpy as np

import rell_ms_ref
import rell_ref
from phylo_amd import _ffi

SEED = 0x9E3779B97F4A7C15
PR_TT, PR_TB, PR_KP = 64, 128, 32                       # phylo_rell.h
PR_CHUNK_BYTES = 256 << 20
PRM_MAX_COLS = 1 << 20                                  # phylo_rell_ms.h
DRAWS = (18, 37, 52)
S0 = 37
CAP = 100                                               # chains of a case's rational sample, about
C_SWAP = (0, 63)                                        # the two panels whose exchange every sampled chain of group C must see


def _frozen(a):
    a.setflags(write=False)
    return a


def dominating_row(S):
    """above exp(-1) at every site (tests/test_gpu_rell_multiscale.py's test_ties): beside factors below exp(-1) it wins every
    replicate of every scale whatever the counts"""
    return np.exp(np.random.default_rng(1).uniform(-0.5, -0.1, size=S))


# ---- inputs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def f_a():
    return _frozen(rell_ref.factors(65, S0, 1265))


@functools.lru_cache(maxsize=None)
def f_b(T, winner=None, tie=None):
    f = rell_ref.factors(T, S0, 2025, special=False).copy()                 # every factor below exp(-1)
    if winner is not None:
        f[winner] = dominating_row(S0)
    if tie is not None:
        f[tie[0]] = f[tie[1]] = dominating_row(S0)
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def f_c(S, seed):
    """special=True: a subnormal, 1.0 and a value above 1 in row 0.  The seeds are searched (upwards from 3048, 3051 and 7051) for
    what test_rell_edges_cpu.py asserts: every sampled chain changes its bits when panels C_SWAP change places.  Every log but
    one is negative, so the accumulator only grows: a term is rounded on the grid of the binade the accumulator is in, and
    terms added within one binade commute.  Panels 0 and 63 lie in the most distant binades, and still one chain in five keeps
    its bits under their exchange."""
    return _frozen(rell_ref.factors(65, S, seed))


@functools.lru_cache(maxsize=None)
def f_d(kind):
    if kind == 'ones':
        return _frozen(np.ones((65, S0)))
    f = np.ones((65, S0))
    if kind == 'zero_wins':
        f[:64] = rell_ref.factors(64, S0, 4064, special=False)              # every other score negative
    else:
        f[:64] = np.random.default_rng(8).uniform(1.1, 4.0, size=(64, S0))  # 'zero_loses': every other score positive
    return _frozen(f)


@functools.lru_cache(maxsize=None)
def f_e():
    return _frozen(rell_ref.factors(5, S0, 5037))


@functools.lru_cache(maxsize=None)
def f_f(S):
    return _frozen(rell_ref.factors(5, S, 2000 + S))


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, f, B, draws=None, chunk=0, winner=None, tie=None, cols='tiles'):
        self.name, self.f, self.B, self.draws, self.chunk, self.winner, self.tie, self.cols = name, f, B, draws, chunk, winner, tie, cols
        self.call = 'rell' if draws is None else 'ms'
        self.K = 1 if draws is None else len(draws)

    @property
    def shape(self):
        return self.f().shape

    @property
    def named(self):
        return tuple(([] if self.winner is None else [self.winner]) + list(self.tie or ()))


CASES = {}


def _add(name, *a, **kw):
    assert name not in CASES
    CASES[name] = Case(name, *a, **kw)


for _B in (127, 128, 129, 256):
    _add('A1-rell-B%d' % _B, f_a, _B)
_add('A2-ms-K3-B128', f_a, 128, DRAWS)
_add('A2-ms-K2-B64', f_a, 64, (18, 37))
_add('A2-ms-K1-B127', f_a, 127, (37,))
_add('A3-rell-B300-chunk128', f_a, 300, chunk=128)
_add('A3-ms-B128-chunk128', f_a, 128, DRAWS, chunk=128)
_add('A3-ms-B128-chunk64', f_a, 128, DRAWS, chunk=64)
for _call, _draws in (('rell', None), ('ms', DRAWS)):
    _add('B1-%s-T1025' % _call, functools.partial(f_b, 1025), 150, _draws)
    _add('B2-%s-winner1024' % _call, functools.partial(f_b, 1025, 1024), 150, _draws, winner=1024)
    for _lo, _hi in ((3, 1000), (64, 65), (63, 64)):
        _add('B3-%s-tie%d-%d' % (_call, _lo, _hi), functools.partial(f_b, 1025, None, (_lo, _hi)), 150, _draws, tie=(_lo, _hi))
    _add('B4-%s-T257' % _call, functools.partial(f_b, 257), 150, _draws)
_add('C1-rell-S2048', functools.partial(f_c, 2048, 3069), 130)
_add('C1-rell-S2051', functools.partial(f_c, 2051, 3052), 130)
_add('C2-ms-S2051', functools.partial(f_c, 2051, 7066), 44, (1025, 2051, 2900))
for _call, _draws in (('rell', None), ('ms', DRAWS)):
    _add('D1-%s-ones' % _call, functools.partial(f_d, 'ones'), 150, _draws)
    _add('D2-%s-zero-wins' % _call, functools.partial(f_d, 'zero_wins'), 150, _draws, winner=64)
    _add('D3-%s-zero-loses' % _call, functools.partial(f_d, 'zero_loses'), 150, _draws)
_add('E1-ms-unsorted', f_e, 150, (52, 18, 37))
_add('E1-ms-repeated', f_e, 150, (37, 37, 37))
_add('E2-ms-unsorted-chunk100', f_e, 150, (52, 18, 37), chunk=100)
_add('F1-ms-S2', functools.partial(f_f, 2), 20, (65535,))
_add('F1-ms-S3', functools.partial(f_f, 3), 20, (65535, 1))
_add('F1-ms-S4', functools.partial(f_f, 4), 20, (65535,))
_add('F2-ms-B5000', f_e, 5000, DRAWS, cols='scales')

NAMES = sorted(CASES)


def group(prefix, call=None, chunked=False):
    return [n for n in NAMES if n.startswith(prefix) and (call is None or CASES[n].call == call) and bool(CASES[n].chunk) == chunked]


# ---- the drivers' chunk plans and launch counts, restated from phylo_hip.hip ------------------------------------------------------
def count_stride(S):
    return (S + 3) & ~3


def chunk_cols(case, scores=True):
    """columns of a chunk (replicates for phylo_rell): what PR_CHUNK_BYTES holds, at most PHYLO_RELL_CHUNK where that is set"""
    T, S = case.shape
    if case.call == 'rell':
        fit, n_all = max(1, PR_CHUNK_BYTES // (count_stride(S) * 2 + T * 8)), case.B
    else:
        tiles = -(-T // PR_TT)
        fit = min(max(1, PR_CHUNK_BYTES // (count_stride(S) * 2 + tiles * 12 + 4 + (T * 8 if scores else 0))), PRM_MAX_COLS)
        n_all = case.K * case.B
    if 0 < case.chunk < fit:
        fit = case.chunk
    return min(n_all, fit)


def chunks(case, scores=True):
    """(first column, columns) of every chunk; a column is c = k B + b"""
    n_all, w = case.K * case.B, chunk_cols(case, scores)
    return [(c0, min(w, n_all - c0)) for c0 in range(0, n_all, w)]


def launches(case, scores=True):
    """phylo_rell: pr_log once; pr_counts, pr_replicates, pr_best per chunk; pr_ones and pr_column with the first chunk.
    phylo_rell_multiscale: pr_log once; prm_counts, prm_product, prm_join per chunk; pr_ones with the first chunk."""
    n = len(chunks(case, scores))
    return 1 + 3 * n + (2 if case.call == 'rell' else 1)


# ---- the sample -----------------------------------------------------------------------------------------------------------------
def sample_trees(case):
    T = case.shape[0]
    rows = set(case.named)
    for t0 in range(0, T, PR_TT):
        rows |= {t0, min(t0 + PR_TT, T) - 1}
    return sorted(rows)


def sample_cols(case):
    """columns c = k B + b: the first and last replicate of every column tile of every chunk, and of every scale"""
    cols = set()
    for k in range(case.K):
        cols |= {k * case.B, k * case.B + case.B - 1}
    if case.cols == 'tiles':
        for c0, n in chunks(case):
            for b0 in range(0, n, PR_TB):
                cols |= {c0 + b0, c0 + min(b0 + PR_TB, n) - 1}
    return sorted(cols)


def sample(case):
    """the (tree, column) pairs: every pair of a named row; of the others, where they are more than CAP, the diagonals
    (i + j) % step == 0, which keep every sampled tree and every sampled column"""
    trees, cols = sample_trees(case), sample_cols(case)
    step = -(-len(trees) * len(cols) // CAP)
    assert step <= min(len(trees), len(cols))
    return [(t, c) for i, t in enumerate(trees) for j, c in enumerate(cols) if t in case.named or (i + j) % step == 0]


def observed_sum(x_TxS):
    """the observed score of every tree: the chain with every count 1.  fma(1.0, x, acc) is the correctly rounded x + acc, so the
    chain is the plain left-to-right sum in doubles, which np.add.accumulate computes (+0.0 + x[0] = x[0]: no log is -0.0)."""
    return np.add.accumulate(np.ascontiguousarray(x_TxS, dtype=np.float64), axis=1)[:, -1].copy()


def swap_panels(a, p, q):
    a = np.array(a)
    lo, hi = slice(p * PR_KP, (p + 1) * PR_KP), slice(q * PR_KP, (q + 1) * PR_KP)
    a[lo], a[hi] = a[hi].copy(), a[lo].copy()
    return a


# ---- references, one per case ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host(name):
    """the library's host loops on the whole case: counts [K][B][S], rep_loglik [K][T][B], best [K][B] (K = 1 for phylo_rell,
    whose best is the first-max argmax of its scores), x [T][S], obs [T] by observed_sum"""
    case = CASES[name]
    f = case.f()
    if case.call == 'rell':
        h = _ffi.debug_rell_host(f, 0, case.B, SEED)
        ref = {'counts': h['counts'][None], 'rep_loglik': h['rep_loglik'][None], 'best': rell_ref.first_argmax(h['rep_loglik'])[None],
               'x': h['site_loglik']}
    else:
        ref = rell_ms_ref.host(f, case.draws, case.B, SEED, _ffi.debug_rell_multiscale_host)
        ref['x'] = _ffi.debug_rell_host(f, 0, 1, SEED)['site_loglik']
    ref['obs'] = observed_sum(ref['x'])
    for a in ref.values():
        a.setflags(write=False)
    return ref


def restated_counts(case, c):
    k, b = divmod(c, case.B)
    S = case.shape[1]
    return rell_ref.counts(S, b, SEED) if case.call == 'rell' else rell_ms_ref.counts(S, case.draws, k, b, SEED)


@functools.lru_cache(maxsize=None)
def rational(name):
    """the independent reference on the sample: 'counts' {c: cnt[S]} from phylo_amd.rng, 'rl' {(t, c): chain} and 'obs' {t: chain of
    ones} in exact rationals, over the contract's logs"""
    case = CASES[name]
    x = host(name)['x']
    pairs = sample(case)
    cnt = {c: restated_counts(case, c) for c in sorted({c for _, c in pairs})}
    return {'counts': cnt, 'rl': {(t, c): rell_ref.chain(cnt[c], x[t]) for t, c in pairs},
            'obs': {t: rell_ref.chain(np.ones(x.shape[1]), x[t]) for t in sample_trees(case)}}
