"""Shared inputs of the edge tests of scored tree sets (DESIGN.md sections 11, 11b, 13, 14): alignments simulated along trees of 129
to 512 taxa with that tree and nearest-neighbour interchanges of it as the set; sets with more work items than ptg_updown has
workgroups; generic leaves scaled by exact powers of two so that chosen site factors land near the floor of the double range;
random columns over 300 and 310 taxa, which reach that floor by themselves.  test_trees_edges_cpu.py holds every case to its
precondition from the NumPy restatement alone; test_gpu_trees_edges.py asserts it again before it compares anything."""
import functools
import math

import numpy as np

import treegrad_ref as TR
from test_gpu_treegrad import nni_neighbours
from test_gpu_trees_loglik import alignment, gtr_Q, random_trees
from treegrad_cases import simulate
from trees_cases import balanced_rows, caterpillar_rows, random_rows

PRIOR = np.array([0.1, 0.2, 0.3, 0.4])
FLOOR = TR.FLOOR                     # 2^-1020: below it a tree's derivatives are NaN (section 13)
ROOMY = 2.0 ** -1000                 # what the cases of parts A and B keep every site factor above
SHAPES = {'balanced': balanced_rows, 'caterpillar': caterpillar_rows, 'random': random_rows}


def su_depth(child):
    """the slots a tree's schedule holds: need(leaf) = 0, need(v) = max(1, n1, n2 + [n1 > 0]) for n1 >= n2 (Sethi-Ullman, section 11)"""
    N = child.shape[0] + 1
    need = []
    for a, b in child:
        n1, n2 = sorted((0 if a < N else need[a - N], 0 if b < N else need[b - N]), reverse=True)
        need.append(max(1, n1, n2 + (n1 > 0)))
    return need[-1]


# ---- A. 129 to 512 taxa ------------------------------------------------------------------------------------------------------
def big(N, S, shape, **kw):
    return dict(N=N, S=S, shape=shape, **kw)


BIG = {'%s-N%d' % (shape, N): big(N, 65, shape) for N in (129, 257, 512) for shape in SHAPES}
BIG['balanced-N512-S130-tile64'] = big(512, 130, 'balanced', tile=64)
BIG['generic-balanced-N512'] = big(512, 65, 'balanced', generic=True)
SEEDS = {}                           # a case that misses ROOMY gets another seed here (none did)


@functools.lru_cache(maxsize=None)
def big_case(name, n=5):
    """(g, child, blen, Q): an alignment simulated along a tree of the case's shape (its lengths + 0.05); the set is that tree and
    n - 1 of its nearest-neighbour interchanges spread over the rows, every length off by a factor in [1/2, 2] -- the generating
    tree's zero-length right-hand branches stay zero in every tree"""
    kw = BIG[name]
    N, S = kw['N'], kw['S']
    Q = gtr_Q()
    rng = np.random.default_rng(SEEDS.get(name, 12))
    c0, b0 = SHAPES[kw['shape']](N, rng)
    g = simulate(c0, b0 + 0.05, Q, PRIOR, S, rng)
    near = nni_neighbours(c0)
    pick = [near[i] for i in np.linspace(0, len(near) - 1, n - 1).astype(int)]
    child = np.array([c0] + pick)
    blen = b0[None] * rng.uniform(0.5, 2.0, size=(n, N - 1, 2))
    if kw.get('generic'):
        g[rng.integers(0, N), rng.integers(0, S)] = [0.5, 0.25, 0.0, 1.0]       # one row that is no indicator: no codes at all
    for a in (g, child, blen):
        a.setflags(write=False)
    return g, child, blen, Q


@functools.lru_cache(maxsize=None)
def two_strip_case(S=200):
    """(g, child, blen, Q): balanced-N257's tree set on an alignment of S sites simulated along the same generating tree (the
    case's seed gives the tree and its lengths, SEEDS['two-strips'] the columns): with a site tile of 256 one tile whose second
    strip of 128 sites holds S - 128 live ones"""
    name = 'balanced-N257'
    _, child, blen, Q = big_case(name)
    c0, b0 = SHAPES['balanced'](257, np.random.default_rng(SEEDS.get(name, 12)))
    assert c0.tobytes() == child[0].tobytes()
    g = simulate(c0, b0 + 0.05, Q, PRIOR, S, np.random.default_rng(SEEDS.get('two-strips', 200)))
    g.setflags(write=False)
    return g, child, blen, Q


# ---- B. more work items than workgroups ----------------------------------------------------------------------------------------
def updown_cap(N, cus):
    """ptg_make_plan's cap on the grid of ptg_updown, the items apart: min(8 CUs, 256 MiB / ((N-1) U 2 KiB)), U = 2"""
    return max(1, min(8 * cus, (256 << 20) // ((N - 1) * 2 * 2048)))


def strided_T(N, ntiles, cus):
    """the fewest trees whose ntiles T items exceed the cap by at least 5 and are no multiple of it"""
    cap = updown_cap(N, cus)
    T = -(-(cap + 5) // ntiles)
    while (T * ntiles) % cap == 0:
        T += 1
    return T


def small_strided(T, generic=False):
    """N = 5, S = 130 (tile 64: three tiles), coded leaves with gaps (or generic ones): T random trees, so a workgroup's second
    item is a tree of another topology and row order"""
    g = alignment(5, 130, 77, gaps=True, generic=generic)
    child, blen = random_trees(5, 78, T)
    return g, child, blen, gtr_Q()


@functools.lru_cache(maxsize=None)
def large_strided(mixed, T=131):
    """N = 512 balanced, S = 65: the generating tree under T length perturbations; mixed: tree t has the topology t mod 3 of
    (generating tree, two of its neighbours), so that trees t and t + 128 -- one workgroup's two items -- differ in row order"""
    N, S = 512, 65
    Q = gtr_Q()
    rng = np.random.default_rng(12)
    c0, b0 = balanced_rows(N, rng)
    g = simulate(c0, b0 + 0.05, Q, PRIOR, S, rng)
    near = nni_neighbours(c0)
    tops = [c0, near[0], near[len(near) // 2]] if mixed else [c0]
    child = np.array([tops[t % len(tops)] for t in range(T)])
    blen = b0[None] * rng.uniform(0.5, 2.0, size=(T, N - 1, 2))
    for a in (g, child, blen):
        a.setflags(write=False)
    return g, child, blen, Q


def small_mixed(T, cap, ntiles=3):
    """N = 5, tiles of 64: an alignment simulated along a tree; tree t has the topology t mod m of (that tree, its neighbours), m
    the smallest period under which the trees of items w and w + cap always differ (cap // ntiles trees apart, or one more)"""
    N, S = 5, 130
    Q = gtr_Q()
    rng = np.random.default_rng(13)
    c0, b0 = random_rows(N, rng)
    g = simulate(c0, b0 + 0.05, Q, PRIOR, S, rng)
    g[rng.random((N, S)) < 0.15] = 1.0
    tops = [c0] + nni_neighbours(c0)
    q = cap // ntiles
    m = next(m for m in range(2, len(tops) + 1) if q % m and (cap % ntiles == 0 or (q + 1) % m))
    child = np.array([tops[t % m] for t in range(T)])
    blen = b0[None] * rng.uniform(0.5, 2.0, size=(T, N - 1, 2))
    return g, child, blen, Q


# ---- C. the floor of the range: generic leaves scaled by exact powers of two ---------------------------------------------------
SCALED_SITES = (0, 63, 64, 129)      # S = 130, tile 64: first and last lane of a step, a second tile, the last live lane of the last step
PLACES = ('2^-900', 'at-the-floor', 'inside', 'just-below', 'subnormal', 'zero')
IN_RANGE = PLACES[:3]


def scaled_base():
    """N = 12, S = 130, generic leaves, 5 trees; and the two leaves that take the scaling (leaves 0 and 1)"""
    g = alignment(12, 130, 242, generic=True)
    child, blen = random_trees(12, 5, 5)
    return g, child, blen, gtr_Q()


def scaled_exponents(place, L0):
    """e [len(SCALED_SITES)]: site s of every tree is multiplied by 2^-e[s].  L0 [trees][S] the unscaled site factors (from the
    restatement).  With m 2^k (1/2 <= m < 1) the largest and the smallest factor of the site over the trees:
    2^-900: the largest lands in [2^-901, 2^-900); at-the-floor: the smallest lands in [2^-1020, 2^-1019); inside: the largest in
    [2^-1003, 2^-1002); just-below: the largest in [2^-1021, 2^-1020); subnormal: the largest in [2^-1051, 2^-1050); zero: e =
    1200, and the product of the two halves underflows to 0."""
    e = []
    for s in SCALED_SITES:
        k_hi, k_lo = math.frexp(L0[:, s].max())[1], math.frexp(L0[:, s].min())[1]
        e.append({'2^-900': k_hi + 900, 'at-the-floor': k_lo + 1019, 'inside': k_hi + 1002, 'just-below': k_hi + 1020,
                  'subnormal': k_hi + 1050, 'zero': 1200}[place])
    return np.array(e)


def scaled_leaves(g, e):
    """leaf 0's row at site s times 2^-(e // 2), leaf 1's times 2^-(e - e // 2): every factor of the site times 2^-e exactly, as
    long as nothing underflows on the way"""
    g = g.copy()
    for s, es in zip(SCALED_SITES, e):
        g[0, s] = np.ldexp(g[0, s], -(int(es) // 2))
        g[1, s] = np.ldexp(g[1, s], -(int(es) - int(es) // 2))
    return g


# ---- C. coded leaves: random columns over 300 and 310 taxa ---------------------------------------------------------------------
def random_columns(N):
    """alignment(N, 64, 100 + N + 64) and random_trees(N, 5, 3): at N = 300 every site factor of every tree stays above FLOOR
    (tree 0's smallest: 2.7e-304); at N = 310 tree 0 has 11 subnormal factors and none zero"""
    g = alignment(N, 64, 100 + N + 64)
    child, blen = random_trees(N, 5, 3)
    return g, child, blen, gtr_Q()
