"""Alignments whose site likelihoods leave the comfortable range, and the replay that says which branch of the site product
every (rank event, particle, tile, column, pair of steps) of a sweep takes -- from the C oracle's node rows, without a GPU.

Generic leaves are ordinary rows (uniform(0.05, 1)) times 2^e(taxon, site).  Scaling by a power of two commutes with the fma
chains of a merge (until something leaves the normal range, which is the point), so the site likelihood of a node is the unscaled
one times 2^(sum of e over the node's leaves): a site's class depends on WHICH taxa the node holds, and so differs between
particles and rank events.  The site kinds (taxa in braces carry the exponent, every other taxon 0):

  A  -260 on {0,1}: a node with both has x ~ 2^-523 -- two of them in a column fall below 2^-1021 together ('small')
  B  +265 on {0,1}: x ~ 2^520 -- two of them overflow together ('inf')
  C  -530 on {2,3}: x ~ 2^-1063, subnormal (pm_log's 2^54 rescale)
  D  -700 on {2,3}: x = 0 by underflow                                      -> -inf
  E  +600 on {4,5}: x = +inf by overflow                                    -> +inf
  F  D and E at one site: a node with all four holds 0 * inf                -> NaN
  M  taxon 2's row is (0.3, 0.3, -0.5, 0.3), every other (0.01, 0.01, 1, 0.01): pi . row > 0 for each leaf, but a node that
     holds taxon 2 has a negative entry where its sibling is large: x < 0  -> NaN
Every LEAF row keeps an ordinary site likelihood, so a forest's weight goes bad only through the nodes it has built, at different
rank events for different particles.  The kinds that spoil a leaf itself -- Z, taxon 1's row is zero (-inf); N, a NaN in taxon
3's row -- make every weight of every rank event non-finite: resampling's all-bad rule, a case of its own.
In SPECIAL a node that holds taxon 2 is NaN at the M sites, so its zeros and subnormals no longer decide a result.  TILES (A..E
alone, laid out by tile_placements) has no NaN FACTOR anywhere: even tiles hold D, odd tiles hold E, so a tile value is finite,
-inf (even tile, {2,3} in the node) or +inf (odd tile, {4,5}), and a row is NaN only because the tile values are added left to
right, -inf + inf.
"""
import numpy as np

from tests import site_product_ref as R

KINDS = {'A': (-260, (0, 1)), 'B': (265, (0, 1)), 'C': (-530, (2, 3)), 'D': (-700, (2, 3)), 'E': (600, (4, 5))}
FINITE, SPECIAL, ALLBAD, TILES = "ABC", "ABCDEFM", "ABCDEZN", "ABCDE"


def tile_placements(S, T):
    """{site: kind} for TILES: per tile, its zero (even tile) or +inf (odd tile) kind at column 0 of the first step, at column 63,
    as the second factor of the first pair, in steps 2 and 3, in an odd tail step and at the tile's last site (so T - 1 holds D and
    T holds E); a small pair, a large pair and subnormals (first and second factor) in every tile that is long enough."""
    put = {}
    for t, s0 in enumerate(range(0, S, T)):
        s1 = min(s0 + T, S)

        def at(off, kind):
            if s0 + off < s1 and s0 + off not in put:
                put[s0 + off] = kind

        lo = 'D' if t % 2 == 0 else 'E'
        at(s1 - 1 - s0, lo); at(0, lo); at(63, lo); at(64 + 1, lo); at(64 + 62, lo); at(128 + 20, lo); at(192 + 33, lo)
        steps = (s1 - s0 + 63) // 64
        if steps % 2 == 1:
            at((steps - 1) * 64 + 3, lo)
        at(20, 'C'); at(64 + 30, 'C'); at(192 + 30, 'C')
        for c in range(5, 13):
            at(c, 'A'); at(64 + c, 'A'); at(35 + c, 'B'); at(64 + 35 + c, 'B')
    return put


def placements(S, T, kinds):
    """{site: kind}: where the kinds go in a row of S sites under site tile T.  Steps are the 64-site steps of a tile (the merge
    takes them two at a time, a last odd one alone); lane = column."""
    if kinds == TILES:
        return tile_placements(S, T)
    put = {}

    def at(s, kind):
        if 0 <= s < S and kind in kinds and s not in put:
            put[s] = kind

    specials = [k for k in "CDEFMZN" if k in kinds]
    # the last site, next to the validity selects, then both sides of every tile boundary: -inf (or the subnormal) on the left,
    # +inf on the right, so that a -inf tile is followed by a +inf tile
    at(S - 1, specials[0])
    left = 'D' if 'D' in kinds else 'C'
    right = 'E' if 'E' in kinds else 'C'
    for b in range(T, S, T):
        at(b - 1, left)
        at(b, right)
    # tile 0: both factors of the first pair of steps small in columns 0..15, large in columns 48..63 (column 0 and column 63);
    for c in range(16):
        at(c, 'A'); at(64 + c, 'A')
        at(48 + c, 'B'); at(64 + 48 + c, 'B')
    # steps 0 and 1, then 2 and 3: a special as the FIRST factor in columns 20.. (0 and 63 too in step 2), as the SECOND factor in
    # columns 30.. (1 and 62 too in step 3)
    for i, k in enumerate(specials):
        at(20 + i, k)
        at(64 + 30 + i, k)
        at(128 + 20 + i, k)
        at(192 + 30 + i, k)
    at(128, specials[0]); at(128 + 63, specials[-1])
    at(192 + 1, specials[0]); at(192 + 62, specials[-1])
    # the last step of the last tile, when it is an odd one: a special in the tail step (column 3 if the row reaches it)
    s0 = ((S - 1) // T) * T
    steps = (S - s0 + 63) // 64
    if steps % 2 == 1:
        at(min(s0 + (steps - 1) * 64 + 3, S - 1), specials[min(1, len(specials) - 1)])
    # every later tile: a small pair and a large pair in its steps 0 and 1 (short tiles: as far as they go)
    for b in range(T, S, T):
        at(b + 5, 'A'); at(b + 64 + 5, 'A'); at(b + 9, 'B'); at(b + 64 + 9, 'B')
    return put


def scaled_leaves(N, S, T, kinds, seed):
    """generic leaves [N, S, 4] with the kinds laid out by placements(S, T, kinds)"""
    assert N >= 6
    rng = np.random.default_rng(seed)
    g = rng.uniform(0.05, 1.0, (N, S, 4))
    put = placements(S, T, kinds)
    for s, k in put.items():
        for kk in ('D', 'E') if k == 'F' else (k,):
            if kk in KINDS:
                e, taxa = KINDS[kk]
                g[list(taxa), s] = np.ldexp(g[list(taxa), s], e)
        if k == 'M':
            g[:, s] = [0.01, 0.01, 1.0, 0.01]
            g[2, s] = [0.3, 0.3, -0.5, 0.3]
        elif k == 'Z':
            g[1, s] = 0.0
        elif k == 'N':
            g[3, s, 2] = np.nan
    return g


def coded_leaves(N, S, seed):
    """one-hot leaves (leaf codes) with random nucleotides: about 3 of 4 sites of a cherry mismatch"""
    rng = np.random.default_rng(seed)
    return np.eye(4)[rng.integers(0, 4, (N, S))]


def site_likelihoods(nodes, pi):
    """x[..., s] = pi . node[..., s, :] (the order of the fma chain, without the fused rounding: classes do not hang on an ulp)"""
    pi = np.asarray(pi, dtype=np.float64).reshape(-1)
    with np.errstate(all='ignore'):
        x = pi[0] * nodes[..., 0]
        for a in (1, 2, 3):
            x = x + pi[a] * nodes[..., a]
    return x


def site_likelihoods_fma(node, pi):
    """x[s] of ONE row [S, 4] with the contract's roundings: pi0 v0, then three fused multiply-adds (exact rationals, rounded to
    binary64 once per step -- subnormal results included, where a product by 1/4 is no longer exact)"""
    from fractions import Fraction
    pi = [Fraction(float(v)) for v in np.asarray(pi, dtype=np.float64).reshape(-1)]
    out = np.empty(len(node))
    for s, row in enumerate(node):
        acc = float(pi[0] * Fraction(float(row[0])))
        for a in (1, 2, 3):
            acc = float(pi[a] * Fraction(float(row[a])) + Fraction(acc))
        out[s] = acc
    return out


def replay(x, T):
    """x: site likelihoods [..., S] of rows as a merge kernel walks them.  Returns the number of (row, tile, column, pair of steps)
    in each branch of the pair form (R.BRANCHES), with the running mantissa of the restatement, plus what the tests assert on
    placement: 'tail' (a special factor in the single last step of a tile), 'last' (special at site S - 1), 'col0' / 'col63'
    (special in that column), 'second' / 'first' (special as that factor of a pair), 'rows' (rows that hold a special) and
    'columns' (distinct columns that hold one)."""
    S = x.shape[-1]
    rows = x.reshape(-1, S)
    n = rows.shape[0]
    counts = {b: 0 for b in R.BRANCHES}
    counts.update(tail=0, last=0, col0=0, col63=0, first=0, second=0)
    special = ~((rows >= R.TINY) & (rows <= R.MAXF))
    counts['last'] = int(special[:, S - 1].sum())
    counts['rows'] = int(special.any(axis=1).sum())
    cols = set()
    for s0 in range(0, S, T):
        s1 = min(s0 + T, S)
        steps = (s1 - s0 + 63) // 64
        tile = np.ones((n, steps * 64))                       # a lane past the end multiplies by exactly 1.0
        tile[:, :s1 - s0] = rows[:, s0:s1]
        tile = tile.reshape(n, steps, 64)
        sp = ~((tile >= R.TINY) & (tile <= R.MAXF))
        counts['col0'] += int(sp[:, :, 0].sum())
        counts['col63'] += int(sp[:, :, 63].sum())
        cols.update(np.flatnonzero(sp.any(axis=(0, 1))).tolist())
        p = np.ones((n, 64))
        for j in range(0, steps - 1, 2):
            xa, xb = tile[:, j], tile[:, j + 1]
            br = R.branch_of(p, xa, xb)
            for i, b in enumerate(R.BRANCHES):
                counts[b] += int((br == i).sum())
            counts['first'] += int(sp[:, j].sum())
            counts['second'] += int(sp[:, j + 1].sum())
            p = R.lp_two_np(p, xa, xb, lambda v: np.zeros(v.shape))[0]
        if steps % 2 == 1:
            counts['tail'] += int(sp[:, steps - 1].sum())
    counts['columns'] = len(cols)
    return counts


def tile_values(x, T):
    """What the sum over sites makes of every (row, tile) of site likelihoods x [..., S], by the rule of a sum of logs: 0 finite,
    1 -inf (a zero factor), 2 +inf, 3 NaN (a NaN or negative factor, or a zero and an infinite one).  [..., tiles]"""
    S = x.shape[-1]
    out = []
    for s0 in range(0, S, T):
        t = x[..., s0:min(s0 + T, S)]
        zero, inf = (t == 0).any(-1), np.isposinf(t).any(-1)
        bad = (np.isnan(t) | (t < 0)).any(-1) | (zero & inf)
        out.append(np.where(bad, 3, np.where(zero, 1, np.where(inf, 2, 0))))
    return np.stack(out, axis=-1)


def rows_decided_by_the_tile_sum(x, T):
    """the rows (flat index) without a NaN tile value that hold a -inf tile value and, LATER, a +inf tile value: NaN only through the
    left-to-right sum of the tile values"""
    tv = tile_values(x, T).reshape(-1, (x.shape[-1] + T - 1) // T)
    hit = []
    for i, row in enumerate(tv):
        if (row == 3).any() or not (row == 1).any():
            continue
        if (row[int(np.argmax(row == 1)) + 1:] == 2).any():
            hit.append(i)
    return hit


def special_spread(x_r):
    """one rank event's site likelihoods [K, S] -> (particles that hold a factor that is not a positive normal number, the columns
    mod 64 -- lanes of the merge wave under the default tile, S <= 2048 -- that hold one)"""
    sp = ~((x_r >= R.TINY) & (x_r <= R.MAXF))
    return int(sp.any(axis=1).sum()), sorted({int(s) % 64 for s in np.flatnonzero(sp.any(axis=0))})


# ---- the cases of tests/test_gpu_site_product_edges.py (tests/test_site_product_host.py shows on the CPU that the oracle reaches
# their classes) ---------------------------------------------------------------------------------------------------------------
PAIR_CLASSES = R.BRANCHES                         # kept, rejected for x1, for x2, for q < 2^-1021, for q = inf
ALL = PAIR_CLASSES + ('first', 'second', 'last', 'col0', 'col63')
SWEEP_CASES = [
    # N, S, T (0: default tile), K, kinds, classes the replay must find.  Every case with a complete pair of steps reaches all five
    # pair classes, but: S = 1 and T = 64 have one step per tile, so no pair at all (inherent); at S = 65 the second step holds site
    # 64 alone, which is S - 1 and carries the special, so column 0 is the only real pair and its second factor is never normal --
    # every other lane pairs its factor with exactly 1.0, which cannot overflow: no 'inf' there (inherent).
    (6, 449, 0, 64, SPECIAL, ALL),                                                             # S - 1 alone in the last step
    (6, 449, 0, 64, FINITE, ALL),
    (6, 129, 0, 32, SPECIAL, PAIR_CLASSES + ('first', 'second', 'tail', 'last', 'col0')),      # an odd number of steps
    (6, 65, 0, 32, SPECIAL, ('kept', 'x1', 'x2', 'small', 'first', 'second', 'last', 'col0')),
    (6, 1, 0, 32, SPECIAL, ('tail', 'last', 'col0')),
    (7, 449, 64, 48, SPECIAL, ('tail', 'last', 'col0', 'col63')),                              # one step per tile: T - 1 and T
    (6, 4100, 0, 32, SPECIAL, ALL + ('tail',)),                                                # three default tiles
    (6, 300, 0, 32, ALLBAD, ALL + ('tail',)),
    (7, 449, 64, 48, TILES, ('tail', 'last', 'col0', 'col63')),                                # -inf tiles then +inf tiles, no NaN factor
    (6, 4100, 0, 32, TILES, ALL + ('tail',)),
]

# Coded leaves are one-hot: a site likelihood leaves the normal range only through the transition matrices.  phylo_set_model takes any
# positive rate; 1e155 puts the off-diagonal entries of expm(Q b) at about 1e-156, so two mismatching leaf x leaf sites of a column
# fall below 2^-1021 together, a third mismatching taxon makes the factor subnormal and a fourth makes it zero.  Probabilities never
# exceed 1: the overflow fall-back ('inf') is NOT reachable through coded leaves.  Nor is any of this under the JC69 closed form:
# 1/4 - 1/4 exp(-t) is exactly 0 for t < 2^-54, so its factors are ordinary or zero (a case below runs it for the zeros).
CODED_NEED = ('kept', 'x1', 'x2', 'small', 'first', 'second', 'last', 'col0', 'col63')
