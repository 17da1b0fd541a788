"""Host side of phylo_trees_loglik, no GPU: Newick <-> rows, the checks on a tree, the slot schedule
the kernel walks (depth bound; replayed in NumPy against the CPU oracle) and the trees of a sweep's final particles."""
import math

import numpy as np
import pytest

from oracle import cpu_ref as O
from phylo_amd import _ffi, treepost
from trees_cases import balanced_rows, caterpillar_rows, random_rows, rows_to_nodes

TAXA = ['A', 'B', 'C', 'D', 'E']


def clade_lengths(child, blen, n):
    """{frozenset of leaves below a non-root node -> length of the branch above it}"""
    below = [frozenset([i]) for i in range(n)]
    out = {}
    for (a, b), (x, y) in zip(child, blen):
        out[below[a]], out[below[b]] = float(x), float(y)
        below.append(below[a] | below[b])
    return out


def test_newick_rows_round_trip():
    nw = '((A:0.1,B:0.25):0.5,((C:1e-3,D:2):0,E:0.7):0.125);'
    child, blen = treepost.newick_to_rows(nw, TAXA)
    assert child.dtype == np.int32 and child.shape == (4, 2) and blen.shape == (4, 2)
    np.testing.assert_array_equal(child, [[0, 1], [2, 3], [6, 4], [5, 7]])
    np.testing.assert_array_equal(blen, [[0.1, 0.25], [1e-3, 2.0], [0.0, 0.7], [0.5, 0.125]])
    back = treepost.rows_to_newick(child, blen, TAXA)
    c2, b2 = treepost.newick_to_rows(back, TAXA)
    np.testing.assert_array_equal(c2, child)
    assert np.array_equal(b2.view(np.uint64), blen.view(np.uint64))
    # internal labels and a root length are skipped; the reader of the summaries sees the same branches
    nw2 = '((A:0.1,B:0.25)0.93:0.5,((C:1e-3,D:2)1:0,E:0.7)0.5:0.125):0.3;'
    c3, b3 = treepost.newick_to_rows(nw2, TAXA)
    np.testing.assert_array_equal(c3, child)
    np.testing.assert_array_equal(b3, blen)
    nb = treepost.newick_branches(nw, TAXA)
    got = clade_lengths(child, blen, 5)
    assert {(k if isinstance(k, frozenset) else frozenset([k])): v for k, v in nb.items()} == got
    # rows that are not numbered in Newick order: the round trip keeps the tree, bit for bit in the lengths
    rng = np.random.default_rng(5)
    for n in (2, 3, 7, 40):
        child, blen = random_rows(n, rng)
        taxa = ['t%d' % i for i in range(n)]
        c2, b2 = treepost.newick_to_rows(treepost.rows_to_newick(child, blen, taxa), taxa)
        assert clade_lengths(c2, b2, n) == clade_lengths(child, blen, n)


def test_polytomy_is_resolved_left_to_right_with_zero_lengths():
    child, blen = treepost.newick_to_rows('(A:1,B:2,C:3,(D:4,E:5):6);', TAXA)
    np.testing.assert_array_equal(child, [[3, 4], [0, 1], [6, 2], [7, 5]])
    np.testing.assert_array_equal(blen, [[4, 5], [1, 2], [0, 3], [0, 6]])
    # the consensus tree of a run is such a tree
    child, blen = treepost.newick_to_rows('((A:1,B:1,C:1)0.8:0.5,D:1,E:2);', TAXA)
    np.testing.assert_array_equal(child, [[0, 1], [5, 2], [6, 3], [7, 4]])
    np.testing.assert_array_equal(blen, [[1, 1], [0, 1], [0.5, 1], [0, 2]])


@pytest.mark.parametrize("nw, what", [
    ('((A:1,B:1):1,((C:1,A:1):1,E:1):1);', 'twice'),              # a leaf used twice
    ('((A:1,B:1):1,(C:1,D:1):1);', 'missing'),                    # a taxon missing
    ('((A:1,B:1):1,((C:1,D):1,E:1):1);', 'no length'),            # a missing length on a leaf
    ('((A:1,B:1),((C:1,D:1):1,E:1):1);', 'no length'),            # ... on an internal branch
    ('((A:1,B:1):1,((C:1,D:-1):1,E:1):1);', '>= 0'),
    ('((A:1,B:1):1,((C:1,D:nan):1,E:1):1);', '>= 0'),
    ('((A:1,B:1):1,((C:1,X:1):1,E:1):1);', 'unknown taxon'),
    ('((A:1,B:1):1,((C:1,D:1):1,(E:1):1):1);', 'one child'),
    ('((A:1,B:1):1,((C:1,D:1):1,E:1):1;', 'malformed'),
])
def test_newick_to_rows_rejects(nw, what):
    with pytest.raises(ValueError, match=what):
        treepost.newick_to_rows(nw, TAXA)


GOOD_CHILD = np.array([[0, 1], [2, 3], [6, 4], [5, 7]], dtype=np.int32)
GOOD_BLEN = np.full((4, 2), 0.1)


def bad_rows():
    c = GOOD_CHILD.copy(); c[2] = [6, 0]
    yield 'leaf twice', c, GOOD_BLEN, 2, 'twice'
    c = GOOD_CHILD.copy(); c[1] = [2, 2]
    yield 'missing taxon', c, GOOD_BLEN, 1, 'twice'               # taxon 3 is missing: another node takes its place
    c = GOOD_CHILD.copy(); c[0] = [0, 6]; c[2] = [1, 4]
    yield 'later row', c, GOOD_BLEN, 0, 'earlier row'
    c = GOOD_CHILD.copy(); c[3] = [5, 8]
    yield 'itself', c, GOOD_BLEN, 3, 'earlier row'
    c = GOOD_CHILD.copy(); c[1] = [2, -1]
    yield 'negative', c, GOOD_BLEN, 1, 'earlier row'
    c = GOOD_CHILD.copy(); c[3] = [5, 5]
    yield 'node twice', c, GOOD_BLEN, 3, 'twice'
    for name, v in (('nan', np.nan), ('negative length', -1e-9), ('inf', np.inf)):
        b = GOOD_BLEN.copy(); b[2, 1] = v
        yield name, GOOD_CHILD, b, 2, '>= 0'


@pytest.mark.parametrize("name, child, blen, row, what", list(bad_rows()), ids=[b[0] for b in bad_rows()])
def test_library_and_python_checks_reject_the_same_rows(name, child, blen, row, what):
    with pytest.raises(_ffi.PhyloError) as e:
        _ffi.debug_tree_schedule(child, blen)
    assert e.value.code == -1 and 'tree 0, row %d' % row in str(e.value) and what in str(e.value)
    with pytest.raises(ValueError, match='row %d' % row):
        treepost.check_rows(child, blen)
    ops, depth = _ffi.debug_tree_schedule(GOOD_CHILD, GOOD_BLEN)   # a refusal leaves nothing behind
    assert depth == 2 and sorted(ops[:, 3]) == [0, 1, 2, 3]


def replay(ops, depth, child, blen, Q, prior, leaves):
    """the kernel's walk: a stack of `depth` slots, the operations in order, the destination written after both sources are read"""
    n = leaves.shape[0]
    stack = [None] * depth
    done = set()
    out = None
    for dst, l, r, row in ops:
        a, b = child[row]
        for src, ch in ((l, a), (r, b)):                   # a source is the child itself (a leaf) or the slot that holds it
            assert (src == ch) if ch < n else (src < 0 and (ch - n) in done)
        L = leaves[l] if l >= 0 else stack[~l]
        R = leaves[r] if r >= 0 else stack[~r]
        assert L is not None and R is not None and 0 <= dst < depth
        out = O.conditional_likelihood(Q, L, R, blen[row, 0], blen[row, 1])
        if l < 0:
            stack[~l] = None
        if r < 0:
            stack[~r] = None
        assert stack[dst] is None, "a live slot is overwritten"
        stack[dst] = out
        done.add(int(row))
    assert int(ops[-1][3]) == n - 2 and len(done) == n - 1
    return float(np.sum(np.log(np.dot(prior, out.T))))


def schedule_cases():
    rng = np.random.default_rng(11)
    for n in (2, 3, 5, 64, 65, 512):
        yield 'caterpillar-%d' % n, caterpillar_rows(n, rng)
        yield 'balanced-%d' % n, balanced_rows(n, rng)
        for j in range(3):
            yield 'random-%d-%d' % (n, j), random_rows(n, rng)


@pytest.mark.parametrize("name, rows", list(schedule_cases()), ids=[c[0] for c in schedule_cases()])
def test_slot_schedule_depth_and_replay(name, rows):
    child, blen = rows
    n = child.shape[0] + 1
    ops, depth = _ffi.debug_tree_schedule(child, blen)
    assert 1 <= depth <= int(math.floor(math.log2(n))) + 1
    assert ops[:, 0].min() >= 0 and ops[:, 0].max() == depth - 1
    if name.startswith('caterpillar'):
        assert depth == 1
    if name.startswith('balanced') and n & (n - 1) == 0:
        assert depth == int(math.log2(n))
    rng = np.random.default_rng(n)
    S = 3
    states = np.tile(rng.integers(0, 4, S), (n, 1))                   # similar sequences: 512 random ones underflow a double
    mut = rng.random((n, S)) < 0.05
    states[mut] = rng.integers(0, 4, int(mut.sum()))
    leaves = np.eye(4)[states]
    leaves[rng.integers(0, n), 0] = 1.0                              # a gap
    Q = O.get_Q(rng.normal(size=(4, 4)))
    prior = np.array([0.1, 0.2, 0.3, 0.4])
    got = replay(ops, depth, child, blen, Q, prior, leaves)
    left, right, bl, br = rows_to_nodes(child, blen)
    ref, _ = O.tree_loglik(Q, prior, 2 * n - 1, left, right, bl, br, 2 * n - 2, leaves)
    assert np.isfinite(ref) and got == pytest.approx(ref, rel=1e-12)


def test_particle_trees_on_a_hand_made_genealogy():
    # N = 4, K = 3.  Rank event 0: every particle merges slots (a, b) of the table [0, 1, 2, 3]
    merges = np.array([[[0, 1], [2, 3], [1, 3]],
                       [[2, 0], [0, 2], [1, 2]],
                       [[0, 1], [1, 0], [0, 1]]], dtype=np.int32)
    ancestors = np.array([[1, 1, 0], [2, 0, 0]], dtype=np.int64)
    lb = np.array([[.1, .2, .3], [.4, .5, .6], [.7, .8, .9]])
    rb = lb + 10.0
    # the slots that stay, in the order they keep (the new node goes last)
    remaining = [np.array([[2, 3], [0, 1], [2, 0]]), np.array([[1], [1], [0]]), np.zeros((3, 0), dtype=np.int64)]
    child, blen = treepost.particle_trees(merges, ancestors, lb, rb, remaining=remaining)
    # after rank event 0: tables p0 [2,3,4], p1 [0,1,4], p2 [2,0,4] with nodes 4 = (0,1), (2,3), (1,3)
    # rank event 1 adopts (1,1,0): p0 <- old p1 [0,1,4]: merges slots (2,0) -> node 5 = (4, 0), table [1,5]
    #                              p1 <- old p1 [0,1,4]: slots (0,2) -> 5 = (0, 4), table [1,5]
    #                              p2 <- old p0 [2,3,4]: slots (1,2) -> 5 = (3, 4), table [2,5]
    # rank event 2 adopts (2,0,0): p0 <- p2: (2,5); p1 <- p0: slots (1,0) -> (5,1); p2 <- p0: (1,5)
    np.testing.assert_array_equal(child[0], [[0, 1], [3, 4], [2, 5]])
    np.testing.assert_array_equal(child[1], [[2, 3], [4, 0], [5, 1]])
    np.testing.assert_array_equal(child[2], [[2, 3], [4, 0], [1, 5]])
    np.testing.assert_array_equal(blen[0], [[.1, 10.1], [.6, 10.6], [.7, 10.7]])
    np.testing.assert_array_equal(blen[1], [[.2, 10.2], [.4, 10.4], [.8, 10.8]])
    np.testing.assert_array_equal(blen[2], [[.2, 10.2], [.4, 10.4], [.9, 10.9]])
    for k in range(3):
        treepost.check_rows(child[k], blen[k])
        _ffi.debug_tree_schedule(child[k], blen[k])
    # without `remaining` and `seed`: descending slots (the twisted proposal's rule)
    c2, _ = treepost.particle_trees(merges[:, :1], ancestors[:, :1] * 0, lb[:, :1], rb[:, :1])
    # p0: (0,1) -> [3,2,4]; slots (2,0) -> (4,3) -> [2,5]; (0,1) -> (2,5)
    np.testing.assert_array_equal(c2[0], [[0, 1], [4, 3], [2, 5]])
    # N = 2: one rank event, no resampling
    c3, b3 = treepost.particle_trees(np.array([[[1, 0]]]), np.zeros((0, 1)), np.array([[.5]]), np.array([[.25]]))
    np.testing.assert_array_equal(c3, [[[1, 0]]])
    np.testing.assert_array_equal(b3, [[[.5, .25]]])
