"""Trees for the tests of phylo_trees_loglik, as rows (child [N-1][2], blen [N-1][2]; leaves 0 .. N-1, row i = node N + i, the
last row the root), and their translation to the node arrays phylo_tree_loglik and the oracles take."""
import numpy as np


def lengths(n, rng, zeros=True):
    """Exp-distributed lengths, some of them zero -- on right-hand branches only: two leaves joined through zero-length branches
    alone would give every site at which they differ the likelihood 0"""
    b = rng.exponential(0.1, (n - 1, 2))
    if zeros and n > 2:
        b[rng.choice(n - 1, max(1, n // 8), replace=False), 1] = 0.0
    return b


def random_rows(n, rng, zeros=True):
    """a random topology: two random roots of the forest are joined until one is left (rows in that order)"""
    roots = list(rng.permutation(n))
    child = []
    for i in range(n - 1):
        a = roots.pop(rng.integers(0, len(roots)))
        b = roots.pop(rng.integers(0, len(roots)))
        child.append((a, b))
        roots.append(n + i)
    return np.array(child, dtype=np.int32).reshape(n - 1, 2), lengths(n, rng, zeros)


def caterpillar_rows(n, rng):
    child = [(0, 1)] + [(n + i - 1, i + 1) for i in range(1, n - 1)]
    return np.array(child, dtype=np.int32).reshape(n - 1, 2), lengths(n, rng)


def balanced_rows(n, rng):
    child = []

    def build(lo, hi):
        if hi - lo == 1:
            return lo
        mid = (lo + hi + 1) // 2
        a, b = build(lo, mid), build(mid, hi)
        child.append((a, b))
        return n + len(child) - 1

    build(0, n)
    return np.array(child, dtype=np.int32).reshape(n - 1, 2), lengths(n, rng)


def rows_to_nodes(child, blen):
    """(left, right, bl, br) over 2N-1 nodes, root 2N-2: what phylo_tree_loglik and the oracles' tree_loglik take"""
    n = child.shape[0] + 1
    left = np.full(2 * n - 1, -1, dtype=np.int32)
    right = left.copy()
    bl, br = np.zeros(2 * n - 1), np.zeros(2 * n - 1)
    left[n:], right[n:] = child[:, 0], child[:, 1]
    bl[n:], br[n:] = blen[:, 0], blen[:, 1]
    return left, right, bl, br


def nodes_to_rows(left, right, bl, br, root, n):
    """the reverse, for node arrays in any numbering: the internal nodes below `root` children-first, renumbered N, N+1, ..."""
    new = {i: i for i in range(n)}
    child, blen = [], []
    stack = [(int(root), False)]
    while stack:
        v, seen = stack.pop()
        if v < n:
            continue
        if not seen:
            stack += [(v, True), (int(right[v]), False), (int(left[v]), False)]
            continue
        child.append((new[int(left[v])], new[int(right[v])]))
        blen.append((float(bl[v]), float(br[v])))
        new[v] = n + len(child) - 1
    return np.array(child, dtype=np.int32).reshape(n - 1, 2), np.array(blen, dtype=np.float64).reshape(n - 1, 2)
