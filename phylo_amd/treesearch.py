"""Nearest-neighbour interchanges (NNI) on sets of trees given as rows: the moves phylo_trees_nni scores,
the neighbour of a move as rows of its own, and a lockstep hill-climber over a function that scores every move of every tree
(Context.trees_nni on the device, any restatement of it in the tests) and treeopt.optimize_branches.  No device code here.

Rows: child [N-1][2], blen [N-1][2]; leaves 0 .. N-1, row i = node N + i, children from earlier rows, the last row the root."""
import numpy as np

from .treeopt import optimize_branches


def nni_moves(child):
    """the (row, side) pairs of the moves that exist: both sides of every row but the last -- 2 (N-2) -- and both sides of the last
    row when both children of the root are internal nodes"""
    child = np.asarray(child)
    R = child.shape[0]
    N = R + 1
    out = [(i, sd) for i in range(R - 1) for sd in range(2)]
    if child[R - 1, 0] >= N and child[R - 1, 1] >= N:
        out += [(R - 1, 0), (R - 1, 1)]
    return out


def _renumber(kids, lens, root, N):
    """rows of the tree below `root` (kids, lens: dicts over internal nodes), children-first, the order of children kept"""
    new, child, blen = {}, [], []
    stack = [(root, False)]
    while stack:
        v, seen = stack.pop()
        if v < N:
            continue
        if not seen:
            stack += [(v, True), (kids[v][1], False), (kids[v][0], False)]
            continue
        child.append([new.get(k, k) for k in kids[v]])
        blen.append(list(lens[v]))
        new[v] = N + len(child) - 1
    return np.array(child, dtype=np.int32).reshape(N - 1, 2), np.array(blen, dtype=np.float64).reshape(N - 1, 2)


def apply_nni(child, blen, row, side):
    """The neighbour of one tree under the move (row, side) of phylo_trees_nni, as rows (child, blen) renumbered children-first
    (after a swap a child may sit in a later row than its parent).  Every subtree keeps the length of the branch above it.

    row < N-2, v = N + row with parent p and sibling c, y = v's child on `side`, z its other child: v = (z, c), p = (v, y).
    row = N-2, v = child[N-2][0] = (a, b), c = child[N-2][1], x = c's child on `side`, w its other: v = (a, x), c = (w, b)."""
    child, blen = np.asarray(child), np.asarray(blen, dtype=np.float64)
    R = child.shape[0]
    N = R + 1
    if (int(row), int(side)) not in nni_moves(child):
        raise ValueError("no NNI move at row %d, side %d of this tree" % (row, side))
    kids = {N + i: [int(child[i, 0]), int(child[i, 1])] for i in range(R)}
    lens = {N + i: [float(blen[i, 0]), float(blen[i, 1])] for i in range(R)}
    if row < R - 1:
        v = N + row
        p, sdv = next((N + i, sd) for i in range(R) for sd in range(2) if child[i, sd] == v)
        (y, ly), (z, lz) = (kids[v][side], lens[v][side]), (kids[v][1 - side], lens[v][1 - side])
        c, lc, lv = kids[p][1 - sdv], lens[p][1 - sdv], lens[p][sdv]
        kids[v], lens[v] = [z, c], [lz, lc]
        kids[p], lens[p] = [v, y], [lv, ly]
    else:
        v, c = kids[N + row]
        b, lb = kids[v][1], lens[v][1]
        x, lx, w, lw = kids[c][side], lens[c][side], kids[c][1 - side], lens[c][1 - side]
        kids[v], lens[v] = [kids[v][0], x], [lens[v][0], lx]
        kids[c], lens[c] = [w, b], [lw, lb]
    return _renumber(kids, lens, N + R - 1, N)


def nni_search(grad_fn, nni_fn, child, blen, max_rounds=20, eps=1e-6, with_index=False, **optimize_kw):
    """Hill-climb T trees over NNI moves, all trees in lockstep.  grad_fn(child [n][N-1][2], blen) -> (loglik [n], grad, curv) and
    nni_fn(child, blen) -> (loglik [n], delta [n][N-1][2]) score any set of trees at once (Context.trees_grad with want_curv and
    Context.trees_nni, or restatements of them); optimize_kw goes to optimize_branches.  With with_index=True both are called as
    grad_fn(child, blen, idx) and nni_fn(child, blen, idx), idx [n] the indices, into the T trees given, of the trees in that
    call: what belongs to a tree (its own rate mixture, say) can follow it through the subsets the search passes.

    Every tree's lengths are climbed first.  Then, per round: one nni_fn call on all unfinished trees; per tree the move with the
    largest finite delta above eps that is not barred is applied (apply_nni); the changed trees are re-optimised in ONE lockstep
    climb; a tree keeps its move only if its optimised log-likelihood rose, otherwise it returns to its tree and lengths and the
    move is barred for it until its topology changes.  A tree with no candidate left is finished.  A tree's sequence of accepted
    log-likelihoods never falls.

    Returns a dict: 'child', 'blen' [T][N-1][2], 'loglik' [T], 'rounds' [T] (rounds in which the tree tried a move), 'moves' (per
    tree the list of accepted (row, side), each in the rows of the tree it was applied to), 'history' (per tree its accepted
    log-likelihoods, the first after the opening climb), 'converged' [T] bool (finished within max_rounds)."""
    child = np.array(child, dtype=np.int32)
    b = np.array(blen, dtype=np.float64)
    if child.ndim == 2:
        child, b = child[None], b[None]
    T = child.shape[0]
    if with_index:
        grad_of = lambda c, x, i: grad_fn(c, x, np.array(i, dtype=np.int64))     # noqa: E731
        nni_of = lambda c, x, i: nni_fn(c, x, np.array(i, dtype=np.int64))       # noqa: E731
    else:
        grad_of = lambda c, x, i: grad_fn(c, x)                                   # noqa: E731
        nni_of = lambda c, x, i: nni_fn(c, x)                                     # noqa: E731
    opt = optimize_branches(lambda x: grad_of(child, x, np.arange(T)), child, b, **optimize_kw)
    b, ll = opt['blen'], np.array(opt['loglik'], dtype=np.float64)
    history = [[float(v)] for v in ll]
    moves = [[] for _ in range(T)]
    barred = [set() for _ in range(T)]
    rounds = np.zeros(T, dtype=np.int64)
    active = np.ones(T, dtype=bool)
    for _ in range(max_rounds):
        idx = np.flatnonzero(active)
        if idx.size == 0:
            break
        _, delta = nni_of(child[idx], b[idx], idx)
        tried, new_child, new_blen = [], [], []
        for k, t in enumerate(idx):
            d = np.array(delta[k], dtype=np.float64)
            d[~np.isfinite(d)] = -np.inf
            for mv in barred[t]:
                d[mv] = -np.inf
            mv = np.unravel_index(int(np.argmax(d)), d.shape)
            if not d[mv] > eps:
                active[t] = False
                continue
            mv = (int(mv[0]), int(mv[1]))
            c2, b2 = apply_nni(child[t], b[t], *mv)
            tried.append((t, mv))
            new_child.append(c2)
            new_blen.append(b2)
        if not tried:
            break
        new_child = np.array(new_child)
        who = [t for t, _ in tried]
        o = optimize_branches(lambda x: grad_of(new_child, x, who), new_child, np.array(new_blen), **optimize_kw)
        for k, (t, mv) in enumerate(tried):
            rounds[t] += 1
            if o['loglik'][k] > ll[t]:
                child[t], b[t], ll[t] = new_child[k], o['blen'][k], o['loglik'][k]
                barred[t] = set()
                moves[t].append(mv)
                history[t].append(float(ll[t]))
            else:
                barred[t].add(mv)
    return {'child': child, 'blen': b, 'loglik': ll, 'rounds': rounds, 'moves': moves, 'history': history, 'converged': ~active}
