"""Host side of the tree posterior summary (VCSMC.tree_posterior; the device tables come from phylo_tree_summary, DESIGN.md
section 10): clades in taxon names with their support, topologies with probability, count, representative and Newick, the
majority-rule consensus tree, credible sets, and a Newick reader that turns a rooted tree back into its clade set; and explicit
trees as the rows Context.trees_loglik scores: from and to Newick, and from a sweep's final particles."""
from __future__ import annotations

import json
import os

import numpy as np


def bits_to_indices(row):
    """taxon indices of one clade bitset (uint64 words, taxon i = bit i % 64 of word i // 64)"""
    out = []
    for w, word in enumerate(np.asarray(row, dtype=np.uint64).reshape(-1)):
        x = int(word)
        while x:
            low = x & -x
            out.append(64 * w + low.bit_length() - 1)
            x ^= low
    return out


def group_table(tab, g=0):
    """Group g's rows of Context.tree_summary()'s tables (a plain sweep has one group)."""
    c0, c1 = int(tab['clade_offsets'][g]), int(tab['clade_offsets'][g + 1])
    t0, t1 = int(tab['topo_offsets'][g]), int(tab['topo_offsets'][g + 1])
    Kg = tab['u'].size // tab['G']
    extra = {}
    if 'clade_stats' in tab:                               # Context.tree_branches()'s tables, merged into tab by the caller
        extra = {'clade_stats': tab['clade_stats'][c0:c1], 'leaf_stats': tab['leaf_stats'][g],
                 'topo_clades': tab['topo_clades'][t0:t1], 'topo_stats': tab['topo_stats'][t0:t1]}
    return {**extra, 'clade_bits': tab['clade_bits'][c0:c1], 'clade_weight': tab['clade_weight'][c0:c1],
            'topo_weight': tab['topo_weight'][t0:t1], 'topo_count': tab['topo_count'][t0:t1], 'topo_rep': tab['topo_rep'][t0:t1],
            'particle_topo': tab['particle_topo'][g * Kg:(g + 1) * Kg], 'u': tab['u'][g * Kg:(g + 1) * Kg], 'U': int(tab['U'][g])}


def _support_label(s, digits):
    return '%.*g' % (digits, s)


def consensus_newick(taxa, clades, threshold=0.5, digits=4):
    """Majority-rule consensus of a clade table as Newick: the clades (taxon-index collections with their support) whose support
    is strictly greater than `threshold`, nested by inclusion, supports as internal-node labels, the root unlabelled, children in
    order of their smallest taxon index.  Clades above 0.5 are pairwise compatible; below that an incompatible pair raises
    ValueError.  No clade above the threshold gives the star tree."""
    n = len(taxa)
    chosen = []
    for members, support in clades:
        m = frozenset(int(i) for i in members)
        if 2 <= len(m) < n and support > threshold:
            chosen.append((m, float(support)))
    chosen.sort(key=lambda cs: (-len(cs[0]), min(cs[0])))
    for i, (a, _) in enumerate(chosen):
        for b, _ in chosen[:i]:
            if not (a <= b or a.isdisjoint(b)):
                raise ValueError("clades %s and %s are incompatible: no tree holds both (threshold %g < 0.5)"
                                 % (sorted(a), sorted(b), threshold))
    nodes = [frozenset(range(n))] + [m for m, _ in chosen]
    support = [None] + [s for _, s in chosen]

    def parent(m):
        best = 0
        for j in range(1, len(nodes)):
            if m < nodes[j] and len(nodes[j]) < len(nodes[best]):
                best = j
        return best

    children = [[] for _ in nodes]
    for j in range(1, len(nodes)):
        children[parent(nodes[j])].append((min(nodes[j]), j))
    for i in range(n):
        children[parent(frozenset([i]))].append((i, -1 - i))

    def render(j):
        parts = []
        for _, x in sorted(children[j]):
            parts.append(str(taxa[-1 - x]) if x < 0 else render(x) + _support_label(support[x], digits))
        return '(' + ','.join(parts) + ')'

    return render(0) + ';'


def newick_clades(newick, taxa):
    """The non-trivial clades (frozensets of taxon indices, sizes 2 .. N-1) of a rooted Newick tree over `taxa`; branch lengths
    and internal-node labels are skipped."""
    index = {str(t): i for i, t in enumerate(taxa)}
    s = newick.strip()
    if s.endswith(';'):
        s = s[:-1]
    pos = 0
    found = []

    def skip_annotation():
        nonlocal pos
        while pos < len(s) and s[pos] not in ',()':
            pos += 1

    def node():
        nonlocal pos
        if s[pos] == '(':
            pos += 1
            members = set()
            while True:
                members |= node()
                if pos < len(s) and s[pos] == ',':
                    pos += 1
                    continue
                if pos < len(s) and s[pos] == ')':
                    pos += 1
                    break
                raise ValueError("malformed Newick at %d: %r" % (pos, s[pos:pos + 20]))
            skip_annotation()
            found.append(frozenset(members))
            return members
        start = pos
        while pos < len(s) and s[pos] not in ',():':
            pos += 1
        name = s[start:pos]
        skip_annotation()
        if name not in index:
            raise ValueError("unknown taxon %r in Newick" % name)
        return {index[name]}

    node()
    if pos != len(s):
        raise ValueError("trailing characters in Newick: %r" % s[pos:])
    n = len(taxa)
    return {c for c in found if 2 <= len(c) < n}


def newick_branches(newick, taxa):
    """{clade (frozenset of taxon indices) or leaf (taxon index) -> length of the branch above it} of a rooted Newick tree over
    `taxa`; nodes without a ':length' (the root, or a branch with no estimate) are absent.  Internal-node labels are skipped."""
    index = {str(t): i for i, t in enumerate(taxa)}
    s = newick.strip()
    if s.endswith(';'):
        s = s[:-1]
    pos = 0
    out = {}

    def annotation(key):
        nonlocal pos
        start = pos
        while pos < len(s) and s[pos] not in ',()':
            pos += 1
        text = s[start:pos]
        if ':' in text:
            out[key] = float(text.split(':', 1)[1])

    def node():
        nonlocal pos
        if s[pos] == '(':
            pos += 1
            members = set()
            while True:
                members |= node()
                if pos < len(s) and s[pos] == ',':
                    pos += 1
                    continue
                if pos < len(s) and s[pos] == ')':
                    pos += 1
                    break
                raise ValueError("malformed Newick at %d: %r" % (pos, s[pos:pos + 20]))
            annotation(frozenset(members))
            return members
        start = pos
        while pos < len(s) and s[pos] not in ',():':
            pos += 1
        name = s[start:pos]
        if name not in index:
            raise ValueError("unknown taxon %r in Newick" % name)
        annotation(index[name])
        return {index[name]}

    node()
    if pos != len(s):
        raise ValueError("trailing characters in Newick: %r" % s[pos:])
    return out


def newick_to_rows(newick, taxa):
    """A rooted Newick tree over `taxa` as the rows Context.trees_loglik takes: (child [N-1][2] int32, blen [N-1][2] float64);
    leaves are nodes 0 .. N-1 in the order of `taxa`, row i is internal node N + i (numbered as its closing bracket is met, so
    children come from earlier rows) and the last row is the root.  A node with more than two children is resolved left to
    right with zero-length branches: (A:a,B:b,C:c) reads ((A:a,B:b):0,C:c).  Every branch needs its ':length' (ValueError
    otherwise; a length at the root is ignored), every taxon appears exactly once, internal-node labels are skipped."""
    index = {str(t): i for i, t in enumerate(taxa)}
    n = len(index)
    s = newick.strip()
    if s.endswith(';'):
        s = s[:-1]
    pos = 0
    child, blen, seen = [], [], set()

    def annotation(what, needed):
        nonlocal pos
        start = pos
        while pos < len(s) and s[pos] not in ',()':
            pos += 1
        text = s[start:pos]
        if ':' not in text:
            if needed:
                raise ValueError("the branch above %s has no length" % what)
            return None
        x = float(text.split(':', 1)[1])
        if not (x >= 0.0 and x != float('inf')):
            raise ValueError("the branch above %s has length %r: need a finite number >= 0" % (what, x))
        return x

    def node(is_root):
        nonlocal pos
        if pos < len(s) and s[pos] == '(':
            pos += 1
            kids = []
            while True:
                kids.append(node(False))
                if pos < len(s) and s[pos] == ',':
                    pos += 1
                    continue
                if pos < len(s) and s[pos] == ')':
                    pos += 1
                    break
                raise ValueError("malformed Newick at %d: %r" % (pos, s[pos:pos + 20]))
            if len(kids) < 2:
                raise ValueError("an internal node with one child at %d" % pos)
            cur = kids[0]
            for nxt in kids[1:-1]:                         # a polytomy: join left to right under zero-length branches
                child.append((cur[0], nxt[0]))
                blen.append((cur[1], nxt[1]))
                cur = (n + len(child) - 1, 0.0)
            child.append((cur[0], kids[-1][0]))
            blen.append((cur[1], kids[-1][1]))
            me = n + len(child) - 1
            return me, annotation("node %d" % me, not is_root)
        start = pos
        while pos < len(s) and s[pos] not in ',():':
            pos += 1
        name = s[start:pos]
        if name not in index:
            raise ValueError("unknown taxon %r in Newick" % name)
        if name in seen:
            raise ValueError("taxon %r appears twice" % name)
        seen.add(name)
        return index[name], annotation("taxon %r" % name, not is_root)

    node(True)
    if pos != len(s):
        raise ValueError("trailing characters in Newick: %r" % s[pos:])
    if len(seen) != n:
        raise ValueError("taxa missing from the Newick: %s" % sorted(set(index) - seen))
    return np.array(child, dtype=np.int32).reshape(n - 1, 2), np.array(blen, dtype=np.float64).reshape(n - 1, 2)


def check_rows(child, blen, n=None):
    """The checks phylo_trees_loglik makes on one tree, in Python: ValueError naming the row."""
    child, blen = np.asarray(child), np.asarray(blen, dtype=np.float64)
    n = child.shape[0] + 1 if n is None else n
    if child.shape != (n - 1, 2) or blen.shape != (n - 1, 2):
        raise ValueError("child and blen must be [N-1][2]")
    used = set()
    for i in range(n - 1):
        for c, b in zip(child[i], blen[i]):
            c = int(c)
            if not 0 <= c < n + i:
                raise ValueError("row %d: child %d is neither a leaf nor a node of an earlier row" % (i, c))
            if c in used:
                raise ValueError("row %d: node %d is a child twice" % (i, c))
            used.add(c)
            if not (b >= 0.0 and np.isfinite(b)):
                raise ValueError("row %d: branch length %r is not a finite number >= 0" % (i, float(b)))


def rows_to_newick(child, blen, taxa):
    """The inverse of newick_to_rows: the Newick string of (child, blen), lengths written so that they read back bit for bit
    (repr), children in row order, the root bare."""
    child, blen = np.asarray(child), np.asarray(blen, dtype=np.float64)
    n = len(taxa)
    check_rows(child, blen, n)
    text = [str(t) for t in taxa] + [None] * (n - 1)
    for i in range(n - 1):                                 # rows are children-first: no recursion
        (a, b), (x, y) = child[i], blen[i]
        text[n + i] = '(%s:%s,%s:%s)' % (text[a], repr(float(x)), text[b], repr(float(y)))
    return text[2 * n - 2] + ';'


def particle_trees(merges, ancestors, lbranch, rbranch, remaining=None, seed=None):
    """The K final particles' trees of a fetched sweep as rows: (child [K][N-1][2] int32, blen [K][N-1][2]).  merges [N-1][K][2]
    (root-table slots coalesced at each rank event), ancestors [N-2][K] (resampling indices before rank events 1 .. N-2),
    lbranch / rbranch [N-1][K].  Row r of particle k is the node its lineage created at rank event r, numbered N + r.  The slots
    that stay move to the front of the table and the new node goes last; their order is `remaining` (one [K][n-2] array of slots
    per rank event), else the plain proposal's pair-order contract for `seed` (phylo_amd.rng.pair_order), else -- both None --
    descending slots, the twisted proposal's rule."""
    merges = np.asarray(merges)
    R, K = merges.shape[0], merges.shape[1]
    N = R + 1
    anc = np.asarray(ancestors).reshape(max(R - 1, 0), K)
    lb, rb = np.asarray(lbranch, dtype=np.float64), np.asarray(rbranch, dtype=np.float64)
    tab = np.tile(np.arange(N, dtype=np.int32), (K, 1))
    child = np.zeros((K, R, 2), dtype=np.int32)
    blen = np.zeros((K, R, 2), dtype=np.float64)
    rows = np.arange(K)
    for r in range(R):
        if r > 0:
            idx = anc[r - 1]
            tab, child, blen = tab[idx], child[idx], blen[idx]
        n = N - r
        co = merges[r].astype(np.int64)
        if remaining is not None:
            rem = np.asarray(remaining[r], dtype=np.int64).reshape(K, n - 2)
        elif seed is not None:
            from . import rng
            pick, rem = rng.pair_order(K, n, seed, r)
            if not np.array_equal(pick, merges[r]):
                raise ValueError("rank event %d: merges are not the pair picks of seed %r" % (r, seed))
            rem = rem.astype(np.int64)
        else:
            rem = np.array([[i for i in range(n - 1, -1, -1) if i != a and i != b] for a, b in co], dtype=np.int64).reshape(K, n - 2)
        child[:, r, 0], child[:, r, 1] = tab[rows, co[:, 0]], tab[rows, co[:, 1]]
        blen[:, r, 0], blen[:, r, 1] = lb[r], rb[r]
        tab = np.concatenate([np.take_along_axis(tab, rem, axis=1), np.full((K, 1), N + r, dtype=np.int32)], axis=1)
    return child, blen


def branch_summary(stats, weight):
    """mean, sd, min, max of one branch from its (S1, S2, min, max) row and the integer weight C it was summed over: mean = S1 / C,
    variance = max(S2 / C - mean^2, 0); C = 0 (held only by particles of integer weight 0) has no estimate: mean and sd None."""
    s1, s2, lo, hi = (float(x) for x in stats)
    if int(weight) == 0:
        return {'mean': None, 'sd': None, 'min': lo, 'max': hi}
    c = float(int(weight))
    mean = s1 / c
    return {'mean': mean, 'sd': max(s2 / c - mean * mean, 0.0) ** 0.5, 'min': lo, 'max': hi}


def _length(mean, digits):
    return '' if mean is None else ':%.*g' % (digits, mean)


def tree_newick(taxa, clades, leaf_means, labels=None, digits=6, label_digits=4):
    """Newick of the tree whose non-trivial clades are `clades` = [(frozenset of taxon indices, mean length or None)] (pairwise
    compatible), with ':mean' on every edge that has an estimate (leaf_means[i] above taxon i); labels: {clade: support} printed
    as internal-node labels.  Children in order of their smallest taxon index, the root bare."""
    n = len(taxa)
    nodes = [frozenset(range(n))] + [m for m, _ in sorted(clades, key=lambda cm: (-len(cm[0]), min(cm[0])))]
    mean = dict(clades)

    def parent(m):
        best = 0
        for j in range(1, len(nodes)):
            if m < nodes[j] and len(nodes[j]) < len(nodes[best]):
                best = j
        return best

    children = [[] for _ in nodes]
    for j in range(1, len(nodes)):
        children[parent(nodes[j])].append((min(nodes[j]), j))
    for i in range(n):
        children[parent(frozenset([i]))].append((i, -1 - i))

    def render(j):
        parts = []
        for _, x in sorted(children[j]):
            if x < 0:
                parts.append(str(taxa[-1 - x]) + _length(leaf_means[-1 - x], digits))
            else:
                lab = '' if labels is None else _support_label(labels[nodes[x]], label_digits)
                parts.append(render(x) + lab + _length(mean[nodes[x]], digits))
        return '(' + ','.join(parts) + ')'

    return render(0) + ';'


class TreePosterior:
    """The summary of one sweep's (or one group's) weighted final particles.

    clades       [(sorted taxon-name tuple, support)], support = C / U, by C descending then bitset ascending
    clade_sets   [(frozenset of taxon indices, support)], same order
    topologies   [dict(probability, weight, count, representative, newick)], by T descending then representative ascending
    particle_topology  [K] index of every particle's topology in `topologies`
    consensus    majority-rule consensus (clades with support > threshold) as Newick with supports as labels
    map          the most probable topology (topologies[0])"""

    def __init__(self, taxa, table, newicks=None, threshold=0.5):
        self.taxa = [str(t) for t in taxa]
        self.threshold = float(threshold)
        self.U = int(table['U'])
        U = float(self.U)
        self.clade_sets, self.clades = [], []
        for row, w in zip(table['clade_bits'], table['clade_weight']):
            idx = bits_to_indices(row)
            sup = float(int(w)) / U
            self.clade_sets.append((frozenset(idx), sup))
            self.clades.append((tuple(sorted(self.taxa[i] for i in idx)), sup))
        self.topologies = []
        for w, n, r in zip(table['topo_weight'], table['topo_count'], table['topo_rep']):
            self.topologies.append({'probability': float(int(w)) / U, 'weight': int(w), 'count': int(n), 'representative': int(r),
                                    'newick': None if newicks is None else newicks[int(r)]})
        self.particle_topology = np.asarray(table['particle_topo'])
        self.consensus = consensus_newick(self.taxa, self.clade_sets, self.threshold)
        self.map = self.topologies[0] if self.topologies else None
        if 'clade_stats' in table:
            self._add_branches(table)

    def _add_branches(self, table):
        """branch lengths (Context.tree_branches): per clade the branch above it, per taxon the pendant branch, per topology its
        clade rows and conditional means, the consensus and the MAP topology with mean lengths"""
        n = len(self.taxa)
        self.clade_branches = [branch_summary(st, w) for st, w in zip(table['clade_stats'], table['clade_weight'])]
        leaves = [branch_summary(st, self.U) for st in table['leaf_stats']]
        self.leaf_branches = {self.taxa[i]: leaves[i] for i in range(n)}
        for t, rows, st in zip(self.topologies, table['topo_clades'], table['topo_stats']):
            br = [branch_summary(x, t['weight']) for x in st]
            t['clades'] = [int(j) for j in rows]
            t['leaf_means'] = [b['mean'] for b in br[:n]]
            t['clade_means'] = [b['mean'] for b in br[n:]]
        chosen = [(m, self.clade_branches[j]['mean']) for j, (m, s) in enumerate(self.clade_sets)
                  if 2 <= len(m) < n and s > self.threshold]
        self.consensus_bl = tree_newick(self.taxa, chosen, [b['mean'] for b in leaves], labels=dict(self.clade_sets))
        self.map_newick = None
        if self.map is not None:
            t = self.map
            self.map_newick = tree_newick(self.taxa, [(self.clade_sets[j][0], m) for j, m in zip(t['clades'], t['clade_means'])],
                                          t['leaf_means'])

    def branches_json(self):
        return {'taxa': self.taxa, 'total_weight': self.U,
                'clades': [dict(taxa=list(names), support=s, **b) for (names, s), b in zip(self.clades, self.clade_branches)],
                'leaves': self.leaf_branches,
                'topologies': [{'probability': t['probability'], 'clades': t['clades'], 'leaf_means': t['leaf_means'],
                                'clade_means': t['clade_means']} for t in self.topologies],
                'consensus_bl': self.consensus_bl, 'map_newick': self.map_newick}

    def write_branches(self, save_dir):
        """consensus_bl.tre, map.tre and tree_branches.json in save_dir (a posterior built with branch lengths)"""
        with open(os.path.join(save_dir, 'tree_branches.json'), 'w') as f:
            json.dump(self.branches_json(), f, indent=1)
        with open(os.path.join(save_dir, 'consensus_bl.tre'), 'w') as f:
            f.write(self.consensus_bl + '\n')
        with open(os.path.join(save_dir, 'map.tre'), 'w') as f:
            f.write((self.map_newick or '') + '\n')

    def credible_set(self, p):
        """The fewest most probable topologies (table order: probability descending, ties by smallest representative) whose
        probabilities add up to at least p; at least one topology."""
        if not 0.0 <= p <= 1.0:
            raise ValueError("p must lie in [0, 1], got %r" % (p,))
        out, acc = [], 0
        for t in self.topologies:
            if out and acc >= p * self.U:
                break
            out.append(t)
            acc += t['weight']
        return out

    def to_json(self):
        def plain(t):                                      # (the branch-length keys go to tree_branches.json)
            return {k: t[k] for k in ('probability', 'weight', 'count', 'representative', 'newick')}

        return {'taxa': self.taxa, 'threshold': self.threshold, 'total_weight': self.U,
                'clades': [{'taxa': list(names), 'support': s} for names, s in self.clades],
                'topologies': [plain(t) for t in self.topologies], 'consensus': self.consensus,
                'map': None if self.map is None else plain(self.map)}

    def write(self, save_dir):
        """tree_posterior.json (everything above) and consensus.tre (the consensus Newick) in save_dir"""
        with open(os.path.join(save_dir, 'tree_posterior.json'), 'w') as f:
            json.dump(self.to_json(), f, indent=1)
        with open(os.path.join(save_dir, 'consensus.tre'), 'w') as f:
            f.write(self.consensus + '\n')
