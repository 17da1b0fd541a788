"""Marginal ancestral reconstruction of scored trees: what Context.trees_ancestral returns, turned into
clade names, sequences, a FASTA file and per-node summaries.  NumPy only, no device.

Row i of every array is internal node N + i of the tree as given (child [N-1][2], leaves 0 .. N-1), the last row the root."""
import numpy as np

NOSTATE = 255          # _ffi.ANC_NOSTATE: a site without a most probable state (its site factor has no usable reciprocal)


def node_clades(child, taxa):
    """the sorted leaf names below every internal row: a list of N-1 lists"""
    child = np.asarray(child)
    R = child.shape[0]
    N = R + 1
    if child.shape != (R, 2) or len(taxa) != N:
        raise ValueError("child must be [N-1][2] and taxa hold N names")
    below = [[str(t)] for t in taxa] + [None] * R
    for i in range(R):
        a, b = int(child[i, 0]), int(child[i, 1])
        if not (0 <= a < N + i and 0 <= b < N + i):
            raise ValueError("row %d: a child is neither a leaf nor a node of an earlier row" % i)
        below[N + i] = sorted(below[a] + below[b])
    return below[N:]


def sequences(state, letters='ACGT', nostate='?'):
    """one string per node from state [R][S] (uint8): letters[state], `nostate` where the site has none"""
    state = np.asarray(state)
    if state.ndim != 2:
        raise ValueError("state must be [nodes][sites]")
    if len(letters) != 4 or len(nostate) != 1:
        raise ValueError("four letters and one character for a missing state")
    if ((state > 3) & (state != NOSTATE)).any():
        raise ValueError("a state is neither 0 .. 3 nor NOSTATE")
    table = np.array(list(letters) + [nostate])
    return [''.join(table[np.where(row == NOSTATE, 4, row)]) for row in state]


def fasta_records(state, child, taxa, tree=0, letters='ACGT', nostate='?'):
    """[(header, sequence)] of one tree: header 'tree{t}_node{N+i} clade=a,b,c'"""
    N = len(taxa)
    return [("tree%d_node%d clade=%s" % (tree, N + i, ','.join(cl)), seq)
            for i, (cl, seq) in enumerate(zip(node_clades(child, taxa), sequences(state, letters, nostate)))]


def write_fasta(path, records, width=0):
    """records [(header, sequence)] as FASTA; width > 0 wraps the sequence lines"""
    with open(path, 'w') as f:
        for head, seq in records:
            f.write('>' + head + '\n')
            if width > 0:
                for k in range(0, len(seq), width):
                    f.write(seq[k:k + width] + '\n')
            else:
                f.write(seq + '\n')


def read_fasta(path):
    """[(header, sequence)] of a FASTA file (what write_fasta wrote)"""
    out = []
    with open(path) as f:
        for line in f:
            line = line.rstrip('\n')
            if line.startswith('>'):
                out.append([line[1:], ''])
            elif line and out:
                out[-1][1] += line
    return [(h, s) for h, s in out]


def summarise(pmax, below=0.9):
    """per node of pmax [R][S]: the mean of pmax and the share of sites with pmax < `below`, both over the sites that have a state;
    NaN sites are excluded and counted.  Returns dict(mean_pmax [R], share_below [R], n_nan [R]); a node with no site left gets NaN."""
    pmax = np.asarray(pmax, dtype=np.float64)
    if pmax.ndim != 2:
        raise ValueError("pmax must be [nodes][sites]")
    ok = ~np.isnan(pmax)
    n = ok.sum(axis=1)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(ok, pmax, 0.0).sum(axis=1) / n
        share = (ok & (pmax < below)).sum(axis=1) / n
    return dict(mean_pmax=mean, share_below=share, n_nan=(~ok).sum(axis=1))


# ---- site-rate posteriors under a rate mixture: what Context.trees_ancestral_rates returns beside the states ----
def category_states(catpost):
    """the most probable category per site of catpost [...][C][S]: uint8 [...][S], the lowest c among equals, NOSTATE where any of
    the site's C posteriors is NaN"""
    catpost = np.asarray(catpost, dtype=np.float64)
    if catpost.ndim < 2:
        raise ValueError("catpost must be [...][categories][sites]")
    if catpost.shape[-2] > NOSTATE:
        raise ValueError("at most %d categories" % NOSTATE)
    bad = np.isnan(catpost).any(axis=-2)
    best = np.argmax(np.where(np.isnan(catpost), -np.inf, catpost), axis=-2).astype(np.uint8)     # argmax: the first of the largest
    best[bad] = NOSTATE
    return best


def summarise_rates(siterate, catpost, quantiles=(0.05, 0.25, 0.5, 0.75, 0.95)):
    """per tree of siterate [T][S] and catpost [T][C][S]: the mean and the quantiles of the site rate and the share of sites per
    most probable category, all over the sites that have a rate; NaN sites are excluded and counted.  Returns dict(mean_rate [T],
    quantiles [T][len(quantiles)], q (the levels), cat_share [T][C], n_nan [T]); a tree with no site left gets NaN."""
    siterate = np.asarray(siterate, dtype=np.float64)
    catpost = np.asarray(catpost, dtype=np.float64)
    if siterate.ndim != 2 or catpost.ndim != 3 or catpost.shape[0] != siterate.shape[0] or catpost.shape[2] != siterate.shape[1]:
        raise ValueError("siterate must be [trees][sites] and catpost [trees][categories][sites]")
    T, C = catpost.shape[0], catpost.shape[1]
    cat = category_states(catpost)
    ok = ~np.isnan(siterate) & (cat != NOSTATE)
    mean, qs, share = np.full(T, np.nan), np.full((T, len(quantiles)), np.nan), np.full((T, C), np.nan)
    for t in range(T):
        if ok[t].any():
            r = siterate[t][ok[t]]
            mean[t] = r.mean()
            qs[t] = np.quantile(r, quantiles)
            share[t] = np.bincount(cat[t][ok[t]], minlength=C)[:C] / r.size
    return dict(mean_rate=mean, quantiles=qs, q=tuple(float(x) for x in quantiles), cat_share=share, n_nan=(~ok).sum(axis=1))


def write_site_rates(path, trees, siterate, catpost):
    """a TSV with one line per (tree, site): tree (trees[t], an integer), site, rate, cat (category_states; NOSTATE where the site
    has none), p0 .. p{C-1}.  Floats are written by repr: read_site_rates gives the same bits back (a NaN comes back as the quiet NaN)."""
    siterate = np.asarray(siterate, dtype=np.float64)
    catpost = np.asarray(catpost, dtype=np.float64)
    if siterate.ndim != 2 or catpost.ndim != 3 or catpost.shape[0] != siterate.shape[0] or catpost.shape[2] != siterate.shape[1]:
        raise ValueError("siterate must be [trees][sites] and catpost [trees][categories][sites]")
    if len(trees) != siterate.shape[0]:
        raise ValueError("one tree number per row of siterate")
    T, C, S = catpost.shape
    cat = category_states(catpost)
    with open(path, 'w') as f:
        f.write('\t'.join(['tree', 'site', 'rate', 'cat'] + ['p%d' % c for c in range(C)]) + '\n')
        for t in range(T):
            for s in range(S):
                f.write('\t'.join([str(int(trees[t])), str(s), repr(float(siterate[t, s])), str(int(cat[t, s]))] +
                                  [repr(float(catpost[t, c, s])) for c in range(C)]) + '\n')


def read_site_rates(path):
    """what write_site_rates wrote: dict(trees [T] (in the file's order), siterate [T][S], cat [T][S] (uint8), catpost [T][C][S])"""
    with open(path) as f:
        head = f.readline().rstrip('\n').split('\t')
        if head[:4] != ['tree', 'site', 'rate', 'cat'] or head[4:] != ['p%d' % c for c in range(len(head) - 4)]:
            raise ValueError("not a table of site rates: %r" % (head,))
        C = len(head) - 4
        trees, rows = [], {}
        for line in f:
            cols = line.rstrip('\n').split('\t')
            if len(cols) != 4 + C:
                raise ValueError("a line of %d columns under a header of %d" % (len(cols), 4 + C))
            t = int(cols[0])
            if t not in rows:
                rows[t] = []
                trees.append(t)
            if int(cols[1]) != len(rows[t]):
                raise ValueError("tree %d: site %s out of order" % (t, cols[1]))
            rows[t].append((float(cols[2]), int(cols[3]), [float(x) for x in cols[4:]]))
    S = len(rows[trees[0]]) if trees else 0
    if any(len(rows[t]) != S for t in trees):
        raise ValueError("the trees do not have one number of sites")
    siterate = np.array([[r[0] for r in rows[t]] for t in trees], dtype=np.float64).reshape(len(trees), S)
    cat = np.array([[r[1] for r in rows[t]] for t in trees], dtype=np.uint8).reshape(len(trees), S)
    catpost = np.array([[r[2] for r in rows[t]] for t in trees], dtype=np.float64).reshape(len(trees), S, C).transpose(0, 2, 1).copy()
    return dict(trees=np.array(trees, dtype=np.int64), siterate=siterate, cat=cat, catpost=catpost)
