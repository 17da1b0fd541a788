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
