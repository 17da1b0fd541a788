"""Shared by tests/test_packed_codes_cpu.py and tests/test_gpu_packed_codes.py: alignments given as codes (0..3 one-hot, 4 a gap =
an all-ones row) with gaps where the packed image of the codes has its edges, and the NumPy restatement of that image's layout
(phylo_amd/csrc/phylo_packed_codes.h)."""
import numpy as np

PAD = 5                                                    # the code of a site >= S in the packed image
ROWS = np.vstack([np.eye(4), np.ones((1, 4))])             # code -> leaf row


def edge_codes(N, S, seed):
    """Random codes 0..4 [N][S]; gaps forced at site 0, at site S - 1, at column 63 of the last full 64-site step, and leaf 1 all
    gaps."""
    c = np.random.default_rng(seed).integers(0, 5, size=(N, S)).astype(np.uint8)
    c[0, 0] = 4
    c[N - 1, S - 1] = 4
    if S >= 64:
        c[0, 64 * (S // 64) - 1] = 4
        c[2 % N, 63] = 4
    c[1, :] = 4
    return c


def genome(codes):
    return np.ascontiguousarray(ROWS[codes], dtype=np.float64)


def n_chunks(S):
    return -(-(-(-S // 64)) // 16)


def packed_reference(codes):
    """[N][nC][64][16]: [leaf][Jc][c][j] = code of site 64 (16 Jc + j) + c, PAD at sites >= S."""
    N, S = codes.shape
    nC = n_chunks(S)
    full = np.full((N, nC * 1024), PAD, dtype=np.uint8)
    full[:, :S] = codes
    # site = 1024 Jc + 64 j + c
    return np.ascontiguousarray(full.reshape(N, nC, 16, 64).transpose(0, 1, 3, 2))
