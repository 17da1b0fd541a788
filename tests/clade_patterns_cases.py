"""Shared by tests/test_clade_patterns_cpu.py and tests/test_gpu_clade_patterns.py: small alignments given as codes whose clades have
known numbers of distinct columns, and the NumPy restatement of a clade's classes (phylo_amd/csrc/phylo_site_patterns.h: the
columns of the alignment restricted to the leaves of a bitset, numbered by first occurrence)."""
import numpy as np

MAX_TAXA = 12                                              # PK_CLADE_MAX_N
MAX_BYTES = 32 << 20                                       # PK_CLADE_MAX_BYTES
HDR = 256                                                  # PK_CLADE_HDR_BYTES


def leaves_of(Z, N):
    return [i for i in range(N) if Z >> i & 1]


def classes(codes, Z):
    """(cls [S], rep [U_Z]): the class of every site among the columns restricted to Z's leaves, numbered by first occurrence, and
    the first site of every class (ascending)."""
    N, S = codes.shape
    sub = codes[leaves_of(Z, N)]
    _, first, inv = np.unique(sub, axis=1, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(first)                              # unique's number -> rank by first occurrence
    rank = np.empty_like(order)
    rank[order] = np.arange(order.size)
    return rank[inv].astype(np.int64), first[order].astype(np.int64)


def layout(N, S, U):
    """The buffer's layout (pk_clade_layout_of)."""
    nC = -(-(-(-S // 64)) // 16)
    codes_bytes, rep_bytes, image_bytes = N * nC * 1024, (-(-U // 64) + 2) * 256, nC * 2048
    stride = HDR + rep_bytes + image_bytes
    return {"codes_bytes": codes_bytes, "rep_bytes": rep_bytes, "image_bytes": image_bytes, "stride": stride,
            "total": codes_bytes + (1 << N) * stride}


def quadruples(S=320, seed=4):
    """4 taxa whose columns are all 256 quadruples of A/C/G/T, then repeats, shuffled: every triple of taxa sees exactly 64 distinct
    columns and the whole alignment 256 -- full phase-1 steps, the pad entry behind a full step."""
    assert 256 <= S <= 384
    rng = np.random.default_rng(seed)
    ids = np.concatenate([np.arange(256), rng.integers(0, 256, size=S - 256)])
    rng.shuffle(ids)
    return np.stack([(ids >> 2 * i) & 3 for i in range(4)]).astype(np.uint8)


def gapped(N=5, S=130, seed=7):
    """5 taxa, S = 130 (three walk steps, the last of two lanes; an odd number of them), states and gaps.  Site number s in mixed
    radix: taxa 3 and 4 its two base-5 digits, taxa 0 and 1 the next two base-3 digits over A, C, gap, taxon 2 a random A or gap.
    All 130 columns are distinct (three phase-1 steps for the whole clade), taxa {0, 3, 4} see 75 (two steps), {0, 1, 2} at most
    12 (one step).  The sites are shuffled."""
    assert (N, S) == (5, 130)
    rng = np.random.default_rng(seed)
    s = rng.permutation(S)
    three = np.array([0, 1, 4], dtype=np.uint8)
    return np.stack([three[s // 25 % 3], three[s // 75 % 3], np.array([0, 4], dtype=np.uint8)[rng.integers(0, 2, size=S)],
                     (s % 5).astype(np.uint8), (s // 5 % 5).astype(np.uint8)])


def few(N=6, S=70, seed=11):
    """6 taxa over three codes, S = 70: small clades repeat columns heavily."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 3, size=(N, S)).astype(np.uint8)
