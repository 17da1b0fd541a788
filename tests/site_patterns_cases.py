"""Shared by tests/test_site_patterns_cpu.py and tests/test_gpu_site_patterns.py: alignments given as codes whose columns are drawn
from a pool of exactly U distinct ones, and the NumPy restatement of the site-pattern tables' layout and of the rule
(phylo_amd/csrc/phylo_site_patterns.h)."""
import numpy as np

CAP = 512                                                  # PK_PAT_MAX_U
# the rule's instruction counts (PK_PAT_C_*): a step of today's mixed loop, a phase-1 step, a walk step, the fixed part
C_STEP, C_PHASE1, C_WALK, C_FIXED = 38, 33, 7, 30


def pool_codes(N, S, U, seed):
    """Codes 0..4 [N][S] with exactly U distinct columns (U <= min(S, 5^N)), every one of them present, in random order."""
    assert 1 <= U <= min(S, 5 ** N)
    rng = np.random.default_rng(seed)
    ids = rng.choice(5 ** N, size=U, replace=False)
    pool = np.stack([(ids // 5 ** i) % 5 for i in range(N)]).astype(np.uint8)        # [N][U]
    pick = np.concatenate([np.arange(U), rng.integers(0, U, size=S - U)])
    rng.shuffle(pick)
    codes = np.ascontiguousarray(pool[:, pick])
    assert len({codes[:, s].tobytes() for s in range(S)}) == U
    return codes


def decode_image(image, S):
    """image uint16 [nC][2][64][8] -> (pat [S], the entries of the sites >= S): site = 1024 Jc + 512 h + 64 j + c."""
    nC = image.shape[0]
    flat = image.transpose(0, 1, 3, 2).reshape(nC * 1024)
    assert (flat % 8 == 0).all()
    return (flat[:S] // 8).astype(np.int64), flat[S:]


def rule(S, U, coded=True, ntiles=1, switch=None):
    if switch == "0" or not coded or ntiles != 1 or not 1 <= U <= CAP:
        return False
    if switch == "force":
        return True
    nS, nU = -(-S // 64), -(-U // 64)
    return 10 * (nU * C_PHASE1 + nS * C_WALK + C_FIXED) <= 8 * nS * C_STEP
