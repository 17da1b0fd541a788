"""Shapes of the one-launch sweep (phylo_persist.h: pp_sweep<256>, pp_sweep<512>) and the grids they claim, shared by
tests/test_one_launch_plan_cpu.py (the rule, no GPU) and tests/test_gpu_one_launch_forms.py (the bits).  Every grid computes the
same bits, so a case that silently lands on another grid, or on the launch path, would still pass every comparison: the CPU test
pins each claim to persist_plan_of, the GPU tests assert it through phylo_debug_persist_of before they compare."""

# The device the grids below are stated for (MI355X): compute units, and the workgroups of pp_sweep the planner may place on one.
# (Both instantiations take 256 VGPRs per lane: four waves of 256 threads at one wave per SIMD, eight of 512 threads at two, so the
# runtime admits one workgroup per CU and persist_plan's "two only with a block of margin" gives 1.)
N_CUS = 256
BLOCKS_PER_CU = 1

# limits of the rule (phylo_persist.h, persist_plan_of)
PP_CHUNK, PP_MAX_M, PP_MAX_KG, MAX_TAXA, MAX_S, MAX_LDS = 16, 1024, 8192, 32, 8192, 150 * 1024
PK_AUX = 8


def lds_bytes(N, m, Kg):
    """pp_layout(N, m, Kg).total: scan scratch | ldf table | flags | own ancestors | adoption flags | PP_CHUNK particle slots | cdf"""
    up = lambda x, a: (x + a - 1) // a * a
    n4 = up(N, 4)
    slot = (PK_AUX + 32 + 40 + 26) * 8 + (3 * n4 + 4) * 4
    p = up(16 * 8 + 16 * 8, 16)
    p += ((N + 2) & ~1) * 8
    p = up(p, 16) + 16
    p += 2 * up(m, 4) * 4
    p = up(p, 16)
    p += PP_CHUNK * up(slot, 16)
    return p + Kg * 8


# ---- part A: PHYLO_PERSIST_NT=512 on the default grid (PHYLO_PERSIST_WGS unset).  name -> N, G, Kg and the claimed Wg, m --------------
DEFAULT_GRID = {
    "k16": dict(N=9, G=1, Kg=16, Wg=16, m=1),             # one particle per workgroup: seven of the eight waves idle
    "k257": dict(N=12, G=1, Kg=257, Wg=1, m=257),          # K prime: one workgroup, 17 chunks, the last of one particle
    "k5000": dict(N=12, G=1, Kg=5000, Wg=250, m=20),       # a second chunk of four particles, fewer than the waves
    "k8192": dict(N=12, G=1, Kg=8192, Wg=256, m=32),       # the largest cdf in LDS
    "ds1-k300": dict(N=27, G=1, Kg=300, Wg=150, m=2),
    "n32-k96": dict(N=32, G=1, Kg=96, Wg=96, m=1),         # every lane of the history rows in use
    "edges-k64": dict(N=5, G=1, Kg=64, Wg=64, m=1),        # the merge loop's S edges
    "tiles-k80": dict(N=6, G=1, Kg=80, Wg=80, m=1),        # uneven site tiles
    "variants-k128": dict(N=7, G=1, Kg=128, Wg=128, m=1),  # CL / CR variants, special values, asymmetric models
    "flat-k64": dict(N=9, G=1, Kg=64, Wg=64, m=1),
    "flat-k1000": dict(N=9, G=1, Kg=1000, Wg=250, m=4),
    "flat-k4096": dict(N=9, G=1, Kg=4096, Wg=256, m=16),   # m exactly one chunk
    "batch-3x32": dict(N=12, G=3, Kg=32, Wg=32, m=1),
    "batch-5x7": dict(N=12, G=5, Kg=7, Wg=7, m=1),
    "batch-8x256": dict(N=12, G=8, Kg=256, Wg=32, m=8),
    "reuse-k192": dict(N=8, G=1, Kg=192, Wg=192, m=1),     # one context: one launch, launches, one launch, then ...
    "reuse-4x48": dict(N=8, G=4, Kg=48, Wg=48, m=1),       # ... a batch with another G
}

# ---- part B: PHYLO_PERSIST_WGS forced, each at 256 and 512 threads.  (WGS, G, Kg, claimed (Wg, m) or None: the launch path runs) ------
FORCED_N, FORCED_S = 8, 130
FORCED = [
    (1, 1, 64, (1, 64)),                                    # four full chunks
    (4, 1, 64, (4, 16)),                                    # m exactly one chunk
    (4, 1, 68, (4, 17)),                                    # a chunk and one particle
    (64, 1, 64, (64, 1)),
    (7, 1, 2048, (4, 512)),                                 # Wg walks down from 7 to a divisor of Kg
    (2, 1, 2048, (2, 1024)),                                # m = PP_MAX_M: taken
    (1, 1, 2048, None),                                     # m = 2048: refused
    (2, 3, 32, None),                                       # fewer workgroups than groups
    (7, 3, 32, (2, 16)),
    (40, 5, 7, (7, 1)),
    (1000000, 1, 2048, (256, 8)),                           # clamped to the device: the unforced grid
]


def forced_id(c):
    return "wgs%d-%dx%d" % c[:3]
