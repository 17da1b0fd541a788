"""The forward sweep at its large-launch forms: the case table shared by tests/test_large_launch_cpu.py (the plan bits each case
claims, the oracle's sweeps as a usable reference, the Pade classes of its branch lengths -- no GPU) and
tests/test_gpu_large_launch.py (the kernels of those forms bit for bit against the C oracle).

Every case is the smallest shape that reaches what its line says, on the far side of a size threshold of
phylo_amd/csrc/phylo_sweep_plan.h.  S stays at 8: the hazards are in the particle dimension, and a short alignment keeps the
oracle well under a second per sweep.

  sorted_prologue   2 R K >= 262144 and not JC69: pk_sweep_prologue_sorted (workgroups of 1024 matrices filed by Pade class in LDS)
  mat_grouped       K > 8192: pk_materialize_adopted_grouped (64 particles per workgroup)
  fold_logz         Kg <= 16384: the last scan sums the log-normalisers; else pk_logz_total (one sweep) / pk_logz_total_groups
  book_width        8 at N <= 16 and K >= 8192 (pk_rank_book_packed<8>), 32 at 17 <= N <= 32
  Kg > 4096         the scan of a group by several workgroups (pp_scan_multi_max / _exp / _cdf), tiles of 2048 weights
"""
import functools

import numpy as np

from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd.datasets import synthetic_alignment

PI = np.array([[0.1, 0.2, 0.3, 0.4]])
SEED0 = 3                                                  # group g takes seed SEED0 + g
# the thresholds of pm_expm4 (phylo_math.h) on ||Q b||_1: Pade 3, 5, 7, 9 up to these, 13 beyond; scaled and squared beyond the last
PADE_THETA = (1.495585217958292e-2, 2.539398330063230e-1, 9.504178996162932e-1, 2.097847961257068e0)
PADE_THETA13 = 5.371920351148152


def _plan(sorted_prologue, mat_grouped, fold_logz, book_width, batched=True):
    return dict(sorted_prologue=sorted_prologue, mat_grouped=mat_grouped, fold_logz=fold_logz, book_width=book_width, use_rec=True,
                batched=batched)


def _case(N, G, Kg, plan, lam_l=10.0, lam_r=10.0, jc=False, q_scale=1.0, classes=None, eager=False, S=8):
    return dict(N=N, S=S, G=G, Kg=Kg, lam_l=lam_l, lam_r=lam_r, jc=jc, q_scale=q_scale, plan=plan, classes=classes, eager=eager)


RAGGED = _plan(True, True, False, 8)                       # K = 2 x 16641: sorted, grouped adopted nodes, pk_logz_total_groups
CASES = {
    # K > 8192: grouped adopted nodes and 8 lanes per particle; Kg > 4096: B = 3 tiles per group with a last tile of ONE weight;
    # the group boundary (4097) falls inside a wave of 8 particles and inside a workgroup of 64.  Not sorted, log Z folded.
    "grouped-8194": _case(5, 2, 4097, _plan(False, True, True, 8), eager=True),
    # 2 R K == 262144 exactly: sorted at the threshold, full workgroups only; Kg == 16384 is the last folded log Z
    "sorted-exact": _case(5, 2, 16384, _plan(True, True, True, 8), classes="all"),
    # 2 R K = 266256 = 260 * 1024 + 16: a last workgroup of 16 matrices; Kg > 16384; B = 9 with a last tile of 257 weights
    "sorted-ragged": _case(5, 2, 16641, RAGGED, classes="all", eager=True),
    # the same launch sizes as one sweep: pk_logz_total, no group seeds
    "single-33282": _case(5, 1, 33282, _plan(True, True, False, 8, batched=False), classes="all"),
    # PK_MAX_GROUPS groups; 2 R K = 260 * 1024; the group seed changes inside a sorted workgroup (520 does not divide 512 pairs);
    # scans of one workgroup with G = 64
    "groups-64": _case(5, 64, 520, _plan(True, True, True, 8)),
    # the same large launch at 32 lanes per particle (2 R K = 262208 = 256 * 1024 + 64: sorted too, a last workgroup of 64)
    "width32-8194": _case(17, 2, 4097, _plan(True, True, True, 32)),
    # a large launch that must NOT take the sorted prologue
    "jc-33282": _case(5, 2, 16641, _plan(False, True, False, 8), jc=True),
    # nearly every matrix Pade 13 and scaled / every matrix Pade 3 (four empty class lists) / the two sides of a particle in
    # opposite classes / a generator that is not row-normalised (the norm in the class estimate matters)
    "long": _case(5, 2, 16641, RAGGED, lam_l=0.05, lam_r=0.05, classes="long"),
    "short": _case(5, 2, 16641, RAGGED, lam_l=1e4, lam_r=1e4, classes="short"),
    "sides": _case(5, 2, 16641, RAGGED, lam_l=0.1, lam_r=1000.0, classes="sides"),
    "x30": _case(5, 2, 16641, RAGGED, q_scale=30.0),
}
NAMES = list(CASES)


def model(name):
    """(genome, Q, pi, lam_l, lam_r, jc, seeds) of a case"""
    c = CASES[name]
    N, S = c["N"], c["S"]
    g = synthetic_alignment(N, S, seed=N + S)['genome'].copy()
    g[1, 2] = 1.0                                          # two all-ones cells: leaf code 4 occurs
    g[N - 1, 5] = 1.0
    Q = (O.jc_Q() if c["jc"] else O.get_Q(O.init_y_q())) * c["q_scale"]
    return g, Q, PI, np.full(N - 1, c["lam_l"]), np.full(N - 1, c["lam_r"]), c["jc"], [SEED0 + i for i in range(c["G"])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """The oracle's sweep of every group (the last one with its nodes), computed once per process; read-only."""
    c = CASES[name]
    g, Q, pi, lam_l, lam_r, jc, seeds = model(name)
    refs = [CO.sweep(g, Q, pi, lam_l, lam_r, c["Kg"], s, jc=jc, want_nodes=(i == c["G"] - 1)) for i, s in enumerate(seeds)]
    for ref in refs:
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return tuple(refs)


def pade_classes(Q, b):
    """(class 0 .. 4 of every branch length, ||Q||_1 b): the estimate pk_sweep_draws_sorted files a matrix under"""
    nrm = np.asarray(b) * np.abs(Q).sum(axis=0).max()
    return sum((nrm > t).astype(np.int64) for t in PADE_THETA), nrm
