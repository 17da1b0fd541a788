"""The matrix function's contract on the CPU (tests/expm_cases.py): the link 50 digits -> C oracle.

  * the committed 50-digit values equal a fresh evaluation, and the NumPy restatement stays within the committed E_REF0;
  * the oracle's pm_expm4 twin is within TOL(name, s) = 2^s (8 E_REF0 + 4) u of the 50-digit value in every entry, relatively,
    over the whole grid; no entry is negative; t = +-0 is the identity bit for bit; rows sum to 1 within 4 TOL; 5e-324 is harmless;
  * the JC69 closed form is exact in absolute, not in relative terms: the bounds that follow from one exp within 1 ulp, one product
    and one sum;
  * the host check of the domain, as a program of its own under the host compiler's sanitizers.

tests/test_gpu_expm_contract.py holds the device to the oracle bit for bit and, independently, to the same 50-digit values.
Measured here: the oracle's worst error / TOL is 0.139 without squarings (hky50) and 0.114 over s = 1 .. 23 (jc); the JC69 closed
form's worst errors are 0.18 u (off-diagonal), 0.98 u (diagonal), 1.02 u / min(t, 1) (off-diagonal, relative).  Three single-edit
mutants of a scratch copy of the oracle (a Pade-9 coefficient off by one in its last digit; theta_5 in place of theta_3; one
squaring dropped) each fail test_oracle_within_tol_of_50_digits, at 57, 60 and 143 of the 714 grid points."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import c_oracle as CO
from oracle import cpu_ref as O
from tests import expm_cases as X

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
U = X.U


@pytest.fixture(scope="module")
def npz():
    return X.load_contract()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_grid_is_what_the_issue_of_the_contract_lists():
    G = X.generators()
    assert tuple(G) == X.NAMES
    for name, Q in G.items():
        ts = X.lengths(Q)
        assert len(ts) == 119 and np.all(X.in_domain(Q, ts)), name          # the device takes every one of them
        ss = np.array([X.kernel_norm_s(Q, t)[1] for t in ts])
        assert ss.max() == X.S_MAX and {0, 1, 3, 6, 9, 12, 16, 20, 23} <= set(ss.tolist()), (name, sorted(set(ss.tolist())))
        norms = np.array([X.kernel_norm_s(Q, t)[0] for t in ts])
        for th in X.THETA:                                                   # lengths within a few ulps of every class boundary
            assert np.sum(np.abs(norms / th - 1.0) <= 8 * U) == 2, (name, th)
    assert abs(X.norm1(G['nonrev']) - 2.4681) < 1e-3 and not np.allclose(G['nonrev'], G['nonrev'].T)


def test_domain_constants_are_the_header_s():
    src = open(os.path.join(ROOT, "phylo_amd", "csrc", "phylo_treeset.h")).read()
    assert int(re.search(r"#define PT2_EXPM_S_MAX (\d+)", src).group(1)) == X.S_MAX == 23
    a, b = re.search(r"#define PT2_EXPM_NORM_MAX \(([0-9.e+-]+) \* ([0-9.]+)\)", src).groups()
    assert float(a) * float(b) == X.NORM_MAX
    assert X.tol('stiff', X.S_MAX) <= 2.0 ** -20 < X.tol('stiff', X.S_MAX + 1)
    assert max(X.E_REF0.values()) == X.E_REF0['stiff']


def test_committed_values_equal_a_fresh_50_digit_evaluation(npz):
    fresh = X.contract()
    assert sorted(fresh) == sorted(npz.files)
    for k, v in fresh.items():
        assert v.shape == npz[k].shape and np.array_equal(bits(v), bits(npz[k])), k
    size = os.path.getsize(os.path.join(X.GOLDEN, "expm_contract.npz"))
    assert size < (1 << 20)
    for name in X.NAMES:                                                     # a pair carries far more than 53 bits
        hi, lo = npz['hi/' + name], npz['lo/' + name]
        assert np.all(np.abs(lo) <= np.abs(hi) * 2.0 ** -53) and np.count_nonzero(lo) > lo.size // 2, name


def test_restatement_stays_within_the_committed_e_ref0(npz):
    for name in X.NAMES:
        e = X.measure_e_ref0(name, npz['Q/' + name], npz['t/' + name], npz['hi/' + name], npz['lo/' + name])
        print("E_REF0[%s]: measured %.3f u, committed %g u" % (name, e, X.E_REF0[name]))
        assert e <= X.E_REF0[name], name
        assert e >= 0.9 * X.E_REF0[name], "the committed constant is the measured error, not a wider one: " + name


@pytest.mark.parametrize("name", X.NAMES)
def test_oracle_within_tol_of_50_digits(npz, name):
    Q, ts, hi, lo = npz['Q/' + name], npz['t/' + name], npz['hi/' + name], npz['lo/' + name]
    P = CO.expm_batched(Q, ts)
    worst = {}
    for k, t in enumerate(ts):
        s = X.kernel_norm_s(Q, t)[1]
        T = X.tol(name, s)
        assert np.all(np.isfinite(P[k])) and np.all(P[k] >= 0.0), (name, t, P[k])
        e = float(X.rel_err(P[k], hi[k], lo[k]).max())
        worst[s > 0] = max(worst.get(s > 0, 0.0), e / T)
        assert e <= T, "%s t=%r s=%d: relative error %.3g u over TOL %.3g u" % (name, t, s, e / U, T / U)
        for i in range(4):
            assert abs(math.fsum(P[k, i]) - 1.0) <= 4 * T, (name, t, i)
        if t == 0.0:                                                         # +0 and -0: the identity, bit for bit
            assert np.array_equal(bits(P[k]), bits(np.eye(4))), (name, t)
        if t == 5e-324:
            assert np.array_equal(np.diag(P[k]), np.ones(4)), (name, P[k])
    assert np.sum(ts == 0.0) == 2 and np.sum(ts == 5e-324) == 1
    print("%s: worst error / TOL %.4f without squarings, %.4f with" % (name, worst[False], worst[True]))


def test_true_entries_below_the_floor_are_the_only_ones_left_out(npz):
    """the relative comparison leaves out entries whose true value lies below 2^-1000: those of 5e-324, and of 1e-300 under the
    generators with rates of 1e-3 and less"""
    for name in X.NAMES:
        ts, hi = npz['t/' + name], npz['hi/' + name]
        out = np.abs(hi) < X.TINY
        assert not out[ts > 1e-290].any(), name
        assert not out[ts == 0.0][:, np.eye(4, dtype=bool)].any()


# ---- the JC69 closed form -----------------------------------------------------------------------------------------------------
def test_jc_closed_form_is_exact_in_absolute_terms(npz):
    ts, ref = npz['jc69/t'], npz['jc69/ref']
    assert len(ts) == 2021 and np.sum(ts < 2.0 ** -54) >= 8
    P = CO.expm_batched(O.jc_Q(), ts, jc=True)
    eo, ed, er = X.check_jc_closed_form(P, ts, ref, "oracle")
    print("JC69 closed form: off-diagonal %.3f u, diagonal %.3f u absolute; off-diagonal %.3f u / min(t, 1) relative" % (eo, ed, er))
    # not relative: at 1e-12 the off-diagonal is wrong in its fifth digit, and the bound says no less
    k = int(np.where(ts == 1e-12)[0][0])
    assert abs(P[k, 0, 1] - ref[2, k]) / ref[2, k] > 1e-6


# ---- the host check of the domain ---------------------------------------------------------------------------------------------
def test_range_check_under_sanitizers(tmp_path):
    """pt2_q_norm1 and pt2_check_expm_range with a main of their own (tests/expm_range_asan_main.cpp): lengths either side of the
    limit, 0, inf and NaN, under the address and undefined-behaviour sanitizers of the host compiler: host code, run as a program."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "expm_range_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "expm_range_asan_main.cpp"),
                           "-o", exe], stderr=subprocess.DEVNULL)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b" 0 checks failed" in p.stdout
