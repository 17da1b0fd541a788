"""phylo_rell's contract without a GPU: the host loop of the library (phylo_debug_rell_host, the same
functions the kernels call) against tests/rell_ref.py -- the counts from phylo_amd.rng and the multiply-high rule, the chain in
exact rational arithmetic, the log within an ulp of numpy's -- and the header under the host compiler's sanitizers.

Every test here needs _ffi.debug_rell_host: AttributeError without it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rell_ref
from phylo_amd import _ffi, rng

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 0x9E3779B97F4A7C15


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_stream_number():
    assert rng.STREAM_BOOT == 4 and len({rng.STREAM_PAIR, rng.STREAM_BRANCH, rng.STREAM_RESAMPLE, rng.STREAM_TWIST, rng.STREAM_BOOT}) == 5


@pytest.mark.parametrize("S", [1, 3, 4, 5, 64, 65, 257, 1949])
def test_counts_are_the_restatement(S):
    for b in (0, 1, 69, 2 ** 20 - 1):
        got = _ffi.debug_rell_host(None, b, 1, SEED, S=S)['counts']
        want = rell_ref.counts(S, b, SEED)
        assert got.shape == (1, S) and got.dtype == np.int32
        np.testing.assert_array_equal(got[0], want, err_msg="S=%d b=%d" % (S, b))
        assert int(want.sum()) == S and int(got.sum()) == S
    if S > 4:
        assert not np.array_equal(rell_ref.counts(S, 0, SEED), rell_ref.counts(S, 0, SEED + 1))       # the seed is the key ...
        assert not np.array_equal(rell_ref.counts(S, 0, SEED), rell_ref.counts(S, 1, SEED))           # ... the replicate the counter


def test_a_window_is_the_rows_of_a_larger_window():
    S = 65
    wide = _ffi.debug_rell_host(None, 60, 20, SEED, S=S)['counts']
    np.testing.assert_array_equal(_ffi.debug_rell_host(None, 67, 5, SEED, S=S)['counts'], wide[7:12])
    f = rell_ref.factors(3, S, 4)
    a, b = _ffi.debug_rell_host(f, 60, 20, SEED), _ffi.debug_rell_host(f, 67, 5, SEED)
    np.testing.assert_array_equal(b['counts'], a['counts'][7:12])
    np.testing.assert_array_equal(bits(b['rep_loglik']), bits(a['rep_loglik'][:, 7:12]))
    np.testing.assert_array_equal(bits(b['site_loglik']), bits(a['site_loglik']))


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("S", [1, 5, 65])
@pytest.mark.parametrize("nB", [1, 7])
def test_chain_bit_for_bit_against_rationals(T, S, nB):
    f = rell_ref.factors(T, S, 100 * T + S)
    got = _ffi.debug_rell_host(f, 3, nB, SEED)
    x = got['site_loglik']
    ulp = np.spacing(np.abs(np.log(f)))
    assert (np.abs(x - np.log(f)) <= ulp).all()                      # the contract's log: within an ulp of numpy's
    assert (x[f == 1.0] == 0.0).all()
    cnt = np.array([rell_ref.counts(S, 3 + b, SEED) for b in range(nB)])
    np.testing.assert_array_equal(got['counts'], cnt)
    want = rell_ref.rep_loglik(cnt, x)
    assert got['rep_loglik'].shape == (T, nB)
    np.testing.assert_array_equal(bits(got['rep_loglik']), bits(want))
    # the order matters at this precision: the chain is not the sorted or the pairwise sum
    if S == 65 and nB == 7:
        assert not np.array_equal(bits(want), bits((x[:, None, :] * cnt[None, :, :]).sum(axis=2)))


def test_zero_counts_and_padding_are_free():
    """a zero count leaves the accumulator unchanged bit for bit: the chain over the drawn sites alone, and over a padded row"""
    f = rell_ref.factors(2, 65, 9)
    x = _ffi.debug_rell_host(f, 0, 1, SEED)['site_loglik']
    cnt = rell_ref.counts(65, 0, SEED)
    assert (cnt == 0).sum() > 5
    full = [rell_ref.chain(cnt, r) for r in x]
    kept = [rell_ref.chain(cnt[cnt > 0], r[cnt > 0]) for r in x]
    padded = [rell_ref.chain(np.concatenate([cnt, [0, 0, 0]]), np.concatenate([r, [0.0, 0.0, 0.0]])) for r in x]
    assert bits(full).tolist() == bits(kept).tolist() == bits(padded).tolist()


def test_hook_outputs_are_optional_and_refusals():
    f = rell_ref.factors(2, 5, 1)
    full = _ffi.debug_rell_host(f, 0, 3, 1)
    only = _ffi.debug_rell_host(f, 0, 3, 1, want_counts=False, want_logs=False)
    assert only['counts'] is None and only['site_loglik'] is None
    np.testing.assert_array_equal(bits(only['rep_loglik']), bits(full['rep_loglik']))
    for v in (0.0, -1.0, np.inf, np.nan):
        g = f.copy()
        g[1, 4] = v
        with pytest.raises(_ffi.PhyloError) as e:
            _ffi.debug_rell_host(g, 0, 3, 1)
        assert e.value.code == -1 and "tree 1, site 4" in str(e.value)
    with pytest.raises(_ffi.PhyloError):
        _ffi.debug_rell_host(None, 0, 1, 1, S=65536)
    with pytest.raises(_ffi.PhyloError):
        _ffi.debug_rell_host(None, 2 ** 20, 1, 1, S=5)
    assert _ffi.debug_rell_host(None, 0, 1, 1, S=65535)['counts'].sum() == 65535


def test_header_under_sanitizers(tmp_path):
    """The host half of phylo_rell.h with a main of its own (tests/rell_asan_main.cpp), address and undefined-behaviour sanitizers
    of the host compiler: host code, run as a program."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rell_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "rell_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 values differ" in p.stdout
