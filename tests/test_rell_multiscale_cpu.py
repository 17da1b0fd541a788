"""phylo_rell_multiscale's contract without a GPU: the host loop of the library
(phylo_debug_rell_multiscale_host, the same functions the kernels call) against tests/rell_ms_ref.py -- the counts of a scale from
phylo_amd.rng, the chain in exact rationals, the lexicographic best -- and the header's host half under the host compiler's
sanitizers.

Every test here needs _ffi.debug_rell_multiscale_host: AttributeError without it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import rell_ms_ref
import rell_ref
from phylo_amd import _ffi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SEED = 0x9E3779B97F4A7C15
hook = _ffi.debug_rell_multiscale_host


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_exports():
    assert 'phylo_rell_multiscale' in _ffi.EXPORTS and 'phylo_debug_rell_multiscale_host' in _ffi.EXPORTS
    lib = _ffi.load()
    assert hasattr(lib, 'phylo_rell_multiscale') and hasattr(lib, 'phylo_debug_rell_multiscale_host')


@pytest.mark.parametrize("S,draws", [(1, (65535,)), (5, (1, 3, 8)), (37, (18, 37, 52))])
def test_counts_are_the_restatement(S, draws):
    for k in range(len(draws)):
        for b in (0, 1, 69, 2 ** 20 - 1):
            got = hook(None, draws, k, b, 1, SEED, S=S)['counts']
            want = rell_ms_ref.counts(S, draws, k, b, SEED)
            assert got.shape == (1, S) and got.dtype == np.int32
            np.testing.assert_array_equal(got[0], want, err_msg="S=%d k=%d b=%d" % (S, k, b))
            assert int(got.sum()) == draws[k] == int(want.sum())
    if S == 37:
        # the scale is counter word 1: the same draw count at another k is another sample; a window is the rows of a wider one
        assert not np.array_equal(hook(None, (37, 37), 0, 0, 1, SEED, S=S)['counts'], hook(None, (37, 37), 1, 0, 1, SEED, S=S)['counts'])
        wide = hook(None, draws, 2, 60, 20, SEED, S=S)['counts']
        np.testing.assert_array_equal(hook(None, draws, 2, 67, 5, SEED, S=S)['counts'], wide[7:12])
        assert not np.array_equal(rell_ms_ref.counts(S, draws, 2, 0, SEED), rell_ms_ref.counts(S, draws, 2, 0, SEED + 1))


def test_scale_zero_with_S_draws_is_phylo_rells_sample():
    S = 65
    f = rell_ref.factors(3, S, 4)
    a, b = hook(f, (S,), 0, 5, 9, SEED), _ffi.debug_rell_host(f, 5, 9, SEED)
    np.testing.assert_array_equal(a['counts'], b['counts'])
    np.testing.assert_array_equal(bits(a['rep_loglik']), bits(b['rep_loglik']))
    np.testing.assert_array_equal(a['best'], rell_ref.first_argmax(b['rep_loglik']))


@pytest.mark.parametrize("S,draws", [(5, (1, 3, 8)), (37, (18, 37, 52))])
def test_scores_and_best_against_rationals(S, draws):
    T, nB = 6, 7
    f = rell_ref.factors(T, S, 100 + S, special=False).copy()             # every factor below exp(-1) ...
    f[4] = np.exp(np.random.default_rng(1).uniform(-0.5, -0.1, size=S))   # ... and this row above it at every site: it wins every
    f[2] = f[4]                                                           # replicate, and so does its copy, at a lower index
    x = _ffi.debug_rell_host(f, 0, 1, SEED)['site_loglik']
    for k in range(len(draws)):
        got = hook(f, draws, k, 3, nB, SEED)
        cnt = np.array([rell_ms_ref.counts(S, draws, k, 3 + b, SEED) for b in range(nB)])
        np.testing.assert_array_equal(got['counts'], cnt)
        want = rell_ms_ref.rep_loglik(cnt, x)
        np.testing.assert_array_equal(bits(got['rep_loglik']), bits(want), err_msg="k=%d" % k)
        np.testing.assert_array_equal(bits(want[2]), bits(want[4]))
        np.testing.assert_array_equal(got['best'], rell_ms_ref.best_lex(want))
        assert (got['best'] == 2).all()
    g = rell_ref.factors(T, S, 7)                                          # no planted winner: the best moves with the replicate
    got = hook(g, draws, len(draws) - 1, 0, 40, SEED)
    np.testing.assert_array_equal(got['best'], rell_ms_ref.best_lex(got['rep_loglik']))
    np.testing.assert_array_equal(got['best'], rell_ref.first_argmax(got['rep_loglik']))
    assert len(set(got['best'].tolist())) > 1


def test_hook_outputs_are_optional_and_refusals():
    f = rell_ref.factors(2, 5, 1)
    full = hook(f, (3, 8), 1, 0, 3, 1)
    only = hook(f, (3, 8), 1, 0, 3, 1, want_counts=False, want_reps=False)
    assert only['counts'] is None and only['rep_loglik'] is None
    np.testing.assert_array_equal(only['best'], full['best'])

    def refused(call, *what):
        with pytest.raises(_ffi.PhyloError) as e:
            call()
        assert e.value.code == -1
        for w in what:
            assert w in str(e.value), str(e.value)

    refused(lambda: hook(f, (3, 0), 0, 0, 3, 1), 'k=1', 'draws[1]=0')
    refused(lambda: hook(f, (3, 8, 65536), 0, 0, 3, 1), 'k=2', '65536')
    refused(lambda: hook(f, [3] * 65, 0, 0, 3, 1), 'K=65')
    refused(lambda: hook(f, (), 0, 0, 3, 1), 'K=0')
    refused(lambda: hook(f, (3, 8), 2, 0, 3, 1), 'k0=2')
    refused(lambda: hook(f, (3, 8), -1, 0, 3, 1), 'k0=-1')
    refused(lambda: hook(None, (3, 8), 0, 2 ** 20, 1, 1, S=5))
    refused(lambda: hook(None, (3, 8), 0, 0, 1, 1, S=65536), 'S=65536')
    g = f.copy()
    g[1, 4] = 0.0
    refused(lambda: hook(g, (3, 8), 0, 0, 3, 1), 'tree 1, site 4')


def test_header_under_sanitizers(tmp_path):
    """The host half of phylo_rell_ms.h with a main of its own (tests/rell_ms_asan_main.cpp) -- shape checks, the column -> (k, b)
    map, the chunk plan, the host loop -- under the address and undefined-behaviour sanitizers of the host compiler."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "rell_ms_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "rell_ms_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 values differ" in p.stdout
