"""The packed image of the leaf codes (phylo_amd/csrc/phylo_packed_codes.h, built by phylo_set_leaves beside the byte codes and
read by pk_rank_merge_nostore) against a NumPy restatement of its layout -- no GPU: the exported packer
(phylo_debug_pack_leaf_codes), and the header alone in a stand-alone program under the host's address and undefined-behaviour
sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import packed_codes_cases as PC
from phylo_amd import _ffi

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SIZES = [1, 2, 63, 64, 65, 898, 1023, 1024, 1025, 2049]


@pytest.mark.parametrize("N", [2, 5])
@pytest.mark.parametrize("S", SIZES)
def test_packer_against_the_layout(N, S):
    codes = PC.edge_codes(N, S, seed=100 * N + S)
    assert codes[0, 0] == 4 and codes[N - 1, S - 1] == 4 and (S < 64 or codes[2 % N, 63] == 4)
    got = _ffi.debug_pack_leaf_codes(codes)
    nC = -(-(-(-S // 64)) // 16)
    assert got.shape == (N, nC, 64, 16) and got.size == N * nC * 1024        # the buffer's size
    want = PC.packed_reference(codes)
    assert np.array_equal(got, want)
    # said again site by site: every code, the pad at every site >= S
    flat = got.transpose(0, 1, 3, 2).reshape(N, nC * 1024)               # [leaf][site]
    assert np.array_equal(flat[:, :S], codes)
    assert (flat[:, S:] == PC.PAD).all()
    for leaf, s in ((0, 0), (N - 1, S - 1)) + (((2 % N, 63),) if S >= 64 else ()):
        assert got[leaf, s // 1024, s % 64, (s // 64) % 16] == 4


def test_packer_refuses_a_short_buffer():
    lib = _ffi.load()
    import ctypes as C
    codes = np.zeros((2, 65), dtype=np.uint8)
    need = C.c_int64(0)
    out = np.zeros(2047, dtype=np.uint8)
    rc = lib.phylo_debug_pack_leaf_codes(codes.ctypes.data_as(C.c_void_p), 2, 65, out.ctypes.data_as(C.c_void_p), C.c_int64(out.size),
                                         C.byref(need))
    assert rc != 0 and need.value == 2048 and not out.any()


def test_packer_header_under_sanitizers(tmp_path):
    """The header with a main of its own (tests/packed_codes_asan_main.cpp), address and undefined-behaviour sanitizers of the host
    compiler: host code, run as a program."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "packed_codes_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "packed_codes_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 bytes differ" in p.stdout
