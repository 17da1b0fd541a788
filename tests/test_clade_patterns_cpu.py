"""The clade tables of the merge's site-pattern form (phylo_amd/csrc/phylo_site_patterns.h: one block per leaf bitset with the
distinct columns of the alignment restricted to the bitset's leaves) and their rule against a NumPy restatement -- no GPU: the
exported builder (phylo_debug_clade_tables), the rule (phylo_debug_clade_patterns_rule), the plan's bit, and the header alone in a
stand-alone program under the host's address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import clade_patterns_cases as CP
import packed_codes_cases as PC
import site_patterns_cases as SP
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset
from test_site_patterns_cpu import codes_of

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def check_blocks(codes, bitsets=None):
    N, S = codes.shape
    t = _ffi.debug_clade_tables(codes)
    g = _ffi.debug_site_patterns(codes)
    U = t["U"]
    assert U == g["U"] and t["layout"] == CP.layout(N, S, U)
    gpat, _ = SP.decode_image(g["image"], S)               # the global pattern of every site
    # the strided byte codes: the codes, then zeros up to the packed image's leaf stride
    assert t["codes"].shape == (N, PC.n_chunks(S) * 1024)
    assert np.array_equal(t["codes"][:, :S], codes) and not t["codes"][:, S:].any()
    want_blocks = [Z for Z in range(1 << N) if bin(Z).count("1") >= 3]
    assert sorted(t["blocks"]) == want_blocks
    for Z in (want_blocks if bitsets is None else bitsets):
        b = t["blocks"][Z]
        cls, rep = CP.classes(codes, Z)
        UZ = rep.size
        assert b["U"] == UZ, Z
        # classes in first-occurrence order: the representative is the first site of its class, and they ascend
        assert (np.diff(rep) > 0).all() and rep[0] == 0
        assert b["rep_off"].size == 64 * (-(-U // 64) + 2)
        assert np.array_equal(b["rep_off"][:UZ], 32 * rep.astype(np.uint32)) and not b["rep_off"][UZ:].any(), Z
        # the image: the global image's layout, 8 * class, the pad entry 8 U_Z
        assert b["image"].shape == (PC.n_chunks(S), 2, 64, 8)
        pat, pads = SP.decode_image(b["image"], S)
        assert np.array_equal(pat, cls), Z
        assert (pads == 8 * UZ).all() and pads.size == PC.n_chunks(S) * 1024 - S
        # the class of every global pattern
        assert np.array_equal(t["cls"][Z][gpat], cls), Z
        # sites of one class agree on the clade's leaves
        lv = CP.leaves_of(Z, N)
        assert np.array_equal(codes[lv][:, rep[cls]], codes[lv]), Z
    return t


@pytest.mark.parametrize("make", [CP.quadruples, CP.gapped, CP.few])
def test_every_bitset_of_a_small_alignment(make):
    check_blocks(make())


def test_quadruples_fill_whole_steps():
    t = _ffi.debug_clade_tables(CP.quadruples())
    assert t["U"] == 256
    assert [t["blocks"][Z]["U"] for Z in (7, 11, 13, 14, 15)] == [64, 64, 64, 64, 256]


def test_three_taxa_have_one_block():
    codes = SP.pool_codes(3, 200, 90, seed=5)
    t = check_blocks(codes)
    assert list(t["blocks"]) == [7] and t["blocks"][7]["U"] == 90


def test_primate():
    """The flagship: U = 413, 18 886 656 bytes; the whole clade is the global table; a sample of the others."""
    codes = codes_of(load_dataset('primate_data')['genome'])
    rng = np.random.default_rng(0)
    some = sorted({4095, 7, 0b111000000000, 0b101010101010} | {int(z) for z in rng.integers(0, 4096, size=40) if bin(int(z)).count("1") >= 3})
    t = check_blocks(codes, some)
    assert t["U"] == 413 and t["blocks"][4095]["U"] == 413 and t["layout"]["total"] == 18886656
    g = _ffi.debug_site_patterns(codes)
    assert np.array_equal(t["blocks"][4095]["image"], g["image"])
    assert np.array_equal(t["blocks"][4095]["rep_off"], g["rep_off"][:t["blocks"][4095]["rep_off"].size])


def test_rule_on_both_sides_of_the_cap():
    rule = _ffi.debug_clade_patterns_rule
    on, nbytes = rule(12, 898, 413)
    assert on and nbytes == 18886656 <= CP.MAX_BYTES
    assert rule(12, 898, 413, switch="force")[0]
    assert not rule(12, 898, 413, switch="0")[0]
    assert not rule(12, 898, 413, pat_taken=False)[0] and not rule(12, 898, 413, pat_taken=False, switch="force")[0]
    # the taxa: 3 .. 12
    assert not rule(2, 898, 20)[0] and rule(3, 898, 100)[0] and not rule(13, 898, 413)[0] and not rule(13, 898, 413, switch="force")[0]
    # the bytes: the layout's total against the cap, from both sides at N = 12 (the stride grows with S and with U)
    for N, S, U in ((12, 898, 413), (12, 898, 512), (12, 2048, 512), (12, 3072, 512), (12, 4096, 64), (11, 4096, 512), (5, 4096, 512)):
        want = CP.layout(N, S, U)["total"]
        got, nbytes = rule(N, S, U)
        assert nbytes == want and got == (want <= CP.MAX_BYTES), (N, S, U)
    assert rule(12, 2048, 512)[0] and not rule(12, 3072, 512)[0]
    assert CP.layout(12, 2048, 512)["total"] <= CP.MAX_BYTES < CP.layout(12, 3072, 512)["total"]


def test_plan_takes_the_form_only_with_records_and_tables():
    plan = _ffi.debug_sweep_plan_clade
    F = _ffi.FLAGS_DEFAULT
    assert plan(12, 2048, 898, flags=F) and plan(12, 40960, 898, G=20, flags=F)
    assert not plan(12, 2048, 898, clade_tables=False, flags=F)
    assert not plan(12, 2048, 898, flags=F | _ffi.KEEP_GRAPH) and not plan(12, 2048, 898, flags=F | _ffi.EAGER_NODES)
    assert not plan(12, 2048, 898, flags=F | _ffi.TWISTING)
    assert not plan(12, 2048, 898, K_local=1024, world=2, transport=True, flags=F)
    assert not plan(12, 2048, 4097, flags=F)                # two site tiles
    # the mask of the plain call is what it was: bit 27 is clear
    assert not _ffi.debug_sweep_plan(12, 2048, 898, flags=F)["mask"] >> 27 & 1


def test_header_under_sanitizers(tmp_path):
    """The builder with a main of its own (tests/clade_patterns_asan_main.cpp), address and undefined-behaviour sanitizers of the
    host compiler: host code, run as a program."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "clade_patterns_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "clade_patterns_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 values differ" in p.stdout
