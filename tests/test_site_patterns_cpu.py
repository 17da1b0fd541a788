"""The site-pattern tables of a coded alignment and the rule that decides whether pk_rank_merge_nostore takes the pattern form
(phylo_amd/csrc/phylo_site_patterns.h, built by phylo_set_leaves) against a NumPy restatement -- no GPU: the exported builder
(phylo_debug_site_patterns) and rule (phylo_debug_site_patterns_rule), and the header alone in a stand-alone program under the
host's address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import packed_codes_cases as PC
import site_patterns_cases as SP
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def codes_of(genome):
    """byte codes of a one-hot / all-ones alignment [N][S][4]"""
    return np.where(genome.sum(axis=2) == 4, 4, genome.argmax(axis=2)).astype(np.uint8)


def check_tables(codes, want_U):
    N, S = codes.shape
    t = _ffi.debug_site_patterns(codes)
    U, rep = t["U"], t["rep"]
    assert U == want_U
    assert rep.shape == (U,) and (np.diff(rep) > 0).all() and (U == 0 or rep[0] == 0)
    pat, pads = SP.decode_image(t["image"], S)
    assert t["image"].shape == (PC.n_chunks(S), 2, 64, 8)
    assert (pat < U).all() and np.array_equal(codes[:, rep[pat]], codes)      # columns[rep[pat[s]]] == columns[s] for every s
    assert np.array_equal(pat[rep], np.arange(U)) and (rep[pat] <= np.arange(S)).all()   # numbered by first occurrence
    assert (pads == 8 * U).all() and pads.size == PC.n_chunks(S) * 1024 - S   # the pad entry at every site >= S
    if U <= SP.CAP:
        off = t["rep_off"]
        assert np.array_equal(off[:U], 32 * rep.astype(np.uint32)) and not off[U:].any()
        assert np.array_equal(t["rep_leaf"], PC.packed_reference(codes[:, rep]))
    else:
        assert t["rep_off"] is None and t["rep_leaf"] is None
    return t


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 898, 1024, 1025, 2049])
def test_all_columns_equal(S):
    codes = np.repeat(np.array([[0], [4], [2], [4], [1]], dtype=np.uint8), S, axis=1)
    check_tables(codes, 1)


@pytest.mark.parametrize("S", [1, 2, 64, 65, 512, 513, 898, 2049])
def test_all_columns_distinct(S):
    check_tables(SP.pool_codes(5, S, S, seed=S), S)


@pytest.mark.parametrize("S,U", [(898, 1), (898, 63), (898, 64), (898, 65), (898, 512), (898, 513), (2048, 512), (1025, 300)])
def test_pools(S, U):
    check_tables(SP.pool_codes(5, S, U, seed=S + U), U)


def test_primate():
    g = load_dataset('primate_data')['genome']
    assert g.shape[:2] == (12, 898)
    check_tables(codes_of(g), 413)


def test_more_columns_than_the_image_holds():
    codes = SP.pool_codes(6, 9000, 8192, seed=3)
    t = _ffi.debug_site_patterns(codes)
    assert t["U"] == 8192 and t["image"] is None and t["rep_off"] is None and len(t["rep"]) == 8192


def test_rule_on_both_sides_of_its_thresholds():
    rule = _ffi.debug_site_patterns_rule
    # the cap: 512 on, 513 off, whatever the switch
    for sw in (None, "force"):
        assert rule(2048, 512, switch=sw) and not rule(2048, 513, switch=sw)
    # one tile, coded leaves, the switch
    assert rule(898, 413) and not rule(898, 413, ntiles=2) and not rule(898, 413, coded=False) and not rule(898, 413, switch="0")
    assert not rule(898, 413, ntiles=2, switch="force") and not rule(898, 413, coded=False, switch="force")
    assert not rule(898, 0) and not rule(898, 0, switch="force")
    # the margin: for every number of steps the largest nU that is taken, and the one after it that is not
    seen_on = seen_off = 0
    for nS in range(1, 33):
        for nU in range(1, min(nS, 8) + 1):
            want = 10 * (nU * SP.C_PHASE1 + nS * SP.C_WALK + SP.C_FIXED) <= 8 * nS * SP.C_STEP
            for S in (64 * nS - 63, 64 * nS):
                for U in (64 * nU - 63, 64 * nU):
                    if U <= S:
                        assert rule(S, U) == want == SP.rule(S, U), (S, U)
                        assert rule(S, U, switch="force")
            seen_on += want
            seen_off += not want
    assert seen_on >= 10 and seen_off >= 10                 # the grid has both sides
    # the bundled alignments: primate.p 15 -> 7 steps; hohna_DS5 6 -> 4, too little; DS1's U is over the cap
    assert rule(898, 413) and rule(738, 311) and rule(1133, 489) and rule(1008, 406) and not rule(1949, 934)
    assert not rule(378, 256) and rule(378, 192) and not rule(64, 64) and not rule(128, 64) and rule(192, 64) and not rule(192, 65)


def test_header_under_sanitizers(tmp_path):
    """The header with a main of its own (tests/site_patterns_asan_main.cpp), address and undefined-behaviour sanitizers of the host
    compiler: host code, run as a program."""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "site_patterns_asan")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", "site_patterns_asan_main.cpp"),
                           "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 values differ" in p.stdout
