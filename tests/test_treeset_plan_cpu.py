"""The plans of the scored-tree-set calls without a GPU: every call states its slab as a list of regions
and one slab builder (phylo_treeset_plan.h) turns the list into bytes per tree, chunk, grid, offsets and total.

(a) the plans are, value for value, what the plan functions gave before they shared that builder (tests/golden/treeset_plans.txt);
for the two loglik calls, whose slab went from 16-byte to 256-byte regions, chunk, the site row and the bytes per tree are;
(b) pt2_make_plan under the host compiler's sanitizers, checked by the generic plan check."""
import os
import shutil
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden", "treeset_plans.txt")


def _build(tmp_path, src, name, flags):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / name)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + flags +
                          ["-I", os.path.join(ROOT, "phylo_amd", "csrc"), os.path.join(ROOT, "tests", src), "-o", exe])
    return exe


def test_plans_are_the_recorded_ones(tmp_path):
    """tests/treeset_plan_table_main.cpp prints one line per plan over a thinned grid of N, tiles, T, compute units, chunk caps,
    leaf forms, categories, directions, option bits and S; every value equals the recorded one.  A loglik line carries its total
    and offsets behind a bar: they are not compared (the alignment changed), but the total is the packed sum plus at most one
    alignment gap per region."""
    exe = _build(tmp_path, "treeset_plan_table_main.cpp", "treeset_plan_table", [])
    out = subprocess.run([exe], stdout=subprocess.PIPE, check=True, timeout=120).stdout.decode().splitlines()
    with open(GOLDEN) as f:
        want = [ln.rstrip("\n") for ln in f if not ln.startswith("#")]
    assert len(out) == len(want) and len(want) == 46 * 9
    calls = set()
    for got, ref in zip(out, want):
        head, _, tail = got.partition(" |")
        assert head == ref
        calls.add(ref.split()[0])
        if tail:
            assert ref.startswith("pt2 ")
            chunk, per_tree = int(ref.split()[-3]), int(ref.split()[-1])
            offs = [int(x) for x in tail.split()]
            total, offs = offs[0], offs[1:]
            assert all(o % 256 == 0 for o in offs) and offs == sorted(offs) and offs[-1] <= total
            assert chunk * per_tree + 256 <= total <= chunk * per_tree + 256 + 255 * 8
        else:
            assert not ref.startswith("pt2 ")
    assert calls == {"pt2", "ptg", "ptgr", "ptm", "ptn", "ptnr", "pta", "ptar"}


def test_loglik_plan_under_sanitizers(tmp_path):
    """pt2_make_plan with a main of its own (tests/treeset_asan_main.cpp), address and undefined-behaviour sanitizers of the host
    compiler: host code, run as a program, nothing loaded into Python."""
    exe = _build(tmp_path, "treeset_asan_main.cpp", "treeset_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0, p.stdout.decode()[-2000:]
    assert b"0 values differ" in p.stdout
