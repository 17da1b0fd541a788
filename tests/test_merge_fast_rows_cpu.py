"""The speculative updates of the running site product that pk_rank_merge_nostore's fast row loops use (phylo_amd/csrc/phylo_math.h:
pm_lp_mul2_spec, pm_lp_mul2_spec_q, pm_lp_mul_spec) against pm_lp_mul2 / pm_lp_mul -- no GPU: the header in a stand-alone program
(tests/merge_fast_rows_main.cpp) under the host compiler's address and undefined-behaviour sanitizers.  Flag clear => the three
fields are bit-equal; the reference takes its fall-back <=> flag set; every class of input occurred."""
import os
import re
import shutil
import subprocess

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CLASSES = ("kept", "x1", "x2", "small", "inf", "single_normal", "single_zero", "single_subnormal", "single_negative", "single_inf",
           "single_nan", "q_kept", "q_small", "q_inf")


def test_speculative_updates_against_the_pair_form(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "merge_fast_rows")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "phylo_amd", "csrc"),
                           os.path.join(ROOT, "tests", "merge_fast_rows_main.cpp"), "-o", exe])
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    out = p.stdout.decode()
    assert p.returncode == 0, out[-3000:]
    assert "\n0 failures" in out, out[-3000:]
    line = [l for l in out.splitlines() if l.startswith("classes:")]
    assert len(line) == 1, out[-3000:]
    counts = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line[0])}
    print(counts)
    for c in CLASSES:
        assert counts.get(c, 0) > 0, "class %r never occurred: %r" % (c, counts)
    assert counts["kept"] + counts["x1"] + counts["x2"] + counts["small"] + counts["inf"] >= 1000000
    # the weighting: products near the subnormal edge and near overflow fall on both sides of it, in numbers
    assert counts["small"] > 10000 and counts["inf"] > 10000 and counts["kept"] > 100000
