"""What tests/test_gpu_large_launch.py stands on, checked without a GPU for every case of tests/large_launch_cases.py: the plan
bits the case claims are the ones phylo_debug_sweep_plan gives (a threshold that moves later fails HERE instead of leaving the
GPU test green and vacuous), the oracle's sweeps are usable as a reference (finite, no rank event collapsed to one ancestor),
and the oracle's branch lengths fall into the Pade classes the case is there for."""
import numpy as np
import pytest

import large_launch_cases as LC
from phylo_amd import _ffi


def plan_of(name, flags=0):
    c = LC.CASES[name]
    return _ffi.debug_sweep_plan(c["N"], c["G"] * c["Kg"], c["S"], G=c["G"], flags=flags, switches=('jc',) if c["jc"] else ())


@pytest.mark.parametrize("name", LC.NAMES)
def test_plan_bits_are_the_claimed_ones(name):
    c = LC.CASES[name]
    p = plan_of(name)
    assert {k: p[k] for k in c["plan"]} == c["plan"]
    assert p["lazy"] and p["mat_after_book"] and not p["book_mat"] and not p["shard_form"] and p["one_tile"]
    R = c["N"] - 1
    # begin; bookkeeping, merge, scan (+ the adopted nodes from the second rank event on); pk_logz_total(_groups) unless folded
    assert p["launches"] == [1, 3] + [4] * (R - 1) + [0 if c["plan"]["fold_logz"] else 1]
    if c["eager"]:
        e = plan_of(name, _ffi.EAGER_NODES)
        assert {k: e[k] for k in c["plan"]} == dict(c["plan"], use_rec=False) and not e["lazy"]
        assert e["launches"] == [1] + [3] * R + [0 if c["plan"]["fold_logz"] else 1]


def test_every_form_is_claimed_by_a_case():
    """each large-launch form by name, and both sides of the bits that only some cases set"""
    plans = {n: dict(LC.CASES[n]["plan"], G=LC.CASES[n]["G"], Kg=LC.CASES[n]["Kg"], K=LC.CASES[n]["G"] * LC.CASES[n]["Kg"])
             for n in LC.NAMES}
    assert any(p["sorted_prologue"] for p in plans.values()) and any(not p["sorted_prologue"] for p in plans.values())
    assert any(not p["fold_logz"] and p["G"] == 1 for p in plans.values())                  # pk_logz_total
    assert any(not p["fold_logz"] and p["G"] > 1 for p in plans.values())                   # pk_logz_total_groups
    assert any(p["G"] > 1 and p["Kg"] > 4096 and p["fold_logz"] for p in plans.values())    # pp_scan_multi_*, G > 1, folded log Z
    assert any(p["G"] > 1 and p["Kg"] > 4096 and not p["fold_logz"] for p in plans.values())
    assert any(p["G"] > 1 and p["mat_grouped"] for p in plans.values())
    assert any(p["book_width"] == 8 and p["Kg"] % 8 for p in plans.values())                 # a group boundary inside a wave
    assert any(p["G"] == 64 for p in plans.values())                                        # PK_MAX_GROUPS
    ragged = plans["sorted-ragged"]
    assert 2 * 4 * ragged["K"] == 260 * 1024 + 16 and 2 * 4 * plans["sorted-exact"]["K"] == 262144
    assert -(-ragged["Kg"] // 2048) == 9 and ragged["Kg"] - 8 * 2048 == 257                 # tiles of the scan, the last one's weights
    assert -(-plans["grouped-8194"]["Kg"] // 2048) == 3 and plans["grouped-8194"]["Kg"] - 2 * 2048 == 1


@pytest.mark.parametrize("name", LC.NAMES)
def test_oracle_sweeps_are_a_usable_reference(name):
    c = LC.CASES[name]
    refs = LC.reference(name)
    assert len(refs) == c["G"]
    for i, ref in enumerate(refs):
        assert np.isfinite(ref["log_weights"]).all() and np.isfinite(ref["log_likelihood"]).all() and np.isfinite(ref["logZ"]), i
        assert ref["ancestors"].shape == (c["N"] - 2, c["Kg"])
        for r, row in enumerate(ref["ancestors"]):
            assert len(np.unique(row)) > 1, "group %d rank event %d collapsed to one ancestor" % (i, r + 1)


@pytest.mark.parametrize("name", [n for n in LC.NAMES if LC.CASES[n]["classes"]])
def test_pade_classes_of_the_oracle_branch_lengths(name):
    c = LC.CASES[name]
    Q = LC.model(name)[1]
    for i, ref in enumerate(LC.reference(name)):
        b = np.concatenate([ref["left_branches"].ravel(), ref["right_branches"].ravel()])
        cls, nrm = LC.pade_classes(Q, b)
        frac = np.bincount(cls, minlength=5) / cls.size
        print("%s group %d: classes %s, scaled %.4f" % (name, i, np.round(frac, 4), (nrm > LC.PADE_THETA13).mean()))
        if c["classes"] == "all":
            assert (frac > 0).all(), frac
        elif c["classes"] == "short":
            assert frac[0] == 1.0, frac
        elif c["classes"] == "long":
            assert frac[4] >= 0.9 and (nrm > LC.PADE_THETA13).mean() >= 0.8, frac
        else:
            assert c["classes"] == "sides"
            assert frac[0] >= 0.4 and frac[4] >= 0.4, frac
            cl, _ = LC.pade_classes(Q, ref["left_branches"].ravel())
            cr, _ = LC.pade_classes(Q, ref["right_branches"].ravel())
            assert ((cl == 4) & (cr == 0)).mean() >= 0.4     # the two sides of ONE particle in opposite classes
