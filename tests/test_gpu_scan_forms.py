"""The four forms of the resampling scan (launch_scan, phylo_hip.hip; the rule is sweep_scan_form_of, phylo_sweep_plan.h) bit for
bit against the oracle.  At the default PHYLO_SCAN_MULTI_MIN (4096) a group of more than 4096 weights goes to the scan of several
workgroups, so pp_resample_scan<1024> (16 waves, the cdf in up to 128 KiB of dynamic LDS) and pk_resample_scan(_groups) (staged in
the cdf buffer itself) run only when the switch is raised, and the scan of several workgroups sees small groups only when it is
lowered.  Both are done here.  The switch is read when a context is created, so it is set before the context is made, and every
test asks its context through phylo_debug_scan_form which form it takes BEFORE it compares: a switch that is not read fails there.

Also here, in every form: a +inf log-weight.  The contract (the oracle's all_bad = !(m > -inf) || m == inf)
makes the draw uniform and the log-normaliser's row 0."""
import numpy as np
import pytest

import large_launch_cases as LC
import test_gpu_large_launch as LL
from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset

pytestmark = pytest.mark.gpu
SWITCH = 'PHYLO_SCAN_MULTI_MIN'
NEVER_MULTI = str(1 << 30)
SCALES = (0.5, 30.0, 400.0)


def make_ctx():
    g = load_dataset('primate_data_wang')['genome'][:3, :16]
    ctx = _ffi.Context(2, 3, 16)
    ctx.set_leaves(g)
    ctx.set_model(O.jc_Q(), np.full((1, 4), 0.25), np.full(2, 10.0), np.full(2, 10.0), jc69_closed_form=False)
    return ctx


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def resample_equals_oracle(ctx, lw, seed, step, numpy_too=False):
    idx = ctx.resample(lw, seed=seed, step=step)
    np.testing.assert_array_equal(idx, CO.resample(lw, seed, step))
    if numpy_too:
        np.testing.assert_array_equal(idx, O.resample_indices(lw, seed, step))
    assert idx.min() >= 0 and idx.max() < lw.size
    return idx


def logz_equals_oracle(ctx, lw, what):
    z, want = ctx.log_zsmc(lw), CO.log_zsmc(lw)
    assert not np.isnan(want) and bits(z) == bits(want), "%s: log Z %r against the oracle's %r" % (what, z, want)
    return z


def inf_rows(K, rng):
    """(name, log-weights): +inf among finite weights, at index 0 and at index K - 1 -- all_bad by the contract: a uniform draw"""
    rows = []
    for name, at in (("+inf among finite", K // 3), ("+inf at index 0", 0), ("+inf at index K - 1", K - 1)):
        lw = rng.normal(scale=30.0, size=K) - 6000.0
        lw[at] = np.inf
        rows.append((name, lw))
    return rows


def check_inf_rows(ctx, K, rng):
    uniform = CO.resample(np.full(K, -np.inf), 5, 2)        # nothing finite: the other all_bad row
    for name, lw in inf_rows(K, rng):
        idx = resample_equals_oracle(ctx, lw, 5, 2, numpy_too=K <= 9000)
        np.testing.assert_array_equal(idx, uniform, err_msg="%s, K = %d: the draw is not the uniform one" % (name, K))
        z = logz_equals_oracle(ctx, np.stack([lw, rng.normal(scale=20.0, size=K) - 500.0]), "%s, K = %d" % (name, K))
        assert np.isfinite(z)


def check_edge_rows(ctx, K, rng):
    lw = rng.normal(scale=40.0, size=K)
    lw[::11] = np.nan                                       # NaN at every 11th weight: never drawn
    idx = resample_equals_oracle(ctx, lw, 5, 2)
    assert not np.isin(idx, np.arange(0, K, 11)).any()
    lw = np.full(K, -np.inf)
    lw[K - 1] = 3.0                                         # one survivor, the last index
    assert (resample_equals_oracle(ctx, lw, 1, 1) == K - 1).all()
    resample_equals_oracle(ctx, np.full(K, -np.inf), 5, 2)  # nothing finite: uniform
    check_inf_rows(ctx, K, rng)


# ---- PHYLO_SCAN_MULTI_MIN = 2^30: one workgroup per group at every size --------------------------------------------------------
LDS1024_KS = (4097, 5000, 8192, 8193, 12000, 16383, 16384)    # pp_resample_scan<1024>; the last is the largest LDS request
IN_PLACE_KS = (16385, 18432, 20003, 100001)                   # pk_resample_scan: a last tile of one weight; whole tiles; a ragged
#                                                               8-element tail (the scalar loads and stores of the last thread)


@pytest.mark.parametrize("K", LDS1024_KS + IN_PLACE_KS)
def test_resample_one_workgroup_forms(monkeypatch, K):
    monkeypatch.setenv(SWITCH, NEVER_MULTI)
    rng = np.random.default_rng(4)
    with make_ctx() as ctx:
        assert ctx.debug_scan_form(K) == ("lds1024" if K <= 16384 else "in_place")
        for scale in SCALES:
            lw = rng.normal(scale=scale, size=K) - 6000.0
            resample_equals_oracle(ctx, lw, 11, 3, numpy_too=True)


@pytest.mark.parametrize("K,form", [(5000, "lds1024"), (20000, "in_place")])
def test_log_zsmc_one_workgroup_forms(monkeypatch, K, form):
    """the log-normaliser alone: no cdf is wanted, nothing is staged"""
    monkeypatch.setenv(SWITCH, NEVER_MULTI)
    rng = np.random.default_rng(4)
    with make_ctx() as ctx:
        assert ctx.debug_scan_form(K) == form
        logz_equals_oracle(ctx, rng.normal(scale=20, size=(5, K)) - 500, "%d weights per row" % K)


@pytest.mark.parametrize("K,form", [(9000, "lds1024"), (20003, "in_place")])
def test_edge_rows_one_workgroup_forms(monkeypatch, K, form):
    monkeypatch.setenv(SWITCH, NEVER_MULTI)
    with make_ctx() as ctx:
        assert ctx.debug_scan_form(K) == form
        check_edge_rows(ctx, K, np.random.default_rng(K))


@pytest.mark.parametrize("K,form", [(300, "lds512"), (9000, "multi")])
def test_plus_infinity_at_the_default_forms(monkeypatch, K, form):
    monkeypatch.delenv(SWITCH, raising=False)
    with make_ctx() as ctx:
        assert ctx.debug_scan_form(K) == form
        check_inf_rows(ctx, K, np.random.default_rng(K))


SWEEPS = {"grouped-8194": "lds1024",       # G = 2, lse_stride, Kg = 4097
          "sorted-exact": "lds1024",       # G = 2, Kg = 16384: the largest LDS request with log Z folded into the last scan
          "jc-33282": "in_place",          # pk_resample_scan_groups, then pk_logz_total_groups
          "single-33282": "in_place"}      # pk_resample_scan, then pk_logz_total


@pytest.mark.parametrize("name", list(SWEEPS))
def test_sweeps_one_workgroup_forms(monkeypatch, name):
    monkeypatch.setenv(SWITCH, NEVER_MULTI)
    c = LC.CASES[name]
    plan = _ffi.debug_sweep_plan(c["N"], c["G"] * c["Kg"], c["S"], G=c["G"], switches=('jc',) if c["jc"] else ())
    assert {k: plan[k] for k in c["plan"]} == c["plan"]     # (the plan does not know the scan's form: fold_logz is a size rule)
    with LL.make_ctx(name) as ctx:
        assert ctx.debug_scan_form(c["Kg"]) == SWEEPS[name]
        out, logz = LL.run(ctx, name)
        assert out['stats']['n_launches'] == LL.launches(name)
        LL.same_as_oracle(out, logz, name, "one workgroup per group")


# ---- PHYLO_SCAN_MULTI_MIN = 64: several workgroups per group at sizes the default never gives them ----------------------------
@pytest.mark.parametrize("K", [65, 100, 2048, 2049, 4096])   # one tile; a whole tile; two tiles, one weight in the second; two whole
def test_resample_small_groups_by_several_workgroups(monkeypatch, K):
    monkeypatch.setenv(SWITCH, '64')
    rng = np.random.default_rng(4)
    with make_ctx() as ctx:
        assert ctx.debug_scan_form(K) == "multi" and ctx.debug_scan_form(64) == "lds512"
        for scale in SCALES:
            lw = rng.normal(scale=scale, size=K) - 6000.0
            resample_equals_oracle(ctx, lw, 11, 3, numpy_too=True)
        if K == 100:
            resample_equals_oracle(ctx, np.full(K, -np.inf), 5, 2, numpy_too=True)
