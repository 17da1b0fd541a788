"""The tail of the resampling scan alone (pp_scan_ancestors, phylo_persist.h; the chain form of a rank event):
every particle's ancestor of the next rank event, the ascending list of the adopted particles of each group and its count, through
phylo_debug_scan_ancestors on caller-given log-weights, seeds and rank event.

References, equal bits throughout:
  * the resampling the library had before, phylo_resample group by group (its cdf, pk_cdf_search with the draw of Philox counter
    (k, r, RESAMPLE, 0) under the group's seed), for every case;
  * a NumPy restatement -- phylo_amd/rng.py for Philox, thr = mulhi64(draw, total), searchsorted(cdf, thr, 'right') -- wherever
    the cdf is known in closed form: integer weights floor(exp(logw - max) 2^44), which is 2^44 at the maximum, 0 at -inf, at NaN
    and 700 below the maximum, and 1 for everybody in the all-bad branch.
The list must be ascending without duplicates, hold exactly the sorted unique ancestors, and nothing behind its count may have been
written (the hook presets -1)."""
import numpy as np
import pytest

from phylo_amd import _ffi, rng

pytestmark = pytest.mark.gpu

KGS = (1, 2, 63, 64, 65, 511, 513, 2047, 2048, 2049, 4096)
GS = (1, 3, 20)
ONE = 1 << 44


@pytest.fixture(scope="module")
def ctx():
    with _ffi.Context(4, 5, 10) as c:
        yield c


def weights(kind, G, Kg, seed):
    """([G][Kg] log-weights, [G][Kg] integer weights or None where only the device knows them)"""
    r = np.random.default_rng(seed)
    if kind == 'equal':
        return np.full((G, Kg), -3.25), np.full((G, Kg), ONE, dtype=object)
    if kind == 'one-heavy':
        w = r.normal(size=(G, Kg))
        iw = np.zeros((G, Kg), dtype=object)
        for g in range(G):
            h = (0, Kg - 1, Kg // 2)[g % 3]
            w[g, h] += 700.0 + 2.0 * np.abs(w[g]).max()
            iw[g, h] = ONE
        return w, iw
    if kind == 'all-neg-inf':
        return np.full((G, Kg), -np.inf), np.full((G, Kg), 1, dtype=object)
    if kind == 'all-nan':
        return np.full((G, Kg), np.nan), np.full((G, Kg), 1, dtype=object)
    if kind in ('half-neg-inf', 'half-nan'):
        # zero-width intervals at both ends and in runs: never adopted.  (One live particle at least; Kg = 1 has only that one.)
        bad = r.random((G, Kg)) < 0.5
        bad[:, 0] = True
        bad[:, -1] = True
        live = np.array([r.integers(0, Kg) for _ in range(G)])
        bad[np.arange(G), live] = False
        w = np.where(bad, -np.inf if kind == 'half-neg-inf' else np.nan, 1.5)
        return w, np.where(bad, 0, ONE).astype(object)
    if kind == 'underflow':
        # a spread of 2000 in log: exp underflows to integer weight 0 for most, partial weights in between
        return -np.abs(r.normal(size=(G, Kg))) * r.choice([0.5, 20.0, 400.0], size=(G, Kg)), None
    raise KeyError(kind)


def restated(iw, seed, r_next):
    Kg = len(iw)
    cdf = np.cumsum(iw)                                    # Python integers: exact
    total = int(cdf[-1])
    x, y, _, _ = rng.philox4x32(np.arange(Kg), r_next, rng.STREAM_RESAMPLE, 0, int(seed))
    draws = (y.astype(object) << 32) | x.astype(object)
    thr = np.array([(int(d) * total) >> 64 for d in draws], dtype=object)
    return np.searchsorted(cdf, thr, 'right').astype(np.int64)             # (object arrays: exact integer comparisons)


def check(ctx, kind, G, Kg, r_next):
    seeds = np.array([0x9E3779B97F4A7C15 * (g + 1) % (1 << 64) ^ (Kg * 1000003 + r_next) for g in range(G)], dtype=np.uint64)
    logw, iw = weights(kind, G, Kg, 7 * Kg + G)
    anc, lst, cnt = ctx.debug_scan_ancestors(logw, seeds, r_next)
    tag = "%s G=%d Kg=%d" % (kind, G, Kg)
    for g in range(G):
        ref = ctx.resample(logw[g], int(seeds[g]), r_next)
        np.testing.assert_array_equal(anc[g], ref, err_msg=tag + " group %d: ancestors against phylo_resample" % g)
        if iw is not None and (g < 2 or Kg <= 513):        # (the restatement walks Python integers: the first groups of the large cases)
            np.testing.assert_array_equal(anc[g], restated(iw[g], seeds[g], r_next), err_msg=tag + " group %d: restatement" % g)
            assert all(iw[g][a] > 0 for a in np.unique(anc[g])), tag + ": a zero-width interval was adopted"
        uniq = np.unique(ref)
        assert cnt[g] == len(uniq), (tag, g, cnt[g], len(uniq))
        np.testing.assert_array_equal(lst[g, :cnt[g]], uniq, err_msg=tag + " group %d: the list" % g)
        assert (np.diff(lst[g, :cnt[g]]) > 0).all(), tag + ": the list is not strictly ascending"
        assert (lst[g, cnt[g]:] == -1).all(), tag + ": written behind the count"
        if kind == 'one-heavy':
            assert cnt[g] == 1
    return cnt


@pytest.mark.parametrize("kind", ['equal', 'one-heavy', 'all-neg-inf', 'all-nan', 'half-neg-inf', 'half-nan', 'underflow'])
def test_tail_against_the_search(ctx, kind):
    for Kg in KGS:
        assert ctx.debug_scan_form(Kg) == 'lds512'
        for G in GS:
            cnt = check(ctx, kind, G, Kg, r_next=1 + (Kg + G) % 10)
            if kind == 'equal' and Kg >= 511:              # 1 - 1/e of the particles are adopted: the list is long
                assert (cnt > 0.55 * Kg).all() and (cnt < 0.72 * Kg).all(), cnt


def test_sixteen_waves(monkeypatch):
    """pp_resample_scan<1024> (groups above 4096 weights when PHYLO_SCAN_MULTI_MIN leaves them to one workgroup): up to sixteen rows
    of 64 per wave in the compaction, LDS beyond 64 KiB"""
    monkeypatch.setenv('PHYLO_SCAN_MULTI_MIN', str(1 << 20))
    with _ffi.Context(4, 5, 10) as c:
        for Kg in (4097, 8192, 16384):
            assert c.debug_scan_form(Kg) == 'lds1024'
            for kind in ('equal', 'half-nan', 'underflow'):
                check(c, kind, 2, Kg, r_next=3)


def test_refused_without_the_cdf_in_lds(ctx):
    """several workgroups per group (above PHYLO_SCAN_MULTI_MIN) have no place for the tail: an error, not another answer"""
    assert ctx.debug_scan_form(4097) == 'multi'
    with pytest.raises(_ffi.PhyloError):
        ctx.debug_scan_ancestors(np.zeros((1, 4097)), np.array([1], dtype=np.uint64), 1)
