"""The form of the reverse pass (phylo_amd/csrc/phylo_revlists.h: pg_plan_form before the first launch, pg_plan_chains once the
lists' counts are known) against a restatement of its rules in Python.  Every form computes the same bits, so a rule that silently
picks another form passes every other test and only shows as a slower step: this is where the selection itself is pinned.  No GPU:
phylo_debug_reverse_plan calls the two functions phylo_sweep_backward's driver calls."""
import itertools

import pytest

from phylo_amd import _ffi

DL_MAX_K = 8192                       # PG_DL_MAX_K (phylo_revlists_dev.h)
BG_MIN = 12 << 20                     # R K S from which the background launch and the reordering pay
SWITCHES = _ffi.PLAN_SWITCHES


def _rules(N, K, K_local, S, world, twist, marks, sw, n_slow, TS, coeff_wgs, in_flight):
    R = N - 1
    host_lists, one, two_s, rows_chain, coeff_chain = (name in sw for name in SWITCHES)
    p = {}
    p["rows_form"] = S <= 4096
    p["whole"] = world > 1
    p["early_free"] = p["rows_form"] and not twist and marks
    p["dev_lists"] = p["early_free"] and not p["whole"] and not host_lists and K_local == K and K <= DL_MAX_K
    p["sort_early"] = p["dev_lists"] and not one
    p["bg_free"] = p["early_free"] and not one and (two_s or R * K * S >= BG_MIN)
    p["two"] = not one and (two_s or R * K >= 65536 or p["bg_free"] or p["dev_lists"])
    p["parents_first"] = p["bg_free"] or p["dev_lists"]
    p["rows_all"] = (p["early_free"] and p["dev_lists"] and p["two"] and not rows_chain and n_slow > 0 and n_slow * TS <= 16384)
    p["rows_overlap"] = p["rows_all"] and n_slow * TS <= 512 and in_flight <= 1
    p["chunks_first"] = not p["rows_all"] or p["rows_overlap"]
    p["interleave"] = p["early_free"] and p["two"] and (p["bg_free"] or p["dev_lists"]) and not p["rows_all"]
    p["coeff_all"] = p["rows_all"] and R - 1 <= 64 and 0 < coeff_wgs <= 2048 and not coeff_chain
    return p


def _plan(N, K, S, **kw):
    out = _ffi.debug_reverse_plan(N, K, S, **kw)
    mask = out.pop("mask")
    assert mask == sum(int(out[name]) << i for i, name in enumerate(_ffi.PLAN_BITS))
    return out


# (N, K, S): every size threshold of pg_plan_form from both sides
SHAPES = [
    (12, 2048, 898),                  # primate.p: device lists, background launch
    (12, 64, 256),                    # small: device lists, no background launch
    (5, 64, 4096), (5, 64, 4097),     # rows form / tiles
    (12, 103991, 11),                 # R K S = 12 * 2^20 - 1 (= 11 * 11 * 103991), K beyond the device builders
    (4, 16384, 256),                  # R K S = 12 * 2^20, R K = 49152: the second stream hangs on the background launch alone
    (13, 2048, 512),                  # R K S = 12 * 2^20 with device lists
    (4, 21845, 8), (5, 16384, 8),     # R K = 65535 / 65536, neither background launch nor device lists
    (5, DL_MAX_K, 64), (5, DL_MAX_K + 1, 64),
    (66, 64, 64), (67, 64, 64),       # R - 1 = 64 / 65
    (2, 8, 16),
]
assert 11 * 103991 * 11 == BG_MIN - 1 and 3 * 16384 * 256 == BG_MIN == 12 * 2048 * 512 and 3 * 21845 == 65535
# (n_slow, TS): n_slow TS at 0, 512 / 513, 16384 / 16385, with one tile and with four
COUNTS = [(0, 1), (512, 1), (513, 1), (16384, 1), (16385, 1), (128, 4), (129, 4), (4096, 4), (4097, 4), (100, 4)]
COEFF_WGS = [0, 1, 2048, 2049]
SWITCH_SETS = [tuple(n for n, on in zip(SWITCHES, bits) if on) for bits in itertools.product((False, True), repeat=len(SWITCHES))]


@pytest.mark.parametrize("N,K,S", SHAPES)
def test_full_grid_against_the_rules(N, K, S):
    n = 0
    for twist, marks, (world, K_local) in itertools.product((False, True), (False, True), ((1, K), (2, K // 2), (1, K // 2))):
        for sw in SWITCH_SETS:
            for (n_slow, TS), wgs, in_flight in itertools.product(COUNTS, COEFF_WGS, (1, 2)):
                got = _plan(N, K, S, K_local=K_local, world=world, twisted=twist, marks=marks, switches=sw, n_slow=n_slow, TS=TS,
                            coeff_wgs=wgs, passes_in_flight=in_flight)
                want = _rules(N, K, K_local, S, world, twist, marks, sw, n_slow, TS, wgs, in_flight)
                assert got == want, (N, K, S, K_local, world, twist, marks, sw, n_slow, TS, wgs, in_flight)
                n += 1
    assert n == 2 * 2 * 3 * 32 * len(COUNTS) * 4 * 2


def test_each_threshold_flips_its_boolean():
    """the grid compares with the restatement; this states the sides outright"""
    assert _plan(5, 64, 4096)["rows_form"] and not _plan(5, 64, 4097)["rows_form"]
    assert not _plan(12, 103991, 11)["bg_free"] and _plan(4, 16384, 256)["bg_free"] and _plan(13, 2048, 512)["bg_free"]
    assert not _plan(12, 103991, 11)["parents_first"] and _plan(12, 103991, 11)["two"]       # (R K >= 65536 alone)
    assert not _plan(4, 21845, 8)["two"] and _plan(5, 16384, 8)["two"]
    assert _plan(4, 16384, 256)["two"] and not _plan(4, 16384, 256, switches=("one_stream",))["two"]
    assert _plan(5, DL_MAX_K, 64)["dev_lists"] and not _plan(5, DL_MAX_K + 1, 64)["dev_lists"]
    base = dict(n_slow=100, TS=4, coeff_wgs=300)
    for n_slow, TS, rows_all, overlap in ((512, 1, True, True), (513, 1, True, False), (128, 4, True, True), (129, 4, True, False),
                                          (16384, 1, True, False), (16385, 1, False, False), (4097, 4, False, False), (0, 1, False, False)):
        p = _plan(12, 2048, 898, n_slow=n_slow, TS=TS, coeff_wgs=300)
        assert (p["rows_all"], p["rows_overlap"]) == (rows_all, overlap), (n_slow, TS)
        assert p["chunks_first"] == (not rows_all or overlap) and p["interleave"] == (not rows_all)
    for wgs, want in ((0, False), (1, True), (2048, True), (2049, False)):
        assert _plan(12, 2048, 898, n_slow=100, TS=4, coeff_wgs=wgs)["coeff_all"] == want
    assert _plan(66, 64, 64, **base)["coeff_all"] and not _plan(67, 64, 64, **base)["coeff_all"]
    assert _plan(67, 64, 64, **base)["rows_all"]
    assert _plan(12, 2048, 898, **base)["rows_overlap"] and not _plan(12, 2048, 898, passes_in_flight=2, **base)["rows_overlap"]
    assert _plan(12, 2048, 898, passes_in_flight=2, **base)["rows_all"]


PRIMATE = dict(n_slow=100, TS=4, coeff_wgs=300)       # primate.p, K = 2048: about 100 adopted nodes, 898 sites = 4 tiles


def test_primate_default_and_each_switch():
    p = _plan(12, 2048, 898, **PRIMATE)
    assert p == dict(rows_form=True, whole=False, early_free=True, dev_lists=True, sort_early=True, bg_free=True, two=True,
                     parents_first=True, rows_all=True, rows_overlap=True, chunks_first=True, interleave=False, coeff_all=True)
    host = _plan(12, 2048, 898, switches=("rev_host_lists",), **PRIMATE)
    assert host == dict(p, dev_lists=False, sort_early=False, rows_all=False, rows_overlap=False, interleave=True, coeff_all=False)
    one = _plan(12, 2048, 898, switches=("one_stream",), **PRIMATE)
    assert one == dict(p, sort_early=False, bg_free=False, two=False, rows_all=False, rows_overlap=False, coeff_all=False)
    assert one["dev_lists"] and one["parents_first"] and not one["interleave"]
    assert _plan(12, 2048, 898, switches=("two_streams",), **PRIMATE) == p
    rows = _plan(12, 2048, 898, switches=("rows_chain",), **PRIMATE)
    assert rows == dict(p, rows_all=False, rows_overlap=False, interleave=True, coeff_all=False)
    coeff = _plan(12, 2048, 898, switches=("coeff_chain",), **PRIMATE)
    assert coeff == dict(p, coeff_all=False)
    both = _plan(12, 2048, 898, switches=("rows_chain", "coeff_chain"), **PRIMATE)
    assert both == rows
    # PHYLO_EAGER_NODES: the sweep leaves no marks
    eager = _plan(12, 2048, 898, marks=False, **PRIMATE)
    assert eager == dict(rows_form=True, whole=False, early_free=False, dev_lists=False, sort_early=False, bg_free=False, two=False,
                         parents_first=False, rows_all=False, rows_overlap=False, chunks_first=True, interleave=False, coeff_all=False)


@pytest.mark.parametrize("kw", [dict(twisted=True), dict(world=2, K_local=1024), dict(S=4097), dict(S=8192, twisted=True)])
def test_twisted_sharded_and_long_rows_take_host_lists_and_a_launch_per_rank_event(kw):
    kw = dict(kw)
    S = kw.pop("S", 898)
    for sw in SWITCH_SETS:
        p = _plan(12, 2048, S, switches=sw, **kw, **PRIMATE)
        assert not p["dev_lists"] and not p["sort_early"] and not p["rows_all"] and not p["rows_overlap"] and not p["coeff_all"]
        assert p["chunks_first"]
        assert p["whole"] == ("world" in kw)
        if "world" not in kw:            # no early pg_nodes_free either: parents' lists behind the coefficient chain, nothing in turn
            assert not p["early_free"] and not p["bg_free"] and not p["parents_first"] and not p["interleave"]


def test_small_sweep_has_no_background_launch():
    p = _plan(12, 64, 256, n_slow=40, TS=1, coeff_wgs=120)
    assert p["dev_lists"] and p["two"] and not p["bg_free"] and p["parents_first"]
    assert p["rows_all"] and p["rows_overlap"] and p["coeff_all"]
    assert _plan(12, 64, 256, switches=("two_streams",), n_slow=40, TS=1, coeff_wgs=120)["bg_free"]
    host = _plan(12, 64, 256, switches=("rev_host_lists",), n_slow=40, TS=1, coeff_wgs=120)
    assert not host["bg_free"] and not host["two"] and not host["parents_first"] and not host["interleave"]


def test_chains_without_counts_are_final_when_the_parents_lists_come_late():
    """the driver issues the coefficient chain before it knows the counts exactly when parents_first is false: there the second
    half of the plan must not depend on them"""
    for (N, K, S), twist, marks, sw in itertools.product(SHAPES, (False, True), (False, True), SWITCH_SETS):
        first = _plan(N, K, S, twisted=twist, marks=marks, switches=sw, n_slow=0, TS=1, coeff_wgs=0)
        if first["parents_first"]:
            continue
        for (n_slow, TS), wgs in itertools.product(COUNTS, COEFF_WGS):
            assert _plan(N, K, S, twisted=twist, marks=marks, switches=sw, n_slow=n_slow, TS=TS, coeff_wgs=wgs) == first


def test_bad_arguments_are_refused():
    for kw in (dict(N=1), dict(K=0), dict(S=0), dict(world=0), dict(TS=0), dict(n_slow=-1), dict(coeff_wgs=-1)):
        args = dict(N=12, K=64, S=256)
        args.update(kw)
        with pytest.raises(_ffi.PhyloError):
            _ffi.debug_reverse_plan(**args)
