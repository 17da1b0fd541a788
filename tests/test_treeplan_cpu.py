"""The form of the tree posterior's two passes (phylo_amd/csrc/phylo_trees_plan.h: pt_plan_form / pb_plan_form, the layouts of
scratch slots 12 and 13, pt_plan_launches / pb_plan_launches) against a restatement in Python of the rules as tree_summary_impl and
tree_branches_impl spelled them before there was a plan: the take() sequence line by line, each sort's bit count, wide, gather,
the refusals and the launch counts.  The wide form needs n_clades * n_topologies near 2^32 or PHYLO_TREE_WIDE_KEYS (force_wide):
its selection and its buffers are pinned here, for both (tests/test_gpu_tree_branches_wide.py runs it).  No GPU:
phylo_debug_tree_plan calls the functions the driver calls."""
import itertools
import json
import os

import pytest

from phylo_amd import _ffi

EINVAL, ESTATE = -1, -6
TEMP_S, TEMP_B = 4097, 777            # rocPRIM's temporary storage is a fact passed in: odd sizes show in the rounding
NS = (3, 4, 12, 64, 65, 70, 128, 129, 130, 512)
KS = (1, 2, 16, 64, 4096, 40960)
GS = (1, 2, 20, 64)
WORLDS = (1, 2, 3)
SHAPES = [(N, K, G, world) for N, K, G, world in itertools.product(NS, KS, GS, WORLDS) if K % G == 0]


def bit_length(v):
    return max(1, int(v).bit_length())


def carve(takes):
    """the take() lambda: a buffer starts where the slab ends, the slab grows by its bytes rounded up to 256"""
    off, offsets, sizes = 0, {}, {}
    for name, elem, n in takes:
        offsets[name], sizes[name] = off, n * elem
        off += (n * elem + 255) // 256 * 256
    return {"offsets": offsets, "sizes": sizes, "total": off}


def summary_rules(N, K, G, world, temp):
    R, Kg, W, L = N - 1, K // G, (N + 63) // 64, N - 2
    E = L * K
    Emax = E if E > K else K
    Ks, Es, Em = K, E, Emax
    takes = [("u", 8, Ks), ("U", 8, G), ("bits", 8, (R - 1) * W * Ks)]
    takes += [("kA", 8, Em), ("kB", 8, Em), ("val", 8, Em), ("scan", 8, Em), ("weight", 8, Em), ("srt", 8, Es), ("hp", 8, Ks)]
    takes += [("o_cbits", 8, Es * W), ("o_cw", 8, Es), ("o_tw", 8, Ks)]
    takes += [("child", 4, R * Ks * 2 if world > 1 else 0), ("slot", 4, R * Ks)]
    takes += [("o_cg", 4, Es), ("o_tn", 4, Ks), ("o_trep", 4, Ks), ("o_tg", 4, Ks), ("o_ptopo", 4, Ks)]
    takes += [("vA", 4, Em), ("vB", 4, Em), ("flag", 4, Em), ("sid", 4, Em), ("cid", 4, Es), ("seg_start", 4, Em)]
    takes += [("count", 4, Em), ("group", 4, Em), ("first", 4, Em), ("tid", 4, Ks), ("pos", 4, Ks), ("err", 4, 4)]
    takes += [("vC", 4, Em), ("vD", 4, Em)]
    takes += [("temp", 1, temp)]
    bits, launches = [], 2                                 # pt_weights, pt_walk
    for w in range(W):                                     # clades: keys + sort per bitset word, then the group
        bits.append(min(64, N - 64 * w))
        launches += 2
    if G > 1:
        bits.append(bit_length(G - 1))
        launches += 2
    launches += 5                                          # heads, scan, scan, seg_ids, seg_sums
    bits.append(64)                                        # clade order
    launches += 2
    if G > 1:
        bits.append(bit_length(G))
        launches += 2
    launches += 1                                          # pt_clade_out
    bits.append(32 + bit_length(K - 1))                    # pt_topo_pairs + the in-particle sort
    launches += 2
    bits.append(64)                                        # pt_topo_hash + sort
    launches += 2
    if G > 1:
        bits.append(bit_length(G - 1))
        launches += 2
    launches += 5
    bits.append(bit_length(K))                             # topology order: representative, weight, group
    bits.append(64)
    launches += 4
    if G > 1:
        bits.append(bit_length(G))
        launches += 2
    launches += 3                                          # pt_topo_out, pt_invert, pt_particle_topo
    return {"R": R, "L": L, "W": W, "E": E, "Emax": Emax, "Kg": Kg, "summary_slab": carve(takes), "sort_bits": bits,
            "summary_launches": launches}


def branches_rules(N, K, G, world, nc, nt, kept_whole, temp, force_wide=False):
    R, L = N - 1, N - 2
    E, nb = L * K, 2 * N - 2
    cbits, tbits = max(1, bit_length(nc - 1)), max(1, bit_length(nt - 1))
    wide = force_wide or cbits + tbits > 32
    gather = world > 1 and not kept_whole
    Ks, Es = K, E
    takes = [("ebr", 8, (R - 1) * Ks), ("lbr", 8, N * Ks)]
    takes += [("gbl", 8, R * Ks if gather else 0), ("gbr", 8, R * Ks if gather else 0)]
    takes += [("o_cs", 8, nc * 4), ("o_ls", 8, G * N * 4), ("o_ts", 8, nt * nb * 4)]
    takes += [("wA", 8, Es if wide else 0), ("wB", 8, Es if wide else 0)]
    takes += [("cpos", 4, Es), ("kA", 4, Es), ("kB", 4, Es), ("vA", 4, Es), ("vB", 4, Es)]
    takes += [("cstart", 4, nc + 1), ("toff", 4, nt), ("o_tc", 4, nt * L)]
    takes += [("temp", 1, temp)]
    # pb_walk; pt_invert, keys, sort, pb_clade_starts, sums; leaf sums; scan, keys, sort, sums (either key width)
    return {"cbits": cbits, "tbits": tbits, "wide": wide, "gather": gather, "branches_slab": carve(takes), "branches_launches": 1 + 5 + 1 + 4}


def check_slab(slab, names):
    assert tuple(slab["offsets"]) == names
    spans = sorted((slab["offsets"][n], slab["sizes"][n]) for n in names if slab["sizes"][n])
    assert all(o % 256 == 0 for o in slab["offsets"].values())
    assert all(o + s <= o2 for (o, s), (o2, _) in zip(spans, spans[1:]))
    assert spans[-1][0] + spans[-1][1] <= slab["total"]


def row_counts(N, K):
    """(n_clades, n_topologies) of the branch plan: 1; the maxima E and K; with nt = K the largest n_clades whose keys still fit
    32 bits and the smallest whose keys do not (more clades than entries: refused)"""
    E = (N - 2) * K
    cb = 32 - bit_length(K - 1)
    return [(1, 1), (E, K), (1 << cb, K), ((1 << cb) + 1, K)]


@pytest.mark.parametrize("N", NS)
def test_plan_equals_the_rules(N):
    wide_seen = narrow32_seen = 0
    for _, K, G, world in (s for s in SHAPES if s[0] == N):
        want = summary_rules(N, K, G, world, TEMP_S)
        E = want["E"]
        for (nc, nt), kept_whole in itertools.product(row_counts(N, K), (False, True)):
            args = dict(G=G, world=world, n_clades=nc, n_topologies=nt, kept_whole=kept_whole, summary_temp=TEMP_S, branches_temp=TEMP_B)
            if nc > E:
                with pytest.raises(_ffi.PhyloError, match="phylo_tree_branches: the summary holds no rows") as e:
                    _ffi.debug_tree_plan(N, K, **args)
                assert e.value.code == ESTATE
                continue
            got = _ffi.debug_tree_plan(N, K, **args)
            want.update(branches_rules(N, K, G, world, nc, nt, kept_whole, TEMP_B))
            assert got == want, (N, K, G, world, nc, nt, kept_whole)
            check_slab(got["summary_slab"], _ffi.TREE_SUMMARY_BUFS)
            check_slab(got["branches_slab"], _ffi.TREE_BRANCHES_BUFS)
            assert got["summary_launches"] == 26 + 2 * got["W"] + (8 if G > 1 else 0) and got["branches_launches"] == 11
            assert got["gather"] == (world > 1 and not kept_whole)
            wide_seen += got["wide"]
            narrow32_seen += got["cbits"] + got["tbits"] == 32
            forced = _ffi.debug_tree_plan(N, K, force_wide=True, **args)
            want.update(branches_rules(N, K, G, world, nc, nt, kept_whole, TEMP_B, force_wide=True))
            assert forced == want and forced["wide"], (N, K, G, world, nc, nt, kept_whole)
            check_slab(forced["branches_slab"], _ffi.TREE_BRANCHES_BUFS)
    if N == 512:                                           # (the grid does reach both sides of the threshold)
        assert wide_seen and narrow32_seen


def test_wide_keys_start_at_33_bits():
    N, K = 512, 40960                                      # tbits = 16 at nt = K
    narrow = _ffi.debug_tree_plan(N, K, n_clades=1 << 16, n_topologies=K)
    wide = _ffi.debug_tree_plan(N, K, n_clades=(1 << 16) + 1, n_topologies=K)
    assert (narrow["cbits"], narrow["tbits"], narrow["wide"]) == (16, 16, False)
    assert (wide["cbits"], wide["tbits"], wide["wide"]) == (17, 16, True)
    E = (N - 2) * K
    assert narrow["branches_slab"]["sizes"]["wA"] == narrow["branches_slab"]["sizes"]["wB"] == 0
    assert wide["branches_slab"]["sizes"]["wA"] == wide["branches_slab"]["sizes"]["wB"] == 8 * E
    assert wide["branches_slab"]["total"] - narrow["branches_slab"]["total"] == 2 * 8 * E + 256   # (and one more block of o_cs)


def test_forced_wide_changes_the_two_key_buffers_and_nothing_else():
    """PHYLO_TREE_WIDE_KEYS as a fact: wide is set, wA / wB get E elements of 8 bytes each, the temporary storage counts the 64-bit
    sort (the caller's fact: a larger branches_temp lands in the slab), and every other word of the plan is the narrow plan's"""
    for N, K, G, world, nc, nt, kept in ((9, 16, 1, 1, 20, 3, False), (9, 100, 1, 1, 61, 7, False), (3, 96, 1, 1, 1, 1, False),
                                         (12, 256, 4, 1, 300, 40, False), (70, 64, 1, 1, 900, 64, False), (9, 64, 1, 2, 30, 5, False),
                                         (9, 64, 1, 2, 30, 5, True)):
        args = dict(G=G, world=world, n_clades=nc, n_topologies=nt, kept_whole=kept, summary_temp=TEMP_S)
        narrow = _ffi.debug_tree_plan(N, K, branches_temp=TEMP_B, **args)
        forced = _ffi.debug_tree_plan(N, K, branches_temp=TEMP_B + 5000, force_wide=True, **args)   # (the 64-bit sort asks for more)
        E = (N - 2) * K
        assert not narrow["wide"] and forced["wide"] and narrow["cbits"] + narrow["tbits"] <= 32
        ns, fs = narrow["branches_slab"], forced["branches_slab"]
        assert ns["sizes"]["wA"] == ns["sizes"]["wB"] == 0 and fs["sizes"]["wA"] == fs["sizes"]["wB"] == 8 * E
        assert ns["sizes"]["temp"] == TEMP_B and fs["sizes"]["temp"] == TEMP_B + 5000
        for name in _ffi.TREE_BRANCHES_BUFS:
            if name not in ("wA", "wB", "temp"):
                assert fs["sizes"][name] == ns["sizes"][name], name
        one = (8 * E + 255) // 256 * 256
        shift = 2 * one
        for i, name in enumerate(_ffi.TREE_BRANCHES_BUFS):  # wB moves by wA's bytes, the buffers behind it by those of both
            moved = min(2, max(0, i - _ffi.TREE_BRANCHES_BUFS.index("wA"))) * one
            assert fs["offsets"][name] - ns["offsets"][name] == moved, name
        assert fs["total"] - ns["total"] == shift + ((TEMP_B + 5000 + 255) // 256 - (TEMP_B + 255) // 256) * 256
        for key in narrow:                                  # key layout, radix bits, launch counts, the summary: untouched
            if key not in ("wide", "branches_slab"):
                assert forced[key] == narrow[key], key
    # a plan that is wide by size is the same plan with and without the fact
    args = dict(n_clades=(1 << 16) + 1, n_topologies=40960, branches_temp=TEMP_B)
    assert _ffi.debug_tree_plan(512, 40960, force_wide=True, **args) == _ffi.debug_tree_plan(512, 40960, **args)


def test_refusals():
    for N, K, code, msg in ((2, 64, EINVAL, "phylo_tree_summary needs N >= 3 taxa (got 2)"),
                            (512, 8421505, EINVAL, "phylo_tree_summary: (N - 2) K = 4294967550 clade entries exceed 2^32 - 1")):
        with pytest.raises(_ffi.PhyloError) as e:
            _ffi.debug_tree_plan(N, K)
        assert e.value.code == code and str(e.value).endswith(msg)
    assert _ffi.debug_tree_plan(512, 8421504)["E"] == 4294967040   # the last K below the bound
    for nc, nt in ((0, 1), (1, 0), (7 * 64 + 1, 1), (1, 65)):
        with pytest.raises(_ffi.PhyloError, match="phylo_tree_branches: the summary holds no rows") as e:
            _ffi.debug_tree_plan(9, 64, n_clades=nc, n_topologies=nt)
        assert e.value.code == ESTATE


def test_recorded_launch_counts():
    """the shapes of profiles/tree_branches_probe.jsonl: 28 for one sweep of <= 64 taxa, 36 for a batch, 11 for the branch pass"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "tree_branches_probe.jsonl")
    rows = [json.loads(line) for line in open(path) if line.strip()]
    assert [(r["N"], r["K"], r["groups"], r["launches"], r["branches_launches"]) for r in rows] == [
        (12, 2048, 1, 28, 11), (27, 4096, 1, 28, 11), (12, 40960, 20, 36, 11)]
    for r in rows:
        p = _ffi.debug_tree_plan(r["N"], r["K"], G=r["groups"], n_clades=r["clades"], n_topologies=r["topologies"])
        assert (p["summary_launches"], p["branches_launches"]) == (r["launches"], r["branches_launches"])
