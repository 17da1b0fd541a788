"""ctypes binding of libphylo_hip.so (include/phylo_hip.h).  No PyTorch, no CPU fallback.

The shared object is built in-tree by phylo_amd/csrc/build.sh (hipcc --offload-arch=gfx950).  Loading
fails loudly if it is missing; every compute call fails loudly (PhyloError) if no HIP device is usable.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libphylo_hip.so")

PHYLO_OK = 0
QUIRK_Q1_RAW_Q = 1 << 0
TWISTING = 1 << 1
TIME_KERNELS = 1 << 2
EAGER_NODES = 1 << 3
KEEP_GRAPH = 1 << 4
ONE_LAUNCH = 1 << 5
FLAGS_DEFAULT = QUIRK_Q1_RAW_Q
COMM_ID_BYTES = 128
ANC_NOSTATE = 255                                          # PHYLO_ANC_NOSTATE: a site of trees_ancestral without a most probable state

EXPORTS = [
    "phylo_version", "phylo_last_error", "phylo_device_count", "phylo_create", "phylo_destroy",
    "phylo_set_leaves", "phylo_set_model", "phylo_expm_batched", "phylo_cond_likelihood_K",
    "phylo_forest_loglik", "phylo_tree_loglik", "phylo_trees_loglik", "phylo_trees_loglik_rates", "phylo_trees_grad", "phylo_trees_grad_rates", "phylo_trees_grad_model", "phylo_trees_ancestral", "phylo_trees_ancestral_rates", "phylo_trees_nni", "phylo_trees_nni_rates", "phylo_rell", "phylo_debug_rell_host", "phylo_rell_multiscale", "phylo_debug_rell_multiscale_host", "phylo_debug_tree_schedule", "phylo_resample", "phylo_log_zsmc", "phylo_sweep",
    "phylo_sweep_async", "phylo_sweep_batch_async", "phylo_sweep_batch_begin", "phylo_sweep_fetch_logz", "phylo_sweep_begin", "phylo_sweep_step", "phylo_sweep_step_a", "phylo_sweep_step_group", "phylo_sweep_finish", "phylo_sweep_fetch",
    "phylo_synchronize", "phylo_sweep_node", "phylo_sweep_backward", "phylo_sweep_backward_batch",
    "phylo_tree_summary", "phylo_tree_summary_fetch", "phylo_tree_branches", "phylo_tree_branches_fetch",
    "phylo_math_probe", "phylo_debug_frechet", "phylo_debug_stamps", "phylo_debug_reverse_lists", "phylo_debug_lookahead_lists", "phylo_debug_reverse_plan", "phylo_debug_reverse_plan_batch", "phylo_debug_sweep_plan", "phylo_debug_sweep_chain", "phylo_debug_sweep_chain_of", "phylo_debug_launch_map", "phylo_debug_sweep_launch", "phylo_debug_sweep_launch_of", "phylo_debug_scan_ancestors", "phylo_debug_pack_leaf_codes", "phylo_debug_site_patterns", "phylo_debug_site_patterns_rule", "phylo_debug_site_patterns_of", "phylo_debug_clade_patterns_rule", "phylo_debug_clade_tables", "phylo_debug_clade_patterns_of", "phylo_debug_tree_plan", "phylo_debug_tree_branches_of", "phylo_debug_scan_form", "phylo_debug_persist_plan", "phylo_debug_persist_of", "phylo_debug_device_lists", "phylo_debug_device_lists_of", "phylo_debug_remote_cache", "phylo_debug_site_product",
    "phylo_vi_gradients", "phylo_vi_gradients_batch", "phylo_vi_apply",
    "phylo_site_tile", "phylo_set_site_tile", "phylo_get_site_tile",
    "phylo_comm_unique_id", "phylo_comm_init", "phylo_comm_share", "phylo_comm_allgather", "phylo_comm_max", "phylo_comm_barrier",
    "phylo_comm_exchange_kind",
]


class PhyloError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libphylo_hip error %d: %s" % (code, msg))
        self.code = code


class Stats(C.Structure):
    _fields_ = [("sweep_ms", C.c_double), ("merge_ms", C.c_double), ("merge_launches", C.c_int32),
                ("n_launches", C.c_int32), ("units", C.c_double), ("alg_bytes", C.c_double)]


_lib = None


def load():
    """Load the library once; raises OSError with a build hint if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError("%s not found: build it with phylo_amd/csrc/build.sh (needs hipcc); "
                          "there is no CPU fallback" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        lib.phylo_version.restype = C.c_char_p
        lib.phylo_last_error.restype = C.c_char_p
        lib.phylo_last_error.argtypes = [C.c_void_p]
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def debug_reverse_lists(N, K, ancestors, child, early_free=True, rows_form=True, lookahead_nodes=None):
    """The host side of the reverse pass's integer lists on given ancestors [N-2][K] and children [N-1][K][2] (no GPU needed).
    Returns a dict of the arrays the device reads plus the per-rank-event offsets."""
    lib = load()
    R = N - 1
    nn = R * K
    cap = 2 * nn // 4 + 1
    n_lists = R * (K + 1) + 9 * nn + 1 + 2 * cap
    lists = np.zeros(n_lists, dtype=np.int32)
    meta = np.zeros(6 + 3 * (R + 1), dtype=np.int32)
    anc = None if R < 2 else np.ascontiguousarray(ancestors, dtype=np.int64)
    ch = np.ascontiguousarray(child, dtype=np.int32)
    la = None if lookahead_nodes is None or len(lookahead_nodes) == 0 else np.ascontiguousarray(lookahead_nodes, dtype=np.int32)
    rc = lib.phylo_debug_reverse_lists(C.c_int(N), C.c_int(K), _ptr(anc), _ptr(ch), C.c_int(int(early_free)), C.c_int(int(rows_form)),
                                       _ptr(la), C.c_int(0 if la is None else la.size), _ptr(lists), C.c_int64(n_lists), _ptr(meta),
                                       C.c_int(meta.size))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return _lists_dict(lists, meta, R, K)


def debug_lookahead_lists(N, K, S, M, roots_ad, slow_flag=None):
    """The twisted proposal's look-ahead lists of the reverse pass on given adopted root tables [N-1][K][N] (no GPU needed).
    Returns the arrays the device reads, the per-rank-event offsets and slow_flag [(N-1) K] with bit 1 set for the touched nodes."""
    lib = load()
    R = N - 1
    rad = np.ascontiguousarray(roots_ad, dtype=np.int32)
    if rad.shape != (R, K, N):
        raise ValueError("roots_ad must be [N-1][K][N]")
    flag = np.zeros(R * K, dtype=np.int32) if slow_flag is None else np.array(slow_flag, dtype=np.int32).reshape(R * K)
    n_image = R * (8 * K * N + 8192) + 1                   # entries <= K N per rank event, chunks <= max(entries, 2048), nodes <= entries
    image = np.zeros(n_image, dtype=np.int32)
    meta = np.zeros(4 + 2 * (R + 1), dtype=np.int32)
    rc = lib.phylo_debug_lookahead_lists(C.c_int(N), C.c_int(K), C.c_int(S), C.c_int(M), _ptr(rad), _ptr(flag), _ptr(image),
                                         C.c_int64(n_image), _ptr(meta), C.c_int(meta.size))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    ne, nc, nx = int(meta[0]), int(meta[1]), int(meta[2])
    out = {"n_xent": ne, "n_xchunks": nc, "n_xnodes": nx, "tw_max_chunks": int(meta[3]), "slow_flag": flag,
           "ev_chunk0": meta[4:4 + R + 1].copy(), "ev_node0": meta[4 + R + 1:4 + 2 * (R + 1)].copy()}
    o = 0
    for name, n in (("xent", ne), ("xchunk_node", nc), ("xchunk_beg", nc), ("xchunk_cnt", nc), ("xchunk_part", nc), ("xnode_id", nx),
                    ("xnode_chunk0", nx), ("xnode_nchunks", nx)):
        out[name] = image[o:o + n].copy()
        o += n
    return out


PLAN_BITS = ("rows_form", "whole", "early_free", "dev_lists", "sort_early", "bg_free", "two", "parents_first", "rows_all", "rows_overlap",
             "chunks_first", "interleave", "coeff_all")
PLAN_SWITCHES = ("rev_host_lists", "one_stream", "two_streams", "rows_chain", "coeff_chain")


def debug_reverse_plan(N, K, S, K_local=None, world=1, twisted=False, marks=True, switches=(), n_slow=0, TS=None, coeff_wgs=0,
                       passes_in_flight=1):
    """The form phylo_sweep_backward takes for a shape, the last sweep's facts, the switches (names of PLAN_SWITCHES) and the lists'
    counts (no GPU needed): a dict of the booleans of PLAN_BITS plus 'mask'."""
    lib = load()
    sw = sum(1 << PLAN_SWITCHES.index(name) for name in switches)
    mask = C.c_uint32(0)
    rc = lib.phylo_debug_reverse_plan(C.c_int(N), C.c_int(K), C.c_int(K if K_local is None else K_local), C.c_int(S), C.c_int(world),
                                      C.c_int(int(twisted)), C.c_int(int(marks)), C.c_uint32(sw), C.c_int64(n_slow),
                                      C.c_int((S + 255) // 256 if TS is None else TS), C.c_int64(coeff_wgs), C.c_int(passes_in_flight),
                                      C.byref(mask))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    out = {name: bool(mask.value >> i & 1) for i, name in enumerate(PLAN_BITS)}
    out["mask"] = mask.value
    return out


SWEEP_PLAN_BITS = ("twist", "graph", "timek", "lazy", "shard_form", "replicated_book", "local_book", "book_mat", "mat_by_draws", "want_rdraw",
                   "use_rec", "sorted_prologue", "mat_grouped", "mat_draws_grouped", "step_a_work", "mat_after_book", "mat_barrier",
                   "fix_rootll", "fold_logz", "no_store_last", "final_missing", "last_graph_eager", "one_tile", "twist_ll", "twist_tables",
                   "tile_epilogue", "batched")
SWEEP_PLAN_SWITCHES = ("eager_nodes", "rehearse_sharded", "replicated_book", "jc", "coded_leaves", "device_exchange")


def debug_sweep_plan(N, K, S, K_local=None, G=1, M=1, world=1, transport=False, flags=0, switches=()):
    """The form the forward sweep's launch path takes for a shape, the flags of a sweep and the switches (names of
    SWEEP_PLAN_SWITCHES: three environment switches, then three facts of the context) -- no GPU needed: a dict of the booleans of
    SWEEP_PLAN_BITS, 'book_width' (lanes per particle of the bookkeeping: 8, 16, 32 or 64; 0 = no bookkeeping launch, the twisted
    proposal), 'mask' and 'launches' (what stats['n_launches'] counts: [0] the begin, [r + 1] rank event r, [N] the finish)."""
    lib = load()
    sw = sum(1 << SWEEP_PLAN_SWITCHES.index(name) for name in switches)
    mask = C.c_uint32(0)
    launches = (C.c_int32 * (max(N, 1) + 1))()
    rc = lib.phylo_debug_sweep_plan(C.c_int(N), C.c_int(K), C.c_int(K if K_local is None else K_local), C.c_int(S), C.c_int(G), C.c_int(M),
                                    C.c_int(world), C.c_int(int(transport)), C.c_uint32(flags), C.c_uint32(sw), C.byref(mask), launches)
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    out = {name: bool(mask.value >> i & 1) for i, name in enumerate(SWEEP_PLAN_BITS)}
    out["book_width"] = (mask.value >> 28) * 8
    out["mask"] = mask.value
    out["launches"] = list(launches)
    return out


def debug_sweep_chain(N, K, S, K_local=None, G=1, M=1, world=1, transport=False, flags=0, switches=(), multi_min=4096, scan_ancestors=1):
    """Whether the rank events of a sweep take the chain form (sweep_chain_form_of; no GPU needed): the arguments of debug_sweep_plan,
    then PHYLO_SCAN_MULTI_MIN and PHYLO_SCAN_ANCESTORS as a context reads them.  A dict: 'taken', 'item_waves' (per group) and
    'parts' (of a node's sites, one per item)."""
    lib = load()
    sw = sum(1 << SWEEP_PLAN_SWITCHES.index(name) for name in switches)
    out = (C.c_int32 * 3)()
    rc = lib.phylo_debug_sweep_chain(C.c_int(N), C.c_int(K), C.c_int(K if K_local is None else K_local), C.c_int(S), C.c_int(G), C.c_int(M),
                                     C.c_int(world), C.c_int(int(transport)), C.c_uint32(flags), C.c_uint32(sw), C.c_int(multi_min),
                                     C.c_int(scan_ancestors), out)
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return {"taken": bool(out[0]), "item_waves": out[1], "parts": out[2]}


def debug_launch_map(n, W, xcd):
    """Which wave takes which item in a launch of n items at W waves per workgroup (phylo_launch_map.h; no GPU needed): the grid and
    an int32 array [grid][W] of items; an entry >= n is a wave without work."""
    lib = load()
    grid = C.c_int32(0)
    rc = lib.phylo_debug_launch_map(C.c_int(n), C.c_int(W), C.c_int(int(xcd)), C.byref(grid), None, C.c_int64(0))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    items = np.zeros((grid.value, W), dtype=np.int32)
    rc = lib.phylo_debug_launch_map(C.c_int(n), C.c_int(W), C.c_int(int(xcd)), C.byref(grid), _ptr(items), C.c_int64(items.size))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return grid.value, items


def debug_sweep_launch(N, K, S, K_local=None, G=1, M=1, world=1, transport=False, flags=0, switches=(), launch_xcd=0):
    """How the plan launches the record-form merge and the chain bookkeeping (no GPU needed): the arguments of debug_sweep_plan
    (switches may also name 'clade_tables'), then PHYLO_LAUNCH_XCD as a context reads it (0 = unset, -1 = off, 1 = on, 2 = the
    merge alone, 3 = the bookkeeping alone).  A dict: 'launch_xcd', 'book_xcd'."""
    lib = load()
    names = SWEEP_PLAN_SWITCHES + ("clade_tables",)
    sw = sum(1 << names.index(name) for name in switches)
    out = (C.c_int32 * 2)()
    rc = lib.phylo_debug_sweep_launch(C.c_int(N), C.c_int(K), C.c_int(K if K_local is None else K_local), C.c_int(S), C.c_int(G),
                                      C.c_int(M), C.c_int(world), C.c_int(int(transport)), C.c_uint32(flags), C.c_uint32(sw),
                                      C.c_int(launch_xcd), out)
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return {"launch_xcd": bool(out[0]), "book_xcd": bool(out[1])}


def debug_pack_leaf_codes(codes):
    """The packed image phylo_set_leaves builds beside byte codes [N][S] (no GPU needed): a uint8 array [N][nC][64][16] with
    [leaf][Jc][c][j] = code of site 64 (16 Jc + j) + c, nC = ceil(ceil(S / 64) / 16), and the pad code 5 at sites >= S."""
    lib = load()
    cd = np.ascontiguousarray(codes, dtype=np.uint8)
    if cd.ndim != 2:
        raise ValueError("codes must be [N][S]")
    N, S = cd.shape
    need = C.c_int64(0)
    rc = lib.phylo_debug_pack_leaf_codes(_ptr(cd), C.c_int(N), C.c_int(S), None, C.c_int64(0), C.byref(need))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    out = np.full(need.value, 0xff, dtype=np.uint8)
    rc = lib.phylo_debug_pack_leaf_codes(_ptr(cd), C.c_int(N), C.c_int(S), _ptr(out), C.c_int64(out.size), C.byref(need))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return out.reshape(N, -1, 64, 16)


SITE_PATTERN_SWITCH = {"0": 0, None: 1, "force": 2}        # PHYLO_SITE_PATTERNS


def debug_site_patterns(codes):
    """The site-pattern tables phylo_set_leaves builds from byte codes [N][S] (phylo_site_patterns.h; no GPU needed): a dict with U,
    rep [U], image (uint16 [nC][2][64][8]: [Jc][h][c][j] = 8 * the column number of site 64 (16 Jc + 8 h + j) + c, 8 U at sites >= S;
    None when U > 8191), rep_off (uint32 [1024]) and rep_leaf (uint8 [N][1][64][16], the packed codes of the representative sites);
    the last two None when U > 512."""
    lib = load()
    cd = np.ascontiguousarray(codes, dtype=np.uint8)
    if cd.ndim != 2:
        raise ValueError("codes must be [N][S]")
    N, S = cd.shape
    nC = -(-(-(-S // 64)) // 16)
    U = C.c_int32(0)
    rep = np.full(S, -1, dtype=np.int32)
    image = np.full(nC * 1024, 0xffff, dtype=np.uint16)
    rep_off = np.full(1024, 0xffffffff, dtype=np.uint32)
    rep_leaf = np.full(N * 1024, 0xff, dtype=np.uint8)
    rc = lib.phylo_debug_site_patterns(_ptr(cd), C.c_int(N), C.c_int(S), C.byref(U), _ptr(rep), _ptr(image), _ptr(rep_off), _ptr(rep_leaf),
                                       C.c_int64(rep_leaf.size))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    u = U.value
    return {"U": u, "rep": rep[:u].copy(), "image": image.reshape(nC, 2, 64, 8) if u <= 8191 else None,
            "rep_off": rep_off if u <= 512 else None,
            "rep_leaf": rep_leaf[:N * 1024 * (-(-(-(-u // 64)) // 16))].reshape(N, -1, 64, 16) if u <= 512 else None}


def debug_site_patterns_rule(S, U, coded=True, ntiles=1, switch=None):
    """Does a context take the merge's site-pattern form (no GPU needed)?  switch: PHYLO_SITE_PATTERNS' value, "0", None or "force"."""
    lib = load()
    rc = lib.phylo_debug_site_patterns_rule(C.c_int(S), C.c_int(U), C.c_int(int(coded)), C.c_int(ntiles), C.c_int(SITE_PATTERN_SWITCH[switch]))
    if rc < 0:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return bool(rc)


CLADE_MAX_TAXA = 12                                        # PK_CLADE_MAX_N
CLADE_MAX_BYTES = 32 << 20                                 # PK_CLADE_MAX_BYTES


def debug_clade_patterns_rule(N, S, U, pat_taken=True, switch=None):
    """(taken, bytes): do leaves of N taxa, S sites and U distinct columns get the clade tables of the pattern form, and the
    tables' size (no GPU needed)?  switch: PHYLO_CLADE_PATTERNS' value, "0", None or "force"."""
    lib = load()
    nbytes = C.c_int64(0)
    rc = lib.phylo_debug_clade_patterns_rule(C.c_int(int(pat_taken)), C.c_int(N), C.c_int(S), C.c_int(U), C.c_int(SITE_PATTERN_SWITCH[switch]),
                                             C.byref(nbytes))
    if rc < 0:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return bool(rc), nbytes.value


def debug_clade_tables(codes):
    """The clade tables phylo_set_leaves builds from byte codes [N][S], N <= 12 (phylo_site_patterns.h; no GPU needed): a dict with U,
    'codes' (uint8 [N][leaf stride], the strided byte codes), 'cls' (uint16 [2^N][U], the class of every global pattern in every
    leaf bitset) and 'blocks': {Z: {'U': U_Z, 'rep_off': uint32 [64 (ceil(U / 64) + 2)], 'image': uint16 [nC][2][64][8]}} for
    every bitset Z of at least three leaves."""
    lib = load()
    cd = np.ascontiguousarray(codes, dtype=np.uint8)
    if cd.ndim != 2:
        raise ValueError("codes must be [N][S]")
    N, S = cd.shape
    U = C.c_int32(0)
    lay = (C.c_int64 * 5)()
    rc = lib.phylo_debug_clade_tables(_ptr(cd), C.c_int(N), C.c_int(S), C.byref(U), lay, None, C.c_int64(0), None)
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    codes_bytes, rep_bytes, image_bytes, stride, total = (int(x) for x in lay)
    buf = np.full(total, 0xff, dtype=np.uint8)
    cls = np.full((1 << N) * U.value, 0xffff, dtype=np.uint16)
    rc = lib.phylo_debug_clade_tables(_ptr(cd), C.c_int(N), C.c_int(S), C.byref(U), lay, _ptr(buf), C.c_int64(total), _ptr(cls))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    blocks = {}
    for Z in range(1 << N):
        if bin(Z).count("1") < 3:
            continue
        b = buf[codes_bytes + Z * stride: codes_bytes + (Z + 1) * stride]
        blocks[Z] = {"U": int(b[:4].view(np.uint32)[0]), "rep_off": b[256:256 + rep_bytes].view(np.uint32).copy(),
                     "image": b[256 + rep_bytes:].view(np.uint16).reshape(-1, 2, 64, 8).copy()}
    return {"U": U.value, "codes": buf[:codes_bytes].reshape(N, -1).copy(), "cls": cls.reshape(1 << N, U.value), "blocks": blocks,
            "layout": {"codes_bytes": codes_bytes, "rep_bytes": rep_bytes, "image_bytes": image_bytes, "stride": stride, "total": total}}


def debug_sweep_plan_clade(N, K, S, clade_tables=True, **kw):
    """The plan's clade_pat (bit 27 of the mask) for debug_sweep_plan's arguments, with the clade tables of the leaves there or not."""
    lib = load()
    sw = sum(1 << SWEEP_PLAN_SWITCHES.index(name) for name in kw.get("switches", ())) | (64 if clade_tables else 0)
    mask = C.c_uint32(0)
    launches = (C.c_int32 * (max(N, 1) + 1))()
    K_local = kw.get("K_local")
    rc = lib.phylo_debug_sweep_plan(C.c_int(N), C.c_int(K), C.c_int(K if K_local is None else K_local), C.c_int(S), C.c_int(kw.get("G", 1)),
                                    C.c_int(kw.get("M", 1)), C.c_int(kw.get("world", 1)), C.c_int(int(kw.get("transport", False))),
                                    C.c_uint32(kw.get("flags", 0)), C.c_uint32(sw), C.byref(mask), launches)
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return bool(mask.value >> 27 & 1)


TREE_SUMMARY_BUFS = ("u", "U", "bits", "kA", "kB", "val", "scan", "weight", "srt", "hp", "o_cbits", "o_cw", "o_tw", "child", "slot", "o_cg",
                     "o_tn", "o_trep", "o_tg", "o_ptopo", "vA", "vB", "flag", "sid", "cid", "seg_start", "count", "group", "first", "tid", "pos",
                     "err", "vC", "vD", "temp")
TREE_BRANCHES_BUFS = ("ebr", "lbr", "gbl", "gbr", "o_cs", "o_ls", "o_ts", "wA", "wB", "cpos", "kA", "kB", "vA", "vB", "cstart", "toff", "o_tc",
                      "temp")


def debug_tree_plan(N, K, G=1, world=1, n_clades=1, n_topologies=1, kept_whole=False, summary_temp=0, branches_temp=0, force_wide=False):
    """The form phylo_tree_summary and phylo_tree_branches take for a sweep of G groups on `world` ranks, a summary of n_clades and
    n_topologies rows, whether the sweep kept whole-K branch lengths, rocPRIM's temporary-storage bytes of either pass and whether
    PHYLO_TREE_WIDE_KEYS is set (force_wide) -- no GPU needed.  A dict: the scalars R, L, W, E, Emax, Kg, cbits, tbits, wide, gather; 'summary_slab' / 'branches_slab' =
    {'offsets': {name: bytes}, 'sizes': {name: bytes}, 'total'} over TREE_SUMMARY_BUFS / TREE_BRANCHES_BUFS (scratch slots 12 and
    13); 'sort_bits', the radix bits of the summary's sort passes in issue order; 'summary_launches', 'branches_launches'."""
    lib = load()
    ns, nb = len(TREE_SUMMARY_BUFS), len(TREE_BRANCHES_BUFS)
    sc = (C.c_int64 * 13)()
    ss, bs = (C.c_int64 * (2 * ns + 1))(), (C.c_int64 * (2 * nb + 1))()
    bits, launches = (C.c_int32 * 17)(), (C.c_int32 * 2)()
    rc = lib.phylo_debug_tree_plan(C.c_int(N), C.c_int(K), C.c_int(G), C.c_int(world), C.c_int64(n_clades), C.c_int64(n_topologies),
                                   C.c_int(int(kept_whole)), C.c_int(int(force_wide)), C.c_int64(summary_temp), C.c_int64(branches_temp),
                                   sc, ss, bs, bits, launches)
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    out = dict(zip(("R", "L", "W", "E", "Emax", "Kg", "cbits", "tbits"), sc[:8]))
    out["wide"], out["gather"] = bool(sc[8]), bool(sc[9])
    if (sc[11], sc[12]) != (ns, nb):
        raise RuntimeError("TREE_SUMMARY_BUFS / TREE_BRANCHES_BUFS do not name the library's buffers")
    for key, names, a in (("summary_slab", TREE_SUMMARY_BUFS, ss), ("branches_slab", TREE_BRANCHES_BUFS, bs)):
        n = len(names)
        out[key] = {"offsets": dict(zip(names, a[:n])), "sizes": dict(zip(names, a[n:2 * n])), "total": a[2 * n]}
    out["sort_bits"] = list(bits[:sc[10]])
    out["summary_launches"], out["branches_launches"] = launches[0], launches[1]
    return out


SCAN_FORMS = ("multi", "lds512", "lds1024", "in_place")   # pp_scan_multi_*, pp_resample_scan<512>, <1024>, pk_resample_scan(_groups)


def debug_scan_form(Kg, multi_min=4096, wanted=True):
    """The form launch_scan takes for groups of Kg log-weights under PHYLO_SCAN_MULTI_MIN = multi_min (sweep_scan_form_of; no GPU
    and no context needed): a name of SCAN_FORMS.  wanted: the caller asks for a cdf or a log-normaliser."""
    lib = load()
    rc = lib.phylo_debug_scan_form(None, C.c_int(Kg), C.c_int(multi_min), C.c_int(int(wanted)))
    if rc < 0:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return SCAN_FORMS[rc]


PERSIST_PLAN_SWITCHES = ("eager_nodes", "one_launch")      # PHYLO_EAGER_NODES, PHYLO_ONE_LAUNCH in the environment


def debug_persist_plan(N, K, S, G=1, flags=FLAGS_DEFAULT | ONE_LAUNCH, switches=(), world=1, transport=False, n_cus=256, blocks_per_cu=1,
                       persist_wgs=0, persist_nt=256):
    """The grid the one-launch sweep takes (persist_plan_of; no GPU and no context needed) for a shape (K: all G groups' particles),
    the flags of a sweep, the switches (names of PERSIST_PLAN_SWITCHES) and the facts of a device and a context: its compute units,
    the workgroups the planner may place on one (0, 1 or 2), PHYLO_PERSIST_WGS (0: unset) and PHYLO_PERSIST_NT.  None when the
    launch path runs instead, else {'nt', 'Wg', 'm', 'lds'}."""
    lib = load()
    sw = sum(1 << PERSIST_PLAN_SWITCHES.index(name) for name in switches)
    out = (C.c_int64 * 5)()
    rc = lib.phylo_debug_persist_plan(C.c_int(N), C.c_int(K), C.c_int(S), C.c_int(G), C.c_uint32(flags), C.c_uint32(sw), C.c_int(world),
                                      C.c_int(int(transport)), C.c_int(n_cus), C.c_int(blocks_per_cu), C.c_int(persist_wgs),
                                      C.c_int(persist_nt), out)
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return {'nt': out[3], 'Wg': out[1], 'm': out[2], 'lds': out[4]} if out[0] else None


def debug_reverse_plan_batch(N, K, G, S, switches=(), n_slow=0, TS=None, coeff_wgs=0, passes_in_flight=1):
    """debug_reverse_plan for the reverse pass of a batched sweep of G groups (K: the total; plain proposal, marks, one GPU)."""
    lib = load()
    sw = sum(1 << PLAN_SWITCHES.index(name) for name in switches)
    mask = C.c_uint32(0)
    rc = lib.phylo_debug_reverse_plan_batch(C.c_int(N), C.c_int(K), C.c_int(G), C.c_int(S), C.c_uint32(sw), C.c_int64(n_slow),
                                            C.c_int((S + 255) // 256 if TS is None else TS), C.c_int64(coeff_wgs),
                                            C.c_int(passes_in_flight), C.byref(mask))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    out = {name: bool(mask.value >> i & 1) for i, name in enumerate(PLAN_BITS)}
    out["mask"] = mask.value
    return out


def _lists_dict(lists, meta, R, K):
    nn = R * K
    cap = 2 * nn // 4 + 1
    out = {}
    o = 0
    for name, n in (("ad_off", R * (K + 1)), ("ad_idx", nn), ("par_off", nn + 1), ("par_idx", 2 * nn), ("heavy", nn), ("chunk_beg", cap),
                    ("chunk_cnt", cap), ("slow_flag", nn), ("slow_idx", nn), ("adp", nn)):
        out[name] = lists[o:o + n]
        o += n
    out["ad_off"] = out["ad_off"].reshape(R, K + 1)
    out["ad_idx"] = out["ad_idx"].reshape(R, K)
    for i, name in enumerate(("n_adp", "n_chunks", "max_chunks", "n_slow", "n_par", "cap")):
        out[name] = int(meta[i])
    out["ev_adp0"] = meta[6:6 + R + 1].copy()
    out["rank_chunk0"] = meta[6 + (R + 1):6 + 2 * (R + 1)].copy()
    out["ev_slow0"] = meta[6 + 2 * (R + 1):6 + 3 * (R + 1)].copy()
    return out


def _site_product(handle, p, x1, x2):
    lib = load()
    p, x1, x2 = _f64(p).reshape(-1), _f64(x1).reshape(-1), _f64(x2).reshape(-1)
    if not (p.size == x1.size == x2.size):
        raise ValueError("p, x1 and x2 must hold the same number of values")
    n = p.size
    op, oE, ox = np.empty((2, n)), np.empty((2, n), dtype=np.int32), np.empty((2, n))
    rc = lib.phylo_debug_site_product(handle, _ptr(p), _ptr(x1), _ptr(x2), C.c_int(n), _ptr(op), _ptr(oE), _ptr(ox))
    if rc:
        raise PhyloError(rc, (lib.phylo_last_error(handle) or b"").decode())
    return {'pair': (op[0], oE[0], ox[0]), 'each': (op[1], oE[1], ox[1])}


def debug_site_product(p, x1, x2):
    """The site-product update on triples (p in [1,2), x1, x2) from a fresh {p, 0, 0.0}, ON THE HOST (no GPU needed): 'pair' =
    (p', E', extra') after pm_lp_mul2(x1, x2), 'each' = the same after pm_lp_mul(x1); pm_lp_mul(x2)."""
    return _site_product(None, p, x1, x2)


def _tree_rows(child, blen, N):
    child = np.ascontiguousarray(child, dtype=np.int32)
    blen = _f64(blen)
    if child.ndim == 2:
        child, blen = child[None], blen[None]
    if child.ndim != 3 or child.shape[1:] != (N - 1, 2) or blen.shape != child.shape:
        raise ValueError("child and blen must be [T][N-1][2] (or [N-1][2]) for N = %d, got %r and %r" % (N, child.shape, blen.shape))
    return child, blen


def debug_tree_schedule(child, blen):
    """The host half of phylo_trees_loglik on one tree (no GPU needed): the checks (PhyloError -1 naming the row) and the slot
    schedule ops [N-1][4] = (destination slot, left source, right source, row), a source >= 0 a leaf, < 0 the slot ~source.
    Returns (ops, depth)."""
    lib = load()
    N = np.asarray(child).shape[-2] + 1
    child, blen = _tree_rows(child, blen, N)
    if child.shape[0] != 1:
        raise ValueError("one tree at a time")
    ops = np.zeros((N - 1, 4), dtype=np.int32)
    depth = C.c_int32(0)
    rc = lib.phylo_debug_tree_schedule(C.c_int(N), _ptr(child), _ptr(blen), _ptr(ops), C.byref(depth))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return ops, depth.value


def debug_rell_host(site_lik, b0, nB, seed, S=None, want_counts=True, want_logs=True, want_reps=True):
    """phylo_rell's contract as a host loop (no GPU needed) for replicates b0 .. b0 + nB - 1 of site_lik [T][S]: a dict with
    'counts' [nB][S] int32, 'site_loglik' [T][S] and 'rep_loglik' [T][nB].  site_lik None (then give S): the counts alone."""
    lib = load()
    if site_lik is None:
        T, S = 1, int(S)
        sl, want_logs, want_reps = None, False, False
    else:
        sl = _f64(site_lik)
        if sl.ndim != 2:
            raise ValueError("site_lik must be [T][S], got %r" % (sl.shape,))
        T, S = sl.shape
    nB = int(nB)
    cnt = np.zeros((nB, S), dtype=np.int32) if want_counts else None
    x = np.empty((T, S)) if want_logs else None
    rl = np.empty((T, nB)) if want_reps else None
    rc = lib.phylo_debug_rell_host(C.c_int(T), C.c_int(S), _ptr(sl), C.c_int(int(b0)), C.c_int(nB), C.c_uint64(int(seed)), _ptr(cnt),
                                   _ptr(x), _ptr(rl))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return {'counts': cnt, 'site_loglik': x, 'rep_loglik': rl}


def debug_rell_multiscale_host(site_lik, draws, k0, b0, nB, seed, S=None, want_counts=True, want_reps=True, want_best=True):
    """phylo_rell_multiscale's contract as a host loop (no GPU needed) for scale k0 of `draws` and its replicates b0 .. b0 + nB - 1:
    a dict with 'counts' [nB][S] int32, 'rep_loglik' [T][nB] and 'best' [nB].  site_lik None (then give S): the counts alone."""
    lib = load()
    if site_lik is None:
        T, S = 1, int(S)
        sl, want_reps, want_best = None, False, False
    else:
        sl = _f64(site_lik)
        if sl.ndim != 2:
            raise ValueError("site_lik must be [T][S], got %r" % (sl.shape,))
        T, S = sl.shape
    dr = np.ascontiguousarray(draws, dtype=np.int32).reshape(-1)
    nB = int(nB)
    cnt = np.zeros((nB, S), dtype=np.int32) if want_counts else None
    rl = np.empty((T, nB)) if want_reps else None
    best = np.empty(nB, dtype=np.int32) if want_best else None
    rc = lib.phylo_debug_rell_multiscale_host(C.c_int(T), C.c_int(S), _ptr(sl), C.c_int(dr.size), _ptr(dr), C.c_int(int(k0)), C.c_int(int(b0)),
                                              C.c_int(nB), C.c_uint64(int(seed)), _ptr(cnt), _ptr(rl), _ptr(best))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    return {'counts': cnt, 'rep_loglik': rl, 'best': best}


def vi_apply(N, jc, packed_vars, packed_grads, kind, lr, beta1=0.9, beta2=0.999, eps=1e-8, state=None):
    """phylo_vi_apply: the optimiser update on the packed variables IN PLACE (kind 0 gradient descent, 1 Adam with state =
    {'t': int, 'm': array, 'v': array}, updated in place too)."""
    lib = load()
    t = C.c_int64(0 if state is None else int(state['t']))
    m = None if state is None else state['m']
    v = None if state is None else state['v']
    rc = lib.phylo_vi_apply(C.c_int(N), C.c_int(int(jc)), _ptr(packed_vars), _ptr(packed_grads), C.c_int(kind), C.c_double(lr),
                            C.c_double(beta1), C.c_double(beta2), C.c_double(eps), C.byref(t), _ptr(m), _ptr(v))
    if rc:
        raise PhyloError(rc, lib.phylo_last_error(None).decode())
    if state is not None:
        state['t'] = t.value


def device_count():
    return int(load().phylo_device_count())


class Context:
    """Owns one phylo_ctx (one GPU).  Mirrors the C ABI one to one; numpy arrays in, numpy arrays out."""

    def __init__(self, K, N, S, A=4, device=0, flags=FLAGS_DEFAULT):
        self._lib = load()
        self._h = C.c_void_p()
        self.K, self.N, self.S, self.A = int(K), int(N), int(S), int(A)
        self.K_local, self.k0 = self.K, 0
        dev = (C.c_int * 1)(int(device))
        rc = self._lib.phylo_create(dev, C.c_int(1), C.c_int(self.K), C.c_int(self.N), C.c_int(self.S), C.c_int(self.A),
                                    C.c_uint32(flags), C.byref(self._h))
        if rc != PHYLO_OK:
            raise PhyloError(rc, (self._lib.phylo_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc != PHYLO_OK:
            raise PhyloError(rc, (self._lib.phylo_last_error(self._h) or b"").decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.phylo_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- state
    def set_site_tile(self, T):
        """contract v5: sites per tile of the canonical sum over sites (0 = the default phylo_site_tile(S))"""
        self._check(self._lib.phylo_set_site_tile(self._h, C.c_int(int(T))))

    def site_tile(self):
        return int(self._lib.phylo_get_site_tile(self._h))

    def set_leaves(self, genome_NxSxA):
        g = _f64(genome_NxSxA)
        if g.shape != (self.N, self.S, self.A):
            raise ValueError("genome shape %r != (%d, %d, %d)" % (g.shape, self.N, self.S, self.A))
        self._check(self._lib.phylo_set_leaves(self._h, _ptr(g)))

    def set_model(self, Q, pi, lam_l, lam_r, jc69_closed_form=False):
        Q, pi, ll, lr = _f64(Q), _f64(pi).reshape(-1), _f64(lam_l), _f64(lam_r)
        if Q.shape != (4, 4) or pi.shape != (4,) or ll.shape != (self.N - 1,) or lr.shape != (self.N - 1,):
            raise ValueError("bad model shapes")
        self._check(self._lib.phylo_set_model(self._h, _ptr(Q), _ptr(pi), _ptr(ll), _ptr(lr), C.c_int(int(jc69_closed_form))))

    # ---- ops
    def expm_batched(self, t):
        """P[i] = expm(Q t[i]) of the model in force, [n][4][4] (phylo_expm_batched; DESIGN.md section 16 is its contract).  A
        length with ||Q||_1 |t| above theta_13 2^23 = 4.50629e7 -- where the squarings have lost the matrix's digits; NaN and inf
        included -- raises PhyloError (PHYLO_EINVAL) naming t[i]; so does every such length, or rate * length, of tree_loglik and
        of all trees_* calls, naming tree and row.  Under jc69_closed_form there is no limit (1/4 everywhere at 1e100); the closed
        form is exact in absolute terms only: its off-diagonal entry is exactly 0 below t = 2^-54."""
        t = _f64(np.atleast_1d(t))
        P = np.empty((t.size, 4, 4))
        self._check(self._lib.phylo_expm_batched(self._h, _ptr(t), C.c_int(t.size), _ptr(P)))
        return P

    def cond_likelihood_K(self, l, r, tl, tr):
        l, r, tl, tr = _f64(l), _f64(r), _f64(tl), _f64(tr)
        if l.ndim != 3 or l.shape != r.shape or l.shape[2] != 4 or tl.shape != (l.shape[0],) or tr.shape != tl.shape:
            raise ValueError("bad shapes for cond_likelihood_K")
        out = np.empty_like(l)
        self._check(self._lib.phylo_cond_likelihood_K(self._h, _ptr(l), _ptr(r), _ptr(tl), _ptr(tr), C.c_int(l.shape[0]),
                                                      C.c_int(l.shape[1]), _ptr(out)))
        return out

    def forest_loglik(self, core_KxXxSx4, record_KxX):
        core = _f64(core_KxXxSx4)
        rec = np.ascontiguousarray(record_KxX, dtype=np.int32)
        if core.ndim != 4 or core.shape[3] != 4 or rec.shape != core.shape[:2]:
            raise ValueError("bad shapes for forest_loglik")
        K, X, S = core.shape[:3]
        out = np.empty(K)
        self._check(self._lib.phylo_forest_loglik(self._h, _ptr(core), _ptr(rec), C.c_int(K), C.c_int(X), C.c_int(S), _ptr(out)))
        return out

    def tree_loglik(self, left, right, bl, br, root, leaves, prior, want_root=True):
        leaves, prior = _f64(leaves), _f64(prior).reshape(-1)
        left = np.ascontiguousarray(left, dtype=np.int32)
        right = np.ascontiguousarray(right, dtype=np.int32)
        bl, br = _f64(bl), _f64(br)
        n_nodes, L, S = left.shape[0], leaves.shape[0], leaves.shape[1]
        out = C.c_double()
        rd = np.empty((S, 4)) if want_root else None
        self._check(self._lib.phylo_tree_loglik(self._h, C.c_int(n_nodes), C.c_int(L), C.c_int(S), _ptr(left), _ptr(right),
                                                _ptr(bl), _ptr(br), C.c_int(int(root)), _ptr(leaves), _ptr(prior),
                                                C.byref(out), _ptr(rd)))
        return out.value, rd

    def trees_loglik(self, child, blen, prior=None, want_sites=False):
        """Log-likelihoods of T explicit trees over the context's resident leaves (phylo_trees_loglik): child, blen [T][N-1][2],
        leaves 0 .. N-1, row i = internal node N + i, the last row the root; prior None = the model's pi.  Returns loglik [T],
        or (loglik, site_lik [T][S]) with want_sites; self.last_trees_stats holds the call's stats.  A tree that is no tree, or a
        length that is not finite and >= 0 or lies outside the matrix function's domain (expm_batched), raises PhyloError naming
        tree and row before anything is queued; every trees_* call does."""
        child, blen = _tree_rows(child, blen, self.N)
        T = child.shape[0]
        pr = None if prior is None else _f64(prior).reshape(-1)
        if pr is not None and pr.shape != (4,):
            raise ValueError("prior must hold 4 values")
        out = np.empty(T)
        sites = np.empty((T, self.S)) if want_sites else None
        st = Stats()
        self._check(self._lib.phylo_trees_loglik(self._h, C.c_int(T), _ptr(child), _ptr(blen), _ptr(pr), _ptr(out), _ptr(sites),
                                                 C.byref(st)))
        self.last_trees_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return (out, sites) if want_sites else out

    def trees_loglik_rates(self, child, blen, rates, weights, prior=None, want_sites=False, want_cats=False):
        """trees_loglik under a mixture of C rate categories (phylo_trees_loglik_rates; phylo_amd.rates.rate_model builds discrete
        Gamma and +I ones): category c scores the tree at rates[c] * blen, a site's value is sum_c weights[c] f_c by the fma chain
        in ascending c.  The weights are used as given (finite, >= 0, not normalised).  Returns loglik [T], followed by site_lik
        [T][S] (the mixed value) with want_sites and by cat_lik [T][C][S] (every category's factor) with want_cats;
        self.last_trees_stats holds the call's stats.  The matrix of category c is the matrix of the single rounded product
        rates[c] * blen; that product is held to the matrix function's domain (expm_batched), as in every trees_*_rates call:
        PhyloError naming tree, row and category."""
        child, blen = _tree_rows(child, blen, self.N)
        T = child.shape[0]
        rates, weights = _f64(rates).reshape(-1), _f64(weights).reshape(-1)
        if rates.shape != weights.shape:
            raise ValueError("rates and weights must hold one value per category, got %r and %r" % (rates.shape, weights.shape))
        nc = rates.size
        pr = None if prior is None else _f64(prior).reshape(-1)
        if pr is not None and pr.shape != (4,):
            raise ValueError("prior must hold 4 values")
        out = np.empty(T)
        sites = np.empty((T, self.S)) if want_sites else None
        cats = np.empty((T, nc, self.S)) if want_cats else None
        st = Stats()
        self._check(self._lib.phylo_trees_loglik_rates(self._h, C.c_int(T), _ptr(child), _ptr(blen), C.c_int(nc), _ptr(rates),
                                                       _ptr(weights), _ptr(pr), _ptr(out), _ptr(sites), _ptr(cats), C.byref(st)))
        self.last_trees_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        res = (out,) + ((sites,) if want_sites else ()) + ((cats,) if want_cats else ())
        return res if len(res) > 1 else out

    def trees_grad(self, child, blen, prior=None, want_curv=False):
        """Derivatives of trees_loglik with respect to every branch length (phylo_trees_grad): returns (loglik [T], grad
        [T][N-1][2]) or, with want_curv, (loglik, grad, curv) -- curv the own second derivative of every length.  loglik is bit
        for bit trees_loglik's; a tree whose loglik is not finite, or which has a site factor below 2^-1020 (a finite loglik
        then), has NaN derivatives.  self.last_trees_stats holds the call's
        stats.  phylo_amd.treeopt.optimize_branches climbs with it."""
        child, blen = _tree_rows(child, blen, self.N)
        T = child.shape[0]
        pr = None if prior is None else _f64(prior).reshape(-1)
        if pr is not None and pr.shape != (4,):
            raise ValueError("prior must hold 4 values")
        out = np.empty(T)
        grad = np.empty(blen.shape)
        curv = np.empty(blen.shape) if want_curv else None
        st = Stats()
        self._check(self._lib.phylo_trees_grad(self._h, C.c_int(T), _ptr(child), _ptr(blen), _ptr(pr), _ptr(out), _ptr(grad), _ptr(curv),
                                               C.byref(st)))
        self.last_trees_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return (out, grad, curv) if want_curv else (out, grad)

    def trees_ancestral(self, child, blen, prior=None, want_post=True, want_state=True, want_pmax=False):
        """Marginal ancestral state posteriors of T explicit trees (phylo_trees_ancestral): returns (loglik [T]) followed by post
        [T][N-1][S][4] with want_post, state [T][N-1][S] (uint8, the most probable state; ANC_NOSTATE where the site has none)
        with want_state and pmax [T][N-1][S] (its posterior) with want_pmax.  Row i is internal node N + i of the tree as given,
        the last row the root.  post is not renormalised; a site whose factor lies below 2^-1020 has NaN / ANC_NOSTATE in its own
        column and leaves every other site alone.  loglik is bit for bit trees_loglik's.  self.last_trees_stats holds the call's
        stats.  phylo_amd.ancestral turns the arrays into sequences, clade names and summaries."""
        child, blen = _tree_rows(child, blen, self.N)
        T = child.shape[0]
        pr = None if prior is None else _f64(prior).reshape(-1)
        if pr is not None and pr.shape != (4,):
            raise ValueError("prior must hold 4 values")
        if not (want_post or want_state or want_pmax):
            raise ValueError("one of want_post, want_state and want_pmax must be set")
        R = self.N - 1
        out = np.empty(T)
        post = np.empty((T, R, self.S, 4)) if want_post else None
        state = np.empty((T, R, self.S), dtype=np.uint8) if want_state else None
        pmax = np.empty((T, R, self.S)) if want_pmax else None
        st = Stats()
        self._check(self._lib.phylo_trees_ancestral(self._h, C.c_int(T), _ptr(child), _ptr(blen), _ptr(pr), _ptr(out), _ptr(post), _ptr(state),
                                                    _ptr(pmax), C.byref(st)))
        self.last_trees_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return (out,) + tuple(x for x in (post, state, pmax) if x is not None)

    def trees_ancestral_rates(self, child, blen, rates, weights, prior=None, want_post=True, want_state=True, want_pmax=False,
                              want_catpost=False, want_siterate=False):
        """trees_ancestral under a mixture of C rate categories, and the site-rate posteriors beside it
        (phylo_trees_ancestral_rates).  rates and weights are [C] (one mixture for all trees) or [T][C] (tree t under row t).
        Returns (loglik [T]) followed, in this order, by post [T][N-1][S][4] with want_post, state [T][N-1][S] (uint8;
        ANC_NOSTATE where the site has none) with want_state, pmax [T][N-1][S] with want_pmax, catpost [T][C][S] (the posterior
        probability that the site evolved in category c) with want_catpost and siterate [T][S] (the posterior mean rate of the
        site, sum_c rates[c] catpost[c]) with want_siterate.  Rows as trees_ancestral.  post and catpost are not renormalised; a
        site whose mixed value lies below 2^-1020 has NaN / ANC_NOSTATE in its own column of every output and leaves every other
        site alone.  loglik is bit for bit trees_loglik_rates'.  self.last_trees_stats holds the call's stats.
        phylo_amd.ancestral turns the arrays into sequences, summaries and a table of site rates."""
        child, blen = _tree_rows(child, blen, self.N)
        T = child.shape[0]
        rates, weights = _f64(rates), _f64(weights)
        if rates.shape != weights.shape:
            raise ValueError("rates and weights must have one shape, got %r and %r" % (rates.shape, weights.shape))
        if rates.ndim == 2:
            if rates.shape[0] != T:
                raise ValueError("per-tree rates must be [T][C] with T = %d, got %r" % (T, rates.shape))
            per_tree = 1
        elif rates.ndim == 1:
            per_tree = 0
        else:
            raise ValueError("rates must be [C] or [T][C], got %r" % (rates.shape,))
        nc = rates.shape[-1]
        pr = None if prior is None else _f64(prior).reshape(-1)
        if pr is not None and pr.shape != (4,):
            raise ValueError("prior must hold 4 values")
        if not (want_post or want_state or want_pmax or want_catpost or want_siterate):
            raise ValueError("one of want_post, want_state, want_pmax, want_catpost and want_siterate must be set")
        R = self.N - 1
        out = np.empty(T)
        post = np.empty((T, R, self.S, 4)) if want_post else None
        state = np.empty((T, R, self.S), dtype=np.uint8) if want_state else None
        pmax = np.empty((T, R, self.S)) if want_pmax else None
        catpost = np.empty((T, nc, self.S)) if want_catpost else None
        siterate = np.empty((T, self.S)) if want_siterate else None
        st = Stats()
        self._check(self._lib.phylo_trees_ancestral_rates(self._h, C.c_int(T), _ptr(child), _ptr(blen), C.c_int(nc), _ptr(rates),
                                                          _ptr(weights), C.c_int(per_tree), _ptr(pr), _ptr(out), _ptr(post), _ptr(state),
                                                          _ptr(pmax), _ptr(catpost), _ptr(siterate), C.byref(st)))
        self.last_trees_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return (out,) + tuple(x for x in (post, state, pmax, catpost, siterate) if x is not None)

    def trees_grad_model(self, child, blen, dirs, prior=None, want_grad=False, want_prior=True):
        """Derivatives of trees_loglik with respect to the substitution model (phylo_trees_grad_model): dirs [P][4][4] are P
        directions in the space of generators (1 <= P <= 16; phylo_amd.modelfit.q_directions builds the twelve of the project's
        row-softmax Q).  Returns (loglik [T], dtheta [T][P]), then grad [T][N-1][2] with want_grad (trees_grad's bits), then
        dprior [T][4] with want_prior (the partial derivatives with respect to the root distribution at fixed Q;
        phylo_amd.modelfit.chain_prior turns them into d / d y_station).  dtheta[t][p] is the derivative of loglik[t] along
        dirs[p] at fixed lengths and prior; a column does not depend on which other directions ride in the call.  loglik is bit
        for bit trees_loglik's; the NaN rule is trees_grad's.  self.last_trees_stats holds the call's stats.
        phylo_amd.treeopt.optimize_model climbs with it."""
        child, blen = _tree_rows(child, blen, self.N)
        T = child.shape[0]
        dirs = _f64(dirs)
        if dirs.ndim == 2 and dirs.shape == (4, 4):
            dirs = dirs[None]
        if dirs.ndim != 3 or dirs.shape[1:] != (4, 4):
            raise ValueError("dirs must be [P][4][4], got %r" % (dirs.shape,))
        dirs = np.ascontiguousarray(dirs)
        npd = dirs.shape[0]
        pr = None if prior is None else _f64(prior).reshape(-1)
        if pr is not None and pr.shape != (4,):
            raise ValueError("prior must hold 4 values")
        out = np.empty(T)
        dtheta = np.empty((T, npd))
        grad = np.empty(blen.shape) if want_grad else None
        dprior = np.empty((T, 4)) if want_prior else None
        st = Stats()
        self._check(self._lib.phylo_trees_grad_model(self._h, C.c_int(T), _ptr(child), _ptr(blen), C.c_int(npd), _ptr(dirs), _ptr(pr),
                                                     _ptr(out), _ptr(grad), _ptr(dtheta), _ptr(dprior), C.byref(st)))
        self.last_trees_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return (out, dtheta) + ((grad,) if want_grad else ()) + ((dprior,) if want_prior else ())

    def trees_grad_rates(self, child, blen, rates, weights, prior=None, want_curv=False, want_params=False):
        """trees_grad under a mixture of C rate categories (phylo_trees_grad_rates): the derivatives of trees_loglik_rates'
        mixture log-likelihood.  rates and weights are [C] (one mixture for all trees) or [T][C] (tree t under row t).  Returns
        (loglik [T], grad [T][N-1][2]), then curv [T][N-1][2] with want_curv (the own second derivative of every length), then
        drate and dweight [T][C] with want_params (the derivatives with respect to every category's rate, at fixed blen, and
        weight; phylo_amd.rates.chain turns them into d/d alpha and d/d p_inv).  loglik is bit for bit trees_loglik_rates'; the
        NaN rule is trees_grad's, on the mixed site value.  self.last_trees_stats holds the call's stats.
        phylo_amd.treeopt.optimize_rates climbs with it."""
        child, blen = _tree_rows(child, blen, self.N)
        T = child.shape[0]
        rates, weights = _f64(rates), _f64(weights)
        if rates.shape != weights.shape:
            raise ValueError("rates and weights must have one shape, got %r and %r" % (rates.shape, weights.shape))
        if rates.ndim == 2:
            if rates.shape[0] != T:
                raise ValueError("per-tree rates must be [T][C] with T = %d, got %r" % (T, rates.shape))
            per_tree = 1
        elif rates.ndim == 1:
            per_tree = 0
        else:
            raise ValueError("rates must be [C] or [T][C], got %r" % (rates.shape,))
        nc = rates.shape[-1]
        pr = None if prior is None else _f64(prior).reshape(-1)
        if pr is not None and pr.shape != (4,):
            raise ValueError("prior must hold 4 values")
        out = np.empty(T)
        grad = np.empty(blen.shape)
        curv = np.empty(blen.shape) if want_curv else None
        drate = np.empty((T, nc)) if want_params else None
        dweight = np.empty((T, nc)) if want_params else None
        st = Stats()
        self._check(self._lib.phylo_trees_grad_rates(self._h, C.c_int(T), _ptr(child), _ptr(blen), C.c_int(nc), _ptr(rates), _ptr(weights),
                                                     C.c_int(per_tree), _ptr(pr), _ptr(out), _ptr(grad), _ptr(curv), _ptr(drate),
                                                     _ptr(dweight), C.byref(st)))
        self.last_trees_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return (out, grad) + ((curv,) if want_curv else ()) + ((drate, dweight) if want_params else ())

    def trees_nni(self, child, blen, prior=None):
        """The NNI neighbourhood of every tree at its current lengths (phylo_trees_nni): returns (loglik [T], delta [T][N-1][2]).
        delta[t][i][side], i < N-2: the change of tree t's log-likelihood when node N + i's child on `side` and the node's sibling
        change places (every subtree keeps its length); delta[t][N-2][side]: node child[N-2][0]'s side-1 child and node
        child[N-2][1]'s child on `side` change places (NaN when a root child is a leaf).  -inf: an impossible neighbour; NaN in
        every entry: trees_grad's rule.  loglik is bit for bit trees_loglik's.  self.last_trees_stats holds the call's stats.
        phylo_amd.treesearch has the moves as rows (apply_nni) and a hill-climber over this call (nni_search)."""
        child, blen = _tree_rows(child, blen, self.N)
        T = child.shape[0]
        pr = None if prior is None else _f64(prior).reshape(-1)
        if pr is not None and pr.shape != (4,):
            raise ValueError("prior must hold 4 values")
        out = np.empty(T)
        delta = np.empty(blen.shape)
        st = Stats()
        self._check(self._lib.phylo_trees_nni(self._h, C.c_int(T), _ptr(child), _ptr(blen), _ptr(pr), _ptr(out), _ptr(delta), C.byref(st)))
        self.last_trees_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return out, delta

    def trees_nni_rates(self, child, blen, rates, weights, prior=None):
        """trees_nni under a mixture of C rate categories (phylo_trees_nni_rates): returns (loglik [T], delta [T][N-1][2]), the
        change of trees_loglik_rates' mixture log-likelihood under every NNI move of every tree at its current lengths; moves,
        rows and sides as trees_nni.  rates and weights are [C] (one mixture for all trees) or [T][C] (tree t under row t).
        loglik is bit for bit trees_loglik_rates'; -inf: a neighbour whose mixed site value is 0 at a site; NaN in every entry:
        trees_grad's rule on the mixed site value.  self.last_trees_stats holds the call's stats."""
        child, blen = _tree_rows(child, blen, self.N)
        T = child.shape[0]
        rates, weights = _f64(rates), _f64(weights)
        if rates.shape != weights.shape:
            raise ValueError("rates and weights must have one shape, got %r and %r" % (rates.shape, weights.shape))
        if rates.ndim == 2:
            if rates.shape[0] != T:
                raise ValueError("per-tree rates must be [T][C] with T = %d, got %r" % (T, rates.shape))
            per_tree = 1
        elif rates.ndim == 1:
            per_tree = 0
        else:
            raise ValueError("rates must be [C] or [T][C], got %r" % (rates.shape,))
        nc = rates.shape[-1]
        pr = None if prior is None else _f64(prior).reshape(-1)
        if pr is not None and pr.shape != (4,):
            raise ValueError("prior must hold 4 values")
        out = np.empty(T)
        delta = np.empty(blen.shape)
        st = Stats()
        self._check(self._lib.phylo_trees_nni_rates(self._h, C.c_int(T), _ptr(child), _ptr(blen), C.c_int(nc), _ptr(rates), _ptr(weights),
                                                    C.c_int(per_tree), _ptr(pr), _ptr(out), _ptr(delta), C.byref(st)))
        self.last_trees_stats = {f: getattr(st, f) for f, _ in Stats._fields_}
        return out, delta

    def rell(self, site_lik, B, seed, want_reps=False, want_counts=False, want_logs=False):
        """RELL bootstrap over the site factors site_lik [T][S] of a scored tree set (phylo_rell; what trees_loglik and
        trees_loglik_rates return with want_sites): B replicates from `seed`.  Returns a dict: 'obs' [T] the observed scores (the
        contract's chain over log site factors), 'best' [B] the best tree of every replicate, 'wins' [T] their histogram, and on
        request 'rep_loglik' [T][B], 'counts' [B][S], 'site_loglik' [T][S]; 'stats' holds the call's stats.
        phylo_amd.treetests.tree_tests turns them into bootstrap proportions and KH / SH / c-ELW values."""
        sl = _f64(site_lik)
        if sl.ndim != 2:
            raise ValueError("site_lik must be [T][S], got %r" % (sl.shape,))
        T, S = sl.shape
        B = int(B)
        obs, best, wins = np.empty(T), np.empty(max(B, 0), dtype=np.int32), np.empty(T, dtype=np.int64)
        reps = np.empty((T, B)) if want_reps and B > 0 else None
        counts = np.empty((B, S), dtype=np.int32) if want_counts and B > 0 else None
        logs = np.empty((T, S)) if want_logs else None
        st = Stats()
        self._check(self._lib.phylo_rell(self._h, C.c_int(T), C.c_int(S), _ptr(sl), C.c_int(B), C.c_uint64(int(seed)), _ptr(obs),
                                         _ptr(best), _ptr(wins), _ptr(reps), _ptr(counts), _ptr(logs), C.byref(st)))
        out = {'obs': obs, 'best': best, 'wins': wins, 'stats': {f: getattr(st, f) for f, _ in Stats._fields_}}
        if want_reps:
            out['rep_loglik'] = reps
        if want_counts:
            out['counts'] = counts
        if want_logs:
            out['site_loglik'] = logs
        return out

    def rell_multiscale(self, site_lik, draws, B, seed, want_best=False, want_reps=False, want_counts=False):
        """Multiscale RELL bootstrap over the site factors site_lik [T][S] (phylo_rell_multiscale): B replicates at each of the
        K scales, scale k drawing draws[k] sites.  Returns a dict: 'obs' [T] (phylo_rell's observed scores), 'wins' [K][T] the
        number of replicates of scale k in which tree t scores highest (ties to the lowest t), 'stats', and on request 'best'
        [K][B], 'rep_loglik' [K][T][B] (not rescaled by S / draws[k]) and 'counts' [K][B][S].  The score matrix is not stored
        on the device unless want_reps asks for it.  treetests.au_scales gives draws, treetests.au_test reads the AU p-values
        off wins.  Scale 0 shares its random stream with rell(): the two calls' samples are not independent."""
        sl = _f64(site_lik)
        if sl.ndim != 2:
            raise ValueError("site_lik must be [T][S], got %r" % (sl.shape,))
        T, S = sl.shape
        dr = np.ascontiguousarray(draws, dtype=np.int32).reshape(-1)
        K, B = dr.size, int(B)
        nb = max(B, 0)
        obs, wins = np.empty(T), np.empty((K, T), dtype=np.int64)
        best = np.empty((K, nb), dtype=np.int32) if want_best else None
        reps = np.empty((K, T, nb)) if want_reps else None
        counts = np.empty((K, nb, S), dtype=np.int32) if want_counts else None
        st = Stats()
        self._check(self._lib.phylo_rell_multiscale(self._h, C.c_int(T), C.c_int(S), _ptr(sl), C.c_int(K), _ptr(dr), C.c_int(B),
                                                    C.c_uint64(int(seed)), _ptr(obs), _ptr(wins), _ptr(best), _ptr(reps), _ptr(counts),
                                                    C.byref(st)))
        out = {'obs': obs, 'wins': wins, 'stats': {f: getattr(st, f) for f, _ in Stats._fields_}}
        if want_best:
            out['best'] = best
        if want_reps:
            out['rep_loglik'] = reps
        if want_counts:
            out['counts'] = counts
        return out

    def resample(self, logw, seed, step):
        w = _f64(logw).reshape(-1)
        idx = np.empty(w.size, dtype=np.int64)
        self._check(self._lib.phylo_resample(self._h, _ptr(w), C.c_int(w.size), C.c_uint64(seed), C.c_uint32(step), _ptr(idx)))
        return idx

    def log_zsmc(self, logw_RxK):
        w = _f64(logw_RxK)
        out = C.c_double()
        self._check(self._lib.phylo_log_zsmc(self._h, _ptr(w), C.c_int(w.shape[0]), C.c_int(w.shape[1]), C.byref(out)))
        return out.value

    def math_probe(self, op, x, y=None):
        x = _f64(x).reshape(-1)
        y = _f64(x if y is None else y).reshape(-1)
        out = np.empty_like(x)
        self._check(self._lib.phylo_math_probe(self._h, C.c_int(op), _ptr(x), _ptr(y), C.c_int(x.size), _ptr(out)))
        return out

    def frechet_probe(self, A, E, form):
        """The reverse pass's Frechet derivative of expm on pairs of 4x4 matrices [n, 4, 4]: form 0 a lane per matrix
        (pg_expm4_frechet), form 1 a quad per matrix (pg_expm4_frechet_row)."""
        A = _f64(A).reshape(-1, 16)
        E = _f64(E).reshape(-1, 16)
        if A.shape != E.shape:
            raise ValueError("A and E must hold the same number of 4x4 matrices")
        L = np.empty_like(A)
        self._check(self._lib.phylo_debug_frechet(self._h, C.c_int(int(form)), _ptr(A), _ptr(E), C.c_int(A.shape[0]), _ptr(L)))
        return L.reshape(-1, 4, 4)

    def site_product_probe(self, p, x1, x2):
        """debug_site_product through a kernel on this context's device"""
        return _site_product(self._h, p, x1, x2)

    # ---- sweep
    def sweep_async(self, seed, flags=FLAGS_DEFAULT, M=1):
        self._check(self._lib.phylo_sweep_async(self._h, C.c_uint64(seed), C.c_uint32(flags), C.c_int(M)))
        self._last_batch = 1

    def sweep_batch_async(self, seeds, flags=FLAGS_DEFAULT):
        """len(seeds) independent sweeps of K/len(seeds) particles each, in one set of launches."""
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        self._check(self._lib.phylo_sweep_batch_async(self._h, _ptr(sd), C.c_int(sd.size), C.c_uint32(flags)))
        self._last_batch = sd.size

    def sweep_batch_begin(self, seeds, flags=FLAGS_DEFAULT):
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        self._check(self._lib.phylo_sweep_batch_begin(self._h, _ptr(sd), C.c_int(sd.size), C.c_uint32(flags)))
        self._last_batch = sd.size

    def sweep_fetch_logz(self, G):
        out = np.empty(int(G))
        self._check(self._lib.phylo_sweep_fetch_logz(self._h, _ptr(out), C.c_int(int(G))))
        return out

    def sweep_begin(self, seed, flags=FLAGS_DEFAULT, M=1):
        self._check(self._lib.phylo_sweep_begin(self._h, C.c_uint64(seed), C.c_uint32(flags), C.c_int(M)))

    def sweep_step(self):
        self._check(self._lib.phylo_sweep_step(self._h))

    def sweep_step_a(self):
        self._check(self._lib.phylo_sweep_step_a(self._h))

    def sweep_finish(self):
        self._check(self._lib.phylo_sweep_finish(self._h))

    def synchronize(self):
        self._check(self._lib.phylo_synchronize(self._h))

    def sweep_fetch(self, arrays=True):
        R, K = self.N - 1, self.K_local
        out = {}
        if arrays:
            out = {'log_weights': np.empty((R, K)), 'log_likelihood': np.empty((R, K)),
                   'left_branches': np.empty((R, K)), 'right_branches': np.empty((R, K)),
                   'merges': np.empty((R, K, 2), dtype=np.int32),
                   'ancestors': np.empty((max(R - 1, 0), K), dtype=np.int64)}
        z = C.c_double()
        st = Stats()
        g = out.get
        self._check(self._lib.phylo_sweep_fetch(self._h, _ptr(g('log_weights')), _ptr(g('log_likelihood')),
                                                _ptr(g('left_branches')), _ptr(g('right_branches')), _ptr(g('merges')),
                                                _ptr(g('ancestors')), C.byref(z), C.byref(st)))
        out['logZ'] = z.value
        out['stats'] = {f: getattr(st, f) for f, _ in Stats._fields_}
        return out

    def sweep(self, seed, flags=FLAGS_DEFAULT, M=1):
        self.sweep_async(seed, flags, M)
        return self.sweep_fetch()

    def sweep_node(self, r, k):
        out = np.empty((self.S, 4))
        self._check(self._lib.phylo_sweep_node(self._h, C.c_int(r), C.c_int(k), _ptr(out)))
        return out

    def sweep_backward(self):
        """Gradient of logZ of the last sweep (run with KEEP_GRAPH) w.r.t. lam_l, lam_r, pi, Q (raw quantities)."""
        R = self.N - 1
        out = {'d_lam_l': np.empty(R), 'd_lam_r': np.empty(R), 'd_pi': np.empty(4), 'd_Q': np.empty((4, 4))}
        st = Stats()
        self._check(self._lib.phylo_sweep_backward(self._h, _ptr(out['d_lam_l']), _ptr(out['d_lam_r']), _ptr(out['d_pi']),
                                                   _ptr(out['d_Q']), C.byref(st)))
        out['backward_ms'] = st.sweep_ms
        out['backward_host_ms'] = st.merge_ms          # host time of the integer lists inside backward_ms (built, or waited for)
        out['backward_lists'] = 'device' if st.merge_launches else 'host'   # who built them (phylo_revlists_dev.h / phylo_revlists.h)
        out['backward_launches'] = st.n_launches
        return out

    def sweep_backward_batch(self, G=None):
        """Gradients of the G log Z-hat of the last batched sweep (run with KEEP_GRAPH): the arrays of sweep_backward with a leading
        G axis, from one reverse pass over the block-diagonal genealogy (phylo_sweep_backward_batch)."""
        R = self.N - 1
        G = int(self._last_batch if G is None else G)
        out = {'d_lam_l': np.empty((G, R)), 'd_lam_r': np.empty((G, R)), 'd_pi': np.empty((G, 4)), 'd_Q': np.empty((G, 4, 4))}
        st = Stats()
        self._check(self._lib.phylo_sweep_backward_batch(self._h, _ptr(out['d_lam_l']), _ptr(out['d_lam_r']), _ptr(out['d_pi']),
                                                         _ptr(out['d_Q']), C.c_int(G), C.byref(st)))
        out['backward_ms'] = st.sweep_ms
        out['backward_host_ms'] = st.merge_ms
        out['backward_lists'] = 'device' if st.merge_launches else 'host'
        out['backward_launches'] = st.n_launches
        return out

    def tree_summary(self):
        """Tree posterior of the last sweep (phylo_tree_summary; every group of a batched sweep; a collective on a sharded context,
        which returns the same tables on every rank).  NumPy arrays, rows group-major (`*_offsets[g]:*_offsets[g+1]` = group g):
        clade_bits [n_clades, W] uint64 (taxon i = bit i % 64 of word i // 64), clade_weight [n_clades] uint64, clade_group;
        topo_weight uint64, topo_count, topo_rep (smallest particle, inside its group), topo_group [n_topologies];
        particle_topo [K] (row inside the particle's group), u [K] uint64, U [G] uint64; G, W, summary_ms (device time)."""
        nc, nt, G = C.c_int64(), C.c_int32(), C.c_int32()
        st = Stats()
        self._check(self._lib.phylo_tree_summary(self._h, C.byref(nc), C.byref(nt), C.byref(G), C.byref(st)))
        nc, nt, G = nc.value, nt.value, G.value
        self._last_counts = (nc, nt, G)
        W = (self.N + 63) // 64
        out = {'clade_bits': np.empty((nc, W), dtype=np.uint64), 'clade_weight': np.empty(nc, dtype=np.uint64),
               'clade_group': np.empty(nc, dtype=np.int32), 'topo_weight': np.empty(nt, dtype=np.uint64),
               'topo_count': np.empty(nt, dtype=np.int32), 'topo_rep': np.empty(nt, dtype=np.int32),
               'topo_group': np.empty(nt, dtype=np.int32), 'particle_topo': np.empty(self.K, dtype=np.int32),
               'u': np.empty(self.K, dtype=np.uint64), 'U': np.empty(G, dtype=np.uint64)}
        names = ('clade_bits', 'clade_weight', 'clade_group', 'topo_weight', 'topo_count', 'topo_rep', 'topo_group', 'particle_topo',
                 'u', 'U')
        self._check(self._lib.phylo_tree_summary_fetch(self._h, *[_ptr(out[n]) for n in names]))
        out['G'], out['W'] = G, W
        out['clade_offsets'] = np.searchsorted(out['clade_group'], np.arange(G + 1))
        out['topo_offsets'] = np.searchsorted(out['topo_group'], np.arange(G + 1))
        out['summary_ms'] = st.sweep_ms
        out['summary_launches'] = st.n_launches
        return out

    def tree_branches(self, summary=None):
        """Branch-length sums of the last tree_summary() of the last sweep (phylo_tree_branches; collective when sharded).  `summary`:
        that call's tables (for the row counts; default: fetched again).  Returns clade_stats [n_clades, 4], leaf_stats [G, N, 4],
        topo_stats [n_topologies, 2N-2, 4] (float64: S1 = sum u b, S2 = sum u b b, min b, max b; the N leaves first, then the
        topology's clades) and topo_clades [n_topologies, N-2] (clade rows inside the group, ascending); branches_ms, branches_launches."""
        st = Stats()
        self._check(self._lib.phylo_tree_branches(self._h, C.byref(st)))
        if summary is None:
            nc, nt, G = self._last_counts
        else:
            nc, nt, G = len(summary['clade_weight']), len(summary['topo_weight']), int(summary['G'])
        N = self.N
        out = {'clade_stats': np.empty((nc, 4)), 'leaf_stats': np.empty((G, N, 4)),
               'topo_clades': np.empty((nt, N - 2), dtype=np.int32), 'topo_stats': np.empty((nt, 2 * N - 2, 4))}
        self._check(self._lib.phylo_tree_branches_fetch(self._h, _ptr(out['clade_stats']), _ptr(out['leaf_stats']),
                                                        _ptr(out['topo_clades']), _ptr(out['topo_stats'])))
        out['branches_ms'] = st.sweep_ms
        out['branches_launches'] = st.n_launches
        return out

    def vi_gradients(self, seed, flags, M, jc, packed_vars):
        """The gradient half of a VI training step in the library (phylo_vi_gradients): packed_vars = a_l | a_r | y_q | y_station.
        Returns (logZ, grads packed alike, forward stats, backward stats)."""
        vars_ = _f64(packed_vars)
        grads = np.empty_like(vars_)
        z, fwd, bwd = C.c_double(), Stats(), Stats()
        self._check(self._lib.phylo_vi_gradients(self._h, C.c_uint64(seed), C.c_uint32(flags), C.c_int(M), C.c_int(int(jc)), _ptr(vars_),
                                                 C.byref(z), _ptr(grads), C.byref(fwd), C.byref(bwd)))
        return z.value, grads, fwd, bwd

    def vi_gradients_batch(self, seeds, flags, jc, packed_vars):
        """vi_gradients for len(seeds) independent systems of K / len(seeds) particles in one batched sweep and one reverse pass
        (phylo_vi_gradients_batch).  Returns (logZ [G], grads [G, 2 (N-1) + 20], forward stats, backward stats)."""
        vars_ = _f64(packed_vars)
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        G = sd.size
        grads = np.empty((G, 2 * (self.N - 1) + 20))
        z = np.empty(G)
        fwd, bwd = Stats(), Stats()
        self._check(self._lib.phylo_vi_gradients_batch(self._h, _ptr(sd), C.c_int(G), C.c_uint32(flags), C.c_int(int(jc)), _ptr(vars_),
                                                       _ptr(z), _ptr(grads), C.byref(fwd), C.byref(bwd)))
        self._last_batch = G
        return z, grads, fwd, bwd

    def debug_device_lists(self, ancestors=None, child=None):
        """The reverse pass's integer lists as the device kernels build them from the last (lazy, KEEP_GRAPH, plain proposal) sweep,
        or from the genealogy given (ancestors [N-2][K], child [N-1][K][2]; the context then needs a new sweep before the next
        sweep_backward): the dict of debug_reverse_lists plus 'ancestors' and 'child' they were built from."""
        R, K = self.N - 1, self.K
        nn = R * K
        cap = 2 * nn // 4 + 1
        n_lists = R * (K + 1) + 9 * nn + 1 + 2 * cap
        lists = np.zeros(n_lists, dtype=np.int32)
        meta = np.zeros(6 + 3 * (R + 1), dtype=np.int32)
        if child is not None:
            anc = np.ascontiguousarray(ancestors if R > 1 else np.zeros((0, K)), dtype=np.int64).reshape(max(R - 1, 0), K)
            child = np.ascontiguousarray(child, dtype=np.int32).reshape(R, K, 2)
            self._check(self._lib.phylo_debug_device_lists_of(self._h, _ptr(anc) if R > 1 else None, _ptr(child), _ptr(lists),
                                                              C.c_int64(n_lists), _ptr(meta), C.c_int(meta.size)))
        else:
            anc = np.zeros((max(R - 1, 0), K), dtype=np.int64)
            child = np.zeros((R, K, 2), dtype=np.int32)
            self._check(self._lib.phylo_debug_device_lists(self._h, _ptr(lists), C.c_int64(n_lists), _ptr(meta), C.c_int(meta.size),
                                                           _ptr(anc) if R > 1 else None, _ptr(child)))
        out = _lists_dict(lists, meta, R, K)
        out['ancestors'] = anc
        out['child'] = child
        return out

    def debug_stamps(self):
        """[N][16] s_memrealtime ticks (100 MHz) of workgroup 0 of the last one-launch sweep (PHYLO_PERSIST_STAMPS=1)."""
        out = np.zeros((self.N, 16), dtype=np.uint64)
        self._check(self._lib.phylo_debug_stamps(self._h, _ptr(out), C.c_int(out.size)))
        return out

    # ---- multi-GPU
    def comm_init(self, rank, world, comm_id):
        buf = C.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        self._check(self._lib.phylo_comm_init(self._h, C.c_int(rank), C.c_int(world), buf))
        self.K_local = self.K // world
        self.k0 = rank * self.K_local

    def comm_share(self, owner):
        """Join `owner`'s communicator (a further sweep in flight on the same rank); keep `owner` alive."""
        self._check(self._lib.phylo_comm_share(self._h, owner._h))
        self._owner = owner
        world = owner.K // owner.K_local
        self.K_local = self.K // world
        self.k0 = (owner.k0 // owner.K_local) * self.K_local

    def comm_allgather_columns(self, a):
        """a: [..., K_local] on every rank -> [..., K] (rank order = particle order).  Collective."""
        a = np.ascontiguousarray(a)
        world = self.K // self.K_local
        if world == 1:
            return a
        out = np.empty((world,) + a.shape, dtype=a.dtype)
        self._check(self._lib.phylo_comm_allgather(self._h, _ptr(a), C.c_size_t(a.nbytes), _ptr(out)))
        return np.concatenate(list(out), axis=-1)

    def comm_allgather_blob(self, a):
        """a: the same shape and dtype on every rank -> [world, ...] (one row per rank).  Collective."""
        a = np.ascontiguousarray(a)
        world = self.K // self.K_local
        if world == 1:
            return a[None]
        out = np.empty((world,) + a.shape, dtype=a.dtype)
        self._check(self._lib.phylo_comm_allgather(self._h, _ptr(a), C.c_size_t(a.nbytes), _ptr(out)))
        return out

    def debug_remote_cache(self):
        """(slots claimed by the last sweep, slots) of the local cache of remote nodes of a sharded context ((0, 0): no cache)"""
        used, cap = C.c_int(0), C.c_int(0)
        self._check(self._lib.phylo_debug_remote_cache(self._h, C.byref(used), C.byref(cap)))
        return used.value, cap.value

    def debug_site_patterns(self):
        """(U, taken): the distinct columns of the current leaves (0: not coded) and whether the record-form merge takes the
        site-pattern form for them (phylo_site_patterns.h)"""
        U, taken = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.phylo_debug_site_patterns_of(self._h, C.byref(U), C.byref(taken)))
        return U.value, bool(taken.value)

    def debug_clade_patterns(self):
        """(eligible, taken, bytes): the current leaves have clade tables that a record-form sweep would use; the last sweep begun on
        the launch path took them (its plan's clade_pat); the tables' size (0: none)"""
        el, taken, nbytes = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._check(self._lib.phylo_debug_clade_patterns_of(self._h, C.byref(el), C.byref(taken), C.byref(nbytes)))
        return bool(el.value), bool(taken.value), nbytes.value

    def debug_tree_branches(self):
        """The plan the last tree_branches() of this context took: {'wide': 64-bit (topology, clade) keys, 'cbits', 'tbits'}"""
        wide, cbits, tbits = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.phylo_debug_tree_branches_of(self._h, C.byref(wide), C.byref(cbits), C.byref(tbits)))
        return {'wide': bool(wide.value), 'cbits': cbits.value, 'tbits': tbits.value}

    def debug_scan_form(self, Kg, wanted=True):
        """debug_scan_form with the PHYLO_SCAN_MULTI_MIN this context read when it was created"""
        rc = self._lib.phylo_debug_scan_form(self._h, C.c_int(Kg), C.c_int(0), C.c_int(int(wanted)))
        if rc < 0:
            raise PhyloError(rc, self._lib.phylo_last_error(self._h).decode())
        return SCAN_FORMS[rc]

    def debug_sweep_chain(self):
        """Did the rank events of this context's last sweep take the chain form (sweep_chain_form_of)?"""
        taken = C.c_int32(0)
        self._check(self._lib.phylo_debug_sweep_chain_of(self._h, C.byref(taken)))
        return bool(taken.value)

    def debug_sweep_launch(self):
        """How this context's last sweep launched its record-form merge and chain bookkeeping: debug_sweep_launch's dict"""
        out = (C.c_int32 * 2)()
        self._check(self._lib.phylo_debug_sweep_launch_of(self._h, out))
        return {"launch_xcd": bool(out[0]), "book_xcd": bool(out[1])}

    def debug_scan_ancestors(self, logw, seeds, r_next):
        """The tail of the resampling scan alone (pp_scan_ancestors) on log-weights [G][Kg] with the groups' seeds, for the draws of rank
        event r_next: (anc [G][Kg] int32, list [G][Kg] int32 with -1 behind the first cnt[g] entries, cnt [G] int32)."""
        w = np.ascontiguousarray(logw, dtype=np.float64)
        if w.ndim != 2:
            raise ValueError("logw must be [G][Kg]")
        G, Kg = w.shape
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        if sd.shape != (G,):
            raise ValueError("one seed per group")
        anc = np.full((G, Kg), -2, dtype=np.int32)
        lst = np.full((G, Kg), -2, dtype=np.int32)
        cnt = np.full(G, -2, dtype=np.int32)
        self._check(self._lib.phylo_debug_scan_ancestors(self._h, _ptr(w), C.c_int(Kg), C.c_int(G), _ptr(sd), C.c_uint32(r_next), _ptr(anc),
                                                         _ptr(lst), _ptr(cnt)))
        return anc, lst, cnt

    def debug_persist(self):
        """The grid the last sweep of this context took as ONE launch: {'nt', 'Wg', 'm', 'lds'} (threads per workgroup, workgroups
        per group, particles per workgroup, dynamic LDS bytes); PhyloError (PHYLO_ESTATE) when it ran on the launch path."""
        nt, Wg, m, lds = C.c_int32(0), C.c_int32(0), C.c_int32(0), C.c_int64(0)
        self._check(self._lib.phylo_debug_persist_of(self._h, C.byref(nt), C.byref(Wg), C.byref(m), C.byref(lds)))
        return {'nt': nt.value, 'Wg': Wg.value, 'm': m.value, 'lds': lds.value}

    def comm_exchange_kind(self):
        """'none' | 'rccl' | 'hostshm' | 'p2p': how the K-vectors of a rank event reach the other ranks"""
        return ('none', 'rccl', 'hostshm', 'p2p')[int(self._lib.phylo_comm_exchange_kind(self._h))]

    def comm_max(self, value):
        v = C.c_double(float(value))
        self._check(self._lib.phylo_comm_max(self._h, C.byref(v)))
        return v.value

    def comm_barrier(self):
        self._check(self._lib.phylo_comm_barrier(self._h))


def sweep_step_group(ctxs):
    """One rank event of several sweeps in flight (same rank event, one shared communicator): one grouped collective."""
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    rc = load().phylo_sweep_step_group(arr, C.c_int(len(ctxs)))
    if rc != PHYLO_OK:
        raise PhyloError(rc, (load().phylo_last_error(None) or b"").decode())


def comm_unique_id():
    buf = C.create_string_buffer(COMM_ID_BYTES)
    rc = load().phylo_comm_unique_id(buf)
    if rc != PHYLO_OK:
        raise PhyloError(rc, (load().phylo_last_error(None) or b"").decode())
    return buf.raw
