"""The form of the forward sweep's launch path (phylo_amd/csrc/phylo_sweep_plan.h: sweep_plan_form once per sweep, sweep_plan_launches
for what stats['n_launches'] counts) against a restatement in Python of the rules as the driver spelled them before there was a
plan: condition by condition, rank event by rank event.  Every form computes the same bits, so a rule that silently picks another
form passes every parity test and only shows as a slower sweep: this is where the selection itself is pinned.  No GPU:
phylo_debug_sweep_plan calls the two functions the driver calls."""
import itertools

import pytest

from phylo_amd import _ffi

TWISTING, KEEP_GRAPH, TIME_KERNELS, EAGER_NODES = _ffi.TWISTING, _ffi.KEEP_GRAPH, _ffi.TIME_KERNELS, _ffi.EAGER_NODES
MAT_GROUP = 64                        # PK_MAT_GROUP (phylo_kernels.h)
SCAN_KERNEL_MAX_KG = 16384            # PP_SCAN_KERNEL_MAX_KG (phylo_persist.h)
KEPT_BITS_TAXA = 65                   # PG_KEPT_BITS_TAXA (phylo_revlists.h)
MAX_GROUPS = 64                       # PK_MAX_GROUPS
TWIST_MAX_M, TWIST_MAX_J = 1024, 1 << 20
SITE_TILE = 2048                      # pm_site_tile (phylo_math.h)
EINVAL = -1                           # PHYLO_EINVAL


def _refused(N, K, S, G, M, world, transport, flags):
    """sweep_begin_impl's argument refusals"""
    twist, graph = bool(flags & TWISTING), bool(flags & KEEP_GRAPH)
    if G < 1 or G > MAX_GROUPS or K % G:
        return True
    if G > 1 and twist:
        return True
    if G > 1 and graph and (world != 1 or transport or S > 4096):
        return True
    if twist and (M < 1 or M > TWIST_MAX_M or (N * (N - 1) // 2) * M > TWIST_MAX_J):
        return True
    return graph and world != 1 and (twist or S > 4096)


def _rules(N, K, Kl, S, G, M, world, transport, flags, sw):
    env_eager, rehearse, env_replicated, jc, coded, p2p = (name in sw for name in _ffi.SWEEP_PLAN_SWITCHES)
    R, Kg = N - 1, K // G
    p = {}
    # --- sweep_begin_impl
    twist = p["twist"] = bool(flags & TWISTING)
    graph = p["graph"] = bool(flags & KEEP_GRAPH)
    p["timek"] = bool(flags & TIME_KERNELS)
    lazy = p["lazy"] = not twist and (not graph or S <= 4096) and not (flags & EAGER_NODES) and not env_eager
    book_mat = p["book_mat"] = lazy and world == 1 and not transport and N <= 64 and S <= 4096 and G == 1 and Kl <= 8192
    shard_form = p["shard_form"] = world > 1 or (transport and rehearse)
    replicated = p["replicated_book"] = env_replicated or (graph and world > 1)
    p["mat_by_draws"] = (lazy and shard_form and not twist and not replicated and S <= 4096
                         and ((Kg <= 4096 and Kl <= 8192) or (Kg % MAT_GROUP == 0 and Kl % MAT_GROUP == 0)))
    p["want_rdraw"] = book_mat or p["mat_by_draws"]
    p["sorted_prologue"] = not twist and not jc and 2 * R * Kl >= 262144
    launches = [1]
    # --- sweep_step_a, sweep_step_impl: rank event by rank event
    p["step_a_work"] = shard_form and lazy and not twist and not replicated
    p["mat_draws_grouped"] = Kg > 4096 or Kl > 8192
    p["mat_grouped"] = S <= 4096 and Kl > 8192
    p["mat_barrier"] = bool(transport)
    p["one_tile"] = S <= 4096                              # the grid of pk_materialize_adopted
    p["twist_ll"] = twist and coded                        # ta.pair_hist
    p["twist_tables"] = twist and bool(transport)          # !ta.own_tables
    p["batched"] = G > 1                                   # the G > 1 branch of the scan: stride R + 1
    ntiles = (S + SITE_TILE - 1) // SITE_TILE
    p["tile_epilogue"] = ntiles > 1
    run_local_book = False                # sweep_run::local_book: assigned by the plain bookkeeping branch alone
    widths, use_rec, mat_after, fix, final_missing = set(), set(), set(), set(), None
    for r in range(R):
        n = 0
        if p["step_a_work"] and r > 0:
            n += 1 if p["mat_by_draws"] else 2
        no_store = r == R - 1 and not graph and not (flags & EAGER_NODES) and not env_eager
        if r == R - 1:
            final_missing = no_store and not lazy
        use_rec.add(not twist and Kl == K and (lazy or no_store))
        if twist:
            n += 3 + (1 if coded else 0) + (1 if transport else 0)
        elif book_mat and r > 0:
            widths.add(16 if N <= 16 else 32 if N <= 32 else 64)
            n += 1
        else:
            run_local_book = (world > 1 or (transport and rehearse)) and not replicated
            nbook = Kl if run_local_book else K
            widths.add(8 if N <= 16 and nbook >= 8192 else 16 if N <= 16 else 32 if N <= 32 else 64)
            n += 1
        mat = lazy and r > 0 and not (run_local_book and not twist) and not book_mat
        if r > 0:
            mat_after.add(mat)
        n += 1 if mat else 0
        n += 2 if ntiles > 1 else 1
        fix.add(bool(transport) and not run_local_book)
        n += 1 if transport and not run_local_book else 0
        n += 1                                # the scan (three launches when several workgroups scan a group: counted once)
        launches.append(n)
    assert len(use_rec) == 1 and len(fix) == 1 and len(mat_after) <= 1
    p["local_book"] = run_local_book
    p["use_rec"] = use_rec.pop()
    p["mat_after_book"] = mat_after.pop() if mat_after else (lazy and not run_local_book and not book_mat)
    p["fix_rootll"] = fix.pop()
    # one width per sweep, 0 only where no bookkeeping is launched (twisted): pk_rank_book_packed has 8, 16, 32 and 64 (a wave per
    # particle, every N > 32), pk_rank_book_mat has 16 (also where the packed launch of rank event 0 took 8), 32, 64
    wide = N <= 16 and (Kl if run_local_book else K) >= 8192
    p["book_width"] = 0 if twist else (8 if wide else 16) if N <= 16 else 32 if N <= 32 else 64
    if not twist:
        packed = p["book_width"]
        mat = max(p["book_width"], 16)
        assert widths <= {packed, mat} and (packed in widths), (widths, p["book_width"])
    p["fold_logz"] = Kg <= SCAN_KERNEL_MAX_KG
    p["no_store_last"] = not graph and not (flags & EAGER_NODES) and not env_eager
    p["final_missing"] = final_missing
    # --- phylo_sweep_finish
    p["last_graph_eager"] = graph and not lazy and not twist and S <= 4096 and world == 1 and Kl == K and N > KEPT_BITS_TAXA
    launches.append((0 if p["fold_logz"] else 1) + ((4 if p2p else 2) if graph and world > 1 else 0))
    p["launches"] = launches
    return p


def _plan(N, K, S, **kw):
    out = _ffi.debug_sweep_plan(N, K, S, **kw)
    mask = out.pop("mask")
    assert mask == sum(int(out[name]) << i for i, name in enumerate(_ffi.SWEEP_PLAN_BITS)) | out["book_width"] // 8 << 28
    return out


# (N, K, S): every size threshold of sweep_plan_form from both sides (K_local = K, K / 2 and G = 1, 2, 4 multiply the cases)
SHAPES = [
    (12, 2048, 898),                                      # primate.p
    (16, 64, 64), (17, 64, 64), (32, 64, 64), (33, 64, 64), (64, 64, 64), (65, 64, 64), (66, 16, 64),   # book widths, kept bits
    (5, 64, 4096), (5, 64, 4097), (5, 16, 2048), (5, 16, 2049),   # one workgroup per node / site tiles; one site tile / two
    (5, 4096, 64), (5, 4098, 64), (5, 4160, 64), (5, 4224, 64),   # K / G = 4096 / 4098 with two ranks; whole groups of 64 or not
    (5, 8192, 64), (5, 8193, 64), (5, 8191, 64),          # K_local = 8192 / 8193; tables advanced 8191 / 8192 at N <= 16
    (5, 16382, 64), (5, 16384, 64), (5, 16386, 64), (5, 16388, 64),   # K_local and K / G around 8192 and 4096 when halved, quartered
    (5, 32768, 64), (5, 32772, 64), (5, 65536, 64), (5, 65540, 64),   # K / G = 16384 / 16386 (the folding scan), multiples of 64 or not
    (3, 32768, 8), (2, 65536, 8), (2, 131071, 8), (2, 131072, 8), (2, 262142, 8), (2, 262144, 8),   # 2 R K_local around 262144; R = 1
    (4, 43691, 8),                                        # 2 R K_local = 262146 with R = 3
    (2, 8, 16),
]
FLAGS = [t | g | e | k for t, g, e, k in itertools.product((0, TWISTING), (0, KEEP_GRAPH), (0, EAGER_NODES), (0, TIME_KERNELS))]
# the three environment switches in every combination, with none and with all of the context's three facts (each fact feeds one
# rule of its own: test_primate_default_and_each_switch takes them one at a time)
SWITCH_SETS = [tuple(n for n, on in zip(_ffi.SWEEP_PLAN_SWITCHES, bits) if on) + facts
               for bits in itertools.product((False, True), repeat=3) for facts in ((), _ffi.SWEEP_PLAN_SWITCHES[3:])]


def _worlds(K):
    """(world, K_local, transport): one GPU; one GPU with a communicator (a one-rank rehearsal); two and four ranks"""
    out = [(1, K, False), (1, K, True)]
    out += [(w, K // w, True) for w in (2, 4) if K % w == 0]
    return out


@pytest.mark.parametrize("N,K,S", SHAPES)
def test_full_grid_against_the_rules(N, K, S):
    n = refused = 0
    for flags, sw, (world, Kl, transport), G in itertools.product(FLAGS, SWITCH_SETS, _worlds(K), (1, 2, 4)):
        kw = dict(K_local=Kl, G=G, M=1, world=world, transport=transport, flags=flags, switches=sw)
        if _refused(N, K, S, G, 1, world, transport, flags):
            with pytest.raises(_ffi.PhyloError) as e:
                _ffi.debug_sweep_plan(N, K, S, **kw)
            assert e.value.code == EINVAL, kw
            refused += 1
            continue
        got = _plan(N, K, S, **kw)
        want = _rules(N, K, Kl, S, G, 1, world, transport, flags, sw)
        assert got == want, (N, K, S, kw, {k: (got[k], want[k]) for k in want if got[k] != want[k]})
        n += 1
    assert n + refused == 16 * 16 * len(_worlds(K)) * 3 and n > 0


def test_each_threshold_flips_its_boolean():
    """the grid compares with the restatement; this states the sides outright"""
    for (lo, hi), (wlo, whi) in (((16, 17), (16, 32)), ((32, 33), (32, 64)), ((64, 65), (64, 64))):
        assert _plan(lo, 64, 64)["book_width"] == wlo and _plan(hi, 64, 64)["book_width"] == whi
    for N in (65, 66, 130, 252, 253, 257, 512):            # a wave per particle up to PK_MAX_TAXA; 0 is the twisted proposal's alone
        assert _plan(N, 16, 64)["book_width"] == 64 and _plan(N, 16, 64, flags=TWISTING)["book_width"] == 0
    assert _plan(64, 64, 64)["book_mat"] and not _plan(65, 64, 64)["book_mat"] and _plan(65, 64, 64)["mat_after_book"]
    # S = 4096 / 4097: the combined launch, a lazy kept graph, the owners' search by the draws
    assert _plan(5, 64, 4096)["book_mat"] and not _plan(5, 64, 4097)["book_mat"] and _plan(5, 64, 4097)["lazy"]
    assert _plan(5, 64, 4096, flags=KEEP_GRAPH)["lazy"] and not _plan(5, 64, 4097, flags=KEEP_GRAPH)["lazy"]
    two = dict(world=2, transport=True)
    assert _plan(5, 64, 4096, K_local=32, **two)["mat_by_draws"] and not _plan(5, 64, 4097, K_local=32, **two)["mat_by_draws"]
    # (the owners' nodes by the draws, else marks + adopted nodes; then bookkeeping, merge, tile epilogue, scan)
    assert _plan(5, 64, 4097, K_local=32, **two)["step_a_work"] and _plan(5, 64, 4097, K_local=32, **two)["launches"][2] == 6
    assert _plan(5, 64, 4096, K_local=32, **two)["launches"][2] == 5
    # K_local = 8192 / 8193
    assert _plan(17, 8192, 64)["book_mat"] and not _plan(17, 8193, 64)["book_mat"]
    assert not _plan(17, 8192, 64)["mat_grouped"] and _plan(17, 8193, 64)["mat_grouped"] and not _plan(17, 8193, 4097)["mat_grouped"]
    # K / G = 4096 / 4097 (K_local small): by the draws only while small, or in whole groups of PK_MAT_GROUP
    small = _plan(5, 4096, 64, K_local=2048, **two)
    assert small["mat_by_draws"] and not small["mat_draws_grouped"] and small["launches"][2] == 4
    assert not _plan(5, 4098, 64, K_local=2049, **two)["mat_by_draws"] and _plan(5, 4098, 64, K_local=2049, **two)["launches"][2] == 5
    big = _plan(5, 4224, 64, K_local=2112, **two)                                 # 2112 = 33 * 64: beyond 4096, whole groups
    assert big["mat_by_draws"] and big["mat_draws_grouped"]
    assert not _plan(5, 4160, 64, K_local=2080, **two)["mat_by_draws"]            # (K / G is a multiple of 64, K_local is not)
    assert not _plan(5, 16388, 64, K_local=8194, **two)["mat_by_draws"] and _plan(5, 16512, 64, K_local=8256, **two)["mat_by_draws"]
    # tables advanced = 8191 / 8192 at N <= 16: all K of them, or this rank's with owner-held tables
    assert _plan(5, 8191, 64)["book_width"] == 16 and _plan(5, 8192, 64)["book_width"] == 8
    assert _plan(5, 16382, 64, K_local=8191, **two)["book_width"] == 16 and _plan(5, 16384, 64, K_local=8192, **two)["book_width"] == 8
    assert _plan(5, 8192, 64, K_local=4096, switches=("replicated_book",), **two)["book_width"] == 8
    assert _plan(17, 8192, 64)["book_width"] == 32
    # 2 R K_local = 262143 / 262144, with and without JC69
    assert not _plan(2, 131071, 8)["sorted_prologue"] and _plan(2, 131072, 8)["sorted_prologue"]
    assert not _plan(2, 131072, 8, switches=("jc",))["sorted_prologue"]
    assert not _plan(2, 262142, 8, K_local=131071, **two)["sorted_prologue"] and _plan(2, 262144, 8, K_local=131072, **two)["sorted_prologue"]
    # K / G = 16384 / 16385: the last scan sums the log-normalisers, else pk_logz_total is one more launch
    assert _plan(5, 16384, 64)["fold_logz"] and _plan(5, 16384, 64)["launches"][-1] == 0
    assert not _plan(5, 16385, 64)["fold_logz"] and _plan(5, 16385, 64)["launches"][-1] == 1
    assert _plan(5, 32768, 64, G=2)["fold_logz"] and not _plan(5, 32772, 64, G=2)["fold_logz"]
    # S = 2048 / 2049: one site tile / the tile epilogue
    assert _plan(5, 16, 2048)["launches"][2] == 3 and _plan(5, 16, 2049)["launches"][2] == 4
    # N = 65 / 66: an eager kept graph whose reverse pass writes the marks itself
    assert not _plan(65, 16, 64, flags=KEEP_GRAPH | EAGER_NODES)["last_graph_eager"]
    assert _plan(66, 16, 64, flags=KEEP_GRAPH | EAGER_NODES)["last_graph_eager"]
    # R = 1
    assert _plan(2, 8, 16)["launches"] == [1, 3, 0]


PRIMATE = dict(
    twist=False, graph=False, timek=False, lazy=True, shard_form=False, replicated_book=False, local_book=False, book_mat=True,
    mat_by_draws=False, want_rdraw=True, use_rec=True, sorted_prologue=False, mat_grouped=False, mat_draws_grouped=False,
    step_a_work=False, mat_after_book=False, mat_barrier=False, fix_rootll=False, fold_logz=True, no_store_last=True,
    final_missing=False, last_graph_eager=False, one_tile=True, twist_ll=False, twist_tables=False, tile_epilogue=False, batched=False,
    book_width=16, launches=[1] + [3] * 11 + [0])


def test_primate_default_and_each_switch():
    p = _plan(12, 2048, 898)
    assert p == PRIMATE
    assert _plan(12, 2048, 898, flags=TIME_KERNELS) == dict(p, timek=True)
    eager = dict(p, lazy=False, book_mat=False, want_rdraw=False, use_rec=False, no_store_last=False)
    assert _plan(12, 2048, 898, flags=EAGER_NODES) == eager
    assert _plan(12, 2048, 898, switches=("eager_nodes",)) == eager
    assert _plan(12, 2048, 898, flags=KEEP_GRAPH) == dict(p, graph=True, no_store_last=False)
    assert _plan(12, 2048, 898, flags=KEEP_GRAPH | EAGER_NODES) == dict(eager, graph=True)
    twisted = dict(eager, twist=True, no_store_last=True, final_missing=True, book_width=0, launches=[1] + [5] * 11 + [0])
    assert _plan(12, 2048, 898, flags=TWISTING) == twisted
    assert _plan(12, 2048, 898, flags=TWISTING, switches=("coded_leaves",)) == dict(twisted, twist_ll=True, launches=[1] + [6] * 11 + [0])
    batched = dict(p, batched=True, book_mat=False, want_rdraw=False, mat_after_book=True, launches=[1, 3] + [4] * 10 + [0])
    assert _plan(12, 2048, 898, G=4) == batched
    # the three switches mean nothing on one GPU without a communicator; nor do the context's facts to a plain sweep
    for sw in ("rehearse_sharded", "coded_leaves", "device_exchange", "jc"):
        assert _plan(12, 2048, 898, switches=(sw,)) == p
    assert _plan(12, 2048, 898, switches=("replicated_book",)) == dict(p, replicated_book=True)
    # a communicator of one rank: the unsharded form plus the exchange's tail; rehearsed, the sharded form
    comm = dict(p, book_mat=False, want_rdraw=False, mat_after_book=True, mat_barrier=True, fix_rootll=True,
                launches=[1, 4] + [5] * 10 + [0])
    assert _plan(12, 2048, 898, transport=True) == comm
    rehearsed = dict(comm, shard_form=True, local_book=True, mat_by_draws=True, want_rdraw=True, step_a_work=True, mat_after_book=False,
                     fix_rootll=False, launches=[1, 3] + [4] * 10 + [0])
    assert _plan(12, 2048, 898, transport=True, switches=("rehearse_sharded",)) == rehearsed
    assert _plan(12, 2048, 898, transport=True, switches=("rehearse_sharded", "replicated_book")) == dict(
        comm, shard_form=True, replicated_book=True)
    # two ranks
    assert _plan(12, 2048, 898, K_local=1024, world=2, transport=True) == dict(rehearsed, use_rec=False)
    kept = dict(comm, shard_form=True, replicated_book=True, graph=True, use_rec=False, no_store_last=False)
    assert _plan(12, 2048, 898, K_local=1024, world=2, transport=True, flags=KEEP_GRAPH) == dict(kept, launches=kept["launches"][:-1] + [2])
    assert _plan(12, 2048, 898, K_local=1024, world=2, transport=True, flags=KEEP_GRAPH,
                 switches=("device_exchange",))["launches"][-1] == 4


def test_use_rec_does_not_depend_on_the_rank_event():
    """the driver used to decide it per rank event, from the last one's no_store too: with the plain proposal a merge that stores
    nothing at the last rank event only is no form (_rules asserts it over the grid; here outright)"""
    for flags in FLAGS:
        p = _plan(12, 2048, 898, flags=flags)
        assert p["use_rec"] == (p["lazy"] and not p["twist"])
        assert not (p["no_store_last"] and not p["lazy"] and not p["twist"])


def test_refusals_are_those_of_sweep_begin():
    for kw, what in ((dict(G=0), "a batch needs"), (dict(G=65), "a batch needs"), (dict(G=3), "divisible by G"),
                     (dict(G=2, flags=TWISTING), "plain proposal"),
                     (dict(G=2, flags=KEEP_GRAPH, transport=True), "unsharded context"),
                     (dict(G=2, flags=KEEP_GRAPH, S=4097), "S <= 4096"),
                     (dict(flags=TWISTING, M=0), "1 <= M <= 1024"), (dict(flags=TWISTING, M=1025), "1 <= M <= 1024"),
                     (dict(flags=TWISTING, N=512, M=9), "exceeds"),
                     (dict(flags=TWISTING | KEEP_GRAPH, world=2, K_local=1024, transport=True), "unsharded context"),
                     (dict(flags=KEEP_GRAPH, world=2, K_local=1024, transport=True, S=4097), "sharded context needs S <= 4096")):
        args = dict(N=12, K=2048, S=898)
        args.update(kw)
        with pytest.raises(_ffi.PhyloError, match=what) as e:
            _ffi.debug_sweep_plan(**args)
        assert e.value.code == EINVAL
    assert _plan(12, 2048, 4096, G=2, flags=KEEP_GRAPH)["graph"] and _plan(12, 2048, 898, flags=TWISTING, M=1024)["twist"]


def test_bad_arguments_are_refused():
    for kw in (dict(N=1), dict(N=513), dict(K=0), dict(K_local=0), dict(K_local=65), dict(S=0), dict(world=0)):
        args = dict(N=12, K=64, S=256)
        args.update(kw)
        with pytest.raises(_ffi.PhyloError):
            _ffi.debug_sweep_plan(**args)


def _scan_form(Kg, multi_min, wanted):
    """launch_scan as it was spelled before sweep_scan_form_of: the scan of several workgroups per group above the switch when
    anything is wanted; else one workgroup per group: the cdf in LDS by 512 threads up to 4096 weights, by 1024 threads up to
    PP_SCAN_KERNEL_MAX_KG, beyond that staged in the cdf buffer itself"""
    if Kg > multi_min and wanted:
        return "multi"
    if Kg <= 4096:
        return "lds512"
    return "lds1024" if Kg <= SCAN_KERNEL_MAX_KG else "in_place"


def test_scan_form_and_its_three_thresholds():
    sizes = (1, 2, 63, 64, 65, 100, 2048, 2049, 4095, 4096, 4097, 5000, 8192, 16383, 16384, 16385, 20003, 100001, 1 << 30, (1 << 31) - 1)
    for multi_min, Kg, wanted in itertools.product((0, 64, 4096, 5000, 16384, 20000, 1 << 30), sizes, (True, False)):
        assert _ffi.debug_scan_form(Kg, multi_min, wanted) == _scan_form(Kg, multi_min, wanted), (Kg, multi_min, wanted)
    # the default switch: nothing above 4096 weights is scanned by one workgroup
    assert [_ffi.debug_scan_form(Kg) for Kg in (4096, 4097, 16384, 16385)] == ["lds512", "multi", "multi", "multi"]
    # the switch out of reach: 4096 and PP_SCAN_KERNEL_MAX_KG are the last sizes of the two LDS forms
    assert [_ffi.debug_scan_form(Kg, 1 << 30) for Kg in (4096, 4097, 16384, 16385)] == ["lds512", "lds1024", "lds1024", "in_place"]
    # the switch itself: the first size beyond it
    assert [_ffi.debug_scan_form(Kg, 64) for Kg in (64, 65)] == ["lds512", "multi"]
    assert [_ffi.debug_scan_form(Kg, 5000) for Kg in (5000, 5001)] == ["lds1024", "multi"]
    assert [_ffi.debug_scan_form(Kg, 20000) for Kg in (20000, 20001)] == ["in_place", "multi"]
    # nothing wanted (no cdf, no log-normaliser): never the three launches
    assert _ffi.debug_scan_form(9000, wanted=False) == "lds1024" and _ffi.debug_scan_form(20000, wanted=False) == "in_place"
    assert _ffi.SCAN_FORMS == ("multi", "lds512", "lds1024", "in_place")
    with pytest.raises(_ffi.PhyloError) as e:
        _ffi.debug_scan_form(0)
    assert e.value.code == EINVAL


def test_fold_logz_is_a_size_rule_not_a_scan_form():
    """the last scan sums the log-normalisers in both LDS kernels and in the scan of several workgroups; pk_resample_scan(_groups)
    cannot, and is only reached beyond PP_SCAN_KERNEL_MAX_KG whatever the switch: fold_logz never names a form that cannot fold"""
    for multi_min, Kg in itertools.product((64, 4096, 1 << 30), (4096, 4097, 16384, 16385, 33282)):
        folds = _plan(5, Kg, 8)["fold_logz"]
        assert folds == (Kg <= SCAN_KERNEL_MAX_KG)
        if _ffi.debug_scan_form(Kg, multi_min) == "in_place":
            assert not folds
