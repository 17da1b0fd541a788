// phylo_sweep_plan.h -- the form of a forward sweep of the launch path (phylo_hip.hip: sweep_begin_impl, the stages of a rank event,
// phylo_sweep_finish).  Plain C++, no HIP, like phylo_revlists.h: the same functions run in the driver and behind
// phylo_debug_sweep_plan (tests/test_sweepplan_cpu.py restates the rules).
//
// Every form computes the same bits (the parity tests assert that), so a rule that silently picks another form passes every one
// of them and only shows as a slower sweep.  Which form is issued is therefore decided HERE and nowhere else, once per sweep:
// sweep_begin_impl computes the plan and stores it in the run, the stages only read it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

// Constants that live in the kernel headers, and the thresholds of the rules below (the driver fills them by name: sweep_limits_of).
struct sweep_limits {
    int max_groups;                    // PK_MAX_GROUPS
    int twist_max_m, twist_max_j;      // PK_TWIST_MAX_M, PK_TWIST_MAX_J
    int mat_group;                     // PK_MAT_GROUP: particles per workgroup of the grouped adopted-node launches
    int scan_fold_max_kg;              // PP_SCAN_KERNEL_MAX_KG: the scan kernels that can also sum the log-normalisers
    int scan_lds512_max_kg;            // 4096: groups that pp_resample_scan<512> takes (32 KiB of cdf in LDS)
    int kept_bits_taxa;                // PG_KEPT_BITS_TAXA
    int one_tile_max_s;                // 4096: sites of a node that one workgroup writes / of the rows form of the reverse pass
    int small_max_kg, small_max_kloc;  // 4096, 8192: launches of at most this many particles count as small (latency chains)
    int book_packed8_min;              // 8192: root tables advanced in one launch from which 8 lanes per particle pay
    int sorted_min_draws;              // 262144: branch-length draws (2 R Kloc) from which the prologue sorts its matrices
};

struct sweep_facts {
    // the shape
    int N, K, Kloc, S, G, M, world;    // (K: all ranks' particles; Kloc: this rank's; G: sweeps batched in the context)
    int ntiles;                        // site tiles of a row (the context's site tile decides: 1 unless S exceeds it)
    bool transport;                    // a communicator is set (phylo_comm_init), whatever the number of ranks
    bool device_exchange;              // ... and its collectives are the device-side exchange (pk_p2p_exchange)
    bool jc;                           // the model is JC69 (closed-form matrices)
    bool coded_leaves;                 // every leaf row is one-hot or all-ones (the twisted proposal's pair histogram)
    // the flag bits
    bool twisting, keep_graph, eager_nodes, time_kernels;
    // the environment switches the launch path reads
    bool env_eager_nodes, env_rehearse_sharded, env_replicated_book;
    // the clade tables of the current leaves are built and the merge's pattern form is taken (phylo_site_patterns.h: pk_clade_take,
    // pk_pat_take -- the rule and PHYLO_CLADE_PATTERNS were applied when the leaves were set)
    bool clade_tables;
    // PHYLO_LAUNCH_XCD as the context read it (A/B runs and tests): 0 = unset, -1 = off, 1 = on; for runs that price the two launches
    // apart, 2 = the merge alone, 3 = the bookkeeping alone
    int env_launch_xcd;
};

struct sweep_plan {
    int R, G, Kg;                      // rank events; batched sweeps and the particles of one
    bool twist, graph, timek;
    bool one_tile;                     // S <= 4096: a node is written by one workgroup
    bool lazy;                         // nodes are written only when adopted (marks say which)
    bool shard_form;                   // the sweep is issued as a sharded one (more than one rank, or a one-rank rehearsal)
    bool replicated_book;              // sharded: every rank advances all K root tables
    bool local_book;                   // sharded, plain proposal: every rank advances its own particles' tables only
    bool book_mat;                     // bookkeeping and the writes of the adopted nodes share one launch (pk_rank_book_mat), r > 0
    bool mat_by_draws;                 // sharded: owners find their adopted nodes from the draws (no pk_all_marks)
    bool want_rdraw;                   // the prologue leaves the resampling draws in d_rdraw
    bool use_rec;                      // the bookkeeping leaves a merge record per particle and the merge starts from it
    bool sorted_prologue;              // pk_sweep_prologue_sorted
    bool mat_grouped;                  // pk_materialize_adopted_grouped instead of pk_materialize_adopted
    bool mat_draws_grouped;            // pk_materialize_by_draws: one workgroup per mat_group particles
    int book_width;                    // lanes per particle of the bookkeeping: 8, 16, 32 or 64; 0 = no bookkeeping launch (twisted).
                                       // (pk_rank_book_mat has no 8: 16)
    bool step_a_work;                  // sweep_step_a issues the adopted-node launches and their barrier for r > 0
    bool mat_after_book;               // ... else the step does, behind its bookkeeping, for r > 0 (not at all: eager, or book_mat)
    bool mat_barrier;                  // that launch is followed by a barrier across the ranks
    bool twist_ll;                     // twisted: coded leaf-leaf pairs go through pk_twist_potentials_ll
    bool twist_tables;                 // twisted: pk_twist_tables advances the tables (a communicator is set)
    bool tile_epilogue;                // rows longer than one site tile: pk_tile_epilogue behind the merge
    bool fix_rootll;                   // sharded without local bookkeeping: pk_fix_rootll behind the exchange
    bool fold_logz;                    // the last scan also sums the log-normalisers (no pk_logz_total launch)
    int lse_stride;                    // the scan's stride between the groups' log-normalisers (0: one sweep)
    bool no_store_last;                // the merge of the last rank event stores no node
    bool final_missing;                // ... and nothing else wrote it: phylo_sweep_node has to
    bool last_graph_eager;             // a kept graph whose reverse pass can write the marks itself (rev_marks)
    int gather_launches;               // kernels of graph_gather behind the last rank event (sharded kept graph)
    bool clade_pat;                    // clade patterns: the root tables carry leaf bitsets, the record's flag word the new clade's,
                                       // and the merge's phase 1 runs over the clade's block
    bool launch_xcd;                   // an XCD owns a contiguous range of particles in the record-form merge ...
    bool book_xcd;                     // ... and in the particle part of the chain form's bookkeeping
};

// PHYLO_EAGER_NODES, as a flag or from the environment: every node is stored by its merge (also read by persist_plan)
inline bool sweep_eager_nodes(bool flag, bool env) { return flag || env; }

// Lanes per particle of the bookkeeping launch that advances `nbook` root tables of N slots.
// Large launches (batched sweeps) are bound by instruction issue: 8 lanes per particle serve 8 particles with one instruction
// stream (3.52e11 -> 3.68e11 units/s for a launch set of 20 sweeps; 4 lanes: no further gain); small launches are latency chains
// and keep the shorter 16-lane form (4 particles per wave: PK_AUX + 2 = 10 <= 16 lanes).  Above 32 taxa: 64, a wave per particle.
inline int sweep_book_width(int N, int nbook, const sweep_limits& L) {
    if (N <= 16) return nbook >= L.book_packed8_min ? 8 : 16;
    return N <= 32 ? 32 : 64;
}

// The argument refusals of a sweep, in the order phylo_sweep_begin checks them: true, and the message, when the facts are refused
// (PHYLO_EINVAL).  First what a batch needs; then, behind the check that leaves and model are set (PHYLO_ESTATE), what the twisted
// proposal and a kept graph need.
inline bool sweep_refuses_batch(const sweep_facts& f, const sweep_limits& L, char* msg, size_t n) {
    const bool sharded = f.world != 1;
    if (f.G < 1 || f.G > L.max_groups || f.K % f.G != 0)
        return snprintf(msg, n, "a batch needs 1 <= G <= %d sweeps and K = %d divisible by G (got %d)", L.max_groups, f.K, f.G), true;
    if (f.G > 1 && f.twisting) return snprintf(msg, n, "batched sweeps need the plain proposal (PHYLO_TWISTING is set)"), true;
    if (f.G > 1 && f.keep_graph) {     // the graph of G systems: one block-diagonal genealogy, rows form, one GPU
        if (sharded || f.transport) return snprintf(msg, n, "batched sweeps with PHYLO_KEEP_GRAPH need an unsharded context"), true;
        if (f.S > L.one_tile_max_s)
            return snprintf(msg, n, "batched sweeps with PHYLO_KEEP_GRAPH need S <= 4096 sites (got %d)", f.S), true;
    }
    return false;
}
inline bool sweep_refuses_form(const sweep_facts& f, const sweep_limits& L, char* msg, size_t n) {
    const bool sharded = f.world != 1;
    if (f.twisting) {
        if (f.M < 1 || f.M > L.twist_max_m)
            return snprintf(msg, n, "twisting needs 1 <= M <= %d (got %d)", L.twist_max_m, f.M), true;
        const size_t Jmax = (size_t)(f.N * (f.N - 1) / 2) * (size_t)f.M;
        if (Jmax > (size_t)L.twist_max_j) return snprintf(msg, n, "twisting: C(N,2)*M = %zu exceeds %d", Jmax, L.twist_max_j), true;
    }
    if (f.keep_graph && sharded) {     // sharded: the plain proposal on nodes of one site tile (graph_gather)
        if (f.twisting) return snprintf(msg, n, "PHYLO_KEEP_GRAPH with PHYLO_TWISTING needs an unsharded context"), true;
        if (f.S > L.one_tile_max_s)
            return snprintf(msg, n, "PHYLO_KEEP_GRAPH on a sharded context needs S <= 4096 sites (got %d)", f.S), true;
    }
    return false;
}

inline sweep_plan sweep_plan_form(const sweep_facts& f, const sweep_limits& L) {
    sweep_plan p{};
    const int N = f.N, K = f.K, Kl = f.Kloc, S = f.S;
    p.R = N - 1; p.G = f.G; p.Kg = K / f.G;
    p.twist = f.twisting; p.graph = f.keep_graph; p.timek = f.time_kernels;
    const bool eager = sweep_eager_nodes(f.eager_nodes, f.env_eager_nodes);
    const bool one_tile = p.one_tile = S <= L.one_tile_max_s;
    // lazy nodes: dead stores are most of the HBM traffic of the plain sweep (a node is read again only if its creator survives
    // the next resampling).  Needs the plain proposal.  Marks are plain stores and the extra launch costs less than the dead
    // stores it removes at every size measured.
    // A kept graph stays lazy too when its reverse pass reads no node but the adopted ones (rows form, S <= 4096: pg_nodes_free
    // recomputes a node's row from its children; everything else that is read was somebody's child, i.e. adopted).
    // Sharded, the owner's write needs one more (tiny) collective per rank event (sweep_step_a); rehearsed with a one-rank RCCL
    // world (PHYLO_REHEARSE_SHARDED=1) the lazy sweep is 0.145 ms against 0.185 ms for the eager one at primate.p's node size, more
    // than a second collective costs.
    p.lazy = !p.twist && (!p.graph || one_tile) && !eager;
    p.shard_form = f.world > 1 || (f.transport && f.env_rehearse_sharded);      // (the switch: a one-rank rehearsal)
    // a sharded sweep that keeps its graph advances all K root tables on every rank: the history planes it writes are then whole
    // everywhere (the owner-held tables that peers read are the two planes of d_tables, not the history)
    p.replicated_book = f.env_replicated_book || (p.graph && f.world > 1);
    // sharded, plain proposal: every rank advances only ITS particles' root tables and reads an adopted ancestor's row from the
    // owner's slab over the peer mapping (ordered by the all-gather of the previous rank event, like the node pool) instead of
    // replicating the bookkeeping of all K particles.  (The twisted proposal advances its tables in kernels of its own.)
    p.local_book = !p.twist && p.shard_form && !p.replicated_book;
    // one sweep alone on one GPU with lazy nodes: the adopted nodes are written in the bookkeeping launch (pk_rank_book_mat), found
    // by the resampling draws, which pk_sweep_prologue then leaves in d_rdraw.  Batched sweeps keep the separate launch (measured:
    // 2.62e11 against 2.64e11 units/s with the grouped form of the combined launch in round 2; round 3, a launch set alone: 3.57e11
    // against 3.77e11).
    p.book_mat = p.lazy && f.world == 1 && !f.transport && N <= 64 && one_tile && f.G == 1 && Kl <= L.small_max_kloc;
    // sharded with lazy nodes: each owner finds ITS adopted nodes the same way (O(Kloc Kg / 64) comparisons) instead of every rank
    // searching the ancestors of all K particles (pk_all_marks, O(K) on every rank whatever the number of GPUs)
    const bool mat_small = p.Kg <= L.small_max_kg && Kl <= L.small_max_kloc;
    p.mat_by_draws = p.lazy && p.local_book && one_tile && (mat_small || (p.Kg % L.mat_group == 0 && Kl % L.mat_group == 0));
    p.mat_draws_grouped = !mat_small;                      // one workgroup per 64 particles when there are many
    p.want_rdraw = p.book_mat || p.mat_by_draws;
    // the node of the LAST rank event is never merged again: its log-likelihood is all the sweep needs
    p.no_store_last = !p.graph && !eager;
    p.final_missing = p.no_store_last && !p.lazy;
    // one rank, plain proposal, a merge that stores nothing: the bookkeeping also leaves a merge record per particle and the merge
    // starts from it (the storing merge and the sharded and twisted sweeps resolve ids: no record is written for them).
    // (The last rank event's stores-nothing adds no case: with the plain proposal, no_store_last implies lazy.)
    p.use_rec = !p.twist && Kl == K && p.lazy;
    // large launches (batched sweeps): the matrices sorted by Pade order inside workgroups of 1024 (pk_sweep_draws_sorted)
    p.sorted_prologue = !p.twist && !f.jc && 2L * p.R * Kl >= L.sorted_min_draws;
    // Adopted nodes in a launch of their own.  Few nodes are marked, almost every workgroup leaves at once: one workgroup per
    // particle for small nodes (a quarter of the empty workgroups), site tiles for large ones (a marked node is then not limited
    // to one CU's bandwidth).  Large launches of small nodes (batched sweeps): dispatching one workgroup per particle costs more
    // than the few writes, one workgroup takes mat_group particles.
    p.mat_grouped = one_tile && Kl > L.small_max_kloc;
    p.step_a_work = p.lazy && p.local_book;                // sharded with owner-held tables: ahead of the bookkeeping, in sweep_step_a
    p.mat_after_book = p.lazy && !p.local_book && !p.book_mat;
    p.mat_barrier = f.transport;                           // peers read these nodes in place: order them before every rank's merge
    p.book_width = p.twist ? 0 : sweep_book_width(N, p.local_book ? Kl : K, L);
    p.twist_ll = p.twist && f.coded_leaves;
    p.twist_tables = p.twist && f.transport;
    p.tile_epilogue = f.ntiles > 1;
    p.fix_rootll = f.transport && !p.local_book;
    p.fold_logz = p.Kg <= L.scan_fold_max_kg;
    p.lse_stride = f.G > 1 ? p.R + 1 : 0;
    // (what made the sweep eager with lazy's other conditions met: the flag or the switch alone; one GPU -- a sharded pass keeps
    //  its own form; above kept_bits_taxa only: up to there every form keeps the bits it had -- phylo_revlists.h)
    p.last_graph_eager = p.graph && !p.lazy && !p.twist && one_tile && f.world == 1 && Kl == K && N > L.kept_bits_taxa;
    // pack, unpack (+ the two barrier kernels of the device-side exchange)
    p.gather_launches = (p.graph && f.world > 1) ? (f.device_exchange ? 4 : 2) : 0;
    // clade patterns: the record-form merge of one site tile, root tables in the two planes (a kept graph writes history planes,
    // which carry no bitsets).  Sharded, twisted and eager sweeps write no record.
    p.clade_pat = f.clade_tables && p.use_rec && !p.graph && f.ntiles == 1;
    // How the record-form merge (one rank, plain proposal) and the chain bookkeeping are launched (phylo_launch_map.h; DESIGN.md
    // section 8 has the measurements).  Neither changes a bit of the result; the switches override for A/B runs and the tests.
    // Large launches only (batched sweeps): there the particles of a sweep share ancestors' rows and clade blocks in one L2 (merge
    // 37.9 -> 36.4 us per rank event of 20 sweeps of 2 048).  A single sweep of 2 048 particles is a latency chain of small launches:
    // its t_sweep read 1 % higher with the remap, so small launches keep the plain deal.
    const int x = f.env_launch_xcd;
    const bool large = (long)Kl * f.ntiles > L.small_max_kloc;
    p.launch_xcd = p.use_rec && (x == 0 ? large : x == 1 || x == 2);
    p.book_xcd = p.use_rec && (x == 0 ? large : x == 1 || x == 3);
    return p;
}

// The form of a resampling scan of groups of Kg log-weights (launch_scan; phylo_resample, phylo_log_zsmc and every rank event of a
// sweep): decided here, from the group size, PHYLO_SCAN_MULTI_MIN as the context read it (default 4096) and whether the caller
// wants anything written (a cdf or a log-normaliser).  All four compute the same bits (tests/test_gpu_scan_forms.py).
enum sweep_scan_form {
    SCAN_MULTI = 0,                    // pp_scan_multi_max / _exp / _cdf: several workgroups per group, a tile of 2048 weights each
    SCAN_LDS_512 = 1,                  // pp_resample_scan<512>: one workgroup per group, the cdf in LDS
    SCAN_LDS_1024 = 2,                 // pp_resample_scan<1024>: 16 waves, up to 128 KiB of LDS
    SCAN_IN_PLACE = 3                  // pk_resample_scan(_groups): one workgroup per group, staged in the cdf buffer itself
};
inline sweep_scan_form sweep_scan_form_of(int Kg, int multi_min, bool wanted, const sweep_limits& L) {
    if (Kg > multi_min && wanted) return SCAN_MULTI;
    if (Kg <= L.scan_lds512_max_kg) return SCAN_LDS_512;
    if (Kg <= L.scan_fold_max_kg) return SCAN_LDS_1024;
    return SCAN_IN_PLACE;
}

// ---- the chain form of a rank event -------------------------------------------------------------------------
// A rank event of a batched sweep is scan -> bookkeeping -> adopted nodes -> merge on one stream, and the three short launches are
// latency chains.  Which ancestor a particle adopts, hence which nodes must be written, is known to the scan's workgroup (the whole
// cdf is in its LDS): in the chain form the scan of rank event r also writes every particle's ancestor of rank event r + 1 and the
// ascending list of the adopted particles of each group (pp_scan_ancestors); the bookkeeping reads its ancestor instead of searching
// the cdf and stores no mark; and the adopted nodes are written from the list by item waves that LEAD the bookkeeping's grid, a wave
// per (list entry, part of the node's sites), which also store the marks (pk_rank_book_chain, pk_mat_listed): they no longer wait
// for the bookkeeping, they run beside it.  Same bits as the launches it replaces (tests/test_gpu_chain_forms.py).
// The rule is a decision of its own beside the plan: sweep_plan, its mask and its launch counts do not know it.
struct sweep_chain_form {
    bool taken;                        // false: the launches of the plan exactly (the other fields are 0)
    int item_waves;                    // W: waves per group that walk the group's list
    int parts;                         // the parts a node's sites are cut into, one per item
};
// `scan_ancestors`: PHYLO_SCAN_ANCESTORS as the context read it (0 = off; unset: 1).  `multi_min`: PHYLO_SCAN_MULTI_MIN likewise.
inline sweep_chain_form sweep_chain_form_of(const sweep_plan& p, int S, int multi_min, int scan_ancestors, const sweep_limits& L) {
    const sweep_chain_form no{};
    if (scan_ancestors == 0) return no;
    if (!(p.use_rec && p.mat_after_book)) return no;       // one rank, plain proposal, lazy nodes, the separate adopted-nodes launch
    if (p.mat_barrier) return no;                          // a communicator is set: peers read these nodes, the launch and its barrier stay
    if (p.R < 2) return no;                                // (no resampling at all)
    const sweep_scan_form s = sweep_scan_form_of(p.Kg, multi_min, true, L);
    if (s != SCAN_LDS_512 && s != SCAN_LDS_1024) return no;
    sweep_chain_form f{};
    f.taken = true;
    // two rows per lane in flight (more would raise the registers of the bookkeeping that shares the kernel): a node is cut so that
    // a part is ONE round trip of its wave where it can be, into at most eight; short rows need no cut
    f.parts = (S + 127) / 128 < 8 ? (S + 127) / 128 : 8;
    // few particles are adopted on real data (about 40 of 2048 at primate.p): 128 waves meet at most three items each there, and the
    // waves without an item leave after one scalar load.  Many adopted nodes (flat weights): the waves stride over the list.
    f.item_waves = p.Kg * f.parts < 128 ? p.Kg * f.parts : 128;
    return f;
}

// What the driver counts into stats.n_launches: r = -1 the begin, 0 .. R-1 rank event r (sweep_step_a's half included), R the
// finish.  This is the driver's count as it always was, which is not everywhere the number of kernels: a scan of several
// workgroups per group counts 1 for its three launches, a twisted rank event counts 3 for adopt + draws, potentials and choose
// even when pk_twist_potentials has no rows and is not launched, and pk_pair_hist and the kernels of the collectives are not
// counted.  Where the chain form puts two stages into one launch (bookkeeping and adopted nodes), the count stays that of the
// stages.  tests/test_gpu_sweep_forms.py pins the totals.
inline int sweep_plan_launches(const sweep_plan& p, int r) {
    if (r < 0) return 1;                                   // pk_sweep_prologue, or pk_init_tables of the twisted proposal
    if (r >= p.R) return (p.fold_logz ? 0 : 1) + p.gather_launches;
    int n = 0;
    if (p.step_a_work && r > 0) n += p.mat_by_draws ? 1 : 2;                     // by the draws, or pk_all_marks + the adopted nodes
    n += p.twist ? 3 + (p.twist_ll ? 1 : 0) + (p.twist_tables ? 1 : 0) : 1;      // the proposal, or the bookkeeping
    if (p.mat_after_book && r > 0) n += 1;
    n += 1 + (p.tile_epilogue ? 1 : 0);                    // the merge
    n += (p.fix_rootll ? 1 : 0) + 1;                       // behind the exchange: the scan
    return n;
}

// ---- the one-launch sweep (phylo_persist.h: pp_sweep<NT>) --------------------------------------------------
// Whether a sweep is issued as ONE launch of resident workgroups, and on which grid: G groups x Wg workgroups of nt threads,
// m = Kg / Wg particles each.  Every grid computes the launch path's bits, so a rule that silently picks another grid (or the launch
// path) passes every comparison: the rule is stated here once, persist_plan (phylo_hip.hip) feeds it the facts it queried, and
// phylo_debug_persist_plan the facts a test names (tests/test_one_launch_plan_cpu.py restates it).
struct persist_limits {
    int max_taxa;                      // 32: one wave per particle, a lane per root slot, history rows in lanes
    int max_kg;                        // PP_MAX_KG: the group's cdf lives in LDS
    int max_m;                         // PP_MAX_M: adoption flags and own ancestors live in LDS
    int max_s;                         // 8192: larger nodes (256 KiB) are spread over several workgroups by the launch path
    size_t max_lds;                    // 150 KiB of the CU's 160
    size_t (*lds_bytes)(int N, int m, int Kg);   // pp_layout(N, m, Kg).total
};

struct persist_facts {
    int N, K, S, G, world;
    bool transport;                    // a communicator is set
    bool one_launch;                   // PHYLO_ONE_LAUNCH, as a flag or from the environment: the form is opt-in
    bool twisting, keep_graph, time_kernels, eager_nodes, env_eager_nodes;
    int n_cus;                         // compute units of the device
    int blocks_per_cu;                 // workgroups of pp_sweep<nt> the planner may place on a CU: 0 (not admitted), 1 or 2
    int persist_wgs;                   // PHYLO_PERSIST_WGS: resident workgroups of the whole launch (<= 0: one per CU)
    int persist_nt;                    // PHYLO_PERSIST_NT as persist_nt_of read it: 256 or 512
};

struct persist_grid {
    bool taken;                        // false: the launch path runs (the other fields are 0)
    int Wg, m, nt;
    size_t lds;                        // dynamic LDS bytes of a workgroup
};

// PHYLO_PERSIST_NT: 512 selects pp_sweep<512>, everything else (unset included: 0) the 256-thread form
inline int persist_nt_of(int requested) { return requested == 512 ? 512 : 256; }

// The refusals that need no fact of the device (persist_plan asks the runtime for the occupancy only behind them).
inline bool persist_refuses_shape(const persist_facts& f, const persist_limits& L) {
    if (!f.one_launch) return true;                                                  // opt-in
    if (f.world != 1 || f.transport) return true;                                    // sharded: collectives between launches
    if (f.twisting || f.keep_graph || f.time_kernels) return true;                   // launch path only
    if (sweep_eager_nodes(f.eager_nodes, f.env_eager_nodes)) return true;            // ... and its A/B switch
    if (f.N > L.max_taxa || f.N < 2) return true;
    if (f.K / f.G > L.max_kg) return true;
    if (f.S > L.max_s) return true;
    return false;
}

inline persist_grid persist_plan_of(const persist_facts& f, const persist_limits& L) {
    const persist_grid no{};
    if (persist_refuses_shape(f, L)) return no;
    if (f.blocks_per_cu < 1 || f.n_cus < 1) return no;
    const int Kg = f.K / f.G;
    int Wt = f.persist_wgs > 0 ? f.persist_wgs : f.n_cus;                            // default: one workgroup per CU
    if (Wt > f.n_cus * f.blocks_per_cu) Wt = f.n_cus * f.blocks_per_cu;              // residency: never more than the device admits
    if (Wt < f.G) return no;
    int Wg = Wt / f.G;
    if (Wg > Kg) Wg = Kg;
    while (Wg > 1 && Kg % Wg) --Wg;                                                  // every workgroup owns the same number of particles
    const int m = Kg / Wg;
    if (m > L.max_m) return no;
    // (no admissible shape reaches this refusal: with N <= 32, m <= 1024 and Kg <= 8192 the layout takes at most 94 240 bytes.
    //  It stays as the guard of the launch's LDS request should a limit above move; tests/test_one_launch_plan_cpu.py pins the maximum.)
    const size_t lds = L.lds_bytes(f.N, m, Kg);
    if (lds > L.max_lds) return no;
    return persist_grid{true, Wg, m, f.persist_nt, lds};
}

// The plan as phylo_debug_sweep_plan returns it: the booleans in this order from bit 0 (SWEEP_PLAN_BITS of phylo_amd/_ffi.py names
// them; `batched` is lse_stride != 0), book_width / 8 in bits 28..31.  gather_launches is the finish's count beyond pk_logz_total.
inline uint32_t sweep_plan_mask(const sweep_plan& p) {
    const bool b[] = {p.twist, p.graph, p.timek, p.lazy, p.shard_form, p.replicated_book, p.local_book, p.book_mat, p.mat_by_draws,
                      p.want_rdraw, p.use_rec, p.sorted_prologue, p.mat_grouped, p.mat_draws_grouped, p.step_a_work, p.mat_after_book,
                      p.mat_barrier, p.fix_rootll, p.fold_logz, p.no_store_last, p.final_missing, p.last_graph_eager,
                      p.one_tile, p.twist_ll, p.twist_tables, p.tile_epilogue, p.lse_stride != 0, p.clade_pat};
    static_assert(sizeof b / sizeof b[0] <= 28, "bits 28..31 hold book_width / 8");
    uint32_t m = (uint32_t)(p.book_width / 8) << 28;
    for (size_t i = 0; i < sizeof b / sizeof b[0]; ++i) m |= b[i] ? 1u << i : 0u;
    return m;
}
