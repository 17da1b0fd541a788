// phylo_hip.hip -- C ABI (include/phylo_hip.h) over the gfx950 kernels in phylo_kernels.h.
// One context = one GPU, one stream.  No CPU fallback: without a HIP device every entry point fails.
#include "../../include/phylo_hip.h"

#include <cstring>                     // (ahead of the HIP headers: rocPRIM's use memcpy unqualified)
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <rocprim/device/device_radix_sort.hpp>   // the two sorts of phylo_revlists_dev.h

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <mutex>
#include <string>
#include <vector>

#include "phylo_comm.h"
#include "phylo_kernels.h"
#include "phylo_packed_codes.h"
#include "phylo_site_patterns.h"
#include "phylo_persist.h"
#include "phylo_grad.h"
#include "phylo_revlists_dev.h"
#include "phylo_sweep_plan.h"
#include "phylo_train.h"
#include "phylo_trees.h"
#include "phylo_trees_plan.h"
#include "phylo_treeset.h"
#include "phylo_rell.h"
#include "phylo_rell_ms.h"
#include "phylo_treegrad.h"
#include "phylo_treegrad_rates.h"
#include "phylo_treenni.h"
#include "phylo_treenni_rates.h"
#include "phylo_treegrad_model.h"
#include "phylo_treeanc.h"
#include "phylo_treeanc_rates.h"

#include <algorithm>
#include <type_traits>

namespace {

thread_local std::string g_last_error;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

}  // namespace

struct sweep_run {                       // a sweep being issued rank event by rank event
    uint64_t seed = 0;
    uint32_t flags = 0;
    int M = 1, launches = 0, next_r = 0;
    bool active = false;
    int a_done_r = -1;                     // rank event whose first half (sweep_step_a) has been issued
    sweep_plan plan{};                     // the form, decided by sweep_begin_impl (phylo_sweep_plan.h)
    sweep_chain_form chain{};              // ... and the chain form of its rank events (sweep_chain_form_of), beside the plan
};

// Switches of DESIGN.md section 6b, read from the environment ONCE (phylo_create): none changes a result bit.  Each one serves a
// tool or a test (section 6b says which); a switch whose only use was to bring back a form that measured slower is not kept.
struct env_switches {
    bool eager_nodes = false, rehearse_sharded = false, replicated_book = false, no_leaf_codes = false, one_launch = false,
         persist_stamps = false, grad_one_stream = false, grad_two_streams = false, rev_host_lists = false, no_remote_cache = false,
         no_p2p = false, grad_rows_chain = false, grad_coeff_chain = false, tree_wide_keys = false;
    int persist_wgs = 0;                 // PHYLO_PERSIST_WGS: resident workgroups of the one-launch sweep (0 = default)
    unsigned long long p2p_wait_ticks = PK_P2P_WAIT_TICKS;   // PHYLO_P2P_WAIT_S: bound of a flag wait of the device-side exchange
    size_t p2p_copy_words = 65536;       // PHYLO_P2P_COPY_WORDS: exchanges beyond this many doubles copy with many workgroups (tests lower it)
    int persist_nt = 256;                // PHYLO_PERSIST_NT: threads per workgroup of the one-launch sweep (256 or 512)
    int remote_cache_cap = 0;            // PHYLO_REMOTE_CACHE_CAP: slots of the local cache of remote nodes (0 = 512 MB worth; tests lower it)
    int scan_multi_min = 4096;           // PHYLO_SCAN_MULTI_MIN: groups of more weights than this are scanned by several workgroups
    int scan_ancestors = 1;              // PHYLO_SCAN_ANCESTORS: 0 = no chain form of a rank event (sweep_chain_form_of)
    int site_patterns = PK_PAT_AUTO;     // PHYLO_SITE_PATTERNS: 0 = never the pattern form of the merge, force = wherever it is valid
    int clade_patterns = PK_CLADE_AUTO;  // PHYLO_CLADE_PATTERNS: 0 = never the clade tables of the pattern form, force = wherever they are eligible
    int trees_chunk = 0;                 // PHYLO_TREES_CHUNK: trees per chunk of phylo_trees_loglik (0 = what PT2_SCRATCH_BYTES holds; tests lower it)
    int launch_xcd = 0;                  // PHYLO_LAUNCH_XCD: 1 / 0 = an XCD owns a contiguous range of particles, or not (unset: the plan's rule)
    int rell_chunk = 0;                  // PHYLO_RELL_CHUNK: replicates per chunk of phylo_rell, columns per chunk of phylo_rell_multiscale (0 = what PR_CHUNK_BYTES holds; tests lower it)
    void read() {
        eager_nodes = getenv("PHYLO_EAGER_NODES") != nullptr;
        rehearse_sharded = getenv("PHYLO_REHEARSE_SHARDED") != nullptr;
        replicated_book = getenv("PHYLO_REPLICATED_BOOK") != nullptr;
        grad_rows_chain = getenv("PHYLO_GRAD_ROWS_CHAIN") != nullptr;
        grad_coeff_chain = getenv("PHYLO_GRAD_COEFF_CHAIN") != nullptr;
        no_leaf_codes = getenv("PHYLO_NO_LEAF_CODES") != nullptr;
        one_launch = getenv("PHYLO_ONE_LAUNCH") != nullptr;
        persist_stamps = getenv("PHYLO_PERSIST_STAMPS") != nullptr;
        grad_one_stream = getenv("PHYLO_GRAD_ONE_STREAM") != nullptr;
        grad_two_streams = getenv("PHYLO_GRAD_TWO_STREAMS") != nullptr;
        rev_host_lists = getenv("PHYLO_REV_HOST_LISTS") != nullptr;
        no_remote_cache = getenv("PHYLO_NO_REMOTE_CACHE") != nullptr;
        { const char* e = getenv("PHYLO_TREE_WIDE_KEYS"); tree_wide_keys = e && atoi(e) != 0; }
        { const char* e = getenv("PHYLO_REMOTE_CACHE_CAP"); remote_cache_cap = e ? atoi(e) : 0; }
        { const char* e = getenv("PHYLO_SITE_PATTERNS"); site_patterns = !e ? PK_PAT_AUTO : !strcmp(e, "force") ? PK_PAT_FORCE : atoi(e) == 0 ? PK_PAT_OFF : PK_PAT_AUTO; }
        { const char* e = getenv("PHYLO_CLADE_PATTERNS"); clade_patterns = !e ? PK_CLADE_AUTO : !strcmp(e, "force") ? PK_CLADE_FORCE : atoi(e) == 0 ? PK_CLADE_OFF : PK_CLADE_AUTO; }
        { const char* e = getenv("PHYLO_SCAN_MULTI_MIN"); scan_multi_min = e ? atoi(e) : 4096; }
        { const char* e = getenv("PHYLO_SCAN_ANCESTORS"); scan_ancestors = e ? atoi(e) : 1; }
        { const char* e = getenv("PHYLO_TREES_CHUNK"); trees_chunk = e ? atoi(e) : 0; }
        { const char* e = getenv("PHYLO_RELL_CHUNK"); rell_chunk = e ? atoi(e) : 0; }
        { const char* e = getenv("PHYLO_LAUNCH_XCD"); launch_xcd = !e ? 0 : atoi(e) > 0 ? atoi(e) : -1; }
        { const char* e = getenv("PHYLO_P2P"); no_p2p = e && atoi(e) == 0; }
        { const char* e = getenv("PHYLO_P2P_COPY_WORDS"); p2p_copy_words = e ? (size_t)atol(e) : 65536; }
        { const char* e = getenv("PHYLO_P2P_WAIT_S"); p2p_wait_ticks = e && atof(e) > 0 ? (unsigned long long)(atof(e) * 1e8) : PK_P2P_WAIT_TICKS; }
        const char* w = getenv("PHYLO_PERSIST_WGS");
        persist_wgs = w ? atoi(w) : 0;
        const char* t = getenv("PHYLO_PERSIST_NT");
        persist_nt = persist_nt_of(t ? atoi(t) : 0);
    }
};

struct phylo_ctx {
    int device = 0;
    env_switches env;
    int n_cus = 0;                       // compute units of the device
    // one-launch sweep (phylo_persist.h)
    unsigned long long* d_rdraw = nullptr;   // [(N-1)][K] resampling draws
    unsigned long long* d_pctr = nullptr;    // [PK_MAX_GROUPS][PP_CTR_STRIDE] monotone arrival counters
    unsigned long long pctr_base = 0;        // their common value (every group receives Wg arrivals per rank event)
    int pctr_Wg = 0, pctr_G = 0;             // workgroups per group / groups the counters were last used with
    bool pctr_dirty = false;                 // a bounded wait timed out: the counters hold partial arrivals
    int persist_blocks_per_cu = -1;          // occupancy of pp_sweep (-1: not asked yet)
    bool last_persistent = false;
    int last_pp_nt = 0, last_pp_Wg = 0, last_pp_m = 0;   // the grid the last one-launch sweep took (phylo_debug_persist_of)
    size_t last_pp_lds = 0;
    unsigned long long* d_stamps = nullptr;  // phase stamps of the one-launch sweep (PHYLO_PERSIST_STAMPS=1)
    int K = 0, N = 0, S = 0, A = 4;      // K = global particle count
    int Kloc = 0, k0 = 0;                // this rank's shard
    int rank = 0, world = 1;
    uint32_t flags = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::vector<hipEvent_t> kev;         // per-merge-launch events (PHYLO_TIME_KERNELS)
    std::string err;
    bool have_leaves = false, have_model = false, swept = false, state_ready = false;
    int jc = 0;
    double q_norm1 = 0.0;                // ||Q||_1 of the model in force (pt2_check_expm_range)
    std::vector<double> h_lam_l, h_lam_r, h_ldf;
    // model + leaves
    double *d_Q = nullptr, *d_pi = nullptr, *d_lam_l = nullptr, *d_lam_r = nullptr, *d_ldf = nullptr;
    double* d_leaves = nullptr;          // [N][S][4]
    uint8_t* d_leaf_codes = nullptr;     // [N][S]; in use only when every leaf row is one-hot or all-ones
    uint8_t* d_leaf_packed = nullptr;    // the same codes as 16-byte words per lane (phylo_packed_codes.h), behind them in one buffer
    uint8_t* d_pat = nullptr;            // behind both, the site-pattern tables (phylo_site_patterns.h): pattern image, representatives,
    int pat_U = 0;                       // representative leaf image; pat_U: distinct columns of the current leaves (0: not coded)
    bool leaves_coded = false;
    // clade patterns (phylo_site_patterns.h): the strided byte codes and one block per leaf bitset, built by phylo_set_leaves where
    // the rule takes them; first-use, grow-only, uploaded from a pinned image of their own
    uint8_t* d_clade = nullptr;
    uint8_t* h_clade_p = nullptr;
    size_t clade_cap = 0;                // bytes both buffers hold
    pk_clade_layout clade_layout{};      // of the current leaves (clade_ready)
    bool clade_ready = false;            // the tables of the current leaves are on the device (or on their way, on the stream)
    hipEvent_t ev_clade = nullptr;
    int32_t* d_bits[2] = {nullptr, nullptr};   // [K][N] leaf bitset of every root, two planes (allocated by the first sweep that takes the form)
    uint32_t* d_pair_hist = nullptr;     // [N][N][32] code-pair site counts of coded leaves (built on the first twisted sweep)
    bool hist_ready = false, codes_valid = false;
    // sweep state
    double* d_pool = nullptr;            // [(N-1)][Kloc][S][4]
    double* d_nodell = nullptr;          // [N + (N-1)*K]
    double *d_bl = nullptr, *d_br = nullptr, *d_Pmat = nullptr;   // [(N-1)][Kloc](x32)
    double *d_logw = nullptr, *d_ll = nullptr;                    // [(N-1)][K] (global columns)
    double* d_aux = nullptr;             // [Kloc][PK_AUX]
    unsigned long long* d_rec = nullptr; // [Kloc][PK_REC] merge records (128-byte lines)
    int tile_override = 0;               // PHYLO_SITE_TILE / phylo_set_site_tile (0: the policy pm_site_tile)
    int site_tile = 0, ntiles = 1;       // contract v5: sites per tile of the canonical sum over sites (multiple of 64), ceil(S / tile)
    double* d_tilev = nullptr;           // [Kloc][ntiles] tile values of the merge (rows longer than one tile)
    double* d_lse = nullptr;             // [PK_MAX_GROUPS][N-1 + total]; group 0 only unless sweeps are batched
    uint64_t* d_group_seeds = nullptr;   // [PK_MAX_GROUPS]
    // root tables, two planes each, carved from ONE slab (so that peers map it with one handle):
    // rootll[0], rootll[1] (double), roots[0], roots[1], cnt[0], cnt[1] (int32), each [K][N]
    char* d_tables = nullptr;
    int32_t *d_roots[2] = {nullptr, nullptr}, *d_cnt[2] = {nullptr, nullptr};   // [K][N]
    double* d_rootll[2] = {nullptr, nullptr};                                   // [K][N]
    const char** d_tab_ptrs = nullptr;   // [world] table slab of every rank (peer mappings)
    int32_t* d_child = nullptr;          // [(N-1)][Kloc][2]: children of every node (kept for lazy materialisation)
    unsigned int* d_mark = nullptr;      // [(N-1)][K]: node is in the pool
    double* d_sync = nullptr;  // [world] dummy payload of the barrier collective used by lazy nodes when sharded
    // device-side exchange between ranks (pk_p2p_exchange): the all-gathered arrays live in ONE fine-grained slab that the peers map
    bool p2p = false;
    char* d_xslab = nullptr;             // logw | ll | nodell | chosen | sync | flags[2][world]
    size_t xslab_bytes = 0, x_flag_off[2] = {0, 0};
    char** d_xslab_ptrs = nullptr;       // [world] every rank's slab as mapped here
    unsigned long long x_epoch[2] = {0, 0};   // exchanges / barriers issued so far (the same on every rank)
    bool last_lazy = false;
    bool leaves_newer = false;           // phylo_set_leaves since the last sweep: its unwritten nodes can no longer be written
    int32_t* d_merges = nullptr;         // [(N-1)][Kloc][2]
    int64_t* d_anc = nullptr;            // [(N-2)][Kloc]
    uint64_t* d_cdf[2] = {nullptr, nullptr};   // [K], double-buffered across rank events
    // the chain form of a rank event: what the scan of rank event r leaves for rank event r + 1 (every count is written by every
    // scan that writes any: nothing to clear between rank events, sweeps or batch sizes)
    int32_t* d_anc_next = nullptr;       // [K] ancestor of each particle, index inside its group
    int32_t* d_adopt_list = nullptr;     // [K] the adopted particles of each group, ascending
    int32_t* d_adopt_cnt = nullptr;      // [PK_MAX_GROUPS]
    int last_chain = 0;                  // the last sweep's rank events took the chain form (phylo_debug_sweep_chain_of)
    unsigned int* d_counter = nullptr;   // [1] timeout word of the bounded waits between workgroups ([0] unused)
    const double** d_pool_ptrs = nullptr; // [world] pool base of every rank (peer mappings)
    // sharded: remote nodes merged by this rank, fetched once per sweep (pk_pull_remote_children)
    int32_t* d_mirror = nullptr;         // [(N-1) K + 4]: node -> slot + 1 | 0 | -2; the last four words: [0] slots taken
    double* d_cache = nullptr;           // [cache_cap][S][4]
    int cache_cap = 0;
    // twisted proposal (allocated on first use)
    int32_t *d_roots_ad = nullptr, *d_cnt_ad = nullptr;
    double *d_rootll_ad = nullptr, *d_chosen = nullptr, *d_tw_b = nullptr, *d_tw_P = nullptr, *d_pot = nullptr;
    size_t tw_capacity = 0;              // in (particle, sub-sample) entries
    double* d_twbuf = nullptr;           // [Kloc][J] softmax weights of pk_twist_choose when J exceeds what LDS holds
    size_t twbuf_cap = 0;
    // ... and its history when the graph is kept (PHYLO_TWISTING | PHYLO_KEEP_GRAPH): every rank event's rows
    double *d_htw_b = nullptr, *d_htw_P = nullptr, *d_hpot = nullptr, *d_hchosen = nullptr;   // [rows][2], [rows][32], [rows], [R][K]
    int32_t* d_hroots_ad = nullptr;      // [R][K][N]
    double *d_tau = nullptr, *d_ctw = nullptr, *d_twpart = nullptr, *d_twnode = nullptr;       // reverse pass
    int64_t* d_joff = nullptr;           // [R+1]
    size_t htw_rows = 0;                 // rows the history holds
    std::vector<int64_t> h_joff;
    bool last_graph_twist = false, last_graph_marks = false;   // marks: the sweep was lazy, d_mark says which nodes were adopted
    bool last_graph_eager = false;       // the sweep stored every node and left no marks, and its reverse pass can use them: rev_marks
    int last_M = 1;
    // graph kept for the reverse pass (PHYLO_KEEP_GRAPH; allocated on first use)
    int32_t *d_hroots = nullptr, *d_hcnt = nullptr, *d_pos = nullptr;   // [(R+1)][K][N], [(R+1)][K][N], [R][K][N]
    double* d_hrootll = nullptr;         // [(R+1)][K][N]
    double *d_adj = nullptr, *d_om = nullptr, *d_G = nullptr, *d_C = nullptr, *d_part = nullptr, *d_nodeg = nullptr;
    double *d_leafpi = nullptr, *d_leafterm = nullptr, *d_terms = nullptr, *d_gout = nullptr;
    int32_t *d_ad_off = nullptr, *d_ad_idx = nullptr, *d_par_off = nullptr, *d_par_idx = nullptr;
    int32_t *d_heavy = nullptr, *d_chunk_beg = nullptr, *d_chunk_cnt = nullptr;   // [R K], [<= 2 R K / PG_PCHUNK + 1] x2
    int32_t *d_slow_flag = nullptr, *d_slow_idx = nullptr, *d_adp = nullptr;      // [R K] x3
    bool graph_ready = false, last_graph = false;
    int last_G = 1;
    bool last_final_missing = false;
    std::vector<uint64_t> h_group_seeds;
    // host copies of the kept graph's integer records, in pinned memory: copied asynchronously when the sweep ends, so that the
    // reverse pass finds them on the host without a synchronous copy; and the pinned staging area of its packed integer lists
    int64_t* h_anc_p = nullptr;          // [(R-1)][K]
    std::vector<int64_t> h_anc_glob;     // a batched sweep's ancestors as global indices (host builders of the reverse pass)
    std::vector<double> h_gout;          // the reverse pass's results on the host: [G][2 R + 20] (+ [G] log Z-hat, batch call)
    double* h_model_p = nullptr;         // pinned image of the model upload (phylo_set_model)
    double* h_leaves_p = nullptr;        // pinned image of the leaf rows and their codes (phylo_set_leaves)
    hipEvent_t ev_leaves = nullptr;
    uint32_t *h_pub = nullptr, *hd_pub = nullptr;
    int32_t *h_dlmeta = nullptr, *hd_dlmeta = nullptr;   // what pg_dl_lists tells the host (phylo_revlists_dev.h), pinned
    const int32_t* d_dlmeta = nullptr;   // ... and its device original inside scratch 8 (set by dev_lists_launch; pg_args::ev_adp0)
    unsigned int* d_row_done = nullptr;  // [R K][tiles of 256 sites]: pg_nodes_rows_all's "this tile of the adjoint row is complete" words
    unsigned int row_epoch = 0;          // their value in the current reverse pass
    hipEvent_t ev_dl = nullptr;
    size_t dl_temp_p = 0, dl_temp_nn = 0;   // rocPRIM's temporary storage for the parents' sort at this R K
    hipGraphExec_t dl_graph = nullptr;     // that sort's launches, captured (dev_lists_launch)
    const void* dl_graph_key[4] = {nullptr, nullptr, nullptr, nullptr};
    bool dl_no_graph = false;
    uint32_t *hd_csr = nullptr, *hd_anc = nullptr, *hd_child = nullptr, *hd_rad = nullptr;   // device views of h_csr_p, h_anc_p, h_child_p, h_rad_p
    int32_t *h_child_p = nullptr, *h_rad_p = nullptr, *h_csr_p = nullptr;   // [R][K][2], [R][K][N] (twisted), the d_ad_off slab
    size_t h_csr_cap = 0;                // int32 elements
    hipEvent_t ev_gcopy = nullptr;
    std::vector<int32_t> h_cur;          // scratch of the counting sorts
    std::vector<double> h_vi_lam;        // phylo_vi_gradients: the rates of the step (phylo_set_model copies them)
    std::vector<double> h_vi_raw;        // ... and the reverse pass's [2 R + 20] gradients ahead of the chain rules
    // sharded PHYLO_KEEP_GRAPH: whole-K copies of the per-rank records the reverse pass reads, made after the last rank event
    // (graph_gather), and their exchange buffer (pk_gx_pack / pk_gx_unpack); node rows stay in their owners' pools
    int32_t* d_gchild = nullptr;         // [R][K][2]
    double *d_gbl = nullptr, *d_gbr = nullptr, *d_gPmat = nullptr;   // [R][K], [R][K], [R][K][32]
    int64_t* d_ganc = nullptr;           // [(R-1)][K]
    unsigned long long* d_gx = nullptr;  // [chunks][world][gx_cl] words (fine-grained: peers read it over their mappings)
    const unsigned long long** d_gx_src = nullptr;   // [world] where rank p's words are read from
    size_t gx_seg = 0, gx_cl = 0;        // words per rank, words per chunk
    std::vector<int32_t> h_xlists;       // ... of its twisted part
    hipEvent_t evb0 = nullptr, evb1 = nullptr, ev_model = nullptr;
    // reverse pass: the adopted nodes' chain runs on gstream beside the coefficient chain on `stream`; ev_coeff[r]: C of rank event r done
    hipStream_t gstream = nullptr;
    hipEvent_t ev_gfork = nullptr, ev_gjoin = nullptr, ev_gup = nullptr;
    hipStream_t bgstream = nullptr;      // lowest priority: pg_nodes_free in the background of the chains
    hipEvent_t ev_bgfork = nullptr, ev_bgdone = nullptr;
    std::vector<hipEvent_t> ev_coeff;
    phylo_stats stats{};
    sweep_run run;
    int n_merge_events = 0;
    // grow-only scratch for the op-level entry points
    DevBuf scratch[24];                  // (8..10: the device-built lists of the reverse pass; 12, 13: the tree summary's and its branch pass's slabs;
                                         //  14: phylo_trees_loglik's chunk; 15: phylo_rell's logs and its chunk of replicates;
                                         //  16: phylo_trees_grad's chunk and node stores; 17: phylo_trees_grad_rates's; 18: phylo_trees_nni's;
                                         //  19: phylo_trees_nni_rates's; 20: phylo_trees_grad_model's; 21: phylo_rell_multiscale's logs and chunk;
                                         //  22: phylo_trees_ancestral's chunk, staged outputs and node stores; 23: phylo_trees_ancestral_rates's)
    phylo_comm comm;
    // the last phylo_tree_summary (phylo_trees.h): its tables live in scratch slot 12 until the next summary
    pt_bufs ts;
    bool ts_done = false;
    int ts_G = 1, ts_nt = 0;
    long long ts_nc = 0;
    hipEvent_t ev_ts0 = nullptr, ev_ts1 = nullptr;
    // the last phylo_tree_branches of that summary (scratch slot 13); a sweep begun since the summary makes both stale for it
    pb_bufs tb;
    bool tb_done = false;
    int tb_wide = -1, tb_cbits = 0, tb_tbits = 0;   // the plan the last finished branch pass took (-1: none yet; phylo_debug_tree_branches_of)
    unsigned long long sweep_serial = 0, ts_serial = 0;
    hipEvent_t ev_tb0 = nullptr, ev_tb1 = nullptr;
    hipEvent_t ev_t0 = nullptr, ev_t1 = nullptr;     // the scored-tree-set calls' one pair (the sweep's and the summaries' stay theirs)
    hipEvent_t ev_rl0 = nullptr, ev_rl1 = nullptr;   // phylo_rell's own pair
    hipEvent_t ev_rm0 = nullptr, ev_rm1 = nullptr;   // phylo_rell_multiscale's own pair
};

namespace {

int fail(phylo_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    g_last_error = buf;
    return code;
}

#define HIPCHK(ctx, call)                                                                             \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess)                                                                         \
            return fail(ctx, e_ == hipErrorOutOfMemory ? PHYLO_ENOMEM : PHYLO_EHIP, "%s failed: %s (%s:%d)", \
                        #call, hipGetErrorString(e_), __FILE__, __LINE__);                            \
    } while (0)

#define CHK(expr)                   \
    do {                            \
        int rc_ = (expr);           \
        if (rc_ != PHYLO_OK) return rc_; \
    } while (0)

template <typename T>
int dalloc(phylo_ctx* ctx, T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    HIPCHK(ctx, hipMalloc((void**)p, count * sizeof(T)));
    return PHYLO_OK;
}

int scratch_get(phylo_ctx* ctx, int slot, size_t bytes, void** out) {
    DevBuf& b = ctx->scratch[slot];
    if (b.bytes < bytes) {
        if (b.p) HIPCHK(ctx, hipFree(b.p));
        b.p = nullptr;
        b.bytes = 0;
        const size_t want = bytes + bytes / 2 + 16;         // (grow by half: sizes that creep up from call to call -- the chunk counts
        HIPCHK(ctx, hipMalloc(&b.p, want));                 //  of the reverse pass -- would free and allocate, 60 us, again and again)
        b.bytes = want;
    }
    *out = b.p;
    return PHYLO_OK;
}

int bind(phylo_ctx* ctx) {
    if (!ctx) return fail(nullptr, PHYLO_EINVAL, "ctx is NULL");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return PHYLO_OK;
}

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// -log (2 max(c,2) - 3)!! by the reference's loop (vcsmc.py:30-57): n, n-2, ... while >= 2
double host_log_double_factorial(int m) {
    double res = 0.0;
    for (int v = m; v >= 2; v -= 2) res = res + pm_log((double)v);
    return res;
}

int launch_check(phylo_ctx* ctx, const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(ctx, PHYLO_EHIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return PHYLO_OK;
}

void free_sweep_state(phylo_ctx* c) {
    // the reverse pass's side streams may still read what is freed below
    if (c->gstream) (void)hipStreamSynchronize(c->gstream);
    if (c->bgstream) (void)hipStreamSynchronize(c->bgstream);
    if (c->d_xslab) {                                       // the exchanged arrays are carved from the slab
        (void)hipFree(c->d_xslab);
        c->d_xslab = nullptr;
        c->d_logw = c->d_ll = c->d_nodell = c->d_sync = nullptr;
        c->d_chosen = nullptr;
    }
    if (c->d_xslab_ptrs) (void)hipFree((void*)c->d_xslab_ptrs);
    c->d_xslab_ptrs = nullptr;
    c->xslab_bytes = 0;
    c->x_epoch[0] = c->x_epoch[1] = 0;
    if (c->d_twbuf) (void)hipFree(c->d_twbuf);
    c->d_twbuf = nullptr;
    c->twbuf_cap = 0;
    void* tw[] = {c->d_roots_ad, c->d_cnt_ad, c->d_rootll_ad, c->d_chosen, c->d_tw_b, c->d_tw_P, c->d_pot};
    for (void* p : tw)
        if (p) (void)hipFree(p);
    c->d_roots_ad = c->d_cnt_ad = nullptr;
    c->d_rootll_ad = c->d_chosen = c->d_tw_b = c->d_tw_P = c->d_pot = nullptr;
    c->tw_capacity = 0;
    void* ht[] = {c->d_htw_b, c->d_htw_P, c->d_hpot, c->d_hchosen, c->d_hroots_ad, c->d_tau, c->d_ctw, c->d_twpart, c->d_twnode, c->d_joff};
    for (void* p : ht)
        if (p) (void)hipFree(p);
    c->d_htw_b = c->d_htw_P = c->d_hpot = c->d_hchosen = c->d_tau = c->d_ctw = c->d_twpart = c->d_twnode = nullptr;
    c->d_hroots_ad = nullptr;
    c->d_joff = nullptr;
    c->htw_rows = 0;
    c->last_graph_twist = false;
    void* gr[] = {c->d_hroots, c->d_hcnt, c->d_pos, c->d_hrootll, c->d_adj, c->d_om, c->d_G, c->d_C, c->d_part, c->d_nodeg,
                  c->d_leafpi, c->d_leafterm, c->d_terms, c->d_gout, c->d_ad_off, c->d_gchild, c->d_gbl, c->d_gbr, c->d_gPmat,
                  c->d_ganc, c->d_gx, (void*)c->d_gx_src};
    for (void* p : gr)
        if (p) (void)hipFree(p);
    c->d_hroots = c->d_hcnt = c->d_pos = nullptr;
    c->d_hrootll = c->d_adj = c->d_om = c->d_G = c->d_C = c->d_part = c->d_nodeg = nullptr;
    c->d_leafpi = c->d_leafterm = c->d_terms = c->d_gout = nullptr;
    c->d_gchild = nullptr; c->d_gbl = c->d_gbr = c->d_gPmat = nullptr; c->d_ganc = nullptr;
    c->d_gx = nullptr; c->d_gx_src = nullptr; c->gx_seg = c->gx_cl = 0;
    c->d_ad_off = c->d_ad_idx = c->d_par_off = c->d_par_idx = nullptr;
    c->d_heavy = c->d_chunk_beg = c->d_chunk_cnt = nullptr;
    c->d_slow_flag = c->d_slow_idx = c->d_adp = nullptr;
    if (c->h_csr_p) (void)hipHostFree(c->h_csr_p);
    if (c->h_anc_p) (void)hipHostFree(c->h_anc_p);
    if (c->h_child_p) (void)hipHostFree(c->h_child_p);
    if (c->h_rad_p) (void)hipHostFree(c->h_rad_p);
    if (c->h_pub) (void)hipHostFree(c->h_pub);
    if (c->d_row_done) (void)hipFree(c->d_row_done);
    c->d_row_done = nullptr;
    if (c->h_dlmeta) (void)hipHostFree(c->h_dlmeta);
    c->h_dlmeta = c->hd_dlmeta = nullptr;
    if (c->ev_dl) (void)hipEventDestroy(c->ev_dl);
    c->ev_dl = nullptr;
    if (c->dl_graph) (void)hipGraphExecDestroy(c->dl_graph);
    c->dl_graph = nullptr;
    c->h_pub = c->hd_pub = nullptr;
    c->h_csr_p = c->h_child_p = c->h_rad_p = nullptr;
    c->h_anc_p = nullptr;
    if (c->ev_gcopy) (void)hipEventDestroy(c->ev_gcopy);
    c->ev_gcopy = nullptr;
    c->graph_ready = false;
    c->last_graph = false;
    if (c->d_stamps) (void)hipFree(c->d_stamps);
    c->d_stamps = nullptr;
    if (c->d_rdraw) (void)hipFree(c->d_rdraw);
    if (c->d_pctr) (void)hipFree(c->d_pctr);
    c->d_rdraw = c->d_pctr = nullptr;
    c->pctr_base = 0;
    c->pctr_Wg = c->pctr_G = 0;
    c->pctr_dirty = false;
    if (c->d_tilev) (void)hipFree(c->d_tilev);
    c->d_tilev = nullptr;
    if (c->d_bits[0]) (void)hipFree(c->d_bits[0]);
    c->d_bits[0] = c->d_bits[1] = nullptr;
    void* ptrs[] = {c->d_pool, c->d_nodell, c->d_bl, c->d_br, c->d_Pmat, c->d_logw, c->d_ll, c->d_aux, c->d_lse, c->d_group_seeds,
                    c->d_tables, (void*)c->d_tab_ptrs, c->d_child, c->d_merges, c->d_anc,
                    c->d_cdf[0], c->d_cdf[1], c->d_anc_next, c->d_adopt_list, c->d_adopt_cnt, c->d_counter, (void*)c->d_pool_ptrs, c->d_mark, c->d_sync, c->d_mirror, c->d_cache, c->d_rec};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    c->d_pool = c->d_nodell = c->d_bl = c->d_br = c->d_Pmat = c->d_logw = c->d_ll = c->d_aux = c->d_lse = nullptr;
    c->d_group_seeds = nullptr;
    c->d_rec = nullptr;
    c->d_roots[0] = c->d_roots[1] = c->d_cnt[0] = c->d_cnt[1] = c->d_child = c->d_merges = nullptr;
    c->d_anc = nullptr;
    c->d_cdf[0] = c->d_cdf[1] = nullptr;
    c->d_anc_next = c->d_adopt_list = c->d_adopt_cnt = nullptr;
    c->d_counter = nullptr;
    c->d_rootll[0] = c->d_rootll[1] = nullptr;
    c->d_tables = nullptr;
    c->d_tab_ptrs = nullptr;
    c->d_pool_ptrs = nullptr;
    c->d_mark = nullptr;
    c->d_sync = nullptr;
    c->d_mirror = nullptr;
    c->d_cache = nullptr;
    c->cache_cap = 0;
}

int alloc_sweep_state(phylo_ctx* c) {
    free_sweep_state(c);
    c->state_ready = false;
    const size_t R = (size_t)c->N - 1, K = c->K, Kl = c->Kloc, N = c->N, S = c->S;
    CHK(dalloc(c, &c->d_pool, R * Kl * S * 4));
    // Sharded: the arrays that cross ranks at every rank event live in one slab of FINE-GRAINED device memory (peers write into
    // it over xGMI and this rank reads it in later kernels: no stale line may survive in this device's L2) that every peer maps.
    c->p2p = c->comm.transport != 0 && c->world > 1 && !c->env.no_p2p && R >= 2;
    if (c->p2p) {
        const size_t al = 32;                               // doubles: 256-byte alignment of every array
        auto up = [&](size_t n) { return (n + al - 1) / al * al; };
        const size_t n_logw = up(R * K), n_nod = up(N + R * K), n_ch = up(K), n_sy = up((size_t)c->world), n_fl = up((size_t)c->world);
        const size_t total = 2 * n_logw + n_nod + n_ch + n_sy + 2 * n_fl;
        void* slab = nullptr;
        if (hipExtMallocWithFlags(&slab, total * 8, hipDeviceMallocFinegrained) != hipSuccess) {
            (void)hipGetLastError();
            HIPCHK(c, hipMalloc(&slab, total * 8));         // (coarse-grained: still correct on one device)
        }
        HIPCHK(c, hipMemset(slab, 0, total * 8));
        c->d_xslab = (char*)slab;
        c->xslab_bytes = total * 8;
        double* base = (double*)slab;
        c->d_logw = base; c->d_ll = base + n_logw; c->d_nodell = base + 2 * n_logw;
        c->d_chosen = c->d_nodell + n_nod;
        c->d_sync = c->d_chosen + n_ch;
        c->x_flag_off[0] = (size_t)((char*)(c->d_sync + n_sy) - c->d_xslab);
        c->x_flag_off[1] = c->x_flag_off[0] + n_fl * 8;
        c->x_epoch[0] = c->x_epoch[1] = 0;
    } else {
    CHK(dalloc(c, &c->d_nodell, N + R * K));
    }
    CHK(dalloc(c, &c->d_bl, R * Kl));
    CHK(dalloc(c, &c->d_br, R * Kl));
    CHK(dalloc(c, &c->d_Pmat, R * Kl * 32));
    if (!c->p2p) {
        CHK(dalloc(c, &c->d_logw, R * K));
        CHK(dalloc(c, &c->d_ll, R * K));
    }
    CHK(dalloc(c, &c->d_aux, Kl * PK_AUX));
    CHK(dalloc(c, &c->d_rec, Kl * PK_REC));
    if (c->ntiles > 1) CHK(dalloc(c, &c->d_tilev, Kl * (size_t)c->ntiles));
    CHK(dalloc(c, &c->d_lse, (R + 1) * PK_MAX_GROUPS));
    CHK(dalloc(c, &c->d_group_seeds, PK_MAX_GROUPS));
    CHK(dalloc(c, &c->d_tables, 32 * K * N));
    for (int i = 0; i < 2; ++i) {
        c->d_rootll[i] = reinterpret_cast<double*>(c->d_tables) + (size_t)i * K * N;
        c->d_roots[i] = reinterpret_cast<int32_t*>(c->d_tables + 16 * K * N) + (size_t)i * K * N;
        c->d_cnt[i] = reinterpret_cast<int32_t*>(c->d_tables + 24 * K * N) + (size_t)i * K * N;
    }
    CHK(dalloc(c, &c->d_child, R * Kl * 2));
    CHK(dalloc(c, &c->d_mark, ((R * K + R + 3) & ~(size_t)3)));      // one mark per node
    if (!c->p2p) CHK(dalloc(c, &c->d_sync, (size_t)c->world));
    CHK(dalloc(c, &c->d_merges, R * Kl * 2));
    CHK(dalloc(c, &c->d_anc, (R > 0 ? R - 1 : 0) * Kl));
    CHK(dalloc(c, &c->d_cdf[0], K));
    CHK(dalloc(c, &c->d_cdf[1], K));
    CHK(dalloc(c, &c->d_anc_next, K));
    CHK(dalloc(c, &c->d_adopt_list, K));
    CHK(dalloc(c, &c->d_adopt_cnt, (size_t)PK_MAX_GROUPS));
    HIPCHK(c, hipMemset(c->d_anc_next, 0, K * 4));         // (indices: never read before a scan wrote them, and in range even so)
    HIPCHK(c, hipMemset(c->d_adopt_list, 0, K * 4));
    HIPCHK(c, hipMemset(c->d_adopt_cnt, 0, (size_t)PK_MAX_GROUPS * 4));
    CHK(dalloc(c, &c->d_counter, ((size_t)N + 3) & ~(size_t)3));
    HIPCHK(c, hipMemset(c->d_counter, 0, (((size_t)N + 3) & ~(size_t)3) * sizeof(unsigned int)));
    CHK(dalloc(c, &c->d_pool_ptrs, (size_t)c->world));
    std::vector<void*> ptrs;
    int rc = phylo_comm_map_pools(c->comm, c->d_pool, &ptrs, c->stream, &c->err);
    if (rc != PHYLO_OK) return rc;
    HIPCHK(c, hipMemcpy((void*)c->d_pool_ptrs, ptrs.data(), ptrs.size() * sizeof(void*), hipMemcpyHostToDevice));
    if ((c->world > 1 || c->env.rehearse_sharded) && !c->env.no_remote_cache) {
        // the local cache of remote nodes: up to 512 MB of rows (primate.p: 17 000 nodes; 128 x 50 000: 320), the rest in place
        const size_t node_bytes = (size_t)S * 32;
        size_t cap = ((size_t)512 << 20) / node_bytes;
        if (c->env.remote_cache_cap > 0) cap = (size_t)c->env.remote_cache_cap;
        if (cap > R * K) cap = R * K;
        if (cap < 1) cap = 1;
        c->cache_cap = (int)cap;
        CHK(dalloc(c, &c->d_mirror, R * K + 4));
        CHK(dalloc(c, &c->d_cache, cap * (size_t)S * 4));
    }
    CHK(dalloc(c, &c->d_tab_ptrs, (size_t)c->world));
    rc = phylo_comm_map_extra(c->comm, c->d_tables, &ptrs, c->stream, &c->err);
    if (rc != PHYLO_OK) return rc;
    HIPCHK(c, hipMemcpy((void*)c->d_tab_ptrs, ptrs.data(), ptrs.size() * sizeof(void*), hipMemcpyHostToDevice));
    if (c->p2p) {
        CHK(dalloc(c, &c->d_xslab_ptrs, (size_t)c->world));
        rc = phylo_comm_map_extra(c->comm, c->d_xslab, &ptrs, c->stream, &c->err);
        if (rc != PHYLO_OK) return rc;
        HIPCHK(c, hipMemcpy((void*)c->d_xslab_ptrs, ptrs.data(), ptrs.size() * sizeof(void*), hipMemcpyHostToDevice));
    }
    c->state_ready = true;
    return PHYLO_OK;
}

// The sweep state (node pool = (N-1) K_local S 32 bytes) is allocated on first use, so that a context created
// with the GLOBAL particle count and then sharded by phylo_comm_init never asks for the unsharded pool.
int ensure_sweep_state(phylo_ctx* c) {
    if (c->state_ready) return PHYLO_OK;
    return alloc_sweep_state(c);
}

// buffers of the reverse pass: table history, adjoint pool, coefficient tables, CSR lists
int ensure_graph_state(phylo_ctx* c) {
    if (c->graph_ready) return PHYLO_OK;
    const size_t R = (size_t)c->N - 1, K = c->K, N = c->N, S = c->S;
    const size_t T = (S + PG_NT - 1) / PG_NT;
    CHK(dalloc(c, &c->d_hroots, (R + 1) * K * N));
    CHK(dalloc(c, &c->d_hcnt, (R + 1) * K * N));
    CHK(dalloc(c, &c->d_hrootll, (R + 1) * K * N));
    CHK(dalloc(c, &c->d_pos, R * K * N));
    CHK(dalloc(c, &c->d_adj, R * K * S * 4));
    CHK(dalloc(c, &c->d_om, R * K));
    CHK(dalloc(c, &c->d_G, R * K));
    CHK(dalloc(c, &c->d_C, R * K * N));
    CHK(dalloc(c, &c->d_part, R * K * T * PG_PART));
    CHK(dalloc(c, &c->d_nodeg, R * K * PG_NODEG));
    CHK(dalloc(c, &c->d_leafpi, N * 4));
    CHK(dalloc(c, &c->d_leafterm, K * 4));
    CHK(dalloc(c, &c->d_terms, R * K * 2));
    CHK(dalloc(c, &c->d_gout, (2 * R + 21) * PK_MAX_GROUPS));   // a batched sweep: a row per group, then the groups' log Z-hat
    {   // the integer lists of the reverse pass live in ONE slab, uploaded with one copy per step
        c->h_csr_cap = pg_lists_ints(R, K);               // (layout: pg_lists_carve, phylo_revlists.h)
        CHK(dalloc(c, &c->d_ad_off, c->h_csr_cap));
        HIPCHK(c, hipHostMalloc((void**)&c->h_csr_p, c->h_csr_cap * 4));
        HIPCHK(c, hipHostMalloc((void**)&c->h_anc_p, (R > 1 ? (R - 1) * K : 1) * 8));
        HIPCHK(c, hipHostMalloc((void**)&c->h_child_p, R * K * 2 * 4));
        // device views of the pinned buffers (pg_copy_words reads / writes them from kernels)
        HIPCHK(c, hipHostGetDevicePointer((void**)&c->hd_csr, c->h_csr_p, 0));
        HIPCHK(c, hipHostGetDevicePointer((void**)&c->hd_anc, c->h_anc_p, 0));
        HIPCHK(c, hipHostGetDevicePointer((void**)&c->hd_child, c->h_child_p, 0));
        HIPCHK(c, hipHostMalloc((void**)&c->h_pub, 16));   // log Z-hat (8 bytes) and the timeout word of a sweep that keeps its graph
        HIPCHK(c, hipHostGetDevicePointer((void**)&c->hd_pub, c->h_pub, 0));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_gcopy, hipEventDisableTiming));
        HIPCHK(c, hipHostMalloc((void**)&c->h_dlmeta, ((size_t)PG_DL_META_INTS(R) + 4) * 4));   // (+ the timeout word of pg_nodes_rows_all)
        c->h_dlmeta[PG_DL_META_INTS(R)] = 0;
        HIPCHK(c, hipHostGetDevicePointer((void**)&c->hd_dlmeta, c->h_dlmeta, 0));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_dl, hipEventDisableTiming));
        c->dl_temp_nn = 0;
        const pg_lists D = pg_lists_carve(c->d_ad_off, R, K);
        c->d_ad_idx = D.ad_idx; c->d_par_off = D.par_off; c->d_par_idx = D.par_idx;
        c->d_heavy = D.heavy; c->d_chunk_beg = D.chunk_beg; c->d_chunk_cnt = D.chunk_cnt;
        c->d_slow_flag = D.slow_flag; c->d_slow_idx = D.slow_idx; c->d_adp = D.adp;
    }
    if (c->world > 1) {                                    // sharded: the whole-K records of graph_gather and its exchange buffer
        const size_t Kl = c->Kloc, W = c->world;
        CHK(dalloc(c, &c->d_gchild, R * K * 2));
        CHK(dalloc(c, &c->d_gbl, R * K));
        CHK(dalloc(c, &c->d_gbr, R * K));
        CHK(dalloc(c, &c->d_gPmat, R * K * 32));
        CHK(dalloc(c, &c->d_ganc, (R > 1 ? R - 1 : 1) * K));
        // words per rank: children 2, branch lengths 2, matrices 32 per (r, k); ancestors
        c->gx_seg = R * Kl * 36 + (R > 1 ? (R - 1) * Kl : 0);
        c->gx_cl = c->gx_seg < PHYLO_SHM_SLOT / 8 ? c->gx_seg : PHYLO_SHM_SLOT / 8;   // (a chunk fits the host-mediated transport's slot)
        const size_t words = (c->gx_seg + c->gx_cl - 1) / c->gx_cl * c->gx_cl * W;
        void* buf = nullptr;
        if (hipExtMallocWithFlags(&buf, words * 8, hipDeviceMallocFinegrained) != hipSuccess) {
            (void)hipGetLastError();
            HIPCHK(c, hipMalloc(&buf, words * 8));
        }
        c->d_gx = (unsigned long long*)buf;
        CHK(dalloc(c, &c->d_gx_src, W));
        std::vector<void*> src(W, buf);                    // collective path: every rank's words land in the own buffer
        if (c->p2p) {                                      // device-side exchange: read from the peers' buffers (collective: mapped once)
            int rc = phylo_comm_map_extra(c->comm, buf, &src, c->stream, &c->err);
            if (rc != PHYLO_OK) return rc;
        }
        HIPCHK(c, hipMemcpy((void*)c->d_gx_src, src.data(), W * sizeof(void*), hipMemcpyHostToDevice));
    }
    if (!c->evb0) {
        HIPCHK(c, hipEventCreate(&c->evb0));
        HIPCHK(c, hipEventCreate(&c->evb1));
        HIPCHK(c, hipStreamCreateWithFlags(&c->gstream, hipStreamNonBlocking));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_gfork, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_gjoin, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_gup, hipEventDisableTiming));
        {
            int least = 0, greatest = 0;
            HIPCHK(c, hipDeviceGetStreamPriorityRange(&least, &greatest));
            HIPCHK(c, hipStreamCreateWithPriority(&c->bgstream, hipStreamNonBlocking, least));
        }
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_bgfork, hipEventDisableTiming));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_bgdone, hipEventDisableTiming));
        c->ev_coeff.assign((size_t)R, nullptr);
        for (auto& e : c->ev_coeff) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    c->graph_ready = true;
    return PHYLO_OK;
}

// One launch with the kernel's own begin / end stamped into a pair of events (what rocprofv3 --kernel-trace reports), or without
template <typename... P, typename... A>
void launch_stamped(void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t e0, hipEvent_t e1, A&&... args) {
    if (e0) hipExtLaunchKernelGGL(kernel, grid, block, lds, s, e0, e1, 0, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, s, args...);
}

// the constants of the kernel headers and the thresholds that the plans read (phylo_sweep_plan.h)
static sweep_limits sweep_limits_of() {
    sweep_limits L{};
    L.max_groups = PK_MAX_GROUPS; L.twist_max_m = PK_TWIST_MAX_M; L.twist_max_j = PK_TWIST_MAX_J;
    L.mat_group = PK_MAT_GROUP; L.scan_fold_max_kg = PP_SCAN_KERNEL_MAX_KG; L.kept_bits_taxa = PG_KEPT_BITS_TAXA;
    L.scan_lds512_max_kg = 4096;
    L.one_tile_max_s = 4096;
    L.small_max_kg = 4096; L.small_max_kloc = 8192;
    L.book_packed8_min = 8192;
    L.sorted_min_draws = 262144;
    return L;
}
static const sweep_limits k_sweep_limits = sweep_limits_of();

// Resampling scan of G groups of Kg log-weights, in the form sweep_scan_form_of decides (phylo_sweep_plan.h): several workgroups per
// group above PHYLO_SCAN_MULTI_MIN weights (three launches); else one workgroup per group, with the cdf in LDS by 512 threads up to
// 4096 weights and by 1024 threads up to PP_SCAN_KERNEL_MAX_KG (phylo_persist.h), and beyond that staged in the cdf buffer itself
// (pk_resample_scan(_groups), phylo_kernels.h).
// `anc` (the chain form of a rank event; the LDS forms alone): the scan also writes the resampling outcome (pp_scan_ancestors).
int launch_scan(phylo_ctx* c, const double* logw, int Kg, int G, uint64_t* cdf, double* lse, int lse_stride, int logz_R = 0,
                const pp_anc_out* anc = nullptr) {
    const pp_anc_out ao = anc ? *anc : pp_anc_out{};
    const sweep_scan_form form = sweep_scan_form_of(Kg, c->env.scan_multi_min, cdf || lse, k_sweep_limits);
    if (ao.anc && (!cdf || logz_R > 0 || (form != SCAN_LDS_512 && form != SCAN_LDS_1024)))
        return fail(c, PHYLO_ESTATE, "launch_scan: the resampling outcome needs a cdf and a scan that holds it in LDS (Kg = %d)", Kg);
    if (form == SCAN_MULTI) {
        pp_scan_multi_args a{};
        a.logw = logw; a.Kg = Kg; a.B = (Kg + PP_SCAN_TILE - 1) / PP_SCAN_TILE;
        void* ws = nullptr;
        const size_t nb = (size_t)G * a.B;
        CHK(scratch_get(c, 11, (nb * 2 + (size_t)G * Kg) * 8, &ws));
        a.gmax = (double*)ws; a.bsum = (unsigned long long*)ws + nb; a.wbits = (unsigned long long*)ws + 2 * nb;
        a.cdf = (unsigned long long*)cdf; a.lse_out = lse; a.lse_stride = lse_stride; a.logz_R = logz_R;
        hipLaunchKernelGGL(pp_scan_multi_max, dim3(a.B, G), dim3(512), 0, c->stream, a);
        CHK(launch_check(c, "pp_scan_multi_max"));
        hipLaunchKernelGGL(pp_scan_multi_exp, dim3(a.B, G), dim3(512), 0, c->stream, a);
        CHK(launch_check(c, "pp_scan_multi_exp"));
        // (no cdf wanted: the log-normaliser's workgroup alone)
        if (cdf) hipLaunchKernelGGL(pp_scan_multi_cdf, dim3(a.B + 1, G), dim3(512), 0, c->stream, a);
        else { a.lse_only = 1; hipLaunchKernelGGL(pp_scan_multi_cdf, dim3(1, G), dim3(512), 0, c->stream, a); }
        return launch_check(c, "pp_scan_multi_cdf");
    }
    if (form == SCAN_LDS_512) {
        if (ao.anc) hipLaunchKernelGGL(pp_resample_scan_anc<512>, dim3(G), dim3(512), pp_resample_scan_lds(Kg, true), c->stream, logw, Kg, cdf, lse, lse_stride, ao);
        else hipLaunchKernelGGL(pp_resample_scan<512>, dim3(G), dim3(512), pp_resample_scan_lds(Kg), c->stream, logw, Kg, cdf, lse, lse_stride, logz_R);
        return launch_check(c, "pp_resample_scan");
    }
    if (form == SCAN_LDS_1024) {
        const size_t lds = pp_resample_scan_lds(Kg, ao.anc != nullptr);
        static bool raised = false, raised_anc = false;                        // (beyond the 64 KB every kernel may ask for: say so once, like dev_lists_adopters)
        if (lds > 65536 && !raised && !ao.anc) {
            HIPCHK(c, hipFuncSetAttribute((const void*)pp_resample_scan<1024>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)pp_resample_scan_lds(PP_SCAN_KERNEL_MAX_KG)));
            raised = true;
        }
        if (ao.anc) {
            if (lds > 65536 && !raised_anc) {
                HIPCHK(c, hipFuncSetAttribute((const void*)pp_resample_scan_anc<1024>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)pp_resample_scan_lds(PP_SCAN_KERNEL_MAX_KG, true)));
                raised_anc = true;
            }
            hipLaunchKernelGGL(pp_resample_scan_anc<1024>, dim3(G), dim3(1024), lds, c->stream, logw, Kg, cdf, lse, lse_stride, ao);
            return launch_check(c, "pp_resample_scan_anc");
        }
        hipLaunchKernelGGL(pp_resample_scan<1024>, dim3(G), dim3(1024), lds, c->stream, logw, Kg, cdf, lse, lse_stride, logz_R);
        return launch_check(c, "pp_resample_scan");
    }
    if (G > 1) hipLaunchKernelGGL(pk_resample_scan_groups, dim3(G), dim3(PK_COLS), 0, c->stream, logw, Kg, cdf, lse, lse_stride);
    else hipLaunchKernelGGL(pk_resample_scan, dim3(1), dim3(PK_COLS), 0, c->stream, logw, Kg, cdf, lse);
    return launch_check(c, "pk_resample_scan");
}

// leaf node log-likelihoods sum_s log(pi . leaf[s]) (depend on pi and the leaves)
// Wait for an event by polling (a blocking hipEventSynchronize wakes the thread tens of microseconds after the event -- a twentieth of
// a training step, twice per step); after 2 ms of polling, block.
int wait_event_spin(phylo_ctx* c, hipEvent_t ev) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return PHYLO_OK;
        if (e != hipErrorNotReady) return fail(c, PHYLO_EHIP, "hipEventQuery: %s", hipGetErrorString(e));
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
        __builtin_ia32_pause();
    }
    HIPCHK(c, hipEventSynchronize(ev));
    return PHYLO_OK;
}

// site tile of an op-level call on rows of S sites (the context's own S has c->site_tile)
int tile_for(const phylo_ctx* c, int S) { return c->tile_override ? c->tile_override : pm_site_tile(S); }

int refresh_leaf_ll(phylo_ctx* c) {
    if (!(c->have_leaves && c->have_model && c->state_ready)) return PHYLO_OK;
    hipLaunchKernelGGL(pk_row_loglik, dim3(c->N), dim3(64), 0, c->stream, c->d_leaves, c->d_pi, c->S, c->site_tile,
                       c->d_nodell);
    return launch_check(c, "pk_row_loglik(leaves)");
}

}  // namespace

extern "C" {

const char* phylo_version(void) { return "phylo_hip 0.1 (gfx950)"; }

const char* phylo_last_error(const phylo_ctx* ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

int phylo_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int phylo_create(const int* device_ids, int n_gpus, int K, int N, int S, int A, uint32_t flags,
                 phylo_ctx** out) {
    if (!out) return fail(nullptr, PHYLO_EINVAL, "out is NULL");
    *out = nullptr;
    if (n_gpus != 1)
        return fail(nullptr, PHYLO_EINVAL, "n_gpus must be 1 (one process per GPU; join ranks with phylo_comm_init)");
    if (A != 4) return fail(nullptr, PHYLO_EINVAL, "A must be 4 (DNA alphabet), got %d", A);
    if (K < 1 || N < 2 || S < 1) return fail(nullptr, PHYLO_EINVAL, "need K >= 1, N >= 2, S >= 1 (K=%d N=%d S=%d)", K, N, S);
    if (N > PK_MAX_TAXA) return fail(nullptr, PHYLO_EINVAL, "N = %d exceeds the supported maximum %d", N, PK_MAX_TAXA);
    if ((double)(N - 1) * K + N > 2.0e9) return fail(nullptr, PHYLO_EINVAL, "node ids overflow int32");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail(nullptr, PHYLO_ENODEVICE, "no HIP device available (%s); this library has no CPU path",
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    const int dev = device_ids ? device_ids[0] : 0;
    if (dev < 0 || dev >= ndev) return fail(nullptr, PHYLO_ENODEVICE, "device id %d out of range [0,%d)", dev, ndev);
    phylo_ctx* c = new phylo_ctx();
    c->device = dev;
    c->K = K; c->N = N; c->S = S; c->A = A;
    c->Kloc = K; c->k0 = 0;
    c->flags = flags;
    c->env.read();
    {   // contract v5: the site tile is part of the arithmetic contract (the oracle takes the same value)
        const char* t = getenv("PHYLO_SITE_TILE");
        int T = t ? atoi(t) : pm_site_tile(S);
        if (T < 64 || (T & 63) || T > PK_MAX_SITE_TILE) { delete c; return fail(nullptr, PHYLO_EINVAL, "PHYLO_SITE_TILE must be a multiple of 64 in [64, %d] (got %d)", PK_MAX_SITE_TILE, T); }
        c->tile_override = t ? T : 0;
        c->site_tile = T;
        c->ntiles = (S + T - 1) / T;
    }
    int rc = PHYLO_OK;
    do {
        if ((rc = bind(c)) != PHYLO_OK) break;
        {
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, dev) != hipSuccess) { rc = fail(c, PHYLO_EHIP, "hipGetDeviceProperties failed"); break; }
            c->n_cus = prop.multiProcessorCount;
        }
        if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { rc = fail(c, PHYLO_EHIP, "hipStreamCreate failed"); break; }
        if (hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess) { rc = fail(c, PHYLO_EHIP, "hipEventCreate failed"); break; }
        if ((rc = dalloc(c, &c->d_Q, 20 + 2 * (size_t)N)) != PHYLO_OK) break;   // one slab: Q[16] pi[4] lam_l[N] lam_r[N]
        c->d_pi = c->d_Q + 16;
        c->d_lam_l = c->d_Q + 20;
        c->d_lam_r = c->d_Q + 20 + N;
        if ((rc = dalloc(c, &c->d_ldf, (size_t)N + 1)) != PHYLO_OK) break;
        if ((rc = dalloc(c, &c->d_leaves, (size_t)N * S * 4)) != PHYLO_OK) break;
        if ((rc = dalloc(c, &c->d_leaf_codes, pk_leaf_image_bytes(N, S))) != PHYLO_OK) break;
        c->d_leaf_packed = c->d_leaf_codes + pk_packed_offset(N, S);
        c->d_pat = c->d_leaf_codes + pk_pat_offset(N, S);
        // table of log (2 max(c,2) - 3)!! by leaf count c = 0..N
        c->h_ldf.resize((size_t)N + 1);
        for (int cnt = 0; cnt <= N; ++cnt) c->h_ldf[cnt] = host_log_double_factorial(2 * (cnt > 2 ? cnt : 2) - 3);
        if (hipMemcpy(c->d_ldf, c->h_ldf.data(), ((size_t)N + 1) * 8, hipMemcpyHostToDevice) != hipSuccess) { rc = fail(c, PHYLO_EHIP, "ldf upload failed"); break; }
    } while (0);
    if (rc != PHYLO_OK) {
        g_last_error = c->err;
        phylo_destroy(c);
        return rc;
    }
    *out = c;
    return PHYLO_OK;
}

int phylo_destroy(phylo_ctx* c) {
    if (!c) return PHYLO_OK;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->gstream) (void)hipStreamSynchronize(c->gstream);
    if (c->bgstream) (void)hipStreamSynchronize(c->bgstream);
    phylo_comm_destroy(&c->comm);
    free_sweep_state(c);
    void* ptrs[] = {c->d_Q, c->d_ldf, c->d_leaves, c->d_leaf_codes, c->d_clade};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (auto& b : c->scratch)
        if (b.p) (void)hipFree(b.p);
    for (hipEvent_t e : c->kev) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->evb0) (void)hipEventDestroy(c->evb0);
    if (c->evb1) (void)hipEventDestroy(c->evb1);
    if (c->ev_model) (void)hipEventDestroy(c->ev_model);
    if (c->ev_tb0) (void)hipEventDestroy(c->ev_tb0);
    if (c->ev_tb1) (void)hipEventDestroy(c->ev_tb1);
    if (c->ev_t0) (void)hipEventDestroy(c->ev_t0);
    if (c->ev_t1) (void)hipEventDestroy(c->ev_t1);
    if (c->ev_rl0) (void)hipEventDestroy(c->ev_rl0);
    if (c->ev_rl1) (void)hipEventDestroy(c->ev_rl1);
    if (c->ev_rm0) (void)hipEventDestroy(c->ev_rm0);
    if (c->ev_rm1) (void)hipEventDestroy(c->ev_rm1);
    if (c->ev_ts0) (void)hipEventDestroy(c->ev_ts0);
    if (c->ev_ts1) (void)hipEventDestroy(c->ev_ts1);
    if (c->ev_gfork) (void)hipEventDestroy(c->ev_gfork);
    if (c->ev_gjoin) (void)hipEventDestroy(c->ev_gjoin);
    if (c->ev_gup) (void)hipEventDestroy(c->ev_gup);
    if (c->ev_bgfork) (void)hipEventDestroy(c->ev_bgfork);
    if (c->ev_bgdone) (void)hipEventDestroy(c->ev_bgdone);
    if (c->bgstream) (void)hipStreamDestroy(c->bgstream);
    for (hipEvent_t e : c->ev_coeff)
        if (e) (void)hipEventDestroy(e);
    if (c->gstream) (void)hipStreamDestroy(c->gstream);
    if (c->h_model_p) (void)hipHostFree(c->h_model_p);
    if (c->ev_leaves) (void)hipEventDestroy(c->ev_leaves);
    if (c->h_leaves_p) (void)hipHostFree(c->h_leaves_p);
    if (c->ev_clade) (void)hipEventDestroy(c->ev_clade);
    if (c->h_clade_p) (void)hipHostFree(c->h_clade_p);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return PHYLO_OK;
}

int phylo_site_tile(int S) { return pm_site_tile(S); }

int phylo_get_site_tile(const phylo_ctx* c) { return c ? c->site_tile : 0; }

int phylo_set_site_tile(phylo_ctx* c, int T) {
    CHK(bind(c));
    if (T < 0 || (T & 63) || T > PK_MAX_SITE_TILE)
        return fail(c, PHYLO_EINVAL, "the site tile must be a multiple of 64 in [64, %d], or 0 for the default (got %d)", PK_MAX_SITE_TILE, T);
    if (c->comm.transport != 0) return fail(c, PHYLO_ESTATE, "phylo_set_site_tile must precede phylo_comm_init (peers map the sweep state)");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tile_override = T;
    c->site_tile = T ? T : pm_site_tile(c->S);
    c->ntiles = (c->S + c->site_tile - 1) / c->site_tile;
    free_sweep_state(c);                                   // tile values, leaf log-likelihoods: rebuilt by the next sweep
    c->state_ready = false;
    c->swept = false; ++c->sweep_serial;
    c->ts_done = c->tb_done = false;                       // the summary's tables belong to the dropped sweep: their fetches refuse too
    return PHYLO_OK;
}

int phylo_set_leaves(phylo_ctx* c, const double* genome) {
    CHK(bind(c));
    if (!genome) return fail(c, PHYLO_EINVAL, "genome_NxSxA is NULL");
    // The rows, their 1-byte codes and the codes' packed image (phylo_packed_codes.h; codes and image are one buffer and one copy) go
    // up from a pinned image that outlives the call, on the context's stream: the call does not
    // wait for the device (a training step on site minibatches sets new leaves every time).  Only a previous upload still in
    // flight has to be over before the image is overwritten.
    const size_t rows = (size_t)c->N * c->S;
    const size_t code_bytes = pk_leaf_image_bytes(c->N, c->S);
    const bool pinned = rows * 32 + code_bytes <= ((size_t)8 << 20);     // (a large alignment goes up straight from the caller's buffer, and waits)
    std::vector<uint8_t> codes_v;
    uint8_t* codes = nullptr;
    if (pinned) {
        if (!c->h_leaves_p) {
            HIPCHK(c, hipHostMalloc((void**)&c->h_leaves_p, rows * 32 + code_bytes));
            HIPCHK(c, hipEventCreateWithFlags(&c->ev_leaves, hipEventDisableTiming));
        } else {
            HIPCHK(c, hipEventSynchronize(c->ev_leaves));
        }
        memcpy(c->h_leaves_p, genome, rows * 32);
        HIPCHK(c, hipMemcpyAsync(c->d_leaves, c->h_leaves_p, rows * 32, hipMemcpyHostToDevice, c->stream));
        codes = (uint8_t*)c->h_leaves_p + rows * 32;
    } else {
        HIPCHK(c, hipMemcpyAsync(c->d_leaves, genome, rows * 32, hipMemcpyHostToDevice, c->stream));
        codes_v.resize(code_bytes);
        codes = codes_v.data();
    }
    // one-hot / all-ones rows (the reference's encoding, runner.py:83-96) also get a 1-byte code per site
    {
        bool ok = true;
        for (size_t i = 0; i < rows && ok; ++i) {
            const double* x = genome + i * 4;
            int ones = 0, zeros = 0, last = 0;
            for (int j = 0; j < 4; ++j) {
                if (pm_bits(x[j]) == pm_bits(1.0)) { ++ones; last = j; }
                else if (pm_bits(x[j]) == 0) ++zeros;
            }
            if (ones == 1 && zeros == 3) codes[i] = (uint8_t)last;
            else if (ones == 4) codes[i] = 4;
            else ok = false;
        }
        c->codes_valid = ok;                                  // a property of the data (the twisting contract uses it)
        c->leaves_coded = ok && !c->env.no_leaf_codes;   // the access-path optimisation can be switched off
        c->hist_ready = false;
        c->pat_U = 0;
        c->clade_ready = false;
        if (ok) {
            pk_pack_leaf_codes(codes, c->N, c->S, codes + pk_packed_offset(c->N, c->S));
            // the site-pattern tables go up only where a launch can read them (U within the table's cap)
            std::vector<int32_t> pat, rep;
            c->pat_U = pk_pat_build(codes, c->N, c->S, codes + pk_pat_offset(c->N, c->S), pat, rep);
            const size_t up_bytes = c->pat_U <= PK_PAT_MAX_U ? code_bytes : pk_codes_image_bytes(c->N, c->S);
            HIPCHK(c, hipMemcpyAsync(c->d_leaf_codes, codes, up_bytes, hipMemcpyHostToDevice, c->stream));
            // the clade tables, where the rule takes them (the site tile may still change: the sweep's plan asks pat_on again)
            if (pk_clade_take(pk_pat_take(c->S, c->pat_U, c->leaves_coded, 1, c->env.site_patterns), c->N, c->S, c->pat_U, c->env.clade_patterns)) {
                const pk_clade_layout L = pk_clade_layout_of(c->N, c->S, c->pat_U);
                if (L.total > c->clade_cap) {
                    if (c->d_clade) HIPCHK(c, hipFree(c->d_clade));
                    if (c->h_clade_p) HIPCHK(c, hipHostFree(c->h_clade_p));
                    c->d_clade = nullptr; c->h_clade_p = nullptr; c->clade_cap = 0;
                    HIPCHK(c, hipMalloc((void**)&c->d_clade, L.total));
                    HIPCHK(c, hipHostMalloc((void**)&c->h_clade_p, L.total));
                    c->clade_cap = L.total;
                }
                if (!c->ev_clade) HIPCHK(c, hipEventCreateWithFlags(&c->ev_clade, hipEventDisableTiming));
                else HIPCHK(c, hipEventSynchronize(c->ev_clade));
                pk_clade_build(codes, c->N, c->S, pat.data(), rep.data(), c->pat_U, c->h_clade_p, nullptr);
                HIPCHK(c, hipMemcpyAsync(c->d_clade, c->h_clade_p, L.total, hipMemcpyHostToDevice, c->stream));
                HIPCHK(c, hipEventRecord(c->ev_clade, c->stream));
                c->clade_layout = L;
                c->clade_ready = true;
            }
        }
    }
    if (pinned) HIPCHK(c, hipEventRecord(c->ev_leaves, c->stream));
    c->have_leaves = true;
    c->last_graph = c->last_graph_twist = false;           // ... and to the leaves
    c->leaves_newer = true;                                // ... and so do the nodes phylo_sweep_node would still have to write
    CHK(refresh_leaf_ll(c));
    if (!pinned) HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

int phylo_set_model(phylo_ctx* c, const double* Q16, const double* pi4, const double* lam_l, const double* lam_r,
                    int jc69_closed_form) {
    CHK(bind(c));
    if (!Q16 || !pi4 || !lam_l || !lam_r) return fail(c, PHYLO_EINVAL, "NULL model pointer");
    const int R = c->N - 1;
    for (int i = 0; i < R; ++i)
        if (!(lam_l[i] > 0.0) || !(lam_r[i] > 0.0)) return fail(c, PHYLO_EINVAL, "branch rates must be positive");
    c->h_lam_l.assign(lam_l, lam_l + R);
    c->h_lam_r.assign(lam_r, lam_r + R);
    c->jc = jc69_closed_form ? 1 : 0;
    c->q_norm1 = pt2_q_norm1(Q16);
    // one upload for the 42 numbers, from a pinned image that outlives the call: everything that uses the model is ordered
    // behind it on the context's stream, so the call does not wait (a training step sets a new model every time).  Only a
    // previous upload still in flight has to be over before the image is overwritten.
    const size_t npack = 20 + 2 * (size_t)c->N;
    if (!c->h_model_p) {
        HIPCHK(c, hipHostMalloc((void**)&c->h_model_p, npack * 8));
        HIPCHK(c, hipEventCreateWithFlags(&c->ev_model, hipEventDisableTiming));
    } else {
        HIPCHK(c, hipEventSynchronize(c->ev_model));
    }
    double* pack = c->h_model_p;
    memset(pack, 0, npack * 8);
    memcpy(pack, Q16, 16 * 8);
    memcpy(pack + 16, pi4, 4 * 8);
    memcpy(pack + 20, lam_l, (size_t)R * 8);
    memcpy(pack + 20 + c->N, lam_r, (size_t)R * 8);
    HIPCHK(c, hipMemcpyAsync(c->d_Q, pack, npack * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_model, c->stream));
    c->have_model = true;
    c->last_graph = c->last_graph_twist = false;           // a kept graph belongs to the model it was swept with
    CHK(refresh_leaf_ll(c));
    return PHYLO_OK;
}

// The 1-norm pt2_check_expm_range holds a call's lengths against: that of the model in force, or 0 (no limit) under the JC69 closed
// form, which is right at every length
static double expm_range_norm(const phylo_ctx* c) { return c->jc ? 0.0 : c->q_norm1; }

// The 2 (N-1) lengths of each of the T trees at every rate of its mixture (tree t's: rate + t * mix_stride; a plain call passes C =
// 1 and the rate 1.0), before anything is queued and after every tree went through the call's other checks: what those refuse (no
// tree, a length or scaled length that is not finite) is named first, whichever tree it is in.
static int check_trees_expm_range(phylo_ctx* c, int T, int R, const double* blen, int C, const double* rate, size_t mix_stride, bool mix) {
    const double qn = expm_range_norm(c);
    if (qn == 0.0) return PHYLO_OK;
    char msg[240];
    int bad = 0;
    for (int t = 0; t < T; ++t)
        for (int k = 0; k < C; ++k)
            if (pt2_check_expm_range(qn, 2 * R, blen + (size_t)t * R * 2, rate[t * mix_stride + k], &bad, msg, sizeof msg)) {
                if (mix) return fail(c, PHYLO_EINVAL, "tree %d, row %d, category %d: %s", t, bad / 2, k, msg);
                return fail(c, PHYLO_EINVAL, "tree %d, row %d: %s", t, bad / 2, msg);
            }
    return PHYLO_OK;
}
static const double expm_rate_one = 1.0;

// ---- the stages of a scored-tree-set call ---------------------------------------------------------------
// The nine entry points (phylo_trees_loglik .. phylo_trees_nni_rates) each keep their own loop over the chunks and own what is
// theirs: argument struct, kernel, finish kernel, downloads.  What they share is below, one stage a function, and trees_call is
// what the stages of one call hand on to one another.  A stage returns its status; the entry point returns early on it (CHK), so an
// error exit leaves queued what it always left queued.
struct trees_call {
    phylo_ctx* c = nullptr;
    int N = 0, R = 0, S = 0, ntiles = 0, T = 0;
    bool coded = false;
    const int32_t* child = nullptr;
    const double *blen = nullptr, *prior4 = nullptr;
    int C = 1;                                              // sets of lengths per tree
    const double *rate = nullptr, *weight = nullptr;        // rate NULL: a plain call, every tree's own lengths
    size_t mix_stride = 0;                                  // tree t's mixture: row t, or the one row
    // the slab: what every call carves (trees_carve) and what some do (d_dops, d_nops, d_b: NULL is neither built nor uploaded)
    char* base = nullptr;
    int chunk = 0;
    double *d_prior = nullptr, *d_P = nullptr, *d_t = nullptr, *d_gap = nullptr, *d_tilev = nullptr, *d_out = nullptr, *d_b = nullptr;
    int32_t *d_ops = nullptr, *d_dops = nullptr, *d_nops = nullptr;
    const double* prior = nullptr;                          // the prior the kernels read: the caller's in the slab, or the model's
    std::vector<int32_t> ops, dops, nops;                   // the chunk on the host, in the slab's layouts
    std::vector<double> ts, bs;
    int n = 0, depth = 1;                                   // the chunk in flight: trees, deepest schedule, matrices
    long n_mat = 0;
    double ms_total = 0.0;
    int launches = 0;
};

static int trees_cus(const phylo_ctx* c) { return c->n_cus > 0 ? c->n_cus : 1; }

// Front, part one: the refusals every call opens with.  C and per_tree: NULL where the call has none.
static int trees_front(phylo_ctx* c, const char* who, int T, const int* C, const int* per_tree) {
    CHK(bind(c));
    if (!c->have_leaves || !c->have_model) return fail(c, PHYLO_ESTATE, "%s needs phylo_set_leaves and phylo_set_model first", who);
    if (T < 1) return fail(c, PHYLO_EINVAL, "need T >= 1 trees (T=%d)", T);
    if (C && (*C < 1 || *C > PT2_MAX_CATS)) return fail(c, PHYLO_EINVAL, "need 1 <= C <= %d rate categories (C=%d)", PT2_MAX_CATS, *C);
    if (per_tree && *per_tree != 0 && *per_tree != 1) return fail(c, PHYLO_EINVAL, "%s: per_tree must be 0 or 1 (per_tree=%d)", who, *per_tree);
    return PHYLO_OK;
}

static trees_call trees_open(phylo_ctx* c, int T, const int32_t* child, const double* blen, const double* prior4) {
    trees_call tc;
    tc.c = c; tc.N = c->N; tc.R = c->N - 1; tc.S = c->S; tc.ntiles = c->ntiles; tc.T = T;
    tc.coded = c->leaves_coded;
    tc.child = child; tc.blen = blen; tc.prior4 = prior4;
    return tc;
}

static void trees_mixture(trees_call& tc, int C, const double* rate, const double* weight, int per_tree) {
    tc.C = C; tc.rate = rate; tc.weight = weight;
    tc.mix_stride = per_tree ? (size_t)C : 0;
}

// Front, part two, after the call's own NULL-pointer refusals: every tree (and its mixture) is checked before anything is queued,
// then every length against the domain of the matrix exponential
static int trees_check(const trees_call& tc) {
    const size_t R2 = (size_t)tc.R * 2;
    for (int t = 0; t < tc.T; ++t) {
        int row = 0;
        char msg[200];
        if (pt2_check_tree(tc.N, tc.child + t * R2, tc.blen + t * R2, &row, msg, sizeof msg))
            return fail(tc.c, PHYLO_EINVAL, "tree %d, row %d: %s", t, row, msg);
        if (tc.rate && ptgr_check_mixture(tc.N, tc.blen + t * R2, tc.C, tc.rate + t * tc.mix_stride, tc.weight + t * tc.mix_stride, msg, sizeof msg))
            return fail(tc.c, PHYLO_EINVAL, "tree %d: %s", t, msg);
    }
    if (!tc.rate) return check_trees_expm_range(tc.c, tc.T, tc.R, tc.blen, 1, &expm_rate_one, 0, false);
    return check_trees_expm_range(tc.c, tc.T, tc.R, tc.blen, tc.C, tc.rate, tc.mix_stride, true);
}

// the pointers every call carves from its slab; Plan: any plan of the family
extern "C++" template <class Plan>
static void trees_carve(trees_call& tc, void* slab, const Plan& pl) {
    char* base = (char*)slab;
    tc.base = base;
    tc.chunk = pl.chunk;
    tc.d_prior = (double*)(base + pl.o_prior);
    tc.d_ops = (int32_t*)(base + pl.o_ops);
    tc.d_P = (double*)(base + pl.o_P);
    tc.d_t = (double*)(base + pl.o_t);
    tc.d_gap = tc.coded ? (double*)(base + pl.o_gap) : nullptr;
    tc.d_tilev = (double*)(base + pl.o_tilev);
    tc.d_out = (double*)(base + pl.o_out);
}

// Before the first chunk: the family's one event pair (no two calls of a context overlap: each ends in a stream synchronise and a
// context is one thread's), the caller's prior, the chunk's host buffers
static int trees_begin(trees_call& tc) {
    phylo_ctx* c = tc.c;
    if (!c->ev_t0) {
        HIPCHK(c, hipEventCreate(&c->ev_t0));
        HIPCHK(c, hipEventCreate(&c->ev_t1));
    }
    if (tc.prior4) HIPCHK(c, hipMemcpyAsync(tc.d_prior, tc.prior4, 32, hipMemcpyHostToDevice, c->stream));
    tc.prior = tc.prior4 ? tc.d_prior : c->d_pi;
    const size_t rows = (size_t)tc.chunk * tc.R;
    tc.ops.resize(rows * 4);
    if (tc.d_dops) tc.dops.resize(rows * 4);                // (the optional pointers are set by the call between trees_carve and here)
    if (tc.d_nops) tc.nops.resize(rows * 4);
    tc.ts.resize(rows * tc.C * 2);
    if (tc.d_b) tc.bs.resize(rows * 2);
    return PHYLO_OK;
}

// Chunk host stage, trees t0 .. t0 + n: one schedule per tree (and its downward and NNI operations), every set of lengths in the
// schedule's order -- gathered once, then rate * length, one rounded product, per category where the call has rates -- and the
// deepest schedule
static int trees_chunk_host(trees_call& tc, int t0) {
    // (locals, not members read through tc inside the loop: the per-tree loop is a measurable part of a small call's wall time)
    const int N = tc.N, R = tc.R, C = tc.C, n = std::min(tc.chunk, tc.T - t0);
    int32_t* const ops = tc.ops.data();
    int32_t* const dops = tc.d_dops ? tc.dops.data() : nullptr;
    int32_t* const nops = tc.d_nops ? tc.nops.data() : nullptr;
    double* const ts = tc.ts.data();
    double* const bs = tc.d_b ? tc.bs.data() : nullptr;
    const double* const rate = tc.rate;
    int depth = 1;
    for (int t = 0; t < n; ++t) {
        int32_t* o = ops + (size_t)t * R * 4;
        int32_t* d = dops ? dops + (size_t)t * R * 4 : nullptr;
        const int32_t* ch = tc.child + (size_t)(t0 + t) * R * 2;
        depth = std::max(depth, pt2_schedule(N, ch, o));
        if ((d && ptg_down_ops(N, ch, o, d)) || (nops && ptn_nni_ops(N, o, d, nops + (size_t)t * R * 4)))
            return fail(tc.c, PHYLO_EINVAL, "tree %d: its schedule and its rows do not fit one another", t0 + t);
        const double* b = tc.blen + (size_t)(t0 + t) * R * 2;
        double* tk = ts + (size_t)t * C * R * 2;
        double* bk = bs ? bs + (size_t)t * R * 2 : tk;      // the tree's own lengths, gathered once: into the first set where no row of theirs is uploaded
        for (int i = 0; i < R; ++i) {
            bk[2 * i] = b[2 * o[4 * i + 3]];
            bk[2 * i + 1] = b[2 * o[4 * i + 3] + 1];
        }
        if (rate) {
            const double* rt = rate + (t0 + t) * tc.mix_stride;
            for (int k = 1; k < C; ++k) {
                double* q = tk + (size_t)k * R * 2;
                for (int i = 0; i < 2 * R; ++i) q[i] = rt[k] * bk[i];
            }
            for (int i = 0; i < 2 * R; ++i) tk[i] = rt[0] * bk[i];      // the first set last: it may be the gathered row itself
        } else if (bs) memcpy(tk, bk, (size_t)R * 16);
    }
    tc.n = n;
    tc.depth = depth;
    tc.n_mat = (long)n * C * R * 2;
    if (depth > PT2_MAX_DEPTH) return fail(tc.c, PHYLO_EINVAL, "a schedule of %d slots exceeds %d", depth, PT2_MAX_DEPTH);
    return PHYLO_OK;
}

// Chunk device prologue: the uploads of what the host stage built (the call's own uploads follow), ...
static int trees_chunk_upload(trees_call& tc) {
    phylo_ctx* c = tc.c;
    const size_t rows = (size_t)tc.n * tc.R * 16;
    HIPCHK(c, hipMemcpyAsync(tc.d_ops, tc.ops.data(), rows, hipMemcpyHostToDevice, c->stream));
    if (tc.d_dops) HIPCHK(c, hipMemcpyAsync(tc.d_dops, tc.dops.data(), rows, hipMemcpyHostToDevice, c->stream));
    if (tc.d_nops) HIPCHK(c, hipMemcpyAsync(tc.d_nops, tc.nops.data(), rows, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tc.d_t, tc.ts.data(), rows * tc.C, hipMemcpyHostToDevice, c->stream));
    if (tc.d_b) HIPCHK(c, hipMemcpyAsync(tc.d_b, tc.bs.data(), rows, hipMemcpyHostToDevice, c->stream));
    return PHYLO_OK;
}

// ... the start event and every matrix of the chunk (the call's own ptg_dmats / ptm_dirmats follow), ...
static int trees_chunk_expm(trees_call& tc) {
    phylo_ctx* c = tc.c;
    HIPCHK(c, hipEventRecord(c->ev_t0, c->stream));
    hipLaunchKernelGGL(pk_expm_batched, dim3(cdiv(tc.n_mat, 64)), dim3(64), 0, c->stream, c->d_Q, (const double*)tc.d_t, (int)tc.n_mat, c->jc, tc.d_P);
    CHK(launch_check(c, "pk_expm_batched"));
    ++tc.launches;
    return PHYLO_OK;
}

// ... and the gap rows of the matrices M where the leaves are coded
static int trees_chunk_gap_rows(trees_call& tc) {
    if (!tc.coded) return PHYLO_OK;
    phylo_ctx* c = tc.c;
    hipLaunchKernelGGL(pt2_gap_rows, dim3(cdiv(tc.n_mat * 4, 256)), dim3(256), 0, c->stream, (const double*)tc.d_P, tc.n_mat, tc.d_gap);
    CHK(launch_check(c, "pt2_gap_rows"));
    ++tc.launches;
    return PHYLO_OK;
}

// the arguments every kernel of the family starts with (site_lik: the loglik calls set their own)
static void trees_args(const trees_call& tc, pt2_args& a) {
    const phylo_ctx* c = tc.c;
    a.ops = tc.d_ops; a.P = tc.d_P; a.gap = tc.d_gap; a.leaves = c->d_leaves; a.codes = c->d_leaf_codes;
    a.prior = tc.prior;
    a.tilev = tc.d_tilev; a.site_lik = nullptr;
    a.N = tc.N; a.S = tc.S; a.T = c->site_tile; a.ntiles = tc.ntiles;
}

// Chunk epilogue: every tree's tile values added (the call's own finish kernels follow), ...
static int trees_chunk_finish(trees_call& tc) {
    phylo_ctx* c = tc.c;
    hipLaunchKernelGGL(pt2_finish, dim3(cdiv(tc.n, 256)), dim3(256), 0, c->stream, (const double*)tc.d_tilev, tc.ntiles, tc.n, tc.d_out);
    CHK(launch_check(c, "pt2_finish"));
    ++tc.launches;
    return PHYLO_OK;
}

// ... the stop event and the log-likelihoods (the call's own downloads follow), ...
static int trees_chunk_stop(trees_call& tc, double* loglik_chunk) {
    phylo_ctx* c = tc.c;
    HIPCHK(c, hipEventRecord(c->ev_t1, c->stream));
    HIPCHK(c, hipMemcpyAsync(loglik_chunk, tc.d_out, (size_t)tc.n * 8, hipMemcpyDeviceToHost, c->stream));
    return PHYLO_OK;
}

// ... and the wait: the chunk's host and device buffers are reused by the next one
static int trees_chunk_end(trees_call& tc) {
    phylo_ctx* c = tc.c;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev_t0, c->ev_t1));
    tc.ms_total += ms;
    return PHYLO_OK;
}

static void trees_stats(const trees_call& tc, phylo_stats* perf, double units, double alg_bytes) {
    if (!perf) return;
    phylo_stats st{};
    st.sweep_ms = tc.ms_total;
    st.n_launches = tc.launches;
    st.units = units;
    st.alg_bytes = alg_bytes;
    *perf = st;
}

int phylo_expm_batched(phylo_ctx* c, const double* t, int n, double* P) {
    CHK(bind(c));
    if (!c->have_model) return fail(c, PHYLO_ESTATE, "phylo_set_model has not been called");
    if (n < 0 || (n > 0 && (!t || !P))) return fail(c, PHYLO_EINVAL, "bad arguments to phylo_expm_batched");
    if (n == 0) return PHYLO_OK;
    {
        char msg[240];
        int bad = 0;
        if (pt2_check_expm_range(expm_range_norm(c), n, t, 1.0, &bad, msg, sizeof msg))
            return fail(c, PHYLO_EINVAL, "phylo_expm_batched: t[%d]: %s", bad, msg);
    }
    void *dt, *dP;
    CHK(scratch_get(c, 0, (size_t)n * 8, &dt));
    CHK(scratch_get(c, 1, (size_t)n * 16 * 8, &dP));
    HIPCHK(c, hipMemcpyAsync(dt, t, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pk_expm_batched, dim3(cdiv(n, 64)), dim3(64), 0, c->stream, c->d_Q, (const double*)dt, n, c->jc,
                       (double*)dP);
    CHK(launch_check(c, "pk_expm_batched"));
    HIPCHK(c, hipMemcpyAsync(P, dP, (size_t)n * 16 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

int phylo_cond_likelihood_K(phylo_ctx* c, const double* l, const double* r, const double* tl, const double* tr, int K,
                            int S, double* out) {
    CHK(bind(c));
    if (!c->have_model) return fail(c, PHYLO_ESTATE, "phylo_set_model has not been called");
    if (K < 0 || S < 0) return fail(c, PHYLO_EINVAL, "negative shape");
    if (K == 0 || S == 0) return PHYLO_OK;
    if (!l || !r || !tl || !tr || !out) return fail(c, PHYLO_EINVAL, "NULL pointer");
    const size_t nb = (size_t)K * S * 4 * 8;
    void *dl, *dr, *dt, *dP, *dout;
    CHK(scratch_get(c, 0, nb, &dl));
    CHK(scratch_get(c, 1, nb, &dr));
    CHK(scratch_get(c, 2, (size_t)2 * K * 8, &dt));
    CHK(scratch_get(c, 3, (size_t)2 * K * 16 * 8, &dP));
    CHK(scratch_get(c, 4, nb, &dout));
    HIPCHK(c, hipMemcpyAsync(dl, l, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dr, r, nb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dt, tl, (size_t)K * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync((double*)dt + K, tr, (size_t)K * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pk_expm_batched, dim3(cdiv(2 * K, 64)), dim3(64), 0, c->stream, c->d_Q, (const double*)dt, 2 * K,
                       c->jc, (double*)dP);
    CHK(launch_check(c, "pk_expm_batched"));
    hipLaunchKernelGGL(pk_merge_api, dim3(K), dim3(PK_COLS), 0, c->stream, (const double*)dl, (const double*)dr,
                       (const double*)dP, K, S, (double*)dout);
    CHK(launch_check(c, "pk_merge_api"));
    HIPCHK(c, hipMemcpyAsync(out, dout, nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

int phylo_forest_loglik(phylo_ctx* c, const double* core, const int32_t* record, int K, int X, int S, double* out) {
    CHK(bind(c));
    if (!c->have_model) return fail(c, PHYLO_ESTATE, "phylo_set_model has not been called");
    if (K < 0 || X < 0 || S < 0) return fail(c, PHYLO_EINVAL, "negative shape");
    if (K == 0) return PHYLO_OK;
    if (!out || (X > 0 && (!core || !record))) return fail(c, PHYLO_EINVAL, "NULL pointer");
    const size_t rows = (size_t)K * X;
    void *dcore, *drec, *drow, *dout;
    CHK(scratch_get(c, 0, rows * S * 4 * 8, &dcore));
    CHK(scratch_get(c, 1, rows * 4, &drec));
    CHK(scratch_get(c, 2, rows * 8, &drow));
    CHK(scratch_get(c, 3, (size_t)K * 8, &dout));
    if (rows) {
        HIPCHK(c, hipMemcpyAsync(dcore, core, rows * S * 4 * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(drec, record, rows * 4, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(pk_row_loglik, dim3((unsigned)rows), dim3(64), 0, c->stream, (const double*)dcore, c->d_pi, S, tile_for(c, S),
                           (double*)drow);
        CHK(launch_check(c, "pk_row_loglik"));
    }
    hipLaunchKernelGGL(pk_forest_tail, dim3(cdiv(K, 256)), dim3(256), 0, c->stream, (const double*)drow,
                       (const int32_t*)drec, c->d_ldf, c->N, K, X, (double*)dout);
    CHK(launch_check(c, "pk_forest_tail"));
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)K * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

int phylo_tree_loglik(phylo_ctx* c, int n_nodes, int n_leaves, int S, const int32_t* left, const int32_t* right,
                      const double* bl, const double* br, int root, const double* leaves, const double* prior4,
                      double* out_loglik, double* root_data) {
    CHK(bind(c));
    if (!c->have_model) return fail(c, PHYLO_ESTATE, "phylo_set_model has not been called (Q is needed)");
    if (n_leaves < 1 || n_nodes < n_leaves || S < 1 || root < 0 || root >= n_nodes)
        return fail(c, PHYLO_EINVAL, "bad tree sizes (n_nodes=%d n_leaves=%d S=%d root=%d)", n_nodes, n_leaves, S, root);
    if (!leaves || !prior4 || !out_loglik || (n_nodes > n_leaves && (!left || !right || !bl || !br)))
        return fail(c, PHYLO_EINVAL, "NULL pointer");
    // children-before-parents order of the internal nodes reachable from root (csmc.py:259-298)
    std::vector<int32_t> order;
    std::vector<double> ts;
    {
        std::vector<char> state((size_t)n_nodes, 0);
        std::vector<int> stack{root};
        while (!stack.empty()) {
            const int v = stack.back();
            if (v < n_leaves) { stack.pop_back(); continue; }
            const int lc = left[v], rc = right[v];
            if (lc < 0 || lc >= n_nodes || rc < 0 || rc >= n_nodes || lc == v || rc == v)
                return fail(c, PHYLO_EINVAL, "node %d has invalid children (%d, %d)", v, lc, rc);
            if (state[v] == 0) {
                state[v] = 1;
                stack.push_back(lc);
                stack.push_back(rc);
            } else {
                stack.pop_back();
                if (state[v] == 1) {
                    state[v] = 2;
                    order.push_back(v); order.push_back(lc); order.push_back(rc);
                    ts.push_back(bl[v]); ts.push_back(br[v]);
                }
            }
            if ((int)stack.size() > 4 * n_nodes + 8) return fail(c, PHYLO_EINVAL, "tree contains a cycle");
        }
    }
    const int n_int = (int)(order.size() / 3);
    {   // the lengths above the children of the reachable internal nodes, in pruning order (row = that node)
        char msg[240];
        int bad = 0;
        if (pt2_check_expm_range(expm_range_norm(c), (int)ts.size(), ts.data(), 1.0, &bad, msg, sizeof msg))
            return fail(c, PHYLO_EINVAL, "tree 0, row %d: %s", (int)order[3 * (size_t)(bad / 2)], msg);
    }
    void *dnodes, *dorder, *dt, *dP, *dpr, *dout;
    CHK(scratch_get(c, 0, (size_t)n_nodes * S * 4 * 8, &dnodes));
    CHK(scratch_get(c, 1, (size_t)(n_int ? n_int : 1) * 3 * 4, &dorder));
    CHK(scratch_get(c, 2, (size_t)(n_int ? n_int : 1) * 2 * 8, &dt));
    CHK(scratch_get(c, 3, (size_t)(n_int ? n_int : 1) * 2 * 16 * 8, &dP));
    CHK(scratch_get(c, 4, 4 * 8, &dpr));
    CHK(scratch_get(c, 5, 8, &dout));
    HIPCHK(c, hipMemcpyAsync(dnodes, leaves, (size_t)n_leaves * S * 4 * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dpr, prior4, 4 * 8, hipMemcpyHostToDevice, c->stream));
    if (n_int) {
        HIPCHK(c, hipMemcpyAsync(dorder, order.data(), order.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dt, ts.data(), ts.size() * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(pk_expm_batched, dim3(cdiv(2 * n_int, 64)), dim3(64), 0, c->stream, c->d_Q, (const double*)dt,
                           2 * n_int, c->jc, (double*)dP);
        CHK(launch_check(c, "pk_expm_batched"));
        hipLaunchKernelGGL(pk_tree_prune, dim3(cdiv(S, 256)), dim3(256), 0, c->stream, (double*)dnodes,
                           (const int32_t*)dorder, n_int, (const double*)dP, S);
        CHK(launch_check(c, "pk_tree_prune"));
    }
    const double* droot = (const double*)dnodes + (size_t)root * S * 4;
    hipLaunchKernelGGL(pk_row_loglik, dim3(1), dim3(64), 0, c->stream, droot, (const double*)dpr, S, tile_for(c, S), (double*)dout);
    CHK(launch_check(c, "pk_row_loglik"));
    HIPCHK(c, hipMemcpyAsync(out_loglik, dout, 8, hipMemcpyDeviceToHost, c->stream));
    if (root_data) HIPCHK(c, hipMemcpyAsync(root_data, droot, (size_t)S * 4 * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

// phylo_trees_loglik (mix false: one set of matrices per tree, pt2_prune) and phylo_trees_loglik_rates (mix true, C rate categories:
// C sets of lengths, matrices and gap rows per tree behind ONE schedule, pt2_prune_rates)
static int trees_loglik_run(phylo_ctx* c, const char* who, int T, const int32_t* child, const double* blen, bool mix, int C, const double* rate_C,
                            const double* weight_C, const double* prior4, double* loglik_T, double* site_lik_TxS,
                            double* cat_lik_TxCxS, phylo_stats* perf) {
    CHK(trees_front(c, who, T, mix ? &C : nullptr, nullptr));
    if (!child || !blen || !loglik_T || (mix && (!rate_C || !weight_C))) return fail(c, PHYLO_EINVAL, "NULL pointer");
    const int nc = mix ? C : 1;                             // sets of lengths per tree; the plain call's set is the tree's own
    for (int k = 0; mix && k < C; ++k) {
        if (!(rate_C[k] >= 0.0) || !std::isfinite(rate_C[k]))
            return fail(c, PHYLO_EINVAL, "rate %g of category %d is not a finite number >= 0", rate_C[k], k);
        if (!(weight_C[k] >= 0.0) || !std::isfinite(weight_C[k]))
            return fail(c, PHYLO_EINVAL, "weight %g of category %d is not a finite number >= 0", weight_C[k], k);
    }
    trees_call tc = trees_open(c, T, child, blen, prior4);
    if (mix) trees_mixture(tc, C, rate_C, weight_C, 0);
    const int N = tc.N, R = tc.R, S = tc.S;
    std::vector<int> need, depth_of(mix ? (size_t)T : 0);   // (rates call) every tree's depth: can a chunk take four site steps?
    for (int t = 0; t < T; ++t) {                          // every tree (and every scaled length) is checked before anything is queued
        int row = 0;
        char msg[200];
        const double* b = blen + (size_t)t * R * 2;
        if (pt2_check_tree(N, child + (size_t)t * R * 2, b, &row, msg, sizeof msg))
            return fail(c, PHYLO_EINVAL, "tree %d, row %d: %s", t, row, msg);
        if (mix) {
            pt2_needs(N, child + (size_t)t * R * 2, need);
            depth_of[t] = need[R - 1];
        }
        for (int k = 0; mix && k < C; ++k)
            for (int i = 0; i < 2 * R; ++i)
                if (!std::isfinite(rate_C[k] * b[i]))
                    return fail(c, PHYLO_EINVAL, "tree %d, row %d, category %d: branch length %g at rate %g is not finite", t, i / 2, k,
                                b[i], rate_C[k]);
    }
    CHK(check_trees_expm_range(c, T, R, blen, nc, mix ? rate_C : &expm_rate_one, 0, mix));
    pt2_plan pl;
    if (pt2_make_plan(N, S, tc.ntiles, T, nc, mix, tc.coded, site_lik_TxS != nullptr, cat_lik_TxCxS != nullptr, c->env.trees_chunk,
                      mix ? depth_of.data() : nullptr, &pl))
        return fail(c, PHYLO_EINVAL, "%s: no plan for N=%d, S=%d, %d tiles, T=%d", who, N, S, tc.ntiles, T);   // (unreachable: a context has N >= 2, S >= 1, tiles >= 1, and T, C were checked above)
    void* slab = nullptr;
    CHK(scratch_get(c, 14, pl.total, &slab));
    trees_carve(tc, slab, pl);
    double* d_site = pl.sites ? (double*)(tc.base + pl.o_site) : nullptr;
    double* d_cat = cat_lik_TxCxS ? (double*)(tc.base + pl.o_cat) : nullptr;
    CHK(trees_begin(tc));
    if (mix) {                                              // the prior, then the weights: one pointer for pt2_prune_rates
        if (!prior4) HIPCHK(c, hipMemcpyAsync(tc.d_prior, c->d_pi, 32, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(tc.d_prior + 4, weight_C, (size_t)C * 8, hipMemcpyHostToDevice, c->stream));
        tc.prior = tc.d_prior;
    }
    for (int t0 = 0; t0 < T; t0 += tc.chunk) {
        CHK(trees_chunk_host(tc, t0));
        const int n = tc.n;
        if (mix && !d_site && pt2_unroll(tc.depth) == 4)    // (never: pt2_make_plan looked at the chunks, by pt2_needs' depths)
            return fail(c, PHYLO_EINVAL, "a chunk of depth %d without the row of site values its kernel needs", tc.depth);
        CHK(trees_chunk_upload(tc));
        CHK(trees_chunk_expm(tc));
        CHK(trees_chunk_gap_rows(tc));
        pt2_rates_args ra{};
        trees_args(tc, ra.a);
        ra.a.site_lik = d_site;
        ra.cat_lik = d_cat; ra.C = C;
        if (mix) pt2_launch_rates(ra, n, tc.depth, tc.coded, c->stream);
        else pt2_launch(ra.a, n, tc.depth, tc.coded, c->stream);
        CHK(launch_check(c, mix ? "pt2_prune_rates" : "pt2_prune"));
        ++tc.launches;
        CHK(trees_chunk_finish(tc));
        CHK(trees_chunk_stop(tc, loglik_T + t0));
        if (site_lik_TxS) HIPCHK(c, hipMemcpyAsync(site_lik_TxS + (size_t)t0 * S, d_site, (size_t)n * S * 8, hipMemcpyDeviceToHost, c->stream));
        if (d_cat) HIPCHK(c, hipMemcpyAsync(cat_lik_TxCxS + (size_t)t0 * nc * S, d_cat, (size_t)n * nc * S * 8, hipMemcpyDeviceToHost, c->stream));
        CHK(trees_chunk_end(tc));
    }
    const double units = (double)T * S * R * nc;
    trees_stats(tc, perf, units, 96.0 * units);
    return PHYLO_OK;
}

int phylo_trees_loglik(phylo_ctx* c, int T, const int32_t* child, const double* blen, const double* prior4, double* loglik_T,
                       double* site_lik_TxS, phylo_stats* perf) {
    return trees_loglik_run(c, "phylo_trees_loglik", T, child, blen, false, 0, nullptr, nullptr, prior4, loglik_T, site_lik_TxS, nullptr, perf);
}

int phylo_trees_loglik_rates(phylo_ctx* c, int T, const int32_t* child, const double* blen, int C, const double* rate_C,
                             const double* weight_C, const double* prior4, double* loglik_T, double* site_lik_TxS,
                             double* cat_lik_TxCxS, phylo_stats* perf) {
    return trees_loglik_run(c, "phylo_trees_loglik_rates", T, child, blen, true, C, rate_C, weight_C, prior4, loglik_T, site_lik_TxS, cat_lik_TxCxS, perf);
}

int phylo_debug_tree_schedule(int N, const int32_t* child, const double* blen, int32_t* ops, int32_t* depth) {
    if (N < 2 || N > PK_MAX_TAXA || !child || !blen || !ops || !depth) return fail(nullptr, PHYLO_EINVAL, "bad arguments to phylo_debug_tree_schedule");
    int row = 0;
    char msg[200];
    if (pt2_check_tree(N, child, blen, &row, msg, sizeof msg)) return fail(nullptr, PHYLO_EINVAL, "tree 0, row %d: %s", row, msg);
    *depth = pt2_schedule(N, child, ops);
    return PHYLO_OK;
}

// ---- RELL bootstrap over a scored tree set's site factors (phylo_rell.h) ----
int phylo_rell(phylo_ctx* c, int T, int S, const double* site_lik_TxS, int B, uint64_t seed, double* obs_T, int32_t* best_B, int64_t* wins_T,
               double* rep_loglik_TxB, int32_t* counts_BxS, double* site_loglik_TxS, phylo_stats* perf) {
    CHK(bind(c));
    if (!site_lik_TxS || !obs_T || !best_B || !wins_T) return fail(c, PHYLO_EINVAL, "phylo_rell: site_lik, obs, best and wins must be given (NULL pointer)");
    {
        char msg[200];                                     // everything is checked before anything is queued
        if (pr_check_shape(T, S, B, msg, sizeof msg) || pr_check_factors(T, S, site_lik_TxS, msg, sizeof msg))
            return fail(c, PHYLO_EINVAL, "phylo_rell: %s", msg);
    }
    // one slab: logs [T][S] (resident for the call) | counts [chunk + 1][Sp] uint16 | scores [T][chunk + 1] | observed [T] |
    // best [chunk] | wins [T] | flag.  Counts and scores of a chunk of replicates stay within PR_CHUNK_BYTES (while one replicate
    // does); the first chunk carries one more column, the row of ones whose chain is the observed score.
    const size_t Sp = pr_count_stride(S), n_x = (size_t)T * S;
    const size_t per_rep = Sp * 2 + (size_t)T * 8;
    size_t fit = PR_CHUNK_BYTES / per_rep;
    if (fit < 1) fit = 1;
    if (c->env.rell_chunk > 0 && (size_t)c->env.rell_chunk < fit) fit = (size_t)c->env.rell_chunk;
    const int chunk = (int)std::min<size_t>((size_t)B, fit);
    const size_t ldr = (size_t)chunk + 1;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_cnt = up(n_x * 8), o_rl = o_cnt + up(ldr * Sp * 2), o_obs = o_rl + up((size_t)T * ldr * 8), o_best = o_obs + up((size_t)T * 8),
                 o_wins = o_best + up((size_t)chunk * 4), o_flag = o_wins + up((size_t)T * 8), total = o_flag + 256;
    void* slab = nullptr;
    CHK(scratch_get(c, 15, total, &slab));
    char* base = (char*)slab;
    double* d_x = (double*)base;
    uint16_t* d_cnt = (uint16_t*)(base + o_cnt);
    double* d_rl = (double*)(base + o_rl);
    double* d_obs = (double*)(base + o_obs);
    int32_t* d_best = (int32_t*)(base + o_best);
    unsigned long long* d_wins = (unsigned long long*)(base + o_wins);
    unsigned int* d_flag = (unsigned int*)(base + o_flag);
    if (!c->ev_rl0) {
        HIPCHK(c, hipEventCreate(&c->ev_rl0));
        HIPCHK(c, hipEventCreate(&c->ev_rl1));
    }
    HIPCHK(c, hipMemcpyAsync(d_x, site_lik_TxS, n_x * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_wins, 0, (size_t)T * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_flag, 0, 4, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_rl0, c->stream));
    hipLaunchKernelGGL(pr_log, dim3((unsigned)((n_x + 255) / 256)), dim3(256), 0, c->stream, d_x, n_x, d_flag);
    CHK(launch_check(c, "pr_log"));
    HIPCHK(c, hipEventRecord(c->ev_rl1, c->stream));
    unsigned int flag = 0;
    HIPCHK(c, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    if (site_loglik_TxS) HIPCHK(c, hipMemcpyAsync(site_loglik_TxS, d_x, n_x * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (flag) return fail(c, PHYLO_EINVAL, "phylo_rell: the device met a site factor that is not a finite number > 0");
    double ms_total = 0.0;
    int launches = 1;
    {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_rl0, c->ev_rl1));
        ms_total += ms;
    }
    std::vector<uint16_t> h_cnt(counts_BxS ? (size_t)chunk * Sp : 0);
    const uint32_t nblk = (uint32_t)(Sp / 4);
    for (int r0 = 0; r0 < B; r0 += chunk) {
        const int n = std::min(chunk, B - r0);
        const int ncols = n + (r0 == 0 ? 1 : 0);
        HIPCHK(c, hipMemsetAsync(d_cnt, 0, (size_t)ncols * Sp * 2, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_rl0, c->stream));
        const size_t n_threads = (size_t)n * nblk;
        hipLaunchKernelGGL(pr_counts, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, c->stream, (unsigned int*)d_cnt, S, Sp, (uint32_t)r0,
                           n_threads, nblk, seed);
        CHK(launch_check(c, "pr_counts"));
        ++launches;
        if (r0 == 0) {
            hipLaunchKernelGGL(pr_ones, dim3(cdiv(S, 256)), dim3(256), 0, c->stream, d_cnt + (size_t)n * Sp, S);
            CHK(launch_check(c, "pr_ones"));
            ++launches;
        }
        hipLaunchKernelGGL(pr_replicates, dim3((unsigned)cdiv(T, PR_TT), (unsigned)cdiv(ncols, PR_TB)), dim3(256), 0, c->stream, (const double*)d_x,
                           (const uint16_t*)d_cnt, T, S, Sp, ncols, d_rl, ldr);
        CHK(launch_check(c, "pr_replicates"));
        hipLaunchKernelGGL(pr_best, dim3(cdiv(n, 64)), dim3(1024), 0, c->stream, (const double*)d_rl, ldr, T, n, d_best, d_wins);
        CHK(launch_check(c, "pr_best"));
        launches += 2;
        if (r0 == 0) {
            hipLaunchKernelGGL(pr_column, dim3(cdiv(T, 256)), dim3(256), 0, c->stream, (const double*)d_rl, ldr, (size_t)n, T, d_obs);
            CHK(launch_check(c, "pr_column"));
            ++launches;
        }
        HIPCHK(c, hipEventRecord(c->ev_rl1, c->stream));
        HIPCHK(c, hipMemcpyAsync(best_B + r0, d_best, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        if (r0 == 0) HIPCHK(c, hipMemcpyAsync(obs_T, d_obs, (size_t)T * 8, hipMemcpyDeviceToHost, c->stream));
        if (rep_loglik_TxB)
            HIPCHK(c, hipMemcpy2DAsync(rep_loglik_TxB + r0, (size_t)B * 8, d_rl, ldr * 8, (size_t)n * 8, (size_t)T, hipMemcpyDeviceToHost, c->stream));
        if (counts_BxS) HIPCHK(c, hipMemcpyAsync(h_cnt.data(), d_cnt, (size_t)n * Sp * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));        // the chunk's buffers are reused by the next one
        if (counts_BxS)
            for (int b = 0; b < n; ++b)
                for (int s = 0; s < S; ++s) counts_BxS[(size_t)(r0 + b) * S + s] = h_cnt[(size_t)b * Sp + s];
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_rl0, c->ev_rl1));
        ms_total += ms;
    }
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "wins are copied as they are");
    HIPCHK(c, hipMemcpyAsync(wins_T, d_wins, (size_t)T * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (perf) {
        phylo_stats st{};
        st.sweep_ms = ms_total;
        st.n_launches = launches;
        st.units = (double)T * S * B;
        st.alg_bytes = 8.0 * (double)T * S + 8.0 * (double)T * B;
        *perf = st;
    }
    return PHYLO_OK;
}

// ---- multiscale RELL bootstrap, the resampling behind the AU test (phylo_rell_ms.h) ----
int phylo_rell_multiscale(phylo_ctx* c, int T, int S, const double* site_lik_TxS, int K, const int32_t* draws_K, int B, uint64_t seed, double* obs_T,
                          int64_t* wins_KxT, int32_t* best_KxB, double* rep_loglik_KxTxB, int32_t* counts_KxBxS, phylo_stats* perf) {
    CHK(bind(c));
    if (!site_lik_TxS || !draws_K || !obs_T || !wins_KxT)
        return fail(c, PHYLO_EINVAL, "phylo_rell_multiscale: site_lik, draws, obs and wins must be given (NULL pointer)");
    {
        char msg[200];                                     // everything is checked before anything is queued
        if (prm_check_shape(T, S, K, draws_K, B, msg, sizeof msg) || pr_check_factors(T, S, site_lik_TxS, msg, sizeof msg))
            return fail(c, PHYLO_EINVAL, "phylo_rell_multiscale: %s", msg);
    }
    // one slab: logs [T][S] (resident for the call) | counts [chunk + 1][Sp] uint16 | partial values, indices [tiles][chunk] |
    // scores [T][chunk] when asked for | observed [T] | best [chunk] | wins [K][T] | draws [K] | flag.  A column is one replicate
    // of one scale, c = k B + b; the first chunk carries one more, the row of ones whose chain is the observed score.
    const bool scores = rep_loglik_KxTxB != nullptr;
    const size_t Sp = pr_count_stride(S), n_x = (size_t)T * S, n_all = (size_t)K * B;
    const int chunk = prm_chunk_cols(T, S, K, B, scores, c->env.rell_chunk);
    const int ntiles = cdiv(T, PR_TT);
    const size_t ld = (size_t)chunk;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_cnt = up(n_x * 8), o_pv = o_cnt + up((ld + 1) * Sp * 2), o_pi = o_pv + up((size_t)ntiles * ld * 8),
                 o_rl = o_pi + up((size_t)ntiles * ld * 4), o_obs = o_rl + up(scores ? (size_t)T * ld * 8 : 0), o_best = o_obs + up((size_t)T * 8),
                 o_wins = o_best + up(ld * 4), o_draws = o_wins + up((size_t)K * T * 8), o_flag = o_draws + up((size_t)K * 4), total = o_flag + 256;
    void* slab = nullptr;
    CHK(scratch_get(c, 21, total, &slab));
    char* base = (char*)slab;
    double* d_x = (double*)base;
    uint16_t* d_cnt = (uint16_t*)(base + o_cnt);
    double* d_pv = (double*)(base + o_pv);
    int32_t* d_pi = (int32_t*)(base + o_pi);
    double* d_rl = scores ? (double*)(base + o_rl) : nullptr;
    double* d_obs = (double*)(base + o_obs);
    int32_t* d_best = (int32_t*)(base + o_best);
    unsigned long long* d_wins = (unsigned long long*)(base + o_wins);
    int32_t* d_draws = (int32_t*)(base + o_draws);
    unsigned int* d_flag = (unsigned int*)(base + o_flag);
    if (!c->ev_rm0) {
        HIPCHK(c, hipEventCreate(&c->ev_rm0));
        HIPCHK(c, hipEventCreate(&c->ev_rm1));
    }
    HIPCHK(c, hipMemcpyAsync(d_x, site_lik_TxS, n_x * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_draws, draws_K, (size_t)K * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_wins, 0, (size_t)K * T * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(d_flag, 0, 4, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_rm0, c->stream));
    hipLaunchKernelGGL(pr_log, dim3((unsigned)((n_x + 255) / 256)), dim3(256), 0, c->stream, d_x, n_x, d_flag);
    CHK(launch_check(c, "pr_log"));
    HIPCHK(c, hipEventRecord(c->ev_rm1, c->stream));
    unsigned int flag = 0;
    HIPCHK(c, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (flag) return fail(c, PHYLO_EINVAL, "phylo_rell_multiscale: the device met a site factor that is not a finite number > 0");
    double ms_total = 0.0;
    int launches = 1;
    {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_rm0, c->ev_rm1));
        ms_total += ms;
    }
    std::vector<uint16_t> h_cnt(counts_KxBxS ? (size_t)chunk * Sp : 0);
    for (size_t c0 = 0; c0 < n_all; c0 += (size_t)chunk) {
        const int n = (int)std::min<size_t>((size_t)chunk, n_all - c0);
        const int ncols = n + (c0 == 0 ? 1 : 0);
        const uint32_t nblk = (uint32_t)((prm_max_draws(draws_K, B, c0, (size_t)n) + 3) / 4);
        HIPCHK(c, hipMemsetAsync(d_cnt, 0, (size_t)ncols * Sp * 2, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_rm0, c->stream));
        const size_t n_threads = (size_t)n * nblk;
        hipLaunchKernelGGL(prm_counts, dim3((unsigned)((n_threads + 255) / 256)), dim3(256), 0, c->stream, (unsigned int*)d_cnt, S, Sp, (uint32_t)c0,
                           (uint32_t)B, (const int32_t*)d_draws, n_threads, nblk, seed);
        CHK(launch_check(c, "prm_counts"));
        ++launches;
        if (c0 == 0) {
            hipLaunchKernelGGL(pr_ones, dim3(cdiv(S, 256)), dim3(256), 0, c->stream, d_cnt + (size_t)n * Sp, S);
            CHK(launch_check(c, "pr_ones"));
            ++launches;
        }
        const dim3 grid((unsigned)ntiles, (unsigned)cdiv(ncols, PR_TB));
        if (scores)
            hipLaunchKernelGGL(prm_product<true>, grid, dim3(256), 0, c->stream, (const double*)d_x, (const uint16_t*)d_cnt, T, S, Sp, ncols, n, d_pv,
                               d_pi, ld, d_obs, d_rl, ld);
        else
            hipLaunchKernelGGL(prm_product<false>, grid, dim3(256), 0, c->stream, (const double*)d_x, (const uint16_t*)d_cnt, T, S, Sp, ncols, n, d_pv,
                               d_pi, ld, d_obs, d_rl, ld);
        CHK(launch_check(c, "prm_product"));
        hipLaunchKernelGGL(prm_join, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, (const double*)d_pv, (const int32_t*)d_pi, ld, ntiles, n, (uint32_t)c0,
                           (uint32_t)B, T, d_best, d_wins);
        CHK(launch_check(c, "prm_join"));
        launches += 2;
        HIPCHK(c, hipEventRecord(c->ev_rm1, c->stream));
        if (best_KxB) HIPCHK(c, hipMemcpyAsync(best_KxB + c0, d_best, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
        if (c0 == 0) HIPCHK(c, hipMemcpyAsync(obs_T, d_obs, (size_t)T * 8, hipMemcpyDeviceToHost, c->stream));
        if (scores)                                        // a chunk may straddle scales: one strided copy per scale it touches
            for (size_t a = c0; a < c0 + (size_t)n;) {
                const size_t k = a / (size_t)B, b = a % (size_t)B, w = std::min<size_t>((size_t)B - b, c0 + (size_t)n - a);
                HIPCHK(c, hipMemcpy2DAsync(rep_loglik_KxTxB + k * (size_t)T * B + b, (size_t)B * 8, d_rl + (a - c0), ld * 8, w * 8, (size_t)T,
                                           hipMemcpyDeviceToHost, c->stream));
                a += w;
            }
        if (counts_KxBxS) HIPCHK(c, hipMemcpyAsync(h_cnt.data(), d_cnt, (size_t)n * Sp * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));        // the chunk's buffers are reused by the next one
        if (counts_KxBxS)
            for (int b = 0; b < n; ++b)
                for (int s = 0; s < S; ++s) counts_KxBxS[(c0 + (size_t)b) * S + s] = h_cnt[(size_t)b * Sp + s];
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->ev_rm0, c->ev_rm1));
        ms_total += ms;
    }
    HIPCHK(c, hipMemcpyAsync(wins_KxT, d_wins, (size_t)K * T * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (perf) {
        phylo_stats st{};
        st.sweep_ms = ms_total;
        st.n_launches = launches;
        st.units = (double)T * S * K * B;
        st.alg_bytes = 8.0 * (double)T * S + 12.0 * (double)ntiles * K * B;
        *perf = st;
    }
    return PHYLO_OK;
}

// ---- branch-length derivatives of a scored tree set (phylo_treegrad.h) ----
int phylo_trees_grad(phylo_ctx* c, int T, const int32_t* child, const double* blen, const double* prior4, double* loglik_T, double* grad,
                     double* curv, phylo_stats* perf) {
    CHK(trees_front(c, "phylo_trees_grad", T, nullptr, nullptr));
    if (!child || !blen || !loglik_T || !grad) return fail(c, PHYLO_EINVAL, "phylo_trees_grad: child, blen, loglik and grad must be given (NULL pointer)");
    trees_call tc = trees_open(c, T, child, blen, prior4);
    CHK(trees_check(tc));
    const int N = tc.N, R = tc.R, S = tc.S, ntiles = tc.ntiles;
    const bool want_curv = curv != nullptr;
    ptg_plan pl;
    if (ptg_make_plan(N, ntiles, T, tc.coded, want_curv, trees_cus(c), c->env.trees_chunk, &pl))
        return fail(c, PHYLO_EINVAL, "phylo_trees_grad: no plan for N=%d, %d tiles, T=%d", N, ntiles, T);
    const int nq = pl.nq;
    void* slab = nullptr;
    CHK(scratch_get(c, 16, pl.total, &slab));
    trees_carve(tc, slab, pl);
    tc.d_dops = (int32_t*)(tc.base + pl.o_dops);            // set: trees_begin sizes the host buffer, the chunk stages build and upload it
    double* d_dtile = (double*)(tc.base + pl.o_dtile);
    double* d_dout = (double*)(tc.base + pl.o_dout);
    CHK(trees_begin(tc));
    for (int t0 = 0; t0 < T; t0 += tc.chunk) {
        CHK(trees_chunk_host(tc, t0));
        const int n = tc.n;
        CHK(trees_chunk_upload(tc));
        CHK(trees_chunk_expm(tc));
        const long n_mat = tc.n_mat;                        // M | M' | M'' packed by this chunk's count
        hipLaunchKernelGGL(ptg_dmats, dim3(cdiv(n_mat * 16, 256)), dim3(256), 0, c->stream, (const double*)c->d_Q, c->jc, (const double*)tc.d_P, n_mat,
                           tc.d_P + n_mat * 16, tc.d_P + 2 * n_mat * 16);
        CHK(launch_check(c, "ptg_dmats"));
        CHK(trees_chunk_gap_rows(tc));
        ptg_args g{};
        trees_args(tc, g.a);
        g.dops = tc.d_dops; g.dtile = d_dtile; g.store = (pk_d2*)(tc.base + pl.o_store);
        g.mat_plane = n_mat * 16;
        g.n_items = n * ntiles; g.depth = tc.depth;
        ptg_launch(g, std::min(pl.grid, g.n_items), tc.coded, want_curv, c->stream);
        CHK(launch_check(c, "ptg_updown"));
        CHK(trees_chunk_finish(tc));
        hipLaunchKernelGGL(ptg_finish, dim3(cdiv((long)n * nq * 2 * R, 256)), dim3(256), 0, c->stream, (const double*)d_dtile, (const int32_t*)tc.d_ops,
                           (const double*)tc.d_out, ntiles, n, R, nq, d_dout);
        CHK(launch_check(c, "ptg_finish"));
        tc.launches += 3;                                   // ptg_dmats, ptg_updown, ptg_finish
        CHK(trees_chunk_stop(tc, loglik_T + t0));
        HIPCHK(c, hipMemcpyAsync(grad + (size_t)t0 * 2 * R, d_dout, (size_t)n * 2 * R * 8, hipMemcpyDeviceToHost, c->stream));
        if (want_curv)
            HIPCHK(c, hipMemcpyAsync(curv + (size_t)t0 * 2 * R, d_dout + (size_t)n * 2 * R, (size_t)n * 2 * R * 8, hipMemcpyDeviceToHost, c->stream));
        CHK(trees_chunk_end(tc));
    }
    const double units = (double)T * S * R;
    trees_stats(tc, perf, units, 96.0 * units);
    return PHYLO_OK;
}

// ---- marginal ancestral state posteriors of a scored tree set (phylo_treeanc.h) ----
int phylo_trees_ancestral(phylo_ctx* c, int T, const int32_t* child, const double* blen, const double* prior4, double* loglik_T,
                          double* post_TxRxSx4, uint8_t* state_TxRxS, double* pmax_TxRxS, phylo_stats* perf) {
    CHK(trees_front(c, "phylo_trees_ancestral", T, nullptr, nullptr));
    if (!child || !blen || !loglik_T) return fail(c, PHYLO_EINVAL, "phylo_trees_ancestral: child, blen and loglik must be given (NULL pointer)");
    if (!post_TxRxSx4 && !state_TxRxS && !pmax_TxRxS)
        return fail(c, PHYLO_EINVAL, "phylo_trees_ancestral: one of post, state and pmax must be given (all three are NULL pointers)");
    trees_call tc = trees_open(c, T, child, blen, prior4);
    CHK(trees_check(tc));
    const int N = tc.N, R = tc.R, S = tc.S, ntiles = tc.ntiles;
    const unsigned outs = (post_TxRxSx4 ? PTA_POST : 0u) | (state_TxRxS ? PTA_STATE : 0u) | (pmax_TxRxS ? PTA_PMAX : 0u);
    pta_plan pl;
    const int prc = pta_make_plan(N, S, ntiles, T, tc.coded, outs, trees_cus(c), c->env.trees_chunk, &pl);
    if (prc == 2)
        return fail(c, PHYLO_EINVAL, "phylo_trees_ancestral: the requested outputs of one tree take %zu bytes, more than %zu (N=%d, S=%d)",
                    pl.out_tree, (size_t)PTA_OUT_MAX, N, S);
    if (prc) return fail(c, PHYLO_EINVAL, "phylo_trees_ancestral: no plan for N=%d, S=%d, %d tiles, T=%d", N, S, ntiles, T);
    void* slab = nullptr;
    CHK(scratch_get(c, 22, pl.total, &slab));
    trees_carve(tc, slab, pl);
    tc.d_dops = (int32_t*)(tc.base + pl.o_dops);            // set: trees_begin sizes the host buffer, the chunk stages build and upload it
    double* d_post = post_TxRxSx4 ? (double*)(tc.base + pl.o_post) : nullptr;
    uint8_t* d_state = state_TxRxS ? (uint8_t*)(tc.base + pl.o_state) : nullptr;
    double* d_pmax = pmax_TxRxS ? (double*)(tc.base + pl.o_pmax) : nullptr;
    CHK(trees_begin(tc));
    const size_t cells_tree = (size_t)R * S;               // node-sites of one tree
    for (int t0 = 0; t0 < T; t0 += tc.chunk) {
        CHK(trees_chunk_host(tc, t0));
        const int n = tc.n;
        CHK(trees_chunk_upload(tc));
        CHK(trees_chunk_expm(tc));
        CHK(trees_chunk_gap_rows(tc));
        pta_args g{};
        trees_args(tc, g.a);
        g.dops = tc.d_dops; g.store = (pk_d2*)(tc.base + pl.o_store);
        g.post = d_post; g.state = d_state; g.pmax = d_pmax;
        g.n_items = n * ntiles; g.depth = tc.depth;
        pta_launch(g, std::min(pl.grid, g.n_items), tc.coded, c->stream);
        CHK(launch_check(c, "pta_updown"));
        ++tc.launches;
        CHK(trees_chunk_finish(tc));
        CHK(trees_chunk_stop(tc, loglik_T + t0));
        if (d_post)                                        // every node-site of the chunk was written: straight into the caller's rows
            HIPCHK(c, hipMemcpyAsync(post_TxRxSx4 + (size_t)t0 * cells_tree * 4, d_post, (size_t)n * cells_tree * 32, hipMemcpyDeviceToHost, c->stream));
        if (d_state) HIPCHK(c, hipMemcpyAsync(state_TxRxS + (size_t)t0 * cells_tree, d_state, (size_t)n * cells_tree, hipMemcpyDeviceToHost, c->stream));
        if (d_pmax) HIPCHK(c, hipMemcpyAsync(pmax_TxRxS + (size_t)t0 * cells_tree, d_pmax, (size_t)n * cells_tree * 8, hipMemcpyDeviceToHost, c->stream));
        CHK(trees_chunk_end(tc));
    }
    trees_stats(tc, perf, (double)T * S * R,
                (double)T * S * R * ((post_TxRxSx4 ? 32.0 : 0.0) + (state_TxRxS ? 1.0 : 0.0) + (pmax_TxRxS ? 8.0 : 0.0)));
    return PHYLO_OK;
}

// ---- derivatives along directions of the generator and with respect to the prior (phylo_treegrad_model.h) ----
int phylo_trees_grad_model(phylo_ctx* c, int T, const int32_t* child, const double* blen, int P, const double* dirs_Px16, const double* prior4,
                           double* loglik_T, double* grad, double* dtheta_TxP, double* dprior_Tx4, phylo_stats* perf) {
    CHK(trees_front(c, "phylo_trees_grad_model", T, nullptr, nullptr));
    if (!child || !blen || !dirs_Px16 || !loglik_T || !dtheta_TxP)
        return fail(c, PHYLO_EINVAL, "phylo_trees_grad_model: child, blen, dirs, loglik and dtheta must be given (NULL pointer)");
    if (P < 1 || P > PTM_MAX_DIRS) return fail(c, PHYLO_EINVAL, "phylo_trees_grad_model: need 1 <= P <= %d directions (P=%d)", PTM_MAX_DIRS, P);
    for (int i = 0; i < P * 16; ++i)
        if (!std::isfinite(dirs_Px16[i]))
            return fail(c, PHYLO_EINVAL, "phylo_trees_grad_model: direction %d, entry %d is not finite (%g)", i / 16, i % 16, dirs_Px16[i]);
    trees_call tc = trees_open(c, T, child, blen, prior4);
    CHK(trees_check(tc));
    const int N = tc.N, R = tc.R, S = tc.S, ntiles = tc.ntiles;
    const bool want_grad = grad != nullptr;
    ptm_plan pl;
    if (ptm_make_plan(N, ntiles, T, P, tc.coded, want_grad, trees_cus(c), c->env.trees_chunk, &pl))
        return fail(c, PHYLO_EINVAL, "phylo_trees_grad_model: no plan for N=%d, %d tiles, T=%d, P=%d", N, ntiles, T, P);
    // From the deepest schedule there is, not a chunk's own, so that nothing is queued before it; with N <= 512, P <= 16 that is
    // 56 KiB, so the refusal cannot fire today: it guards a larger PT2_MAX_DEPTH or PTM_MAX_DIRS (the arithmetic is in the sanitizer program)
    if (ptm_lds_bytes(N, PT2_MAX_DEPTH, P, want_grad) > PTM_MAX_LDS)
        return fail(c, PHYLO_EINVAL, "phylo_trees_grad_model: %zu bytes of LDS for a wave exceed %zu (N=%d, P=%d)",
                    ptm_lds_bytes(N, PT2_MAX_DEPTH, P, want_grad), PTM_MAX_LDS, N, P);
    const int nm = pl.nm;
    void* slab = nullptr;
    CHK(scratch_get(c, 20, pl.total, &slab));
    trees_carve(tc, slab, pl);
    tc.d_dops = (int32_t*)(tc.base + pl.o_dops);            // set: trees_begin sizes the host buffer, the chunk stages build and upload it
    double* d_dirs = (double*)(tc.base + pl.o_dirs);
    double* d_D = (double*)(tc.base + pl.o_D);
    double* d_dtile = want_grad ? (double*)(tc.base + pl.o_dtile) : nullptr;
    double* d_dout = want_grad ? (double*)(tc.base + pl.o_dout) : nullptr;
    double* d_mtile = (double*)(tc.base + pl.o_mtile);
    double* d_mout = (double*)(tc.base + pl.o_mout);       // dtheta [n][P] | dprior [n][4]
    CHK(trees_begin(tc));
    HIPCHK(c, hipMemcpyAsync(d_dirs, dirs_Px16, (size_t)P * 128, hipMemcpyHostToDevice, c->stream));
    for (int t0 = 0; t0 < T; t0 += tc.chunk) {
        CHK(trees_chunk_host(tc, t0));
        const int n = tc.n;
        CHK(trees_chunk_upload(tc));
        CHK(trees_chunk_expm(tc));
        const long n_mat = tc.n_mat;                        // M | M' packed by this chunk's count
        if (want_grad) {                                    // M'' is ptg_dmats' second output: it goes where D is built next
            hipLaunchKernelGGL(ptg_dmats, dim3(cdiv(n_mat * 16, 256)), dim3(256), 0, c->stream, (const double*)c->d_Q, c->jc, (const double*)tc.d_P, n_mat,
                               tc.d_P + n_mat * 16, d_D);
            CHK(launch_check(c, "ptg_dmats"));
            ++tc.launches;
        }
        hipLaunchKernelGGL(ptm_dirmats, dim3(cdiv(n_mat * P, 64)), dim3(64), 0, c->stream, (const double*)c->d_Q, c->jc, (const double*)d_dirs, P,
                           (const double*)tc.d_t, n_mat, d_D);
        CHK(launch_check(c, "ptm_dirmats"));
        ++tc.launches;
        CHK(trees_chunk_gap_rows(tc));
        ptm_args m{};
        ptg_args& g = m.g;
        trees_args(tc, g.a);
        g.dops = tc.d_dops; g.dtile = d_dtile; g.store = (pk_d2*)(tc.base + pl.o_store);
        g.mat_plane = n_mat * 16;
        g.n_items = n * ntiles; g.depth = tc.depth;
        m.D = d_D; m.mtile = d_mtile; m.P = P;
        ptm_launch(m, std::min(pl.grid, g.n_items), tc.coded, want_grad, c->stream);
        CHK(launch_check(c, "ptm_updown"));
        ++tc.launches;
        CHK(trees_chunk_finish(tc));
        if (want_grad) {
            hipLaunchKernelGGL(ptg_finish, dim3(cdiv((long)n * 2 * R, 256)), dim3(256), 0, c->stream, (const double*)d_dtile, (const int32_t*)tc.d_ops,
                               (const double*)tc.d_out, ntiles, n, R, 1, d_dout);
            CHK(launch_check(c, "ptg_finish"));
            ++tc.launches;
        }
        hipLaunchKernelGGL(ptm_finish, dim3(cdiv((long)n * nm, 256)), dim3(256), 0, c->stream, (const double*)d_mtile, (const double*)tc.d_out, ntiles, n, P,
                           d_mout, d_mout + (size_t)n * P);
        CHK(launch_check(c, "ptm_finish"));
        ++tc.launches;
        CHK(trees_chunk_stop(tc, loglik_T + t0));
        if (want_grad) HIPCHK(c, hipMemcpyAsync(grad + (size_t)t0 * 2 * R, d_dout, (size_t)n * 2 * R * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(dtheta_TxP + (size_t)t0 * P, d_mout, (size_t)n * P * 8, hipMemcpyDeviceToHost, c->stream));
        if (dprior_Tx4)
            HIPCHK(c, hipMemcpyAsync(dprior_Tx4 + (size_t)t0 * 4, d_mout + (size_t)n * P, (size_t)n * 32, hipMemcpyDeviceToHost, c->stream));
        CHK(trees_chunk_end(tc));
    }
    trees_stats(tc, perf, (double)T * S * R * (1 + P), 96.0 * (double)T * S * R);
    return PHYLO_OK;
}

// ---- the same under a mixture of rate categories (phylo_treegrad_rates.h) ----
int phylo_trees_grad_rates(phylo_ctx* c, int T, const int32_t* child, const double* blen, int C, const double* rate, const double* weight,
                           int per_tree, const double* prior4, double* loglik_T, double* grad, double* curv, double* drate_TxC,
                           double* dweight_TxC, phylo_stats* perf) {
    CHK(trees_front(c, "phylo_trees_grad_rates", T, &C, &per_tree));
    if (!child || !blen || !rate || !weight || !loglik_T || !grad)
        return fail(c, PHYLO_EINVAL, "phylo_trees_grad_rates: child, blen, rate, weight, loglik and grad must be given (NULL pointer)");
    trees_call tc = trees_open(c, T, child, blen, prior4);
    trees_mixture(tc, C, rate, weight, per_tree);
    CHK(trees_check(tc));
    const int N = tc.N, R = tc.R, S = tc.S, ntiles = tc.ntiles;
    const bool want_curv = curv != nullptr, want_params = drate_TxC != nullptr || dweight_TxC != nullptr;
    ptgr_plan pl;
    if (ptgr_make_plan(N, ntiles, T, C, tc.coded, want_curv, want_params, trees_cus(c), c->env.trees_chunk, &pl))
        return fail(c, PHYLO_EINVAL, "phylo_trees_grad_rates: no plan for N=%d, %d tiles, T=%d, C=%d", N, ntiles, T, C);
    const int nq = pl.nq, np = pl.np;
    void* slab = nullptr;
    CHK(scratch_get(c, 17, pl.total, &slab));
    trees_carve(tc, slab, pl);
    tc.d_dops = (int32_t*)(tc.base + pl.o_dops);            // set: trees_begin sizes the host buffer, the chunk stages build and upload it
    tc.d_b = (double*)(tc.base + pl.o_b);                   // set: the given lengths in schedule order are kept per tree and uploaded, beside the scaled ones
    double* d_coef = (double*)(tc.base + pl.o_coef);
    double* d_dtile = (double*)(tc.base + pl.o_dtile);
    double* d_dout = (double*)(tc.base + pl.o_dout);
    double* d_ptile = want_params ? (double*)(tc.base + pl.o_ptile) : nullptr;
    double* d_pout = want_params ? (double*)(tc.base + pl.o_pout) : nullptr;
    CHK(trees_begin(tc));
    std::vector<double> coef((size_t)tc.chunk * pl.ncoef);
    for (int t0 = 0; t0 < T; t0 += tc.chunk) {
        CHK(trees_chunk_host(tc, t0));
        const int n = tc.n;
        for (int t = 0; t < n; ++t)                         // (one mixture for all trees: the first tree's block, copied)
            if (t && !per_tree) memcpy(coef.data() + (size_t)t * pl.ncoef, coef.data(), (size_t)pl.ncoef * 8);
            else ptgr_coefficients(C, rate + (t0 + t) * tc.mix_stride, weight + (t0 + t) * tc.mix_stride, coef.data() + (size_t)t * pl.ncoef);
        if (ptgr_lds_bytes(N, tc.depth, C, want_curv, want_params) > PTGR_MAX_LDS)
            return fail(c, PHYLO_EINVAL, "phylo_trees_grad_rates: %zu bytes of LDS for a wave exceed %zu (depth %d, N=%d, C=%d)",
                        ptgr_lds_bytes(N, tc.depth, C, want_curv, want_params), PTGR_MAX_LDS, tc.depth, N, C);
        CHK(trees_chunk_upload(tc));
        HIPCHK(c, hipMemcpyAsync(d_coef, coef.data(), (size_t)n * pl.ncoef * 8, hipMemcpyHostToDevice, c->stream));
        CHK(trees_chunk_expm(tc));
        const long n_mat = tc.n_mat;                        // M | M' | M'' packed by this chunk's count
        hipLaunchKernelGGL(ptg_dmats, dim3(cdiv(n_mat * 16, 256)), dim3(256), 0, c->stream, (const double*)c->d_Q, c->jc, (const double*)tc.d_P, n_mat,
                           tc.d_P + n_mat * 16, tc.d_P + 2 * n_mat * 16);
        CHK(launch_check(c, "ptg_dmats"));
        CHK(trees_chunk_gap_rows(tc));
        ptgr_args g{};
        trees_args(tc, g.a);
        g.dops = tc.d_dops; g.coef = d_coef; g.blen = tc.d_b; g.dtile = d_dtile; g.ptile = d_ptile; g.store = (pk_d2*)(tc.base + pl.o_store);
        g.mat_plane = n_mat * 16;
        g.n_items = n * ntiles; g.depth = tc.depth; g.C = C;
        ptgr_launch(g, std::min(pl.grid, g.n_items), tc.coded, want_curv, want_params, c->stream);
        CHK(launch_check(c, "ptgr_updown"));
        CHK(trees_chunk_finish(tc));
        hipLaunchKernelGGL(ptgr_finish, dim3(cdiv((long)n * (nq * 2 * R + np * C), 256)), dim3(256), 0, c->stream, (const double*)d_dtile,
                           (const double*)d_ptile, (const int32_t*)tc.d_ops, (const double*)tc.d_out, ntiles, n, R, nq, np, C, d_dout, d_pout);
        CHK(launch_check(c, "ptgr_finish"));
        tc.launches += 3;                                   // ptg_dmats, ptgr_updown, ptgr_finish
        CHK(trees_chunk_stop(tc, loglik_T + t0));
        HIPCHK(c, hipMemcpyAsync(grad + (size_t)t0 * 2 * R, d_dout, (size_t)n * 2 * R * 8, hipMemcpyDeviceToHost, c->stream));
        if (want_curv)
            HIPCHK(c, hipMemcpyAsync(curv + (size_t)t0 * 2 * R, d_dout + (size_t)n * 2 * R, (size_t)n * 2 * R * 8, hipMemcpyDeviceToHost, c->stream));
        if (drate_TxC) HIPCHK(c, hipMemcpyAsync(drate_TxC + (size_t)t0 * C, d_pout, (size_t)n * C * 8, hipMemcpyDeviceToHost, c->stream));
        if (dweight_TxC)
            HIPCHK(c, hipMemcpyAsync(dweight_TxC + (size_t)t0 * C, d_pout + (size_t)n * C, (size_t)n * C * 8, hipMemcpyDeviceToHost, c->stream));
        CHK(trees_chunk_end(tc));
    }
    const double units = (double)T * S * R * C;
    trees_stats(tc, perf, units, 96.0 * units);
    return PHYLO_OK;
}

// ---- marginal ancestral state posteriors and site-rate posteriors under a mixture (phylo_treeanc_rates.h) ----
int phylo_trees_ancestral_rates(phylo_ctx* c, int T, const int32_t* child, const double* blen, int C, const double* rate, const double* weight,
                                int per_tree, const double* prior4, double* loglik_T, double* post_TxRxSx4, uint8_t* state_TxRxS,
                                double* pmax_TxRxS, double* catpost_TxCxS, double* siterate_TxS, phylo_stats* perf) {
    CHK(trees_front(c, "phylo_trees_ancestral_rates", T, &C, &per_tree));
    if (!child || !blen || !rate || !weight || !loglik_T)
        return fail(c, PHYLO_EINVAL, "phylo_trees_ancestral_rates: child, blen, rate, weight and loglik must be given (NULL pointer)");
    if (!post_TxRxSx4 && !state_TxRxS && !pmax_TxRxS && !catpost_TxCxS && !siterate_TxS)
        return fail(c, PHYLO_EINVAL,
                    "phylo_trees_ancestral_rates: one of post, state, pmax, catpost and siterate must be given (all five are NULL pointers)");
    trees_call tc = trees_open(c, T, child, blen, prior4);
    trees_mixture(tc, C, rate, weight, per_tree);
    CHK(trees_check(tc));
    const int N = tc.N, R = tc.R, S = tc.S, ntiles = tc.ntiles;
    const unsigned outs = (post_TxRxSx4 ? PTAR_POST : 0u) | (state_TxRxS ? PTAR_STATE : 0u) | (pmax_TxRxS ? PTAR_PMAX : 0u) |
                          (catpost_TxCxS ? PTAR_CATPOST : 0u) | (siterate_TxS ? PTAR_SITERATE : 0u);
    ptar_plan pl;
    const int prc = ptar_make_plan(N, S, ntiles, T, C, tc.coded, outs, trees_cus(c), c->env.trees_chunk, &pl);
    if (prc == 2)
        return fail(c, PHYLO_EINVAL, "phylo_trees_ancestral_rates: the requested outputs of one tree take %zu bytes, more than %zu (N=%d, S=%d, C=%d)",
                    pl.out_tree, (size_t)PTA_OUT_MAX, N, S, C);
    if (prc) return fail(c, PHYLO_EINVAL, "phylo_trees_ancestral_rates: no plan for N=%d, S=%d, %d tiles, T=%d, C=%d", N, S, ntiles, T, C);
    void* slab = nullptr;
    CHK(scratch_get(c, 23, pl.total, &slab));
    trees_carve(tc, slab, pl);
    tc.d_dops = (int32_t*)(tc.base + pl.o_dops);            // set: trees_begin sizes the host buffer, the chunk stages build and upload it
    double* d_coef = (double*)(tc.base + pl.o_coef);
    double* d_post = post_TxRxSx4 ? (double*)(tc.base + pl.o_post) : nullptr;
    uint8_t* d_state = state_TxRxS ? (uint8_t*)(tc.base + pl.o_state) : nullptr;
    double* d_pmax = pmax_TxRxS ? (double*)(tc.base + pl.o_pmax) : nullptr;
    double* d_cat = catpost_TxCxS ? (double*)(tc.base + pl.o_cat) : nullptr;
    double* d_rate = siterate_TxS ? (double*)(tc.base + pl.o_rate) : nullptr;
    CHK(trees_begin(tc));
    std::vector<double> coef((size_t)tc.chunk * pl.ncoef);
    const size_t cells_tree = (size_t)R * S;               // node-sites of one tree
    for (int t0 = 0; t0 < T; t0 += tc.chunk) {
        CHK(trees_chunk_host(tc, t0));
        const int n = tc.n;
        for (int t = 0; t < n; ++t)                         // (one mixture for all trees: the first tree's block, copied)
            if (t && !per_tree) memcpy(coef.data() + (size_t)t * pl.ncoef, coef.data(), (size_t)pl.ncoef * 8);
            else ptar_coefficients(C, rate + (t0 + t) * tc.mix_stride, weight + (t0 + t) * tc.mix_stride, coef.data() + (size_t)t * pl.ncoef);
        CHK(trees_chunk_upload(tc));
        HIPCHK(c, hipMemcpyAsync(d_coef, coef.data(), (size_t)n * pl.ncoef * 8, hipMemcpyHostToDevice, c->stream));
        CHK(trees_chunk_expm(tc));
        CHK(trees_chunk_gap_rows(tc));
        ptar_args g{};
        trees_args(tc, g.a);
        g.dops = tc.d_dops; g.coef = d_coef; g.store = (pk_d2*)(tc.base + pl.o_store);
        g.post = d_post; g.state = d_state; g.pmax = d_pmax; g.catpost = d_cat; g.siterate = d_rate;
        g.n_items = n * ntiles; g.depth = tc.depth; g.C = C;
        ptar_launch(g, std::min(pl.grid, g.n_items), tc.coded, c->stream);
        CHK(launch_check(c, "ptar_updown"));
        ++tc.launches;
        CHK(trees_chunk_finish(tc));
        CHK(trees_chunk_stop(tc, loglik_T + t0));
        if (d_post)                                        // every cell of the chunk was written: straight into the caller's rows
            HIPCHK(c, hipMemcpyAsync(post_TxRxSx4 + (size_t)t0 * cells_tree * 4, d_post, (size_t)n * cells_tree * 32, hipMemcpyDeviceToHost, c->stream));
        if (d_state) HIPCHK(c, hipMemcpyAsync(state_TxRxS + (size_t)t0 * cells_tree, d_state, (size_t)n * cells_tree, hipMemcpyDeviceToHost, c->stream));
        if (d_pmax) HIPCHK(c, hipMemcpyAsync(pmax_TxRxS + (size_t)t0 * cells_tree, d_pmax, (size_t)n * cells_tree * 8, hipMemcpyDeviceToHost, c->stream));
        if (d_cat) HIPCHK(c, hipMemcpyAsync(catpost_TxCxS + (size_t)t0 * C * S, d_cat, (size_t)n * C * S * 8, hipMemcpyDeviceToHost, c->stream));
        if (d_rate) HIPCHK(c, hipMemcpyAsync(siterate_TxS + (size_t)t0 * S, d_rate, (size_t)n * S * 8, hipMemcpyDeviceToHost, c->stream));
        CHK(trees_chunk_end(tc));
    }
    trees_stats(tc, perf, (double)T * S * R * C,
                (double)T * S * (R * ((post_TxRxSx4 ? 32.0 : 0.0) + (state_TxRxS ? 1.0 : 0.0) + (pmax_TxRxS ? 8.0 : 0.0)) +
                                 (catpost_TxCxS ? 8.0 * C : 0.0) + (siterate_TxS ? 8.0 : 0.0)));
    return PHYLO_OK;
}

int phylo_debug_rell_host(int T, int S, const double* site_lik_TxS, int b0, int nB, uint64_t seed, int32_t* counts, double* x, double* rl) {
    char msg[200];
    if (pr_rell_host(T, S, site_lik_TxS, b0, nB, seed, counts, x, rl, msg, sizeof msg)) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_rell_host: %s", msg);
    return PHYLO_OK;
}

int phylo_debug_rell_multiscale_host(int T, int S, const double* site_lik_TxS, int K, const int32_t* draws_K, int k0, int b0, int nB, uint64_t seed,
                                     int32_t* counts, double* rl, int32_t* best) {
    char msg[200];
    if (prm_rell_host(T, S, site_lik_TxS, K, draws_K, k0, b0, nB, seed, counts, rl, best, msg, sizeof msg))
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_rell_multiscale_host: %s", msg);
    return PHYLO_OK;
}

int phylo_resample(phylo_ctx* c, const double* logw, int K, uint64_t seed, uint32_t step, int64_t* idx) {
    CHK(bind(c));
    if (K < 0) return fail(c, PHYLO_EINVAL, "negative K");
    if (K == 0) return PHYLO_OK;
    if (!logw || !idx) return fail(c, PHYLO_EINVAL, "NULL pointer");
    void *dw, *dcdf, *didx;
    CHK(scratch_get(c, 0, (size_t)K * 8, &dw));
    CHK(scratch_get(c, 1, (size_t)K * 8, &dcdf));
    CHK(scratch_get(c, 2, (size_t)K * 8, &didx));
    HIPCHK(c, hipMemcpyAsync(dw, logw, (size_t)K * 8, hipMemcpyHostToDevice, c->stream));
    CHK(launch_scan(c, (const double*)dw, K, 1, (uint64_t*)dcdf, (double*)nullptr, 0));
    hipLaunchKernelGGL(pk_resample_search, dim3(cdiv(K, 256)), dim3(256), 0, c->stream, (const uint64_t*)dcdf, K, K, 0, seed,
                       step, (int64_t*)didx);
    CHK(launch_check(c, "pk_resample_search"));
    HIPCHK(c, hipMemcpyAsync(idx, didx, (size_t)K * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

int phylo_log_zsmc(phylo_ctx* c, const double* logw, int R, int K, double* out) {
    CHK(bind(c));
    if (R < 0 || K < 1 || !out || (R > 0 && !logw)) return fail(c, PHYLO_EINVAL, "bad arguments to phylo_log_zsmc");
    void *dw, *dlse;
    CHK(scratch_get(c, 0, (size_t)(R ? R : 1) * K * 8, &dw));
    CHK(scratch_get(c, 1, (size_t)(R + 1) * 8, &dlse));
    if (R) HIPCHK(c, hipMemcpyAsync(dw, logw, (size_t)R * K * 8, hipMemcpyHostToDevice, c->stream));
    for (int r = 0; r < R; ++r) CHK(launch_scan(c, (const double*)dw + (size_t)r * K, K, 1, (uint64_t*)nullptr, (double*)dlse + r, 0));
    hipLaunchKernelGGL(pk_logz_total, dim3(1), dim3(64), 0, c->stream, (const double*)dlse, R, (double*)dlse + R);
    CHK(launch_check(c, "pk_logz_total"));
    HIPCHK(c, hipMemcpyAsync(out, (double*)dlse + R, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

// ---- the NNI neighbourhood of a scored tree set (phylo_treenni.h) ----
int phylo_trees_nni(phylo_ctx* c, int T, const int32_t* child, const double* blen, const double* prior4, double* loglik_T, double* delta,
                    phylo_stats* perf) {
    CHK(trees_front(c, "phylo_trees_nni", T, nullptr, nullptr));
    if (!child || !blen || !loglik_T || !delta) return fail(c, PHYLO_EINVAL, "phylo_trees_nni: child, blen, loglik and delta must be given (NULL pointer)");
    trees_call tc = trees_open(c, T, child, blen, prior4);
    CHK(trees_check(tc));
    const int N = tc.N, R = tc.R, S = tc.S, ntiles = tc.ntiles;
    ptn_plan pl;
    if (ptn_make_plan(N, ntiles, T, tc.coded, trees_cus(c), c->env.trees_chunk, &pl))
        return fail(c, PHYLO_EINVAL, "phylo_trees_nni: no plan for N=%d, %d tiles, T=%d", N, ntiles, T);
    void* slab = nullptr;
    CHK(scratch_get(c, 18, pl.total, &slab));
    trees_carve(tc, slab, pl);
    tc.d_dops = (int32_t*)(tc.base + pl.o_dops);            // set: trees_begin sizes the host buffer, the chunk stages build and upload it
    tc.d_nops = (int32_t*)(tc.base + pl.o_nops);            // (the same for the NNI operations)
    double* d_dtile = (double*)(tc.base + pl.o_dtile);
    double* d_dout = (double*)(tc.base + pl.o_dout);
    CHK(trees_begin(tc));
    for (int t0 = 0; t0 < T; t0 += tc.chunk) {
        CHK(trees_chunk_host(tc, t0));
        const int n = tc.n;
        CHK(trees_chunk_upload(tc));
        CHK(trees_chunk_expm(tc));
        CHK(trees_chunk_gap_rows(tc));
        ptn_args g{};
        trees_args(tc, g.a);
        g.dops = tc.d_dops; g.nops = tc.d_nops; g.dtile = d_dtile; g.store = (pk_d2*)(tc.base + pl.o_store);
        g.n_items = n * ntiles; g.depth = tc.depth;
        ptn_launch(g, std::min(pl.grid, g.n_items), tc.coded, c->stream);
        CHK(launch_check(c, "ptn_updown"));
        CHK(trees_chunk_finish(tc));
        hipLaunchKernelGGL(ptn_finish, dim3(cdiv((long)n * 2 * R, 256)), dim3(256), 0, c->stream, (const double*)d_dtile, (const int32_t*)tc.d_ops,
                           (const double*)tc.d_out, ntiles, n, R, d_dout);
        CHK(launch_check(c, "ptn_finish"));
        tc.launches += 2;                                   // ptn_updown, ptn_finish
        CHK(trees_chunk_stop(tc, loglik_T + t0));
        HIPCHK(c, hipMemcpyAsync(delta + (size_t)t0 * 2 * R, d_dout, (size_t)n * 2 * R * 8, hipMemcpyDeviceToHost, c->stream));
        CHK(trees_chunk_end(tc));
    }
    const double units = (double)T * S * R;
    trees_stats(tc, perf, units, 96.0 * units);
    return PHYLO_OK;
}

// ---- the same under a mixture of rate categories (phylo_treenni_rates.h) ----
int phylo_trees_nni_rates(phylo_ctx* c, int T, const int32_t* child, const double* blen, int C, const double* rate, const double* weight,
                          int per_tree, const double* prior4, double* loglik_T, double* delta, phylo_stats* perf) {
    CHK(trees_front(c, "phylo_trees_nni_rates", T, &C, &per_tree));
    if (!child || !blen || !rate || !weight || !loglik_T || !delta)
        return fail(c, PHYLO_EINVAL, "phylo_trees_nni_rates: child, blen, rate, weight, loglik and delta must be given (NULL pointer)");
    trees_call tc = trees_open(c, T, child, blen, prior4);
    trees_mixture(tc, C, rate, weight, per_tree);
    CHK(trees_check(tc));
    const int N = tc.N, R = tc.R, S = tc.S, ntiles = tc.ntiles;
    ptnr_plan pl;
    if (ptnr_make_plan(N, ntiles, T, C, tc.coded, trees_cus(c), c->env.trees_chunk, &pl))
        return fail(c, PHYLO_EINVAL, "phylo_trees_nni_rates: no plan for N=%d, %d tiles, T=%d, C=%d", N, ntiles, T, C);
    std::vector<int32_t> sched((size_t)R * 4);
    for (int t = 0; t < T; ++t) {                          // the LDS of every tree's schedule, too, before anything is queued
        const int depth = pt2_schedule(N, child + (size_t)t * R * 2, sched.data());
        if (depth > PT2_MAX_DEPTH) return fail(c, PHYLO_EINVAL, "a schedule of %d slots exceeds %d", depth, PT2_MAX_DEPTH);
        if (ptnr_lds_bytes(N, depth) > PTGR_MAX_LDS)
            return fail(c, PHYLO_EINVAL, "phylo_trees_nni_rates: %zu bytes of LDS for a wave exceed %zu (tree %d, depth %d, N=%d)",
                        ptnr_lds_bytes(N, depth), PTGR_MAX_LDS, t, depth, N);
    }
    void* slab = nullptr;
    CHK(scratch_get(c, 19, pl.total, &slab));
    trees_carve(tc, slab, pl);
    tc.d_dops = (int32_t*)(tc.base + pl.o_dops);            // set: trees_begin sizes the host buffer, the chunk stages build and upload it
    tc.d_nops = (int32_t*)(tc.base + pl.o_nops);            // (the same for the NNI operations)
    double* d_w = (double*)(tc.base + pl.o_w);
    double* d_dtile = (double*)(tc.base + pl.o_dtile);
    double* d_dout = (double*)(tc.base + pl.o_dout);
    CHK(trees_begin(tc));
    std::vector<double> ws((size_t)tc.chunk * C);
    for (int t0 = 0; t0 < T; t0 += tc.chunk) {
        CHK(trees_chunk_host(tc, t0));                     // (its depth refusal cannot fire: every tree's was looked at above)
        const int n = tc.n;
        for (int t = 0; t < n; ++t)
            for (int k = 0; k < C; ++k) ws[(size_t)t * C + k] = weight[(t0 + t) * tc.mix_stride + k];
        CHK(trees_chunk_upload(tc));
        HIPCHK(c, hipMemcpyAsync(d_w, ws.data(), (size_t)n * C * 8, hipMemcpyHostToDevice, c->stream));
        CHK(trees_chunk_expm(tc));
        CHK(trees_chunk_gap_rows(tc));
        ptnr_args g{};
        trees_args(tc, g.a);
        g.dops = tc.d_dops; g.nops = tc.d_nops; g.w = d_w; g.dtile = d_dtile; g.store = (pk_d2*)(tc.base + pl.o_store);
        g.n_items = n * ntiles; g.depth = tc.depth; g.C = C;
        ptnr_launch(g, std::min(pl.grid, g.n_items), tc.coded, c->stream);
        CHK(launch_check(c, "ptnr_updown"));
        CHK(trees_chunk_finish(tc));
        hipLaunchKernelGGL(ptnr_finish, dim3(cdiv((long)n * 2 * R, 256)), dim3(256), 0, c->stream, (const double*)d_dtile, (const int32_t*)tc.d_ops,
                           (const double*)tc.d_out, ntiles, n, R, d_dout);
        CHK(launch_check(c, "ptnr_finish"));
        tc.launches += 2;                                   // ptnr_updown, ptnr_finish
        CHK(trees_chunk_stop(tc, loglik_T + t0));
        HIPCHK(c, hipMemcpyAsync(delta + (size_t)t0 * 2 * R, d_dout, (size_t)n * 2 * R * 8, hipMemcpyDeviceToHost, c->stream));
        CHK(trees_chunk_end(tc));
    }
    const double units = (double)T * S * R * C;
    trees_stats(tc, perf, units, 96.0 * units);
    return PHYLO_OK;
}

// ---- the forward sweep, launch path ---------------------------------------------------------------------------------------------
// The form is decided once per sweep (phylo_sweep_plan.h): sweep_begin_impl computes the plan from the facts below and stores it
// in the run; sweep_step_a, the stages of a rank event and phylo_sweep_finish read it and nothing else (no environment switch, no
// flag bit).  The order of the HIP calls on the stream is what the measurements in that header's comments paid for.
// the flag bits of phylo_sweep_begin as facts (the driver and phylo_debug_sweep_plan decode them here)
static void sweep_facts_flags(sweep_facts& f, uint32_t flags) {
    f.twisting = (flags & PHYLO_TWISTING) != 0; f.keep_graph = (flags & PHYLO_KEEP_GRAPH) != 0;
    f.eager_nodes = (flags & PHYLO_EAGER_NODES) != 0; f.time_kernels = (flags & PHYLO_TIME_KERNELS) != 0;
}

static sweep_facts sweep_facts_of(const phylo_ctx* c, uint32_t flags, int M, int G) {
    sweep_facts f{};
    f.N = c->N; f.K = c->K; f.Kloc = c->Kloc; f.S = c->S; f.G = G; f.M = M; f.world = c->world; f.ntiles = c->ntiles;
    f.transport = c->comm.transport != 0; f.device_exchange = c->p2p; f.jc = c->jc != 0; f.coded_leaves = c->codes_valid;
    sweep_facts_flags(f, flags);
    f.env_eager_nodes = c->env.eager_nodes; f.env_rehearse_sharded = c->env.rehearse_sharded;
    f.env_replicated_book = c->env.replicated_book;
    f.env_launch_xcd = c->env.launch_xcd;
    f.clade_tables = c->clade_ready && pk_pat_take(c->S, c->pat_U, c->leaves_coded, c->ntiles, c->env.site_patterns);
    return f;
}

// What every sweep needs before its first launch, on the launch path and as one launch alike: bind, no run in progress, ...
static int sweep_bind(phylo_ctx* c) {
    CHK(bind(c));
    c->run.active = false;
    return PHYLO_OK;
}
// ... leaves and model, the first-use state and the leaves' log-likelihoods
static int sweep_ready(phylo_ctx* c) {
    if (!c->have_leaves || !c->have_model)
        return fail(c, PHYLO_ESTATE, "phylo_set_leaves and phylo_set_model must be called before a sweep");
    if (!c->state_ready) {
        CHK(ensure_sweep_state(c));
        CHK(refresh_leaf_ll(c));
    }
    return PHYLO_OK;
}

// ... and what every finished sweep leaves for the calls that follow it
static void sweep_publish(phylo_ctx* c, bool lazy, bool graph, int G, bool final_missing, int merge_events, int launches, double units) {
    c->swept = true;
    c->leaves_newer = false;
    c->last_lazy = lazy;                                   // only adopted nodes are in the pool (marks say which)
    c->last_graph = graph;
    c->last_G = G;
    c->last_final_missing = final_missing;
    c->n_merge_events = merge_events;
    c->stats.n_launches = launches;
    c->stats.units = units;
    c->stats.alg_bytes = 96.0 * units;
}

// The twisted proposal's buffers (allocated on first use, grow-only) and the code-pair histogram of coded leaves
static int sweep_alloc_twist(phylo_ctx* c, int M) {
    const int N = c->N, K = c->K, Kl = c->Kloc;
    const size_t Jmax = (size_t)(N * (N - 1) / 2) * M;
    if (Jmax > PK_TWIST_LDS_J && c->twbuf_cap < (size_t)Kl * Jmax) {     // weights of more sub-samples than LDS holds
        if (c->d_twbuf) (void)hipFree(c->d_twbuf);
        c->d_twbuf = nullptr;
        c->twbuf_cap = 0;
        CHK(dalloc(c, &c->d_twbuf, (size_t)Kl * Jmax));
        c->twbuf_cap = (size_t)Kl * Jmax;
    }
    if (!c->d_roots_ad) {
        CHK(dalloc(c, &c->d_roots_ad, (size_t)K * N));
        CHK(dalloc(c, &c->d_cnt_ad, (size_t)K * N));
        CHK(dalloc(c, &c->d_rootll_ad, (size_t)K * N));
        if (!c->p2p) CHK(dalloc(c, &c->d_chosen, (size_t)K));
    }
    if (c->tw_capacity < (size_t)Kl * Jmax) {
        if (c->d_tw_b) { (void)hipFree(c->d_tw_b); (void)hipFree(c->d_tw_P); (void)hipFree(c->d_pot); }
        c->d_tw_b = c->d_tw_P = c->d_pot = nullptr;
        c->tw_capacity = 0;
        CHK(dalloc(c, &c->d_tw_b, (size_t)Kl * Jmax * 2));
        CHK(dalloc(c, &c->d_tw_P, (size_t)Kl * Jmax * 32));
        CHK(dalloc(c, &c->d_pot, (size_t)Kl * Jmax));
        c->tw_capacity = (size_t)Kl * Jmax;
    }
    if (c->codes_valid && !c->hist_ready) {
        if (!c->d_pair_hist) CHK(dalloc(c, &c->d_pair_hist, (size_t)N * N * 32));
        hipLaunchKernelGGL(pk_pair_hist, dim3(N, N), dim3(256), 0, c->stream, (const uint8_t*)c->d_leaf_codes, N, c->S, c->d_pair_hist);
        CHK(launch_check(c, "pk_pair_hist"));
        c->hist_ready = true;
    }
    return PHYLO_OK;
}

// The twisted proposal with a kept graph: every rank event keeps its sub-samples, rows [r][k][J_r]
static int sweep_alloc_twist_history(phylo_ctx* c, int M) {
    const int N = c->N, K = c->K, R = N - 1;
    c->h_joff.assign((size_t)R + 1, 0);
    for (int r = 0; r < R; ++r) c->h_joff[r + 1] = c->h_joff[r] + (int64_t)K * (((N - r) * (N - r - 1)) / 2) * M;
    const size_t rows = (size_t)c->h_joff[R];
    if (c->htw_rows < rows) {
        void* old[] = {c->d_htw_b, c->d_htw_P, c->d_hpot, c->d_tau, c->d_twpart};
        for (void* p : old)
            if (p) (void)hipFree(p);
        c->d_htw_b = c->d_htw_P = c->d_hpot = c->d_tau = c->d_twpart = nullptr;
        c->htw_rows = 0;
        CHK(dalloc(c, &c->d_htw_b, rows * 2));
        CHK(dalloc(c, &c->d_htw_P, rows * 32));
        CHK(dalloc(c, &c->d_hpot, rows));
        CHK(dalloc(c, &c->d_tau, rows));
        CHK(dalloc(c, &c->d_twpart, rows * PG_PART));
        c->htw_rows = rows;
    }
    if (!c->d_hroots_ad) {
        CHK(dalloc(c, &c->d_hroots_ad, (size_t)R * K * N));
        CHK(dalloc(c, &c->d_hchosen, (size_t)R * K));
        CHK(dalloc(c, &c->d_ctw, (size_t)R * K * N));
        CHK(dalloc(c, &c->d_twnode, (size_t)R * K * PG_NODEG));
        CHK(dalloc(c, &c->d_joff, (size_t)R + 1));
        HIPCHK(c, hipHostMalloc((void**)&c->h_rad_p, (size_t)R * K * N * 4));
        HIPCHK(c, hipHostGetDevicePointer((void**)&c->hd_rad, c->h_rad_p, 0));
    }
    HIPCHK(c, hipMemcpyAsync(c->d_joff, c->h_joff.data(), ((size_t)R + 1) * 8, hipMemcpyHostToDevice, c->stream));
    return PHYLO_OK;
}

// First-use and grow-only allocations of the form `p`
static int sweep_alloc(phylo_ctx* c, const sweep_plan& p, int M) {
    if (p.twist) CHK(sweep_alloc_twist(c, M));
    while (p.timek && (int)c->kev.size() < 2 * p.R) {
        hipEvent_t e;
        HIPCHK(c, hipEventCreate(&e));
        c->kev.push_back(e);
    }
    if (p.graph) {
        CHK(ensure_graph_state(c));
        if (p.twist) CHK(sweep_alloc_twist_history(c, M));
    }
    if (p.want_rdraw && !c->d_rdraw) CHK(dalloc(c, &c->d_rdraw, (size_t)p.R * c->K));
    if (p.clade_pat && !c->d_bits[0]) {
        CHK(dalloc(c, &c->d_bits[0], 2 * (size_t)c->K * c->N));
        c->d_bits[1] = c->d_bits[0] + (size_t)c->K * c->N;
    }
    return PHYLO_OK;
}

// Draws, initial tables and cleared marks: one launch (the twisted proposal draws per rank event: its tables alone)
static int sweep_prologue(phylo_ctx* c, const sweep_plan& p, uint64_t seed, const uint64_t* group_seeds) {
    const int N = c->N, K = c->K, Kl = c->Kloc, R = p.R, G = p.G;
    const size_t mark_words = ((size_t)R * K + R + 3) & ~(size_t)3;
    int32_t* t_roots = p.graph ? c->d_hroots : c->d_roots[0];
    int32_t* t_cnt = p.graph ? c->d_hcnt : c->d_cnt[0];
    double* t_rootll = p.graph ? c->d_hrootll : c->d_rootll[0];
    if (!p.twist) {
        if (G > 1) HIPCHK(c, hipMemcpyAsync(c->d_group_seeds, group_seeds, (size_t)G * 8, hipMemcpyHostToDevice, c->stream));
        pk_prologue_args pa{};
        pa.Q = c->d_Q; pa.lam_l = c->d_lam_l; pa.lam_r = c->d_lam_r; pa.jc = c->jc; pa.seed = seed; pa.R = R; pa.Kloc = Kl; pa.k0 = c->k0;
        pa.bl = c->d_bl; pa.br = c->d_br; pa.Pmat = c->d_Pmat; pa.Kg = p.Kg;
        pa.group_seeds = G > 1 ? (const uint64_t*)c->d_group_seeds : (const uint64_t*)nullptr;
        pa.rdraw = p.want_rdraw ? c->d_rdraw : (unsigned long long*)nullptr;
        pa.roots = t_roots; pa.cnt = t_cnt; pa.rootll = t_rootll; pa.nodell = c->d_nodell; pa.K = K; pa.N = N;
        pa.bits = p.clade_pat ? c->d_bits[0] : (int32_t*)nullptr;
        pa.mark = p.lazy ? c->d_mark : (unsigned int*)nullptr;
        pa.mark_words = p.lazy ? (unsigned int)mark_words : 0u;
        const int NT = p.sorted_prologue ? 256 : 64;
        pa.draw_blocks = p.sorted_prologue ? cdiv(2L * R * Kl, PK_DRAW_ITEMS) : cdiv(2L * R * Kl, 64);
        pa.init_blocks = cdiv((long)K * N, 4 * NT);
        pa.mark_blocks = p.lazy ? cdiv((long)mark_words, 4 * NT) : 0;
        const int rdraw_blocks = p.want_rdraw ? cdiv((long)(R - 1) * K, NT) : 0;
        const dim3 pgrid(pa.draw_blocks + pa.init_blocks + pa.mark_blocks + rdraw_blocks);
        if (p.sorted_prologue) hipLaunchKernelGGL(pk_sweep_prologue_sorted, pgrid, dim3(256), 0, c->stream, pa);
        else hipLaunchKernelGGL(pk_sweep_prologue, pgrid, dim3(64), 0, c->stream, pa);
        CHK(launch_check(c, "pk_sweep_prologue"));
    } else {
        if (p.lazy) HIPCHK(c, hipMemsetAsync(c->d_mark, 0, mark_words * sizeof(unsigned int), c->stream));
        hipLaunchKernelGGL(pk_init_tables, dim3(cdiv((long)K * N, 256)), dim3(256), 0, c->stream, t_roots, t_cnt, t_rootll,
                           (const double*)c->d_nodell, K, N);
    }
    CHK(launch_check(c, "pk_init_tables"));
    if (c->d_mirror) HIPCHK(c, hipMemsetAsync(c->d_mirror, 0, ((size_t)R * K + 4) * 4, c->stream));   // the cache of remote nodes is per sweep
    return PHYLO_OK;
}

// validate (the batch, then -- behind the leaves / model check, as ever -- the proposal and the graph), plan, allocate, prologue,
// store the run
static int sweep_begin_impl(phylo_ctx* c, uint64_t seed, uint32_t flags, int M, const uint64_t* group_seeds, int G) {
    CHK(sweep_bind(c));
    const sweep_facts f = sweep_facts_of(c, flags, M, G);
    char why[160];
    if (sweep_refuses_batch(f, k_sweep_limits, why, sizeof why)) return fail(c, PHYLO_EINVAL, "%s", why);
    CHK(sweep_ready(c));
    if (sweep_refuses_form(f, k_sweep_limits, why, sizeof why)) return fail(c, PHYLO_EINVAL, "%s", why);
    const sweep_plan p = sweep_plan_form(f, k_sweep_limits);
    CHK(sweep_alloc(c, p, M));
    c->swept = false; ++c->sweep_serial;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    CHK(sweep_prologue(c, p, seed, group_seeds));
    c->run = sweep_run{};
    c->run.seed = seed; c->run.flags = flags; c->run.M = M;
    c->run.plan = p;
    c->run.chain = sweep_chain_form_of(p, c->S, c->env.scan_multi_min, c->env.scan_ancestors, k_sweep_limits);
    c->last_chain = c->run.chain.taken ? 1 : 0;
    c->run.launches = sweep_plan_launches(p, -1);
    c->run.active = true;
    c->last_persistent = false;
    return PHYLO_OK;
}

// ---- the sweep as ONE launch (phylo_persist.h) ------------------------------------------------------------------
// Resident-workgroup kernels of different contexts must not be dispatched together: each waits inside the launch for ALL of
// its own workgroups, and two partially resident grids would wait for each other's CU slots for ever (the bounded spins turn
// that into a timeout error, not a hang).  So the one-launch sweeps of a process run one after the other on a device: every
// launch waits for the event the previous one recorded.  (Kernels of the launch path still overlap with them freely.)
static std::mutex g_persist_mu;
static hipEvent_t g_persist_done[64] = {};
static int persist_chain(phylo_ctx* c, bool after_launch) {
    std::lock_guard<std::mutex> lock(g_persist_mu);
    if (c->device < 0 || c->device >= 64) return fail(c, PHYLO_EINVAL, "device id out of range for the one-launch sweep");
    hipEvent_t& ev = g_persist_done[c->device];
    if (!after_launch) {
        if (ev) HIPCHK(c, hipStreamWaitEvent(c->stream, ev, 0));
        return PHYLO_OK;
    }
    if (!ev) HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(ev, c->stream));
    return PHYLO_OK;
}

static size_t persist_lds_bytes(int N, int m, int Kg) { return pp_layout(N, m, Kg).total; }
static const persist_limits k_persist_limits = {32, PP_MAX_KG, PP_MAX_M, 8192, (size_t)150 * 1024, persist_lds_bytes};

static persist_facts persist_facts_flags(int N, int K, int S, int G, int world, bool transport, uint32_t flags, bool env_one_launch,
                                         bool env_eager_nodes) {
    persist_facts f{};
    f.N = N; f.K = K; f.S = S; f.G = G; f.world = world; f.transport = transport;
    f.one_launch = env_one_launch || (flags & PHYLO_ONE_LAUNCH);
    f.twisting = (flags & PHYLO_TWISTING) != 0; f.keep_graph = (flags & PHYLO_KEEP_GRAPH) != 0;
    f.time_kernels = (flags & PHYLO_TIME_KERNELS) != 0; f.eager_nodes = (flags & PHYLO_EAGER_NODES) != 0;
    f.env_eager_nodes = env_eager_nodes;
    return f;
}

// Plan: G groups x Wg resident workgroups, m = Kg / Wg particles each.  Returns false when this context / sweep is
// not eligible (the launch-per-rank-event path runs instead).
// The rule is persist_plan_of (phylo_sweep_plan.h); here only the facts of this context and device.
static bool persist_plan(phylo_ctx* c, uint32_t flags, int G, int* Wg_out, int* m_out) {
    persist_facts f = persist_facts_flags(c->N, c->K, c->S, G, c->world, c->comm.transport != 0, flags, c->env.one_launch, c->env.eager_nodes);
    if (persist_refuses_shape(f, k_persist_limits)) return false;
    if (c->persist_blocks_per_cu < 0) {
        // residency of ONE workgroup per CU is all the kernel needs; ask the runtime whether it is admitted at all
        int nb = 0;
        const size_t lds = pp_layout(c->N, PP_CHUNK, 2048).total;
        hipError_t e = c->env.persist_nt == 512
            ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pp_sweep<512>, 512, lds)
            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, pp_sweep<256>, 256, lds);
        c->persist_blocks_per_cu = (e == hipSuccess && nb >= 1) ? (nb >= 3 ? 2 : 1) : 0;   // one workgroup per CU by default; two only with a block of margin
    }
    f.n_cus = c->n_cus; f.blocks_per_cu = c->persist_blocks_per_cu;
    f.persist_wgs = c->env.persist_wgs; f.persist_nt = c->env.persist_nt;
    const persist_grid p = persist_plan_of(f, k_persist_limits);
    if (!p.taken) return false;
    *Wg_out = p.Wg;
    *m_out = p.m;
    return true;
}

static int sweep_persistent(phylo_ctx* c, uint64_t seed, uint32_t flags, const uint64_t* group_seeds, int G, int Wg, int m) {
    CHK(sweep_bind(c));
    CHK(sweep_ready(c));
    const int N = c->N, K = c->K, S = c->S, R = N - 1, Kg = K / G;
    if (!c->d_rdraw) CHK(dalloc(c, &c->d_rdraw, (size_t)R * K));       // (the launch path's pk_rank_book_mat shares this buffer)
    if (!c->d_pctr) {
        CHK(dalloc(c, &c->d_pctr, (size_t)PK_MAX_GROUPS * PP_CTR_STRIDE));
        c->pctr_Wg = 0;
    }
    // Every group owns one monotone counter and expects it to equal ctr_base at launch.  Another grid shape, another number of
    // groups (the groups the previous launches did not use are behind) or a timed-out wait (partial arrivals): start again from 0.
    if (c->pctr_Wg != Wg || c->pctr_G != G || c->pctr_dirty) {
        HIPCHK(c, hipMemsetAsync(c->d_pctr, 0, (size_t)PK_MAX_GROUPS * PP_CTR_STRIDE * 8, c->stream));
        c->pctr_base = 0;
        c->pctr_Wg = Wg;
        c->pctr_G = G;
        c->pctr_dirty = false;
    }
    pp_args a{};
    a.N = N; a.S = S; a.K = K; a.Kg = Kg; a.G = G; a.R = R; a.Wg = Wg; a.m = m;
    a.T = c->site_tile;
    a.seed = seed; a.flags = flags; a.jc = c->jc;
    if (G > 1) {
        HIPCHK(c, hipMemcpyAsync(c->d_group_seeds, group_seeds, (size_t)G * 8, hipMemcpyHostToDevice, c->stream));
        a.group_seeds = c->d_group_seeds;
    }
    a.Q = c->d_Q; a.lam_l = c->d_lam_l; a.lam_r = c->d_lam_r; a.pi = c->d_pi; a.ldf = c->d_ldf;
    a.leaves = c->d_leaves; a.leaf_codes = c->leaves_coded ? c->d_leaf_codes : nullptr; a.pool = c->d_pool;
    for (int i = 0; i < 2; ++i) { a.roots[i] = c->d_roots[i]; a.cnt[i] = c->d_cnt[i]; a.rootll[i] = c->d_rootll[i]; }
    a.nodell = c->d_nodell; a.bl = c->d_bl; a.br = c->d_br; a.Pmat = c->d_Pmat; a.logw = c->d_logw; a.ll = c->d_ll;
    a.child = c->d_child; a.merges = c->d_merges; a.anc = c->d_anc; a.mark = c->d_mark;
    a.rdraw = c->d_rdraw;
    a.lse = c->d_lse; a.lse_stride = R + 1;
    a.ctr = c->d_pctr; a.ctr_base = c->pctr_base;
    a.timeout_word = c->d_counter + 1;
    if (c->env.persist_stamps) {
        if (!c->d_stamps) CHK(dalloc(c, &c->d_stamps, (size_t)(R + 1) * PP_NSTAMP));
        a.stamps = c->d_stamps;
    }
    const size_t lds = pp_layout(N, m, Kg).total;
    c->swept = false; ++c->sweep_serial;
    CHK(persist_chain(c, false));
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    if (c->env.persist_nt == 512) hipLaunchKernelGGL((pp_sweep<512>), dim3(G * Wg), dim3(512), lds, c->stream, a);
    else hipLaunchKernelGGL((pp_sweep<256>), dim3(G * Wg), dim3(256), lds, c->stream, a);
    CHK(launch_check(c, "pp_sweep"));
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    CHK(persist_chain(c, true));
    c->pctr_base += (unsigned long long)R * Wg;
    sweep_publish(c, true, false, G, false, 0, 1, (double)K * S * R);      // lazy: only adopted nodes are in the pool
    c->last_persistent = true;
    c->last_chain = 0;
    c->last_pp_nt = c->env.persist_nt; c->last_pp_Wg = Wg; c->last_pp_m = m; c->last_pp_lds = lds;
    return PHYLO_OK;
}


int phylo_sweep_begin(phylo_ctx* c, uint64_t seed, uint32_t flags, int M) { return sweep_begin_impl(c, seed, flags, M, nullptr, 1); }

// All-gather of this rank's segments of `n_arrays` arrays (`count` doubles per rank; arrays[i] = the array's base, rank p's segment
// at + p * count), or with n_arrays == 0 a barrier across the ranks, on the context's stream.  With the exchange slab
// (c->p2p) it is ONE launch of pk_p2p_exchange -- peers' slabs written over xGMI, flags, bounded wait: no collective call, no
// second stream; otherwise the RCCL / host-mediated collective of phylo_comm.h.  purpose 0: the rank event's K-vectors; 1: barriers
// and the twisted proposal's choices (own flags and epochs: every rank issues the same sequence of each).
static int comm_exchange(phylo_ctx* c, double* const* arrays, int n_arrays, size_t count, int purpose) {
    if (c->comm.transport == 0) return PHYLO_OK;
    if (!c->p2p) {
        if (n_arrays == 0) { double* rows[1] = {c->d_sync}; return phylo_comm_allgather_inplace(c->comm, rows, 1, 1, c->stream, &c->err); }
        return phylo_comm_allgather_inplace(c->comm, arrays, n_arrays, count, c->stream, &c->err);
    }
    if (n_arrays > 4) return fail(c, PHYLO_EINVAL, "comm_exchange: at most four arrays");
    pk_p2p_args a{};
    a.slabs = c->d_xslab_ptrs; a.world = c->world; a.me = c->rank;
    a.n_seg = n_arrays; a.seg_count = (int)count;
    for (int i = 0; i < n_arrays; ++i) {
        const ptrdiff_t off = (const char*)arrays[i] - c->d_xslab;
        if (off < 0 || (size_t)off + (size_t)c->world * count * 8 > c->xslab_bytes) return fail(c, PHYLO_EINVAL, "comm_exchange: array outside the exchange slab");
        a.seg_off[i] = (size_t)off;
    }
    a.flag_off = c->x_flag_off[purpose];
    a.epoch = ++c->x_epoch[purpose];
    a.timeout_word = c->d_counter + 1;
    a.wait_ticks = c->env.p2p_wait_ticks;
    const size_t words = (size_t)n_arrays * count * (size_t)(c->world - 1);
    if (words > c->env.p2p_copy_words) {                   // large exchange: the copy over many workgroups, then the flags alone
        const size_t wgs = (words + 4095) / 4096;
        hipLaunchKernelGGL(pk_p2p_copy, dim3((unsigned)(wgs < 512 ? wgs : 512)), dim3(1024), 0, c->stream, a);
        CHK(launch_check(c, "pk_p2p_copy"));
        a.n_seg = 0;
    }
    hipLaunchKernelGGL(pk_p2p_exchange, dim3(1), dim3(1024), 0, c->stream, a);
    return launch_check(c, "pk_p2p_exchange");
}

// The kernel arguments of rank event r, for sweep_step_a's launches and for the stages of the step alike.  (What only the step's kernels read -- tables, weights, records, tiles -- the kernels of
// sweep_step_a never touch: pk_all_marks reads K, Kg, group_seeds, seed, r, cdf and mark; pk_materialize_adopted(_grouped) and
// pk_materialize_by_draws read those, rdraw, k0, Kloc, N, S, child_all, Pmat_all, leaves, pool, pool_ptrs, mirror and cache.
// rdraw is read by pk_materialize_by_draws and pk_rank_book_mat alone, tab_ptrs by the bookkeeping kernels alone.)
// does the record-form merge of the current leaves take the pattern form (phylo_site_patterns.h: the rule)?
static bool pat_on(const phylo_ctx* c) { return pk_pat_take(c->S, c->pat_U, c->leaves_coded, c->ntiles, c->env.site_patterns); }

static pk_rank_args rank_args(const phylo_ctx* c, int r) {
    const sweep_plan& p = c->run.plan;
    const int N = c->N, K = c->K, Kl = c->Kloc, cur = r & 1, nxt = cur ^ 1;
    const size_t plane = (size_t)K * N;
    pk_rank_args b{};
    b.r = r; b.n = N - r; b.N = N; b.S = c->S; b.K = K; b.Kloc = Kl; b.k0 = c->k0;
    b.seed = c->run.seed; b.flags = c->run.flags;
    b.Kg = p.Kg; b.group_seeds = p.G > 1 ? c->d_group_seeds : nullptr;
    b.no_store = (r == p.R - 1 && p.no_store_last) ? 1 : 0;
    if (p.graph) {                                         // every rank event keeps its tables: plane r -> plane r + 1
        b.roots_old = c->d_hroots + plane * r; b.cnt_old = c->d_hcnt + plane * r;
        b.roots_new = c->d_hroots + plane * (r + 1); b.cnt_new = c->d_hcnt + plane * (r + 1);
        b.rootll_old = c->d_hrootll + plane * r; b.rootll_new = c->d_hrootll + plane * (r + 1);
        b.pos_hist = c->d_pos + plane * r;
    } else {
        b.roots_old = c->d_roots[cur]; b.cnt_old = c->d_cnt[cur];
        b.roots_new = c->d_roots[nxt]; b.cnt_new = c->d_cnt[nxt];
        b.rootll_old = c->d_rootll[cur]; b.rootll_new = c->d_rootll[nxt];
        if (p.clade_pat) { b.bits_old = c->d_bits[cur]; b.bits_new = c->d_bits[nxt]; }   // (never with a kept graph: the plan)
    }
    if (p.local_book) {                                    // an ancestor's rows of the previous plane, inside its owner's slab
        b.tab_ptrs = c->d_tab_ptrs;
        b.tab_off_rootll = (size_t)cur * K * N * 8;
        b.tab_off_roots = (size_t)16 * K * N + (size_t)cur * K * N * 4;
        b.tab_off_cnt = (size_t)24 * K * N + (size_t)cur * K * N * 4;
    }
    b.cdf = c->d_cdf[cur];
    b.rdraw = p.want_rdraw ? c->d_rdraw + (size_t)r * K : nullptr;
    b.ll_prev = r > 0 ? c->d_ll + (size_t)(r - 1) * K : nullptr;
    b.nodell = c->d_nodell;
    b.ldf = c->d_ldf; b.ldf_n = N;
    b.bl = c->d_bl; b.br = c->d_br;
    b.lam_l = c->h_lam_l[r]; b.lam_r = c->h_lam_r[r];
    b.loglam_l = pm_log(b.lam_l); b.loglam_r = pm_log(b.lam_r);
    b.ll_tilde0 = pm_log(1.0 / (double)p.Kg);              // vcsmc.py:422
    b.leaves = c->d_leaves; b.pool = c->d_pool; b.pool_ptrs = c->d_pool_ptrs;
    // the cache of remote nodes is filled by the bookkeeping launch, which must come behind the owners' writes of this rank
    // event's adopted nodes: not so with replicated bookkeeping (and the twisted proposal reads its roots elsewhere)
    b.mirror = (p.twist || p.replicated_book) ? nullptr : c->d_mirror; b.cache = c->d_cache; b.cache_cap = c->cache_cap;
    b.leaf_codes = c->leaves_coded ? c->d_leaf_codes : nullptr;
    b.leaf_packed = c->leaves_coded ? c->d_leaf_packed : nullptr;
    b.packed_leaf_bytes = pk_packed_leaf_bytes(c->S);
    b.Pmat = c->d_Pmat + (size_t)r * Kl * 32;
    b.pi = c->d_pi;
    b.logw_r = c->d_logw + (size_t)r * K;
    b.ll_r = c->d_ll + (size_t)r * K;
    b.merges = c->d_merges; b.ancestors = c->d_anc;
    b.child = c->d_child + (size_t)r * Kl * 2; b.aux = c->d_aux;
    b.rec = p.use_rec ? c->d_rec : nullptr;
    b.lazy = p.lazy ? 1 : 0; b.mark = c->d_mark; b.child_all = c->d_child; b.Pmat_all = c->d_Pmat;
    b.T = c->site_tile; b.ntiles = c->ntiles; b.tilev = c->d_tilev;
    if (c->run.chain.taken && r > 0) {
        b.anc_in = c->d_anc_next; b.adopt_list = c->d_adopt_list; b.adopt_cnt = c->d_adopt_cnt;
        b.item_waves = c->run.chain.item_waves; b.item_parts = c->run.chain.parts;
    }
    b.book_xcd = c->run.chain.taken && p.book_xcd;
    return b;
}

// The adopted nodes of rank event r - 1, in a launch of their own, and the barrier that orders them before every rank's merge.
// Once per rank event r > 0: from sweep_step_a with owner-held tables (plan.step_a_work: the owners find their nodes by the draws,
// or every rank marks the adopted nodes of all K particles first), else from the step behind its bookkeeping (plan.mat_after_book).
static int step_materialize(phylo_ctx* c, const pk_rank_args& b) {
    const sweep_plan& p = c->run.plan;
    const int Kl = c->Kloc, S = c->S;
    if (c->run.chain.taken) return PHYLO_OK;               // the chain form: written from the scan's list inside the bookkeeping's launch
    if (p.mat_by_draws) {
        const int grouped = p.mat_draws_grouped ? 1 : 0;
        hipLaunchKernelGGL(pk_materialize_by_draws, dim3(grouped ? Kl / PK_MAT_GROUP : Kl), dim3(PK_COLS), 0, c->stream, b, grouped);
        CHK(launch_check(c, "pk_materialize_by_draws"));
    } else {
        if (p.step_a_work) {
            hipLaunchKernelGGL(pk_all_marks, dim3(cdiv(c->K, 4)), dim3(64), 0, c->stream, b);
            CHK(launch_check(c, "pk_all_marks"));
        }
        if (p.mat_grouped) hipLaunchKernelGGL(pk_materialize_adopted_grouped, dim3(cdiv(Kl, PK_MAT_GROUP)), dim3(PK_COLS), 0, c->stream, b);
        else hipLaunchKernelGGL(pk_materialize_adopted, dim3(p.one_tile ? 1 : cdiv(S, PK_MAT_TILE), Kl), dim3(PK_COLS), 0, c->stream, b);
        CHK(launch_check(c, "pk_materialize_adopted"));
    }
    if (p.mat_barrier) CHK(comm_exchange(c, nullptr, 0, 0, 1));
    return PHYLO_OK;
}

// Sharded lazy nodes, first half of a rank event: the owners write the nodes adopted at this resampling, and one tiny collective
// orders those writes before every rank's merge (step_materialize).  A no-op otherwise.  phylo_sweep_step runs it when the caller
// has not (phylo_sweep_step_a).
static int sweep_step_a(phylo_ctx* c) {
    CHK(bind(c));
    if (!c->run.active) return fail(c, PHYLO_ESTATE, "phylo_sweep_step without phylo_sweep_begin");
    const int R = c->N - 1, r = c->run.next_r;
    if (r >= R) return fail(c, PHYLO_ESTATE, "all %d rank events of this sweep have been issued", R);
    c->run.a_done_r = r;
    if (!c->run.plan.step_a_work || r == 0) return PHYLO_OK;
    return step_materialize(c, rank_args(c, r));
}

// The twisted proposal of a rank event: adopt + draws, potentials, choose, the exchange of the choices, tables
static int step_twist(phylo_ctx* c, const pk_rank_args& b) {
    const sweep_plan& p = c->run.plan;
    const int N = c->N, K = c->K, Kl = c->Kloc, r = b.r;
    pk_twist_args ta{};
    ta.a = b;
    ta.M = c->run.M;
    ta.J = ((N - r) * (N - r - 1) / 2) * ta.M;
    ta.roots_ad = c->d_roots_ad; ta.cnt_ad = c->d_cnt_ad; ta.rootll_ad = c->d_rootll_ad;
    ta.tw_b = c->d_tw_b; ta.tw_P = c->d_tw_P; ta.pot = c->d_pot; ta.chosen = c->d_chosen;
    if (p.graph) {                                         // the reverse pass reads every rank event's sub-samples
        const size_t j0 = (size_t)c->h_joff[r];
        ta.tw_b = c->d_htw_b + j0 * 2; ta.tw_P = c->d_htw_P + j0 * 32; ta.pot = c->d_hpot + j0;
        ta.roots_ad = c->d_hroots_ad + (size_t)K * N * r; ta.chosen = c->d_hchosen + (size_t)r * K;
    }
    ta.Pmat_r = c->d_Pmat + (size_t)r * Kl * 32;
    ta.pair_hist = p.twist_ll ? c->d_pair_hist : nullptr;
    ta.codes = p.twist_ll ? c->d_leaf_codes : nullptr;
    ta.bl_r = c->d_bl + (size_t)r * Kl; ta.br_r = c->d_br + (size_t)r * Kl;
    ta.own_tables = p.twist_tables ? 0 : 1;
    ta.wbuf = c->d_twbuf;
    hipLaunchKernelGGL(pk_twist_adopt_draws, dim3(K + cdiv(2L * Kl * ta.J, 64)), dim3(64), 0, c->stream, ta, (const double*)c->d_Q, c->jc);
    CHK(launch_check(c, "pk_twist_adopt_draws"));
    if (p.twist_ll) {                                      // coded leaf-leaf pairs: 25 code pairs per row instead of S sites
        hipLaunchKernelGGL(pk_twist_potentials_ll, dim3((ta.J + 7) / 8, Kl), dim3(256), 0, c->stream, ta);
        CHK(launch_check(c, "pk_twist_potentials_ll"));
    }
    // every other row: one wave each (at rank event 0 of a coded alignment every root is a leaf: nothing is left)
    const bool any_rows = !(p.twist_ll && r == 0);
    const dim3 pgrid((unsigned)((((size_t)Kl * ta.J + 7) / 8) * 8));
    if (p.timek) {   // a twisted sweep's dominant kernel is this one: PHYLO_TIME_KERNELS stamps it instead of the merge
        if (any_rows) hipExtLaunchKernelGGL(pk_twist_potentials, pgrid, dim3(64), 0, c->stream, c->kev[2 * r], c->kev[2 * r + 1], 0, ta);
        else { HIPCHK(c, hipEventRecord(c->kev[2 * r], c->stream)); HIPCHK(c, hipEventRecord(c->kev[2 * r + 1], c->stream)); }
    } else if (any_rows) {
        hipLaunchKernelGGL(pk_twist_potentials, pgrid, dim3(64), 0, c->stream, ta);
    }
    CHK(launch_check(c, "pk_twist_potentials"));
    hipLaunchKernelGGL(pk_twist_choose, dim3(Kl), dim3(64), (size_t)(ta.J <= PK_TWIST_LDS_J ? ta.J : 0) * 8, c->stream, ta);
    CHK(launch_check(c, "pk_twist_choose"));
    if (p.twist_tables) {
        double* rows[1] = {c->d_chosen};
        CHK(comm_exchange(c, rows, 1, (size_t)Kl, 1));
        hipLaunchKernelGGL(pk_twist_tables, dim3(cdiv(K, 128)), dim3(128), 0, c->stream, ta);
        CHK(launch_check(c, "pk_twist_tables"));
    }
    return PHYLO_OK;
}

// The bookkeeping of a rank event at plan.book_width lanes per particle: with the adopted nodes in the same launch
// (pk_rank_book_mat, r > 0), else over the root tables this rank advances (pk_rank_book_packed)
static int step_book(phylo_ctx* c, const pk_rank_args& b) {
    const sweep_plan& p = c->run.plan;
    const int K = c->K, w = p.book_width;
    const size_t lds = pk_book_lds_bytes(c->N) + (p.clade_pat ? pk_book_bits_lds_bytes(c->N) : 0);   // (per group; pk_book_carve_sub)
    if (p.book_mat && b.r > 0) {
        const int lp = w < 16 ? 16 : w, per = PK_COLS / lp;   // particles per workgroup; behind them, a workgroup per particle's node
        const int bb = cdiv(K, per);
        const dim3 grid(bb + K);
        if (p.clade_pat) {                                 // (N <= 12: 16 lanes)
            if (lp != 16) return fail(c, PHYLO_ESTATE, "step_book: clade patterns at %d lanes", lp);
            hipLaunchKernelGGL(pk_rank_book_mat_clade<16>, grid, dim3(PK_COLS), lds * per, c->stream, b, bb);
            return launch_check(c, "pk_rank_book_mat");
        }
        switch (lp) {
        case 16: hipLaunchKernelGGL(pk_rank_book_mat<16>, grid, dim3(PK_COLS), lds * per, c->stream, b, bb); break;
        case 32: hipLaunchKernelGGL(pk_rank_book_mat<32>, grid, dim3(PK_COLS), lds * per, c->stream, b, bb); break;
        case 64: hipLaunchKernelGGL(pk_rank_book_mat<64>, grid, dim3(PK_COLS), lds * per, c->stream, b, bb); break;
        default: return fail(c, PHYLO_ESTATE, "step_book: no pk_rank_book_mat of %d lanes", lp);
        }
        return launch_check(c, "pk_rank_book_mat");
    }
    const int per = 64 / (w > 0 ? w : 64);                                       // particles per wave
    const sweep_chain_form& ch = c->run.chain;
    if (ch.taken) {                                        // the ancestors from the scan; the item waves of the adopted nodes lead the grid
        const int items = b.r > 0 ? p.G * ch.item_waves : 0;
        const dim3 grid(items + pk_launch_grid(cdiv(K, per), 1, p.book_xcd));
        if (p.clade_pat) {
            if (w == 8) hipLaunchKernelGGL(pk_rank_book_chain_clade<8>, grid, dim3(64), lds * per, c->stream, b, items);
            else if (w == 16) hipLaunchKernelGGL(pk_rank_book_chain_clade<16>, grid, dim3(64), lds * per, c->stream, b, items);
            else return fail(c, PHYLO_ESTATE, "step_book: clade patterns at %d lanes", w);
            return launch_check(c, "pk_rank_book_chain");
        }
        switch (w) {
        case 8: hipLaunchKernelGGL(pk_rank_book_chain<8>, grid, dim3(64), lds * per, c->stream, b, items); break;
        case 16: hipLaunchKernelGGL(pk_rank_book_chain<16>, grid, dim3(64), lds * per, c->stream, b, items); break;
        case 32: hipLaunchKernelGGL(pk_rank_book_chain<32>, grid, dim3(64), lds * per, c->stream, b, items); break;
        case 64: hipLaunchKernelGGL(pk_rank_book_chain<64>, grid, dim3(64), lds * per, c->stream, b, items); break;
        default: return fail(c, PHYLO_ESTATE, "step_book: no pk_rank_book_chain of %d lanes", w);
        }
        return launch_check(c, "pk_rank_book_chain");
    }
    const dim3 grid(cdiv(p.local_book ? c->Kloc : K, per));
    if (p.clade_pat) {
        if (w == 8) hipLaunchKernelGGL(pk_rank_book_packed_clade<8>, grid, dim3(64), lds * per, c->stream, b);
        else if (w == 16) hipLaunchKernelGGL(pk_rank_book_packed_clade<16>, grid, dim3(64), lds * per, c->stream, b);
        else return fail(c, PHYLO_ESTATE, "step_book: clade patterns at %d lanes", w);
        return launch_check(c, "pk_rank_book_packed");
    }
    switch (w) {
    case 8: hipLaunchKernelGGL(pk_rank_book_packed<8>, grid, dim3(64), lds * per, c->stream, b); break;
    case 16: hipLaunchKernelGGL(pk_rank_book_packed<16>, grid, dim3(64), lds * per, c->stream, b); break;
    case 32: hipLaunchKernelGGL(pk_rank_book_packed<32>, grid, dim3(64), lds * per, c->stream, b); break;
    case 64: hipLaunchKernelGGL(pk_rank_book_packed<64>, grid, dim3(64), lds * per, c->stream, b); break;
    default: return fail(c, PHYLO_ESTATE, "step_book: no pk_rank_book_packed of %d lanes", w);
    }
    return launch_check(c, "pk_rank_book_packed");
}

// The merge of a rank event: one wave per (particle, site tile) when nothing is stored -- from the merge records, or resolving
// ids -- and pk_rank_merge only when the node is stored
static int step_merge(phylo_ctx* c, const pk_rank_args& b) {
    const sweep_plan& p = c->run.plan;
    const int S = c->S;
    const dim3 mgrid((unsigned)((size_t)c->Kloc * c->ntiles));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (p.timek && !p.twist) { e0 = c->kev[2 * b.r]; e1 = c->kev[2 * b.r + 1]; }
    if (!(b.lazy || b.no_store)) {
        const size_t lds = (size_t)(c->site_tile < S ? c->site_tile : S) * 8 + 16 + PK_STORE_STAGE_BYTES;
        launch_stamped(pk_rank_merge, mgrid, dim3(PK_COLS), lds, c->stream, e0, e1, b);
    } else if (b.rec) {
        // pi by value, from the pinned image of the model upload.  Invariant: phylo_set_model is the only writer of d_Q / d_pi and
        // of that image, and it rewrites the image only after the previous upload has finished, so for every launch issued after
        // it returns the image equals the model the other kernels read from d_pi.  A model update made on the device would have
        // to refresh the image too.
        pk_pi4 pi4;
        memcpy(pi4.v, c->h_model_p + 16, sizeof pi4.v);
        // the pattern form: the table's LDS and U go with the launch; U = 0 is today's form
        pk_pat_args pat = {nullptr, nullptr, 0, 0, 0u, 0u, nullptr};
        size_t lds = 0;
        if (p.clade_pat) {                                 // (implies pat_on: sweep_facts_of)
            const pk_clade_layout& L = c->clade_layout;
            pat.clade = (const char*)c->d_clade + L.codes_bytes;
            pat.cstride = (unsigned int)L.stride; pat.crep = (unsigned int)L.rep_bytes;
            pat.rep_delta = (long long)(c->d_clade - c->d_leaf_packed);
            pat.U = c->pat_U;
            lds = pk_pat_lds_bytes(c->pat_U);
        } else if (pat_on(c)) {
            pat.pimg = (const char*)c->d_pat;
            pat.roff = (const char*)c->d_pat + pk_pat_image_bytes(S);
            pat.rep_delta = (long long)((c->d_pat + pk_pat_image_bytes(S) + pk_pat_rep_bytes()) - c->d_leaf_packed);
            pat.U = c->pat_U;
            lds = pk_pat_lds_bytes(c->pat_U);
        }
        // which wave takes which item: phylo_launch_map.h, by the plan's launch_xcd (the kernel reads it off the sign of the count)
        const int n = (int)mgrid.x, grid = pk_launch_grid(n, 1, p.launch_xcd), n_xcd = p.launch_xcd ? -n : n;
        launch_stamped(pk_rank_merge_nostore, dim3((unsigned)grid), dim3(64), lds, c->stream, e0, e1, (const unsigned long long*)b.rec, b.Pmat,
                       S, b.T, b.ntiles, n_xcd, b.tilev, pi4, pat);
    } else {
        launch_stamped(pk_rank_merge_nostore_ids, mgrid, dim3(64), 0, c->stream, e0, e1, b);
    }
    return launch_check(c, "pk_rank_merge");
}

// rows longer than one tile: tile values left to right, then the particle's weight terms
static int step_tiles(phylo_ctx* c, const pk_rank_args& b) {
    hipLaunchKernelGGL(pk_tile_epilogue, dim3(cdiv(c->Kloc, 256)), dim3(256), 0, c->stream, b);
    return launch_check(c, "pk_tile_epilogue");
}

// the all-gather of the rank event's three K-vectors (nothing without a communicator)
static int step_exchange(phylo_ctx* c, int r) {
    const size_t K = c->K;
    double* rows[3] = {c->d_logw + r * K, c->d_ll + r * K, c->d_nodell + c->N + r * K};
    return comm_exchange(c, rows, 3, (size_t)c->Kloc, 0);
}

// replicated tables: the new roots' log-likelihoods of the other ranks' particles, known since the exchange
static int step_fix_rootll(phylo_ctx* c, int r) {
    const int N = c->N, K = c->K;
    double* rootll_new = c->run.plan.graph ? c->d_hrootll + (size_t)K * N * (r + 1) : c->d_rootll[(r & 1) ^ 1];
    hipLaunchKernelGGL(pk_fix_rootll, dim3(cdiv(K, 256)), dim3(256), 0, c->stream, rootll_new,
                       (const double*)(c->d_nodell + N + (size_t)r * K), K, N, N - r, c->k0, c->Kloc);
    return launch_check(c, "pk_fix_rootll");
}

// the resampling scan of the rank event's weights, one workgroup set per batched sweep; the last one also sums the log-normalisers
static int step_scan(phylo_ctx* c, int r) {
    const sweep_plan& p = c->run.plan;
    const bool last = r + 1 == p.R;
    pp_anc_out ao{};
    if (c->run.chain.taken && !last) {                     // the resampling outcome of rank event r + 1
        ao.anc = c->d_anc_next; ao.list = c->d_adopt_list; ao.cnt = c->d_adopt_cnt;
        ao.group_seeds = p.G > 1 ? c->d_group_seeds : nullptr; ao.seed = c->run.seed; ao.r_next = (uint32_t)(r + 1);
    }
    return launch_scan(c, (const double*)(c->d_logw + (size_t)r * c->K), p.Kg, p.G, last ? (uint64_t*)nullptr : c->d_cdf[(r & 1) ^ 1],
                       c->d_lse + r, p.lse_stride, (last && p.fold_logz) ? p.R : 0, ao.anc ? &ao : nullptr);
}

// phase 0: the whole rank event; 1: up to and including the merge; 2: what follows the all-gather of the rank
// event's three K-vectors (phylo_sweep_step_group issues that collective once for several sweeps)
static int sweep_step_impl(phylo_ctx* c, int phase) {
    CHK(bind(c));
    if (!c->run.active) return fail(c, PHYLO_ESTATE, "phylo_sweep_step without phylo_sweep_begin");
    const sweep_plan& p = c->run.plan;
    const int r = c->run.next_r;
    if (r >= p.R) return fail(c, PHYLO_ESTATE, "all %d rank events of this sweep have been issued", p.R);
    if (phase != 2) {
        if (c->run.a_done_r != r) CHK(sweep_step_a(c));
        const pk_rank_args b = rank_args(c, r);
        if (p.twist) CHK(step_twist(c, b));
        else CHK(step_book(c, b));
        if (p.mat_after_book && r > 0) CHK(step_materialize(c, b));
        CHK(step_merge(c, b));
        if (p.tile_epilogue) CHK(step_tiles(c, b));
    }
    if (phase == 0) CHK(step_exchange(c, r));
    if (phase == 1) return PHYLO_OK;
    if (p.fix_rootll) CHK(step_fix_rootll(c, r));
    CHK(step_scan(c, r));
    c->run.launches += sweep_plan_launches(p, r);
    ++c->run.next_r;
    return PHYLO_OK;
}

int phylo_sweep_step(phylo_ctx* c) { return sweep_step_impl(c, 0); }

int phylo_sweep_step_a(phylo_ctx* c) { return sweep_step_a(c); }

int phylo_sweep_step_group(phylo_ctx** ctxs, int n) {
    if (!ctxs || n < 1) return fail(nullptr, PHYLO_EINVAL, "phylo_sweep_step_group needs at least one context");
    for (int i = 0; i < n; ++i)
        if (!ctxs[i]) return fail(nullptr, PHYLO_EINVAL, "NULL context");
    if (n == 1 || ctxs[0]->comm.transport == 0) {          // nothing to fuse
        for (int i = 0; i < n; ++i) CHK(sweep_step_impl(ctxs[i], 0));
        return PHYLO_OK;
    }
    for (int i = 0; i < n; ++i) {
        if (!ctxs[i]->run.active || ctxs[i]->run.next_r != ctxs[0]->run.next_r)
            return fail(ctxs[i], PHYLO_ESTATE, "the sweeps of a group must be at the same rank event");
        if (&phylo_comm_link(ctxs[i]->comm) != &phylo_comm_link(ctxs[0]->comm))
            return fail(ctxs[i], PHYLO_EINVAL, "the contexts of a group must share one communicator (phylo_comm_share)");
    }
    for (int i = 0; i < n; ++i) CHK(sweep_step_impl(ctxs[i], 1));
    std::vector<phylo_comm*> comms(n);
    std::vector<double*> rows((size_t)3 * n);
    std::vector<hipStream_t> streams(n);
    for (int i = 0; i < n; ++i) {
        phylo_ctx* c = ctxs[i];
        const size_t r = (size_t)c->run.next_r, K = c->K;
        comms[i] = &c->comm;
        streams[i] = c->stream;
        rows[3 * i] = c->d_logw + r * K;
        rows[3 * i + 1] = c->d_ll + r * K;
        rows[3 * i + 2] = c->d_nodell + c->N + r * K;
    }
    if (ctxs[0]->p2p) {                                    // device-side exchange: every context has its own slab and flags
        for (int i = 0; i < n; ++i) {
            if (!ctxs[i]->p2p) return fail(ctxs[i], PHYLO_EINVAL, "the contexts of a group must use the same exchange");
            CHK(comm_exchange(ctxs[i], rows.data() + 3 * (size_t)i, 3, (size_t)ctxs[i]->Kloc, 0));
        }
    } else {
        phylo_ctx* c0 = ctxs[0];
        std::vector<size_t> counts(n);
        for (int i = 0; i < n; ++i) counts[i] = (size_t)ctxs[i]->Kloc;
        int rc = phylo_comm_allgather_group(comms.data(), rows.data(), 3, counts.data(), streams.data(), n, &c0->err);
        if (rc != PHYLO_OK) { g_last_error = c0->err; return rc; }
    }
    for (int i = 0; i < n; ++i) CHK(sweep_step_impl(ctxs[i], 2));
    return PHYLO_OK;
}

// Sharded PHYLO_KEEP_GRAPH, behind the last rank event: every rank's records of its particles (children, branch lengths, matrices,
// ancestors) into whole-K arrays on every rank (pk_gx_pack / pk_gx_unpack).  Node rows are not copied: the reverse pass reads
// them from their owners' pools over the peer mappings (pg_node_row).  Device-side exchange: barrier, the peers' buffers read
// over the mappings, barrier (nobody packs again before every reader is done); collective path: the all-gather of the buffers in
// chunks, then the same tail.  A collective: every rank's sweep ends here.
static int graph_gather(phylo_ctx* c) {
    const int K = c->K, Kl = c->Kloc, R = c->N - 1;
    pk_gx_args a{};
    a.world = c->world; a.me = c->rank; a.Kloc = Kl; a.K = K;
    a.seg = c->gx_seg; a.cl = c->gx_cl;
    a.xbuf = c->d_gx; a.xsrc = c->d_gx_src;
    int nf = 0;
    auto field = [&](const void* src, size_t stride, size_t off, void* dst, int rows, int w, int wide) {
        pk_gx_field& f = a.f[nf++];
        f.src = src; f.src_stride = stride; f.src_off = off; f.dst = dst; f.rows = rows; f.w = w; f.wide = wide;
    };
    field(c->d_child, (size_t)Kl * 2, 0, c->d_gchild, R, 2, 0);
    field(c->d_bl, (size_t)Kl, 0, c->d_gbl, R, 1, 1);
    field(c->d_br, (size_t)Kl, 0, c->d_gbr, R, 1, 1);
    field(c->d_Pmat, (size_t)Kl * 32, 0, c->d_gPmat, R, 32, 1);
    if (R > 1) field(c->d_anc, (size_t)Kl, 0, c->d_ganc, R - 1, 1, 1);
    a.n_fields = nf;
    {   // (the word count the buffer was sized for)
        size_t words = 0;
        for (int i = 0; i < nf; ++i) words += (size_t)a.f[i].rows * Kl * a.f[i].w;
        if (words != a.seg) return fail(c, PHYLO_EINVAL, "graph_gather: %zu words against a buffer of %zu per rank", words, a.seg);
    }
    const unsigned pack_wgs = (unsigned)(a.seg / 256 + 1 < 2048 ? a.seg / 256 + 1 : 2048);
    hipLaunchKernelGGL(pk_gx_pack, dim3(pack_wgs), dim3(256), 0, c->stream, a);
    CHK(launch_check(c, "pk_gx_pack"));
    if (c->p2p) {
        CHK(comm_exchange(c, nullptr, 0, 0, 1));
    } else {
        const size_t chunks = (a.seg + a.cl - 1) / a.cl;
        for (size_t j = 0; j < chunks; ++j) {
            double* arr[1] = {reinterpret_cast<double*>(c->d_gx + j * (size_t)c->world * a.cl)};
            int rc = phylo_comm_allgather_inplace(c->comm, arr, 1, a.cl, c->stream, &c->err);
            if (rc != PHYLO_OK) return rc;
        }
    }
    const size_t total = a.seg * (size_t)c->world;
    hipLaunchKernelGGL(pk_gx_unpack, dim3((unsigned)(total / 256 + 1 < 4096 ? total / 256 + 1 : 4096)), dim3(256), 0, c->stream, a);
    CHK(launch_check(c, "pk_gx_unpack"));
    return comm_exchange(c, nullptr, 0, 0, 1);
}

int phylo_sweep_finish(phylo_ctx* c) {
    CHK(bind(c));
    const int N = c->N, Kl = c->Kloc, S = c->S, R = N - 1;
    if (!c->run.active || c->run.next_r != R)
        return fail(c, PHYLO_ESTATE, "phylo_sweep_finish needs phylo_sweep_begin and all %d phylo_sweep_step calls", R);
    const sweep_plan& p = c->run.plan;
    if (!p.fold_logz) {
        if (p.G > 1)
            hipLaunchKernelGGL(pk_logz_total_groups, dim3(p.G), dim3(64), 0, c->stream, c->d_lse, R, R + 1);
        else
            hipLaunchKernelGGL(pk_logz_total, dim3(1), dim3(64), 0, c->stream, (const double*)c->d_lse, R, c->d_lse + R);
        CHK(launch_check(c, "pk_logz_total"));
    }
    if (p.gather_launches) CHK(graph_gather(c));           // sharded: the reverse pass reads the whole graph on every rank
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    if (p.graph) {                                         // the reverse pass builds its lists from these on the host
        pg_copy3 cp{};                                     // (by a kernel into the pinned buffers: pg_copy_words says why)
        const bool whole = c->world > 1;
        cp.src[0] = (const uint32_t*)(whole ? c->d_ganc : c->d_anc); cp.dst[0] = c->hd_anc; cp.n[0] = R > 1 ? (size_t)(R - 1) * c->K * 2 : 0;
        cp.src[1] = (const uint32_t*)(whole ? c->d_gchild : c->d_child); cp.dst[1] = c->hd_child; cp.n[1] = (size_t)R * c->K * 2;
        if (p.twist) { cp.src[2] = (const uint32_t*)c->d_hroots_ad; cp.dst[2] = c->hd_rad; cp.n[2] = (size_t)R * c->K * N; }
        // ... and what phylo_sweep_fetch would otherwise copy one by one: log Z-hat, the timeout word of the bounded waits
        cp.src[3] = (const uint32_t*)(c->d_lse + R); cp.dst[3] = c->hd_pub; cp.n[3] = 2;
        cp.src[4] = (const uint32_t*)(c->d_counter + 1); cp.dst[4] = c->hd_pub + 2; cp.n[4] = 1;
        const size_t words = cp.n[0] + cp.n[1] + cp.n[2];
        hipLaunchKernelGGL(pg_copy_words, dim3((unsigned)(words / 1024 < 1 ? 1 : (words / 1024 > 1024 ? 1024 : words / 1024))), dim3(256), 0, c->stream, cp);
        CHK(launch_check(c, "pg_copy_words"));
        HIPCHK(c, hipEventRecord(c->ev_gcopy, c->stream));
    }
    c->run.active = false;
    sweep_publish(c, p.lazy, p.graph, p.G, p.final_missing, p.timek ? R : 0, c->run.launches + sweep_plan_launches(p, R),
                  (double)Kl * S * R);
    c->last_graph_twist = p.graph && p.twist;
    c->last_graph_marks = p.graph && p.lazy;
    c->last_graph_eager = p.last_graph_eager;
    c->last_M = c->run.M;
    if (p.twist) {                                         // + K M S C(N+1,3) look-ahead merges, 64 B each (no store)
        const double ut = (double)Kl * c->run.M * S * ((double)(N + 1) * N * (N - 1) / 6.0);
        c->stats.units += ut;
        c->stats.alg_bytes += 64.0 * ut;
    }
    return PHYLO_OK;
}

int phylo_sweep_async(phylo_ctx* c, uint64_t seed, uint32_t flags, int M) {
    if (!c) return fail(nullptr, PHYLO_EINVAL, "ctx is NULL");
    int Wg = 0, m = 0;
    if (persist_plan(c, flags, 1, &Wg, &m)) return sweep_persistent(c, seed, flags, nullptr, 1, Wg, m);
    c->last_persistent = false;
    CHK(phylo_sweep_begin(c, seed, flags, M));
    for (int r = 0; r < c->N - 1; ++r) CHK(phylo_sweep_step(c));
    return phylo_sweep_finish(c);
}

int phylo_sweep_batch_begin(phylo_ctx* c, const uint64_t* seeds, int G, uint32_t flags) {
    if (!c) return fail(nullptr, PHYLO_EINVAL, "ctx is NULL");
    if (!seeds) return fail(c, PHYLO_EINVAL, "seeds is NULL");
    c->h_group_seeds.assign(seeds, seeds + (G > 0 ? G : 0));          // stays alive until the copy has run
    return sweep_begin_impl(c, G > 0 ? seeds[0] : 0, flags, 1, c->h_group_seeds.data(), G);
}

int phylo_sweep_batch_async(phylo_ctx* c, const uint64_t* seeds, int G, uint32_t flags) {
    if (!c) return fail(nullptr, PHYLO_EINVAL, "ctx is NULL");
    int Wg = 0, m = 0;
    if (seeds && G >= 1 && G <= PK_MAX_GROUPS && c->K % G == 0 && persist_plan(c, flags, G, &Wg, &m)) {
        c->h_group_seeds.assign(seeds, seeds + G);          // stays alive until the copy has run
        return sweep_persistent(c, seeds[0], flags, c->h_group_seeds.data(), G, Wg, m);
    }
    c->last_persistent = false;
    CHK(phylo_sweep_batch_begin(c, seeds, G, flags));
    for (int r = 0; r < c->N - 1; ++r) CHK(phylo_sweep_step(c));
    return phylo_sweep_finish(c);
}

static int check_timeout_word(phylo_ctx* c, bool pub);

int phylo_sweep_fetch_logz(phylo_ctx* c, double* logZ, int G) {
    CHK(bind(c));
    if (!c->swept) return fail(c, PHYLO_ESTATE, "no sweep has been run");
    if (!logZ || G != c->last_G) return fail(c, PHYLO_EINVAL, "the last sweep batched %d sweep(s), asked for %d", c->last_G, G);
    const size_t R = (size_t)c->N - 1;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    CHK(check_timeout_word(c, false));
    std::vector<double> all((R + 1) * G);
    HIPCHK(c, hipMemcpy(all.data(), c->d_lse, all.size() * 8, hipMemcpyDeviceToHost));
    for (int g = 0; g < G; ++g) logZ[g] = all[g * (R + 1) + R];
    return PHYLO_OK;
}

int phylo_synchronize(phylo_ctx* c) {
    CHK(bind(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

// The word every bounded wait between workgroups sets when it gives up (one-launch sweep, device-side exchange): a sweep that
// timed out is invalid.  The stream must be idle.  `pub`: the sweep's copy kernel left the word in pinned memory.
static int check_timeout_word(phylo_ctx* c, bool pub) {
    unsigned int tmo = 0;
    if (pub) tmo = c->h_pub[2];
    else HIPCHK(c, hipMemcpy(&tmo, c->d_counter + 1, sizeof tmo, hipMemcpyDeviceToHost));
    if (tmo) {
        HIPCHK(c, hipMemset(c->d_counter + 1, 0, sizeof tmo));
        c->pctr_dirty = true;                              // the one-launch sweep's arrival counters hold partial arrivals
        return fail(c, PHYLO_EHIP, "a bounded wait between workgroups timed out inside a launch; results are invalid");
    }
    return PHYLO_OK;
}

int phylo_sweep_fetch(phylo_ctx* c, double* log_weights, double* log_lik, double* lbranch, double* rbranch,
                      int32_t* merges, int64_t* ancestors, double* logZ, phylo_stats* perf) {
    CHK(bind(c));
    if (!c->swept) return fail(c, PHYLO_ESTATE, "no sweep has been run");
    const size_t R = (size_t)c->N - 1, K = c->K, Kl = c->Kloc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const bool pub = c->last_graph && c->h_pub;            // the sweep kept its graph: its copy kernel left these in pinned memory
    CHK(check_timeout_word(c, pub));
    // log_weights / log_lik are stored with global columns; hand back this rank's columns
    if (Kl == K) {                      // one rank: rows are contiguous
        if (log_weights) HIPCHK(c, hipMemcpy(log_weights, c->d_logw, R * K * 8, hipMemcpyDeviceToHost));
        if (log_lik) HIPCHK(c, hipMemcpy(log_lik, c->d_ll, R * K * 8, hipMemcpyDeviceToHost));
    } else {
        if (log_weights)
            HIPCHK(c, hipMemcpy2D(log_weights, Kl * 8, c->d_logw + c->k0, K * 8, Kl * 8, R, hipMemcpyDeviceToHost));
        if (log_lik) HIPCHK(c, hipMemcpy2D(log_lik, Kl * 8, c->d_ll + c->k0, K * 8, Kl * 8, R, hipMemcpyDeviceToHost));
    }
    if (lbranch) HIPCHK(c, hipMemcpy(lbranch, c->d_bl, R * Kl * 8, hipMemcpyDeviceToHost));
    if (rbranch) HIPCHK(c, hipMemcpy(rbranch, c->d_br, R * Kl * 8, hipMemcpyDeviceToHost));
    if (merges) HIPCHK(c, hipMemcpy(merges, c->d_merges, R * Kl * 2 * 4, hipMemcpyDeviceToHost));
    if (ancestors && R > 1) HIPCHK(c, hipMemcpy(ancestors, c->d_anc, (R - 1) * Kl * 8, hipMemcpyDeviceToHost));
    if (logZ) {
        if (pub) memcpy(logZ, c->h_pub, 8);
        else HIPCHK(c, hipMemcpy(logZ, c->d_lse + R, 8, hipMemcpyDeviceToHost));
    }
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    c->stats.sweep_ms = ms;
    c->stats.merge_ms = 0.0;
    c->stats.merge_launches = c->n_merge_events;
    for (int r = 0; r < c->n_merge_events; ++r) {
        float km = 0.f;
        HIPCHK(c, hipEventElapsedTime(&km, c->kev[2 * r], c->kev[2 * r + 1]));
        c->stats.merge_ms += km;
    }
    if (perf) *perf = c->stats;
    return PHYLO_OK;
}

int phylo_sweep(phylo_ctx* c, uint64_t seed, uint32_t flags, int M, double* log_weights, double* log_lik,
                double* lbranch, double* rbranch, int32_t* merges, int64_t* ancestors, double* logZ,
                phylo_stats* perf) {
    CHK(phylo_sweep_async(c, seed, flags, M));
    return phylo_sweep_fetch(c, log_weights, log_lik, lbranch, rbranch, merges, ancestors, logZ, perf);
}

int phylo_sweep_node(phylo_ctx* c, int r, int k, double* out) {
    CHK(bind(c));
    if (!c->swept) return fail(c, PHYLO_ESTATE, "no sweep has been run");
    if (c->leaves_newer)                // the nodes not yet written would come from the new leaves under the old sweep's records
        return fail(c, PHYLO_ESTATE, "phylo_set_leaves has been called since the last sweep: its nodes belong to the old leaves");
    if (r < 0 || r >= c->N - 1 || k < 0 || k >= c->Kloc || !out) return fail(c, PHYLO_EINVAL, "bad (r, k)");
    if (c->last_lazy) {                 // write every node that the lazy sweep skipped, oldest rank event first
        // a kept graph on one GPU is then what an eager sweep leaves: every node stored, marks that no longer say who was adopted.
        // rev_marks writes those again from the ancestors, so that the reverse pass has the same bits before and after this call
        if (c->last_graph && c->last_graph_marks && c->world == 1 && c->Kloc == c->K) c->last_graph_eager = true;
        pk_rank_args b{};
        b.N = c->N; b.S = c->S; b.K = c->K; b.Kloc = c->Kloc; b.k0 = c->k0;
        b.leaves = c->d_leaves; b.pool = c->d_pool; b.pool_ptrs = c->d_pool_ptrs;
        b.mark = c->d_mark; b.child_all = c->d_child; b.Pmat_all = c->d_Pmat;
        for (int rho = 0; rho < c->N - 1; ++rho) {       // sharded: a collective (every rank must call phylo_sweep_node)
            hipLaunchKernelGGL(pk_materialize_rank, dim3(c->Kloc), dim3(PK_COLS), 0, c->stream, b, rho);
            CHK(launch_check(c, "pk_materialize_rank"));
            c->last_graph_marks = false;                   // the marks now cover more than the adopted nodes
            if (c->comm.transport != 0) {
                CHK(comm_exchange(c, nullptr, 0, 0, 1));
            }
        }
        c->last_lazy = false;
    }
    if (c->last_final_missing && r == c->N - 2) {        // the sweep did not store the last rank event's nodes: write them now
        pk_rank_args b{};
        b.N = c->N; b.S = c->S; b.K = c->K; b.Kloc = c->Kloc; b.k0 = c->k0;
        b.leaves = c->d_leaves; b.pool = c->d_pool; b.pool_ptrs = c->d_pool_ptrs;
        b.child_all = c->d_child; b.Pmat_all = c->d_Pmat;
        hipLaunchKernelGGL(pk_materialize_all, dim3(c->Kloc), dim3(PK_COLS), 0, c->stream, b, c->N - 2);
        CHK(launch_check(c, "pk_materialize_all"));
        c->last_final_missing = false;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t node_sz = (size_t)c->S * 4;
    HIPCHK(c, hipMemcpy(out, c->d_pool + ((size_t)r * c->Kloc + k) * node_sz, node_sz * 8, hipMemcpyDeviceToHost));
    return PHYLO_OK;
}

// ---- the reverse pass's integer lists built on the device (phylo_revlists_dev.h): launches, then the few integers the host needs
static unsigned bit_length(size_t v) { unsigned b = 0; while (v) { ++b; v >>= 1; } return b ? b : 1; }
extern "C++" {
template <int ITEMS>
static int dev_lists_adopters(phylo_ctx* c, const pg_dl_args& d, hipStream_t s) {
    const size_t lds = pg_dl_sort<ITEMS>::storage_bytes + (size_t)d.Kg * 4;
    static bool raised = false;                            // (beyond the 64 KB every kernel may ask for: say so once)
    if (lds > 65536 && !raised) {
        HIPCHK(c, hipFuncSetAttribute((const void*)pg_dl_adopters<ITEMS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        raised = true;
    }
    hipLaunchKernelGGL(pg_dl_adopters<ITEMS>, dim3(d.R, d.K / d.Kg), dim3(PG_DL_BLOCK), lds, s, d, bit_length((size_t)d.Kg));
    return launch_check(c, "pg_dl_adopters");
}
}  // extern "C++"
// The list kernels on sL; ev_dl is recorded when the lists that the coefficient chain and the host need are there (pg_dl_lists);
// the parents' sort on sS (sort = false: the caller issues it later with dev_lists_sort).  Nothing here waits for the host;
// dev_lists_wait does.
static int dev_lists_launch(phylo_ctx* c, hipStream_t sL, hipStream_t sS, bool kernels = true, bool sort = true) {
    const int N = c->N, K = c->K, R = N - 1;
    const size_t nn = (size_t)R * K, nb = (nn + PG_DL_BLOCK - 1) / PG_DL_BLOCK;
    const size_t meta_ints = (size_t)PG_DL_META_INTS(R);
    void* ws = nullptr;
    CHK(scratch_get(c, 8, (8 * nn + 4 * nb + meta_ints + 32) * 4, &ws));
    pg_dl_args d{};
    d.N = N; d.R = R; d.K = K;
    d.Kg = c->last_graph ? K / c->last_G : K;              // (a genealogy given by a test hook: one group)
    d.anc = c->d_anc; d.child = c->d_child;
    int32_t* w = (int32_t*)ws;
    d.cnt_par = w; d.ticket = w + nn; w += nn + 16;
    d.adopted = w; w += nn;
    d.bsum = w; w += 4 * nb;
    d.dmeta = w; w += meta_ints;
    c->d_dlmeta = d.dmeta;
    d.pkey = (uint32_t*)w; d.pval = (uint32_t*)w + 2 * nn; w += 4 * nn;
    uint32_t* pkey_out = (uint32_t*)w;
    d.L = pg_lists_carve(c->d_ad_off, (size_t)R, (size_t)K);
    d.meta = c->hd_dlmeta;
    const unsigned pbits = bit_length(2 * nn);
    if (c->dl_temp_nn != nn) {                             // (the size query launches nothing)
        size_t tp = 0;
        HIPCHK(c, rocprim::radix_sort_pairs(nullptr, tp, d.pkey, pkey_out, d.pval, (uint32_t*)d.L.par_idx, 2 * nn, 0u, pbits, sL));
        c->dl_temp_p = tp; c->dl_temp_nn = nn;
    }
    void* tp = nullptr;
    CHK(scratch_get(c, 9, c->dl_temp_p + 16, &tp));
    if (kernels) {
        if (d.Kg <= 1024) CHK(dev_lists_adopters<1>(c, d, sL));
        else if (d.Kg <= 2048) CHK(dev_lists_adopters<2>(c, d, sL));
        else if (d.Kg <= 4096) CHK(dev_lists_adopters<4>(c, d, sL));
        else CHK(dev_lists_adopters<8>(c, d, sL));
        if (R > 1) {
            hipLaunchKernelGGL(pg_dl_count, dim3(cdiv((long)(2 * nn - 2 * (size_t)K), 256)), dim3(256), 0, sL, d);
            CHK(launch_check(c, "pg_dl_count"));
        }
        hipLaunchKernelGGL(pg_dl_sums, dim3((unsigned)nb), dim3(PG_DL_BLOCK), 0, sL, d);
        CHK(launch_check(c, "pg_dl_sums"));
        hipLaunchKernelGGL(pg_dl_lists, dim3((unsigned)nb), dim3(PG_DL_BLOCK), 0, sL, d);
        CHK(launch_check(c, "pg_dl_lists"));
        HIPCHK(c, hipEventRecord(c->ev_dl, sL));
    }
    if (!sort) return PHYLO_OK;
    sL = sS;
    // the parents' sort: six small launches through rocPRIM's host code, 8 us of host time each -- captured once per shape (the
    // buffers are the context's own and stay where they are), replayed with one call
    const void* key[4] = {ws, tp, (const void*)c->d_ad_off, (const void*)nn};
    if (c->dl_graph && memcmp(key, c->dl_graph_key, sizeof key) != 0) {
        (void)hipGraphExecDestroy(c->dl_graph);
        c->dl_graph = nullptr;
    }
    if (!c->dl_graph && !c->dl_no_graph) {
        hipGraph_t gr = nullptr;
        bool ok = hipStreamBeginCapture(sL, hipStreamCaptureModeThreadLocal) == hipSuccess;
        if (ok) {
            size_t bytes = c->dl_temp_p;
            const hipError_t e1 = rocprim::radix_sort_pairs(tp, bytes, d.pkey, pkey_out, d.pval, (uint32_t*)d.L.par_idx, 2 * nn, 0u, pbits, sL);
            const hipError_t e2 = hipStreamEndCapture(sL, &gr);
            ok = e1 == hipSuccess && e2 == hipSuccess && gr && hipGraphInstantiate(&c->dl_graph, gr, nullptr, nullptr, 0) == hipSuccess;
            if (gr) (void)hipGraphDestroy(gr);
        }
        if (!ok) {                                         // no capture on this runtime: the plain launches every time
            (void)hipGetLastError();
            c->dl_graph = nullptr;
            c->dl_no_graph = true;
        } else {
            memcpy(c->dl_graph_key, key, sizeof key);
        }
    }
    if (c->dl_graph) {
        HIPCHK(c, hipGraphLaunch(c->dl_graph, sL));
        } else {
        size_t bytes = c->dl_temp_p;
        HIPCHK(c, rocprim::radix_sort_pairs(tp, bytes, d.pkey, pkey_out, d.pval, (uint32_t*)d.L.par_idx, 2 * nn, 0u, pbits, sL));
    }
    return PHYLO_OK;
}
static int dev_lists_wait(phylo_ctx* c, pg_list_counts& m) {
    CHK(wait_event_spin(c, c->ev_dl));
    const int R = c->N - 1;
    const int32_t* h = c->h_dlmeta;
    m.ev_adp0.assign(h, h + R + 1);
    m.ev_slow0.assign(h + R + 1, h + 2 * (R + 1));
    m.rank_chunk0.assign((size_t)R + 1, 0);                // (heavy[] holds global chunk indices)
    const int32_t* t = h + 2 * (R + 1);
    m.n_adp = t[0]; m.n_chunks = (size_t)t[1]; m.max_chunks = 0; m.n_slow = t[2]; m.n_par = t[3];
    return PHYLO_OK;
}

static int sweep_backward_impl(phylo_ctx* c, double* d_lam_l, double* d_lam_r, double* d_pi, double* d_Q, phylo_stats* perf, int G);
// reverse passes in flight in this process (several host threads, each with its own context): a launch that waits inside the GPU for
// another launch of its own pass (pg_nodes_rows_all beside pg_coeff_all) assumes the two share the GPU with nobody who waits likewise
static std::atomic<int> g_backward_in_flight{0};

// G = 0: phylo_sweep_backward (one system); G >= 1: phylo_sweep_backward_batch, a row per group of the last sweep
static int sweep_backward_guarded(phylo_ctx* c, double* d_lam_l, double* d_lam_r, double* d_pi, double* d_Q, phylo_stats* perf, int G) {
    if (c && c->swept && c->last_graph) {                  // the wrong call for the kept graph: refused, the graph stays
        if (G == 0 && c->last_G > 1)
            return fail(c, PHYLO_ESTATE, "the last sweep batched %d systems: phylo_sweep_backward_batch returns a gradient per system", c->last_G);
        if (G != 0 && G != c->last_G)
            return fail(c, PHYLO_EINVAL, "phylo_sweep_backward_batch: the last sweep batched %d system(s), asked for %d", c->last_G, G);
    }
    struct in_flight { in_flight() { ++g_backward_in_flight; } ~in_flight() { --g_backward_in_flight; } } guard;
    const int rc = sweep_backward_impl(c, d_lam_l, d_lam_r, d_pi, d_Q, perf, G);
    if (rc != PHYLO_OK && c) {
        // an early return may have left kernels on the side streams that still read the pinned list image and the graph: join them
        // before anything rebuilds or frees those, and drop the graph (the next backward needs a new sweep)
        if (c->gstream) (void)hipStreamSynchronize(c->gstream);
        if (c->bgstream) (void)hipStreamSynchronize(c->bgstream);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        c->last_graph = false;
    }
    return rc;
}

int phylo_sweep_backward(phylo_ctx* c, double* d_lam_l, double* d_lam_r, double* d_pi, double* d_Q, phylo_stats* perf) {
    return sweep_backward_guarded(c, d_lam_l, d_lam_r, d_pi, d_Q, perf, 0);
}

int phylo_sweep_backward_batch(phylo_ctx* c, double* d_lam_l, double* d_lam_r, double* d_pi, double* d_Q, int G, phylo_stats* perf) {
    if (G < 1) return fail(c, PHYLO_EINVAL, "phylo_sweep_backward_batch needs G >= 1 (got %d)", G);
    return sweep_backward_guarded(c, d_lam_l, d_lam_r, d_pi, d_Q, perf, G);
}

// ---- the reverse pass's driver ("driver"): the form is decided in phylo_revlists.h (pg_plan_form before the
//      first launch, pg_plan_chains once the lists' counts are known); the stages below read the plan and issue the pass in the
//      order sweep_backward_impl names them.  The order of the HIP calls on each stream, and where the host builders run between
//      them, is what the measurements in the comments paid for.
struct rev_pass {
    phylo_ctx* c = nullptr;
    pg_args g{};
    pg_plan plan{};
    pg_list_counts n;                    // the lists' counts, from the host builders or from pg_dl_lists
    pg_lookahead x;                      // twisted proposal: the look-ahead lists' counts
    pg_lists L{};                        // the pinned image of the device slab (what the host builders write)
    const int64_t* anc = nullptr;        // the ancestors the host builders read (a batched sweep's: with global indices)
    bool batch = false;                  // phylo_sweep_backward_batch: a row per group, the groups' log Z-hat behind them
    hipStream_t sB = nullptr;            // the adopted nodes' chain: the second stream (plan.two), else the context's
    int node_launches = 0, tw_launches = 0, mark_launches = 0;
    std::chrono::steady_clock::time_point host_t0;
    double host_ms = 0.0;
};

static pg_plan_in rev_plan_in(const phylo_ctx* c) {
    pg_plan_in in{};
    in.N = c->N; in.K = c->K; in.K_local = c->Kloc; in.S = c->S; in.world = c->world;
    in.twist = c->last_graph_twist; in.marks = c->last_graph_marks;
    in.rev_host_lists = c->env.rev_host_lists; in.one_stream = c->env.grad_one_stream; in.two_streams = c->env.grad_two_streams;
    in.rows_chain = c->env.grad_rows_chain; in.coeff_chain = c->env.grad_coeff_chain;
    in.dl_max_k = PG_DL_MAX_K;
    in.groups = c->last_G;
    return in;
}

// (0.) After a sweep that stored every node (PHYLO_EAGER_NODES) nothing marked the adopted ones.  The marks say who was adopted and
// nothing else, and the ancestors say that too: written here, once per sweep, they give such a sweep the reverse pass of a lazy one
// -- the same launches, the same sums in the same order, the same bits -- instead of the form without marks (which the twisted
// proposal, S > 4096 and, on a sharded context, phylo_sweep_node's widened marks still take).  phylo_sweep_node on one GPU asks
// for the same: its widened marks are written again here, and the pass before and after that call has the same bits.
static int rev_marks(rev_pass& p) {
    phylo_ctx* c = p.c;
    if (c->last_graph_marks || !c->last_graph_eager) return PHYLO_OK;
    const int R = c->N - 1, K = c->K;
    const size_t mark_words = ((size_t)R * K + R + 3) & ~(size_t)3;
    HIPCHK(c, hipMemsetAsync(c->d_mark, 0, mark_words * sizeof(unsigned int), c->stream));
    if (R > 1) {
        hipLaunchKernelGGL(pg_mark_adopted_dev, dim3(cdiv((long)(R - 1) * K, 256)), dim3(256), 0, c->stream, (const int64_t*)c->d_anc, c->d_mark,
                           R, K, K / c->last_G);
        CHK(launch_check(c, "pg_mark_adopted_dev"));
    }
    c->last_graph_marks = true;
    p.mark_launches = 2;
    return PHYLO_OK;
}

// 1. the pointer block
static int rev_bind(rev_pass& p) {
    phylo_ctx* c = p.c;
    pg_args& g = p.g;
    const int N = c->N, K = c->K, S = c->S, R = N - 1;
    const bool whole = p.plan.whole;
    g.N = N; g.S = S; g.K = K; g.R = R; g.T = p.plan.rows_form ? 1 : (S + PG_NT - 1) / PG_NT; g.jc = c->jc;
    g.ngrp = c->last_G; g.Kg = K / c->last_G; g.lse_stride = c->last_G > 1 ? R + 1 : 0;   // (the batched sweep's lse: [G][R + 1])
    g.twist = p.plan.twist ? 1 : 0;
    g.leaves = c->d_leaves; g.pool = c->d_pool; g.adj = c->d_adj; g.Pmat = whole ? c->d_gPmat : c->d_Pmat;
    g.pool_ptrs = whole ? (const double* const*)c->d_pool_ptrs : nullptr; g.Kloc = c->Kloc;
    g.bl = whole ? c->d_gbl : c->d_bl; g.br = whole ? c->d_gbr : c->d_br; g.logw = c->d_logw; g.lse = c->d_lse;
    g.pi = c->d_pi; g.Q = c->d_Q; g.lam_l = c->d_lam_l; g.lam_r = c->d_lam_r;
    g.child = whole ? c->d_gchild : c->d_child; g.pos = c->d_pos; g.roots = c->d_hroots;
    g.ad_off = c->d_ad_off; g.ad_idx = c->d_ad_idx; g.par_off = c->d_par_off; g.par_idx = c->d_par_idx;
    g.heavy_first = c->d_heavy; g.chunk_beg = c->d_chunk_beg; g.chunk_cnt = c->d_chunk_cnt;
    g.slow_flag = c->d_slow_flag; g.slow_idx = c->d_slow_idx;
    g.om = c->d_om; g.G = c->d_G; g.C = c->d_C; g.part = c->d_part; g.nodeg = c->d_nodeg;
    g.leafpi = c->d_leafpi; g.leafterm = c->d_leafterm; g.terms = c->d_terms; g.out = c->d_gout;
    g.alpha_om = p.plan.early_free ? 1 : 0;                // a free parent then is a node nobody adopted: alpha = omega
    if (p.plan.early_free) g.mark = c->d_mark;
    if (p.plan.twist) {
        g.tw.M = c->last_M; g.tw.joff = c->d_joff; g.tw.roots_ad = c->d_hroots_ad;
        g.tw.tw_b = c->d_htw_b; g.tw.tw_P = c->d_htw_P; g.tw.pot = c->d_hpot; g.tw.chosen = c->d_hchosen;
        g.tw.tau = c->d_tau; g.tw.ctw = c->d_ctw; g.tw.twpart = c->d_twpart; g.tw.twnode = c->d_twnode;
        g.tw.pair_hist = (c->codes_valid && c->hist_ready) ? c->d_pair_hist : nullptr;
        const size_t J0 = (size_t)((N * (N - 1)) / 2) * c->last_M;
        void* sl = nullptr;
        CHK(scratch_get(c, 4, (size_t)K * ((J0 + 255) / 256) * PG_NODEG * 8, &sl));
        g.tw.twslice = (double*)sl;
    }
    return PHYLO_OK;
}

// (2.) the twisted proposal's kernels over the look-ahead potentials: they need no list either
static int rev_early_twist(rev_pass& p) {
    phylo_ctx* c = p.c;
    const pg_args& g = p.g;
    const int N = g.N, K = g.K, R = g.R;
    const size_t J0 = (size_t)((N * (N - 1)) / 2) * c->last_M;
    hipLaunchKernelGGL(pg_twist_tau, dim3(R * K), dim3(64), (J0 <= 8192 ? J0 : 8192) * 8, c->stream, g);   // later rank events have fewer rows and use LDS
    CHK(launch_check(c, "pg_twist_tau"));
    hipLaunchKernelGGL(pg_twist_pbar, dim3((unsigned)((c->h_joff[R] + 3) / 4)), dim3(256), 0, c->stream, g);
    CHK(launch_check(c, "pg_twist_pbar"));
    if (g.tw.pair_hist)
        for (int r = 0; r < R; ++r) {
            const long rows_r = (long)(c->h_joff[r + 1] - c->h_joff[r]);
            hipLaunchKernelGGL(pg_twist_pbar_ll, dim3(cdiv(rows_r, 64)), dim3(64), 0, c->stream, g, r);
            CHK(launch_check(c, "pg_twist_pbar_ll"));
            ++p.tw_launches;
        }
    for (int r = 0; r < R; ++r) {
        const int Jr = (((N - r) * (N - r - 1)) / 2) * c->last_M;
        const int KB = Jr >= 256 ? 1 : 256 / Jr;
        const int nsl = Jr > 256 ? cdiv(Jr, 256) : 1;
        hipLaunchKernelGGL(pg_twist_finish, dim3(cdiv(K, KB), nsl), dim3(256), 0, c->stream, g, r);
        CHK(launch_check(c, "pg_twist_finish"));
        ++p.tw_launches;
        if (nsl > 1) {
            hipLaunchKernelGGL(pg_twist_finish_sum, dim3(cdiv((long)K * PG_NODEG, 256)), dim3(256), 0, c->stream, g, r, nsl);
            CHK(launch_check(c, "pg_twist_finish_sum"));
            ++p.tw_launches;
        }
    }
    p.tw_launches += 2;
    return PHYLO_OK;
}

// 2. what does not need the integer lists is launched first: the GPU works while the host builds them (or waits for them)
static int rev_early(rev_pass& p) {
    phylo_ctx* c = p.c;
    const pg_args& g = p.g;
    const size_t nn = (size_t)g.R * g.K;
    HIPCHK(c, hipEventRecord(c->evb0, c->stream));
    // The list kernels need the sweep's ancestors and children and nothing else: they are queued right behind the sweep on its own
    // stream, ahead of the early kernels below (they head the longest chain: lists -> sort -> chunk sums -> adopted nodes).
    if (p.plan.dev_lists) CHK(dev_lists_launch(c, c->stream, c->stream, true, false));
    hipLaunchKernelGGL(pg_omega, dim3(g.R, g.ngrp), dim3(PG_OMEGA_NT), 0, c->stream, g);
    CHK(launch_check(c, "pg_omega"));
    hipLaunchKernelGGL(pg_leafpi, dim3(g.N), dim3(256), 0, c->stream, g);
    CHK(launch_check(c, "pg_leafpi"));
    if (p.plan.bg_free) {                                  // pg_nodes_free in the background (rev_bg_free): here only what it waits for
        hipLaunchKernelGGL(pg_fill_free, dim3(cdiv((long)nn, 256)), dim3(256), 0, c->stream, g);
        CHK(launch_check(c, "pg_fill_free"));
        HIPCHK(c, hipEventRecord(c->ev_bgfork, c->stream));
        // (its launch follows the wait for the sweep's end: a second queue with a pending wait slows the sweep's own
        //  dependent launches by half a microsecond each -- 19 us per sweep, measured)
    } else if (p.plan.early_free) {
        hipLaunchKernelGGL(pg_nodes_free, dim3((unsigned)((nn + 3) / 4)), dim3(256), 0, c->stream, g, 0);
        CHK(launch_check(c, "pg_nodes_free"));
    }
    if (p.plan.twist) CHK(rev_early_twist(p));
    return PHYLO_OK;
}

// the background launch: every node nobody adopted, on the stream of the lowest priority
static int rev_bg_free(rev_pass& p) {
    phylo_ctx* c = p.c;
    const size_t nn = (size_t)p.g.R * p.g.K;
    HIPCHK(c, hipStreamWaitEvent(c->bgstream, c->ev_bgfork, 0));
    hipLaunchKernelGGL(pg_nodes_free, dim3((unsigned)((nn + 3) / 4)), dim3(256), 0, c->bgstream, p.g, 3);
    CHK(launch_check(c, "pg_nodes_free"));
    HIPCHK(c, hipEventRecord(c->ev_bgdone, c->bgstream));
    return PHYLO_OK;
}

// 3. the host has seen the sweep end: the background launch, the early sort, the fork of the second stream.
// ---- integer bookkeeping of the reverse pass: who adopted whom, and which nodes have which parents.  The sweep left the
//      ancestors and children in pinned host memory (asynchronous copies behind its last launch); the lists are built straight
//      into the pinned image of the device slab (ad_off | ad_idx | par_off | par_idx | heavy | chunk_beg | chunk_cnt).
static int rev_fork(rev_pass& p) {
    phylo_ctx* c = p.c;
    const int R = p.g.R, K = p.g.K;
    CHK(wait_event_spin(c, c->ev_gcopy));
    if (p.plan.bg_free && !p.plan.dev_lists) CHK(rev_bg_free(p));
    p.host_t0 = std::chrono::steady_clock::now();
    p.anc = c->h_anc_p;
    if (!p.plan.dev_lists && p.g.ngrp > 1) {               // the host builders take the one genealogy's global indices
        pg_global_ancestors(R, K, p.g.Kg, c->h_anc_p, c->h_anc_glob);
        p.anc = c->h_anc_glob.data();
    }
    p.L = pg_lists_carve(c->h_csr_p, (size_t)R, (size_t)K);     // (phylo_revlists.h: the builders, tested on the CPU)
    if (!p.plan.dev_lists) pg_lists_clear(p.L, R, K);
    p.sB = p.plan.two ? c->gstream : c->stream;
    // (the host has seen the sweep end: the second stream needs no event to start on its outputs, and the list kernels run
    //  beside the early kernels)
    if (p.plan.sort_early) {
        // (the list kernels run on the context's stream, ahead of the coefficient chain)
        HIPCHK(c, hipStreamWaitEvent(c->gstream, c->ev_dl, 0));
        CHK(dev_lists_launch(c, c->gstream, c->gstream, false, true));
    }
    // the list kernels are workgroups of 1024 threads that everything else waits for: on a GPU that the background launch has
    // filled they wait for a whole free CU each, kernel after kernel (lists ready after 120 us instead of 55): the background
    // launch starts behind them.  (Measured, primate.p K = 2048 / DS1 K = 4096, reverse pass: background launch first 0.504 /
    //  1.634 ms, behind the lists 0.486 / 1.653, behind the parents' sort 0.510 / 1.746; a high-priority second stream
    //  changes nothing.)
    if (p.plan.bg_free && p.plan.dev_lists) {
        HIPCHK(c, hipStreamWaitEvent(c->bgstream, c->ev_dl, 0));
        CHK(rev_bg_free(p));
    }
    if (p.plan.two) {
        HIPCHK(c, hipEventRecord(c->ev_gfork, c->stream));                 // everything launched so far (the early kernels)
        HIPCHK(c, hipStreamWaitEvent(p.sB, c->ev_gfork, 0));
    }
    if (p.plan.early_free && !p.plan.dev_lists) pg_mark_adopted(R, K, p.anc, p.L);
    return PHYLO_OK;
}

// The parents' sort when it was not queued early, then the chunk sums.  The parents of a heavy node are nearly all nodes nobody
// merged again: their share of the node's adjoint needs their alpha = omega and nothing else.  ONE launch sums them for the chunks
// of all rank events; the chain is then pg_nodes_rows alone, which adds the flagged parents.
static int rev_sort_and_chunk_sums(rev_pass& p) {
    phylo_ctx* c = p.c;
    const pg_args& g = p.g;
    if (p.plan.dev_lists && !p.plan.sort_early) CHK(dev_lists_launch(c, p.sB, p.sB, false, true));   // (the host has seen the list kernels end)
    if (!p.plan.early_free) return PHYLO_OK;               // (else: a rank event's chunks at a time, in the chain)
    const size_t rowlen = (size_t)g.S * 4;
    for (size_t cbeg = 0; cbeg < p.n.n_chunks; cbeg += 65535) {
        const size_t cn = p.n.n_chunks - cbeg < 65535 ? p.n.n_chunks - cbeg : 65535;
        pg_args g2 = g;
        g2.cpart = g.cpart + cbeg * rowlen;
        hipLaunchKernelGGL(pg_parent_chunks_rows, dim3(cdiv(g.S, 64), (unsigned)cn), dim3(256), 0, p.sB, g2, (int)cbeg);
        CHK(launch_check(c, "pg_parent_chunks_rows"));
    }
    return PHYLO_OK;
}

// (4.) pg_nodes_rows_all's completion words, one epoch per pass, and what it needs to follow pg_coeff_all
static int rev_row_words(rev_pass& p) {
    phylo_ctx* c = p.c;
    pg_args& g = p.g;
    const int R = g.R, K = g.K;
    const size_t row_words = (size_t)R * K * (size_t)cdiv(c->S, 256);
    if (!c->d_row_done) {
        const size_t words = row_words + 2 * (size_t)R;      // + coeff_done[R] | coeff_ticket[R]
        CHK(dalloc(c, &c->d_row_done, words));
        HIPCHK(c, hipMemsetAsync(c->d_row_done, 0, words * 4, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));     // (once per context: ahead of every launch, on any stream, that touches them)
        c->row_epoch = 0;
    }
    if (++c->row_epoch == 0) ++c->row_epoch;             // (0 is what the words hold before their first pass)
    g.row_done = c->d_row_done;
    g.row_epoch = c->row_epoch;
    g.row_timeout = (unsigned int*)(c->hd_dlmeta + PG_DL_META_INTS(R));
    g.coeff_done = c->d_row_done + row_words;
    g.coeff_ticket = g.coeff_done + R;
    // which rank events have a pg_coeff launch to wait for: read from pg_dl_lists' own starts on the device (rows_all implies
    // dev_lists; the host has seen those kernels end in dev_lists_wait, ahead of every launch that reads them, on any stream) --
    // a word per rank event for any R, no upload
    g.ev_adp0 = c->d_dlmeta;
    return PHYLO_OK;
}

// workgroups of the coefficient chain's launches together (the adopted particles of every rank event but the last)
static long rev_coeff_wgs(const rev_pass& p) {
    long wgs = 0;
    for (int r = p.g.R - 2; r >= 0; --r) wgs += (long)(p.n.ev_adp0[r + 1] - p.n.ev_adp0[r]) * cdiv(p.g.N - r - 1, 4);
    return wgs;
}

// 4. parents, heavy nodes' chunks, flagged nodes by rank event (pg_build_parents, or what pg_dl_lists reports); with the counts the
//    second half of the plan.  Runs ahead of the adopters' stage (plan.parents_first) or behind the look-ahead lists.
static int rev_parents(rev_pass& p) {
    phylo_ctx* c = p.c;
    pg_args& g = p.g;
    const int N = g.N, K = g.K, S = g.S, R = g.R;
    const size_t nn = (size_t)R * K;
    if (p.plan.dev_lists) CHK(dev_lists_wait(c, p.n));
    else {
        pg_build_parents(N, R, K, c->h_child_p, p.plan.rows_form, p.plan.early_free, p.L, c->h_cur, p.n);
        // (the order the device builders leave: the same bits -- where no gradient existed before, phylo_revlists.h)
        if (p.plan.early_free && N > PG_KEPT_BITS_TAXA) pg_flagged_tails_ascending(p.L, p.n.n_slow);
    }
    void* cpart = nullptr;
    // rows form: the chunk sums of ALL rank events are produced by one launch (free parents only: nothing of the chain is
    // needed for them), so the buffer holds every chunk; else one rank event's at a time
    CHK(scratch_get(c, 5, (p.plan.early_free ? p.n.n_chunks : p.n.max_chunks) * (size_t)S * 4 * 8, &cpart));
    g.cpart = (double*)cpart;
    g.chunks_free_only = p.plan.early_free ? 1 : 0;
    g.TS = cdiv(S, 256);
    void* fp = nullptr;
    // (batched: pg_node_finish's workgroups are cut per (rank event, group))
    const size_t fin_wgs = g.ngrp > 1 ? (size_t)R * g.ngrp * (((size_t)g.Kg + 31) / 32) : (nn + 31) / 32;
    CHK(scratch_get(c, 2, fin_wgs * 20 * 8, &fp));
    g.fin_part = (double*)fp;
    if (p.plan.rows_form) {
        void* sp = nullptr;
        CHK(scratch_get(c, 3, (size_t)(p.n.n_slow ? p.n.n_slow : 1) * g.TS * PG_PART * 8, &sp));
        g.slowpart = (double*)sp;
    }
    if (!p.plan.dev_lists) {   // what was used of everything between the adopters' lists and the adopted particles, by a kernel (pg_copy_words)
        const pg_lists& L = p.L;
        pg_copy3 cp{};
        const size_t o0 = (size_t)(L.par_off - L.ad_off), o1 = (size_t)(L.heavy - L.ad_off), o2 = (size_t)(L.slow_flag - L.ad_off);
        cp.src[0] = c->hd_csr + o0; cp.dst[0] = (uint32_t*)(c->d_ad_off + o0); cp.n[0] = nn + 1 + (size_t)L.par_off[nn];   // par_off | par_idx
        cp.src[1] = c->hd_csr + o1; cp.dst[1] = (uint32_t*)(c->d_ad_off + o1); cp.n[1] = nn + L.cap + p.n.n_chunks;        // heavy | chunk_beg | chunk_cnt
        cp.src[2] = c->hd_csr + o2; cp.dst[2] = (uint32_t*)(c->d_ad_off + o2); cp.n[2] = nn + (size_t)p.n.ev_slow0[R];     // slow_flag | slow_idx
        const size_t words = cp.n[0] + cp.n[1] + cp.n[2];
        hipLaunchKernelGGL(pg_copy_words, dim3((unsigned)(words / 1024 < 1 ? 1 : (words / 1024 > 1024 ? 1024 : words / 1024))), dim3(256), 0, p.sB, cp);
        CHK(launch_check(c, "pg_copy_words"));
        if (p.plan.two) HIPCHK(c, hipEventRecord(c->ev_gup, p.sB));
    }
    // (the adopters' counts are there with the device's lists only; no form without them takes pg_coeff_all)
    pg_plan_chains(p.plan, p.n.n_slow, g.TS, p.plan.dev_lists ? rev_coeff_wgs(p) : 0, g_backward_in_flight.load(), R);
    if (p.plan.rows_all) CHK(rev_row_words(p));
    if (p.plan.chunks_first) CHK(rev_sort_and_chunk_sums(p));
    return PHYLO_OK;
}

// 5. the adopters' lists, their upload, pg_G
static int rev_adopters(rev_pass& p) {
    phylo_ctx* c = p.c;
    pg_args& g = p.g;
    const int K = g.K, R = g.R;
    if (!p.plan.dev_lists) {
        pg_build_adopters(R, K, p.anc, p.L, c->h_cur, p.n);
        // the adopters' lists are all the coefficient chain needs: it runs while the host goes on with the parents' lists
        const size_t ad_ints = (size_t)R * (K + 1) + (size_t)R * K;
        HIPCHK(c, hipMemcpyAsync(c->d_ad_off, c->h_csr_p, ad_ints * 4, hipMemcpyHostToDevice, c->stream));
    }
    if (!p.plan.early_free) {
        hipLaunchKernelGGL(pg_G, dim3(R * K), dim3(64), 0, c->stream, g);
        return launch_check(c, "pg_G");
    }
    // When the early pg_nodes_free has dealt with everybody nobody adopted, pg_G and the chain run over the adopted particles alone.
    const int32_t n_adp = p.n.n_adp;
    if (!p.plan.dev_lists) HIPCHK(c, hipMemcpyAsync(c->d_adp, p.L.adp, (size_t)(n_adp ? n_adp : 1) * 4, hipMemcpyHostToDevice, c->stream));
    g.adp = c->d_adp;
    if (n_adp > 0) {
        hipLaunchKernelGGL(pg_G, dim3(n_adp), dim3(64), 0, c->stream, g);
        CHK(launch_check(c, "pg_G"));
    }
    if (p.plan.two) HIPCHK(c, hipEventRecord(c->ev_coeff[R - 1], c->stream));   // (the last rank event has no adopters: C is there)
    return PHYLO_OK;
}

// the coefficients of rank event r: over its adopted particles after the early pg_nodes_free, else over all K
static int rev_coeff(rev_pass& p, int r) {
    phylo_ctx* c = p.c;
    const int na = p.plan.early_free ? p.n.ev_adp0[r + 1] - p.n.ev_adp0[r] : p.g.K;
    if (na > 0) {
        hipLaunchKernelGGL(pg_coeff, dim3(na, cdiv(p.g.N - r - 1, 4)), dim3(256), 0, c->stream, p.g, r, p.plan.early_free ? (int)p.n.ev_adp0[r] : 0);
        CHK(launch_check(c, "pg_coeff"));
    }
    if (p.plan.two) HIPCHK(c, hipEventRecord(c->ev_coeff[r], c->stream));
    return PHYLO_OK;
}

static int rev_leafterm(rev_pass& p) {
    hipLaunchKernelGGL(pg_leafterm, dim3(cdiv(p.g.K, 256)), dim3(256), 0, p.c->stream, p.g);
    return launch_check(p.c, "pg_leafterm");
}

// 6. the coefficient chain, newest rank event first: one launch, a launch per rank event, or -- interleaved -- left to the node chain
static int rev_coeff_chain(rev_pass& p) {
    phylo_ctx* c = p.c;
    const pg_args& g = p.g;
    const int N = g.N, R = g.R;
    if (p.plan.coeff_all) {
        pg_coeff_plan pl{};
        int at = 0;
        for (int r = R - 2; r >= 0; --r) {
            pl.first[r] = at; pl.adp0[r] = p.n.ev_adp0[r]; pl.ny[r] = cdiv(N - r - 1, 4);
            at += (p.n.ev_adp0[r + 1] - p.n.ev_adp0[r]) * pl.ny[r];
        }
        hipLaunchKernelGGL(pg_coeff_all, dim3((unsigned)at), dim3(256), 0, c->stream, g, pl);
        CHK(launch_check(c, "pg_coeff_all"));
        if (p.plan.two) HIPCHK(c, hipEventRecord(c->ev_coeff[0], c->stream));
    } else if (!p.plan.interleave) {
        // (after the early pg_nodes_free the last rank event has no adopters: rev_adopters has recorded its event)
        for (int r = p.plan.early_free ? R - 2 : R - 1; r >= 0; --r) CHK(rev_coeff(p, r));
    }
    if (!p.plan.interleave) CHK(rev_leafterm(p));
    return PHYLO_OK;
}

// 7. twisted proposal: the look-ahead lists (pg_build_lookahead), all rank events in one upload
static int rev_lookahead(rev_pass& p) {
    phylo_ctx* c = p.c;
    pg_args& g = p.g;
    if (!p.plan.twist) return PHYLO_OK;
    std::vector<int32_t>& pk = c->h_xlists;
    pg_build_lookahead(g.N, g.K, g.S, PG_XCH, c->h_rad_p, p.L.slow_flag, pk, p.x);   // (h_rad_p: pinned copy made when the sweep ended)
    void *d_xlists = nullptr, *d_tpart = nullptr;
    CHK(scratch_get(c, 6, pk.size() * 4, &d_xlists));
    HIPCHK(c, hipMemcpyAsync(d_xlists, pk.data(), pk.size() * 4, hipMemcpyHostToDevice, p.sB));
    CHK(scratch_get(c, 7, p.x.max_chunks * (size_t)g.S * 4 * 8, &d_tpart));
    const int32_t* xl = (const int32_t*)d_xlists;
    g.tw.xent = xl; xl += p.x.n_xent;
    g.tw.xchunk_node = xl; xl += p.x.n_xchunks;
    g.tw.xchunk_beg = xl; xl += p.x.n_xchunks;
    g.tw.xchunk_cnt = xl; xl += p.x.n_xchunks;
    g.tw.xchunk_part = xl; xl += p.x.n_xchunks;
    g.tw.xnode_id = xl; xl += p.x.n_xnodes;
    g.tw.xnode_chunk0 = xl; xl += p.x.n_xnodes;
    g.tw.xnode_nchunks = xl;
    g.tw.tpart = (double*)d_tpart;
    return PHYLO_OK;
}

// one rank event of the adopted nodes' chain: look-ahead entries, chunk sums (when not summed in one launch), the nodes
static int rev_nodes_of(rev_pass& p, int r) {
    phylo_ctx* c = p.c;
    const pg_args& g = p.g;
    const pg_list_counts& n = p.n;
    if (p.plan.twist && p.x.ev_chunk0[r + 1] > p.x.ev_chunk0[r]) {
        const int32_t ch0 = p.x.ev_chunk0[r], nd0 = p.x.ev_node0[r];
        hipLaunchKernelGGL(pg_twist_xchunks, dim3(p.x.ev_chunk0[r + 1] - ch0, cdiv(g.S, 256)), dim3(256), 0, p.sB, g, r, (int)ch0);
        CHK(launch_check(c, "pg_twist_xchunks"));
        hipLaunchKernelGGL(pg_twist_xsum, dim3(p.x.ev_node0[r + 1] - nd0, cdiv((long)g.S * 4, 256)), dim3(256), 0, p.sB, g, (int)nd0, (int)ch0);
        CHK(launch_check(c, "pg_twist_xsum"));
        p.tw_launches += 2;
    }
    const int nch = p.plan.early_free ? 0 : n.rank_chunk0[r + 1] - n.rank_chunk0[r];   // (after the early pg_nodes_free: summed already, all rank events at once)
    if (nch > 0) {
        hipLaunchKernelGGL(pg_parent_chunks_rows, dim3(cdiv(g.S, 64), nch), dim3(256), 0, p.sB, g, (int)n.rank_chunk0[r]);
        CHK(launch_check(c, "pg_parent_chunks_rows"));
        ++p.node_launches;
    }
    if (p.plan.rows_form) {
        const int nslow = n.ev_slow0[r + 1] - n.ev_slow0[r];
        if (nslow > 0) {
            hipLaunchKernelGGL(pg_nodes_rows, dim3(nslow, g.TS), dim3(256), 0, p.sB, g, r, (int)n.ev_slow0[r],
                               p.plan.early_free ? (int)n.rank_chunk0[r] : 0);   // (device-built lists: heavy[] is the global chunk index, rank_chunk0 zero)
            ++p.node_launches;
        }
    } else {
        hipLaunchKernelGGL(pg_nodes, dim3(g.T, g.K), dim3(256), 0, p.sB, g, r);
        ++p.node_launches;
    }
    return launch_check(c, "pg_nodes");
}

// 8. the adopted nodes' chain on sB: pg_nodes_rows_all, or a rank event at a time behind that rank event's coefficients
static int rev_node_chain(rev_pass& p) {
    phylo_ctx* c = p.c;
    const pg_args& g = p.g;
    const int R = g.R;
    const size_t nn = (size_t)R * g.K;
    p.node_launches = p.plan.early_free ? 1 : 0;
    if (p.plan.rows_form && !p.plan.early_free) {          // the sweep left no marks: every node nobody merged again, now
        ++p.node_launches;
        if (p.plan.two) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_gup, 0));   // (needs the flags of the second upload)
        hipLaunchKernelGGL(pg_nodes_free, dim3((unsigned)((nn + 3) / 4)), dim3(256), 0, c->stream, g, 1);
        CHK(launch_check(c, "pg_nodes_free"));
    }
    if (!p.plan.chunks_first) CHK(rev_sort_and_chunk_sums(p));   // (behind the coefficient launches: they head the longer chain)
    if (p.plan.rows_all) {
        if (!p.plan.rows_overlap) HIPCHK(c, hipStreamWaitEvent(p.sB, c->ev_coeff[0], 0));   // every alpha is there
        hipLaunchKernelGGL(pg_nodes_rows_all, dim3((unsigned)p.n.n_slow, g.TS), dim3(256), 0, p.sB, g, (int)p.n.n_slow);
        CHK(launch_check(c, "pg_nodes_rows_all"));
        ++p.node_launches;
    } else {
        for (int r = R - 1; r >= 0; --r) {
            if (p.plan.interleave && r >= 1) CHK(rev_coeff(p, r - 1));
            if (p.plan.two) HIPCHK(c, hipStreamWaitEvent(p.sB, c->ev_coeff[r], 0));
            CHK(rev_nodes_of(p, r));
        }
    }
    if (p.plan.interleave) CHK(rev_leafterm(p));
    return PHYLO_OK;
}

// 9. join the streams, finish the nodes, reduce, fetch
static int rev_finish(rev_pass& p, double* d_lam_l, double* d_lam_r, double* d_pi, double* d_Q, phylo_stats* perf) {
    phylo_ctx* c = p.c;
    const pg_args& g = p.g;
    const int R = g.R;
    if (p.plan.two) {
        HIPCHK(c, hipEventRecord(c->ev_gjoin, p.sB));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_gjoin, 0));
    }
    if (p.plan.bg_free) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_bgdone, 0));
    const long fin_wgs = g.ngrp > 1 ? (long)R * g.ngrp * cdiv(g.Kg, 32) : cdiv((long)R * g.K, 32);
    hipLaunchKernelGGL(pg_node_finish, dim3((unsigned)fin_wgs), dim3(256), 0, c->stream, g);
    CHK(launch_check(c, "pg_node_finish"));
    hipLaunchKernelGGL(pg_scalars, dim3(cdiv((long)R * g.K, 256)), dim3(256), 0, c->stream, g);
    CHK(launch_check(c, "pg_scalars"));
    hipLaunchKernelGGL(pg_reduce, dim3(2 * R + 20 + (p.batch ? 1 : 0), g.ngrp), dim3(256), 0, c->stream, g);
    CHK(launch_check(c, "pg_reduce"));
    // sharded: the pass read node rows from the peers' pools; no owner may write its pool again (its next sweep) before every
    // rank's pass is done -- the barrier makes phylo_sweep_backward a collective call
    if (p.plan.whole) CHK(comm_exchange(c, nullptr, 0, 0, 1));
    HIPCHK(c, hipEventRecord(c->evb1, c->stream));
    const size_t row = (size_t)2 * R + 20, G = (size_t)g.ngrp;
    std::vector<double>& out = c->h_gout;
    out.resize(row * G + (p.batch ? G : 0));
    HIPCHK(c, hipMemcpyAsync(out.data(), c->d_gout, out.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->ev_gjoin, c->stream));     // (free again: the stream has waited for it above)
    CHK(wait_event_spin(c, c->ev_gjoin));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (p.plan.rows_all && c->h_dlmeta[PG_DL_META_INTS(R)] != 0) {
        c->h_dlmeta[PG_DL_META_INTS(R)] = 0;
        return fail(c, PHYLO_EHIP, "reverse pass: a workgroup of pg_nodes_rows_all gave up waiting for a parent's adjoint tile "
                                       "(PHYLO_GRAD_ROWS_CHAIN=1 runs a launch per rank event instead)");
    }
    for (size_t gi = 0; gi < G; ++gi) {
        const double* o = out.data() + gi * row;
        if (d_lam_l) memcpy(d_lam_l + gi * R, o, (size_t)R * 8);
        if (d_lam_r) memcpy(d_lam_r + gi * R, o + R, (size_t)R * 8);
        if (d_pi) memcpy(d_pi + gi * 4, o + 2 * R, 4 * 8);
        if (d_Q) memcpy(d_Q + gi * 16, o + 2 * R + 4, 16 * 8);
    }
    if (perf) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->evb0, c->evb1));
        *perf = c->stats;
        perf->sweep_ms = ms;
        // (R + 7 stands for the coefficient chain's launch per rank event and the fixed launches: not a true count under
        //  pg_coeff_all, where that chain is one launch; kept as it is, tools compare it between runs)
        perf->n_launches = R + 7 + p.node_launches + p.tw_launches + p.mark_launches;
        perf->merge_ms = p.host_ms;                        // here: host time of the integer lists (built, or waited for: device lists)
        perf->merge_launches = p.plan.dev_lists ? 1 : 0;   // here: 1 = the lists were built by kernels (phylo_revlists_dev.h)
    }
    return PHYLO_OK;
}

static int sweep_backward_impl(phylo_ctx* c, double* d_lam_l, double* d_lam_r, double* d_pi, double* d_Q, phylo_stats* perf, int G) {
    CHK(bind(c));
    if (!c->swept || !c->last_graph)
        return fail(c, PHYLO_ESTATE, "%s needs a preceding sweep with PHYLO_KEEP_GRAPH", G ? "phylo_sweep_backward_batch" : "phylo_sweep_backward");
    rev_pass p;
    p.c = c;
    p.batch = G != 0;
    CHK(rev_marks(p));
    p.plan = pg_plan_form(rev_plan_in(c));                 // decision point one: before anything is launched
    CHK(rev_bind(p));
    CHK(rev_early(p));
    CHK(rev_fork(p));
    if (p.plan.parents_first) CHK(rev_parents(p));         // (decision point two, pg_plan_chains, is inside: the counts are known there)
    CHK(rev_adopters(p));
    CHK(rev_coeff_chain(p));
    CHK(rev_lookahead(p));
    if (!p.plan.parents_first) CHK(rev_parents(p));
    p.host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - p.host_t0).count();
    CHK(rev_node_chain(p));
    return rev_finish(p, d_lam_l, d_lam_r, d_pi, d_Q, perf);
}

// ---- a VI training step's host half in C++ (phylo_train.h): variables -> model -> sweep + reverse pass -> gradients of the variables
int phylo_vi_gradients(phylo_ctx* c, uint64_t seed, uint32_t flags, int M, int jc, const double* vars, double* logZ, double* grads,
                       phylo_stats* fwd, phylo_stats* bwd) {
    CHK(bind(c));
    if (!vars || !grads) return fail(c, PHYLO_EINVAL, "phylo_vi_gradients: NULL argument");   // (ahead of phylo_set_model and the sweep:
    const int R = c->N - 1;                                                                    //  a refused call leaves nothing in flight)
    double Q[16], pi[4];
    std::vector<double>& lam = c->h_vi_lam;
    lam.resize((size_t)2 * R);
    for (int r = 0; r < 2 * R; ++r) lam[r] = std::exp(vars[r]);
    if (jc) pt_jc_Q(Q); else pt_get_Q(vars + 2 * R, Q);
    pt_get_pi(vars + 2 * R + 16, pi);
    CHK(phylo_set_model(c, Q, pi, lam.data(), lam.data() + R, jc));
    CHK(phylo_sweep_async(c, seed, flags | PHYLO_KEEP_GRAPH, M));
    std::vector<double>& rawv = c->h_vi_raw;                // d_lam_l[R] | d_lam_r[R] | d_pi[4] | d_Q[16], any R
    rawv.resize((size_t)2 * R + 20);
    double* raw = rawv.data();
    CHK(phylo_sweep_backward(c, raw, raw + R, raw + 2 * R, raw + 2 * R + 4, bwd));
    CHK(phylo_sweep_fetch(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, logZ, fwd));
    pt_chain_rules(R, jc, Q, pi, lam.data(), lam.data() + R, raw, raw + R, raw + 2 * R, raw + 2 * R + 4, grads);
    return PHYLO_OK;
}

// ... for G systems behind one set of launches: row g of `grads` is the gradient of log Z-hat_g alone (no mean is taken here)
int phylo_vi_gradients_batch(phylo_ctx* c, const uint64_t* seeds, int G, uint32_t flags, int jc, const double* vars, double* logZ, double* grads,
                             phylo_stats* fwd, phylo_stats* bwd) {
    CHK(bind(c));
    if (!vars || !grads || !seeds) return fail(c, PHYLO_EINVAL, "phylo_vi_gradients_batch: NULL argument");
    if (G < 1 || G > PK_MAX_GROUPS) return fail(c, PHYLO_EINVAL, "phylo_vi_gradients_batch: 1 <= G <= %d (got %d)", PK_MAX_GROUPS, G);
    const int R = c->N - 1;
    double Q[16], pi[4];
    std::vector<double>& lam = c->h_vi_lam;
    lam.resize((size_t)2 * R);
    for (int r = 0; r < 2 * R; ++r) lam[r] = std::exp(vars[r]);
    if (jc) pt_jc_Q(Q); else pt_get_Q(vars + 2 * R, Q);
    pt_get_pi(vars + 2 * R + 16, pi);
    CHK(phylo_set_model(c, Q, pi, lam.data(), lam.data() + R, jc));
    CHK(phylo_sweep_batch_async(c, seeds, G, flags | PHYLO_KEEP_GRAPH));
    // rows of the driver's own host buffer: d_lam_l, d_lam_r, d_pi, d_Q contiguous per group, the groups' log Z-hat behind them
    CHK(sweep_backward_guarded(c, nullptr, nullptr, nullptr, nullptr, bwd, G));
    CHK(phylo_sweep_fetch(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, fwd));   // (the timeout word, the sweep's stats)
    const size_t row = (size_t)2 * R + 20;
    for (int g = 0; g < G; ++g) {
        const double* raw = c->h_gout.data() + (size_t)g * row;
        pt_chain_rules(R, jc, Q, pi, lam.data(), lam.data() + R, raw, raw + R, raw + 2 * R, raw + 2 * R + 4, grads + (size_t)g * row);
        if (logZ) logZ[g] = c->h_gout[(size_t)G * row + g];
    }
    return PHYLO_OK;
}

int phylo_vi_apply(int n_taxa, int jc, double* vars, const double* grads, int kind, double lr, double beta1, double beta2, double eps, int64_t* t,
                   double* m, double* v) {
    if (n_taxa < 2 || !vars || !grads || (kind != 0 && (!t || !m || !v)))
        return fail(nullptr, PHYLO_EINVAL, "phylo_vi_apply: bad arguments");
    const int R = n_taxa - 1;
    pt_apply(jc ? 2 * R : 2 * R + 20, vars, grads, kind, lr, beta1, beta2, eps, t, m, v);
    return PHYLO_OK;
}

int phylo_debug_stamps(phylo_ctx* c, uint64_t* out, int n) {
    CHK(bind(c));
    if (!c->d_stamps) return fail(c, PHYLO_ESTATE, "no stamps: create the context with PHYLO_PERSIST_STAMPS=1 and run a one-launch sweep");
    const int have = c->N * PP_NSTAMP;
    if (!out || n < have) return fail(c, PHYLO_EINVAL, "phylo_debug_stamps needs room for N * %d = %d values", PP_NSTAMP, have);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->d_stamps, (size_t)have * 8, hipMemcpyDeviceToHost));
    return PHYLO_OK;
}

// meta of the two list hooks: n_adp, n_chunks, max_chunks, n_slow, n_par, cap, then ev_adp0[R+1], rank_chunk0[R+1], ev_slow0[R+1]
static void debug_lists_meta(const pg_list_counts& n, size_t cap, int R, int32_t* meta) {
    meta[0] = n.n_adp; meta[1] = (int32_t)n.n_chunks; meta[2] = (int32_t)n.max_chunks; meta[3] = n.n_slow; meta[4] = n.n_par;
    meta[5] = (int32_t)cap;
    for (int r = 0; r <= R; ++r) {
        meta[6 + r] = n.ev_adp0[r];
        meta[6 + (R + 1) + r] = n.rank_chunk0[r];
        meta[6 + 2 * (R + 1) + r] = n.ev_slow0[r];
    }
}

int phylo_debug_reverse_lists(int N, int K, const int64_t* ancestors, const int32_t* child, int early_free, int rows_form,
                              const int32_t* lookahead_nodes, int n_lookahead, int32_t* lists, int64_t n_lists, int32_t* meta, int n_meta) {
    if (N < 2 || K < 1 || !child || !lists || !meta || (N > 2 && !ancestors) || (n_lookahead > 0 && !lookahead_nodes))
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_reverse_lists: bad arguments");
    const int R = N - 1;
    if (n_lists < (int64_t)pg_lists_ints((size_t)R, (size_t)K) || n_meta < 6 + 3 * (R + 1))
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_reverse_lists: lists needs %zu ints, meta %d", pg_lists_ints((size_t)R, (size_t)K), 6 + 3 * (R + 1));
    const pg_lists L = pg_lists_carve(lists, (size_t)R, (size_t)K);
    pg_lists_clear(L, R, K);
    std::vector<int32_t> cur;
    pg_list_counts n;
    pg_build_adopters(R, K, ancestors, L, cur, n);
    if (early_free) pg_mark_adopted(R, K, ancestors, L);
    for (int i = 0; i < n_lookahead; ++i) {
        if (lookahead_nodes[i] < N || lookahead_nodes[i] >= N + R * K) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_reverse_lists: node id out of range");
        L.slow_flag[lookahead_nodes[i] - N] |= 2;
    }
    pg_build_parents(N, R, K, child, rows_form != 0, rows_form != 0 && early_free != 0, L, cur, n);
    debug_lists_meta(n, L.cap, R, meta);
    return PHYLO_OK;
}

int phylo_debug_lookahead_lists(int N, int K, int S, int M, const int32_t* roots_ad, int32_t* slow_flag, int32_t* image, int64_t n_image,
                                int32_t* meta, int n_meta) {
    if (N < 2 || K < 1 || S < 1 || M < 1 || !roots_ad || !slow_flag || !image || !meta)
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_lookahead_lists: bad arguments");
    const int R = N - 1;
    if (n_meta < 4 + 2 * (R + 1)) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_lookahead_lists: meta needs %d ints", 4 + 2 * (R + 1));
    for (int r = 1; r < R; ++r)                              // slots 0 .. N - r - 1 of rank event r: a leaf or a node of an earlier rank event
        for (int k = 0; k < K; ++k)
            for (int i = 0; i < N - r; ++i) {
                const int32_t x = roots_ad[((size_t)r * K + k) * N + i];
                if (x < 0 || x >= N + r * K) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_lookahead_lists: root id out of range");
            }
    std::vector<int32_t> pk;
    pg_lookahead x;
    pg_build_lookahead(N, K, S, PG_XCH, roots_ad, slow_flag, pk, x);
    if ((int64_t)pk.size() > n_image) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_lookahead_lists: image needs %zu ints", pk.size());
    memcpy(image, pk.data(), pk.size() * 4);
    meta[0] = (int32_t)x.n_xent; meta[1] = (int32_t)x.n_xchunks; meta[2] = (int32_t)x.n_xnodes; meta[3] = (int32_t)x.max_chunks;
    for (int r = 0; r <= R; ++r) {
        meta[4 + r] = x.ev_chunk0[r];
        meta[4 + (R + 1) + r] = x.ev_node0[r];
    }
    return PHYLO_OK;
}

int phylo_debug_reverse_plan(int N, int K, int K_local, int S, int world, int twisted, int marks, uint32_t switches, int64_t n_slow, int TS,
                             int64_t coeff_wgs, int passes_in_flight, uint32_t* mask) {
    if (N < 2 || K < 1 || K_local < 1 || S < 1 || world < 1 || TS < 1 || n_slow < 0 || coeff_wgs < 0 || !mask)
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_reverse_plan: bad arguments");
    pg_plan_in in{};
    in.N = N; in.K = K; in.K_local = K_local; in.S = S; in.world = world;
    in.twist = twisted != 0; in.marks = marks != 0;
    in.rev_host_lists = switches & 1; in.one_stream = switches & 2; in.two_streams = switches & 4;
    in.rows_chain = switches & 8; in.coeff_chain = switches & 16;
    in.dl_max_k = PG_DL_MAX_K;
    pg_plan p = pg_plan_form(in);
    pg_plan_chains(p, (long)n_slow, TS, (long)coeff_wgs, passes_in_flight, N - 1);
    *mask = pg_plan_mask(p);
    return PHYLO_OK;
}

int phylo_debug_sweep_plan(int N, int K, int K_local, int S, int G, int M, int world, int transport, uint32_t flags, uint32_t switches,
                           uint32_t* mask, int32_t* launches) {
    if (N < 2 || N > PK_MAX_TAXA || K < 1 || K_local < 1 || K_local > K || S < 1 || world < 1 || !mask || !launches)
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_sweep_plan: bad arguments");
    sweep_facts f{};
    f.N = N; f.K = K; f.Kloc = K_local; f.S = S; f.G = G; f.M = M; f.world = world;
    f.ntiles = (S + pm_site_tile(S) - 1) / pm_site_tile(S);
    f.transport = transport != 0;
    sweep_facts_flags(f, flags);
    f.env_eager_nodes = switches & 1; f.env_rehearse_sharded = switches & 2; f.env_replicated_book = switches & 4;
    f.jc = switches & 8; f.coded_leaves = switches & 16; f.device_exchange = switches & 32; f.clade_tables = switches & 64;
    char why[160];
    if (sweep_refuses_batch(f, k_sweep_limits, why, sizeof why) || sweep_refuses_form(f, k_sweep_limits, why, sizeof why))
        return fail(nullptr, PHYLO_EINVAL, "%s", why);
    const sweep_plan p = sweep_plan_form(f, k_sweep_limits);
    *mask = sweep_plan_mask(p);
    for (int r = -1; r <= p.R; ++r) launches[r + 1] = sweep_plan_launches(p, r);
    return PHYLO_OK;
}

int phylo_debug_sweep_chain(int N, int K, int K_local, int S, int G, int M, int world, int transport, uint32_t flags, uint32_t switches,
                            int multi_min, int scan_ancestors, int32_t* out) {
    if (N < 2 || N > PK_MAX_TAXA || K < 1 || K_local < 1 || K_local > K || S < 1 || world < 1 || !out)
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_sweep_chain: bad arguments");
    sweep_facts f{};
    f.N = N; f.K = K; f.Kloc = K_local; f.S = S; f.G = G; f.M = M; f.world = world;
    f.ntiles = (S + pm_site_tile(S) - 1) / pm_site_tile(S);
    f.transport = transport != 0;
    sweep_facts_flags(f, flags);
    f.env_eager_nodes = switches & 1; f.env_rehearse_sharded = switches & 2; f.env_replicated_book = switches & 4;
    f.jc = switches & 8; f.coded_leaves = switches & 16; f.device_exchange = switches & 32;
    char why[160];
    if (sweep_refuses_batch(f, k_sweep_limits, why, sizeof why) || sweep_refuses_form(f, k_sweep_limits, why, sizeof why))
        return fail(nullptr, PHYLO_EINVAL, "%s", why);
    const sweep_chain_form ch = sweep_chain_form_of(sweep_plan_form(f, k_sweep_limits), S, multi_min, scan_ancestors, k_sweep_limits);
    out[0] = ch.taken ? 1 : 0; out[1] = ch.item_waves; out[2] = ch.parts;
    return PHYLO_OK;
}

int phylo_debug_sweep_launch(int N, int K, int K_local, int S, int G, int M, int world, int transport, uint32_t flags, uint32_t switches,
                             int launch_xcd, int32_t* out) {
    if (N < 2 || N > PK_MAX_TAXA || K < 1 || K_local < 1 || K_local > K || S < 1 || world < 1 || !out)
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_sweep_launch: bad arguments");
    sweep_facts f{};
    f.N = N; f.K = K; f.Kloc = K_local; f.S = S; f.G = G; f.M = M; f.world = world;
    f.ntiles = (S + pm_site_tile(S) - 1) / pm_site_tile(S);
    f.transport = transport != 0;
    sweep_facts_flags(f, flags);
    f.env_eager_nodes = switches & 1; f.env_rehearse_sharded = switches & 2; f.env_replicated_book = switches & 4;
    f.jc = switches & 8; f.coded_leaves = switches & 16; f.device_exchange = switches & 32; f.clade_tables = switches & 64;
    f.env_launch_xcd = launch_xcd;
    char why[160];
    if (sweep_refuses_batch(f, k_sweep_limits, why, sizeof why) || sweep_refuses_form(f, k_sweep_limits, why, sizeof why))
        return fail(nullptr, PHYLO_EINVAL, "%s", why);
    const sweep_plan p = sweep_plan_form(f, k_sweep_limits);
    out[0] = p.launch_xcd ? 1 : 0; out[1] = p.book_xcd ? 1 : 0;
    return PHYLO_OK;
}

int phylo_debug_sweep_launch_of(phylo_ctx* c, int32_t* out) {
    if (!c || !out) return fail(c, PHYLO_EINVAL, "phylo_debug_sweep_launch_of: NULL argument");
    const sweep_plan& p = c->run.plan;
    out[0] = p.launch_xcd ? 1 : 0; out[1] = p.book_xcd ? 1 : 0;
    return PHYLO_OK;
}

int phylo_debug_launch_map(int n, int W, int xcd, int32_t* grid, int32_t* items, int64_t cap) {
    if (n < 1 || (W != 1 && W != 2 && W != 4) || !grid)
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_launch_map: bad arguments");
    const int g = pk_launch_grid(n, W, xcd != 0);
    *grid = g;
    if (!items) return PHYLO_OK;
    if (cap < (int64_t)g * W) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_launch_map: items needs %lld entries", (long long)g * W);
    for (int b = 0; b < g; ++b)
        for (int w = 0; w < W; ++w) items[(size_t)b * W + w] = pk_launch_item(b, g, W, w, xcd != 0);
    return PHYLO_OK;
}

int phylo_debug_sweep_chain_of(phylo_ctx* c, int32_t* taken) {
    if (!c || !taken) return fail(c, PHYLO_EINVAL, "phylo_debug_sweep_chain_of: NULL argument");
    *taken = c->last_chain;
    return PHYLO_OK;
}

int phylo_debug_scan_ancestors(phylo_ctx* c, const double* logw, int Kg, int G, const uint64_t* seeds, uint32_t r_next, int32_t* anc,
                               int32_t* list, int32_t* cnt) {
    CHK(bind(c));
    if (!logw || !seeds || !anc || !list || !cnt || Kg < 1 || G < 1 || G > PK_MAX_GROUPS)
        return fail(c, PHYLO_EINVAL, "phylo_debug_scan_ancestors: bad arguments");
    const size_t K = (size_t)Kg * G;
    void *dw, *dcdf, *dout, *dseed;
    CHK(scratch_get(c, 0, K * 8, &dw));
    CHK(scratch_get(c, 1, K * 8, &dcdf));
    CHK(scratch_get(c, 2, (2 * K + (size_t)G) * 4, &dout));
    CHK(scratch_get(c, 3, (size_t)G * 8, &dseed));
    HIPCHK(c, hipMemcpyAsync(dw, logw, K * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dseed, seeds, (size_t)G * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dout, 0xff, (2 * K + (size_t)G) * 4, c->stream));      // (what the scan does not write shows as -1)
    pp_anc_out ao{};
    ao.anc = (int32_t*)dout; ao.list = ao.anc + K; ao.cnt = ao.list + K;
    ao.group_seeds = (const uint64_t*)dseed; ao.r_next = r_next;
    CHK(launch_scan(c, (const double*)dw, Kg, G, (uint64_t*)dcdf, (double*)nullptr, 0, 0, &ao));
    HIPCHK(c, hipMemcpyAsync(anc, ao.anc, K * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(list, ao.list, K * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cnt, ao.cnt, (size_t)G * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

int phylo_debug_pack_leaf_codes(const uint8_t* codes, int N, int S, uint8_t* packed, int64_t cap, int64_t* need) {
    if (N < 1 || S < 1 || !need || (packed && !codes)) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_pack_leaf_codes: bad arguments");
    *need = (int64_t)pk_packed_bytes(N, S);
    if (!packed) return PHYLO_OK;
    if (cap < *need) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_pack_leaf_codes: the image takes %lld bytes (got %lld)", (long long)*need, (long long)cap);
    pk_pack_leaf_codes(codes, N, S, packed);
    return PHYLO_OK;
}

int phylo_debug_site_patterns(const uint8_t* codes, int N, int S, int32_t* U, int32_t* rep, uint16_t* image, uint32_t* rep_off,
                              uint8_t* rep_leaf, int64_t rep_leaf_cap) {
    if (N < 1 || S < 1 || !codes || !U) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_site_patterns: bad arguments");
    std::vector<int32_t> pat((size_t)S), rp((size_t)S);
    *U = pk_pat_columns(codes, N, S, pat.data(), rp.data());
    if (rep) memcpy(rep, rp.data(), (size_t)*U * sizeof(int32_t));
    if (image && *U <= PK_PAT_IMAGE_MAX_U) pk_pat_pack_image(pat.data(), S, *U, image);
    if (rep_off && *U <= PK_PAT_MAX_U) pk_pat_rep_offsets(rp.data(), *U, rep_off);
    if (rep_leaf && *U <= PK_PAT_MAX_U) {
        if (rep_leaf_cap < (int64_t)pk_packed_bytes(N, *U))
            return fail(nullptr, PHYLO_EINVAL, "phylo_debug_site_patterns: the representative leaf image takes %lld bytes (got %lld)",
                        (long long)pk_packed_bytes(N, *U), (long long)rep_leaf_cap);
        pk_pat_rep_leaf_image(codes, N, S, rp.data(), *U, rep_leaf, pk_packed_leaf_bytes(*U));
    }
    return PHYLO_OK;
}

int phylo_debug_site_patterns_rule(int S, int U, int coded, int ntiles, int sw) {
    if (S < 1 || U < 0 || ntiles < 1 || sw < PK_PAT_OFF || sw > PK_PAT_FORCE) {
        (void)fail(nullptr, PHYLO_EINVAL, "phylo_debug_site_patterns_rule: bad arguments");
        return -1;
    }
    return pk_pat_take(S, U, coded != 0, ntiles, sw) ? 1 : 0;
}

int phylo_debug_site_patterns_of(phylo_ctx* c, int32_t* U, int32_t* taken) {
    if (!c || !U || !taken) return fail(c, PHYLO_EINVAL, "phylo_debug_site_patterns_of: NULL argument");
    if (!c->have_leaves) return fail(c, PHYLO_ESTATE, "phylo_debug_site_patterns_of needs leaves");
    *U = c->pat_U;
    *taken = pat_on(c) ? 1 : 0;
    return PHYLO_OK;
}

int phylo_debug_clade_patterns_rule(int pat_taken, int N, int S, int U, int sw, int64_t* bytes) {
    if (N < 1 || S < 1 || U < 0 || sw < PK_CLADE_OFF || sw > PK_CLADE_FORCE) {
        (void)fail(nullptr, PHYLO_EINVAL, "phylo_debug_clade_patterns_rule: bad arguments");
        return -1;
    }
    if (bytes) *bytes = (int64_t)pk_clade_layout_of(N, S, U).total;
    return pk_clade_take(pat_taken != 0, N, S, U, sw) ? 1 : 0;
}

// The clade tables of byte codes [N][S] (N <= PK_CLADE_MAX_N) as phylo_set_leaves builds them: layout[5] = codes_bytes, rep_bytes,
// image_bytes, stride, total; with `tables` (cap >= total bytes) the buffer, with `cls` ([2^N][U] uint16) every bitset's classes.
int phylo_debug_clade_tables(const uint8_t* codes, int N, int S, int32_t* U, int64_t* layout, uint8_t* tables, int64_t cap, uint16_t* cls) {
    if (N < 1 || N > PK_CLADE_MAX_N || S < 1 || !codes || !U || !layout) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_clade_tables: bad arguments");
    std::vector<int32_t> pat((size_t)S), rp((size_t)S);
    *U = pk_pat_columns(codes, N, S, pat.data(), rp.data());
    const pk_clade_layout L = pk_clade_layout_of(N, S, *U);
    layout[0] = (int64_t)L.codes_bytes; layout[1] = (int64_t)L.rep_bytes; layout[2] = (int64_t)L.image_bytes;
    layout[3] = (int64_t)L.stride; layout[4] = (int64_t)L.total;
    if (!tables) return PHYLO_OK;
    if (*U > PK_PAT_MAX_U) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_clade_tables: U = %d exceeds %d", *U, PK_PAT_MAX_U);
    if (cap < (int64_t)L.total) return fail(nullptr, PHYLO_EINVAL, "phylo_debug_clade_tables: the tables take %lld bytes (got %lld)", (long long)L.total, (long long)cap);
    pk_clade_build(codes, N, S, pat.data(), rp.data(), *U, tables, cls);
    return PHYLO_OK;
}

// eligible: the tables of the current leaves are built and the pattern form is taken; taken: the last sweep begun took the form
int phylo_debug_clade_patterns_of(phylo_ctx* c, int32_t* eligible, int32_t* taken, int64_t* bytes) {
    if (!c || !eligible || !taken || !bytes) return fail(c, PHYLO_EINVAL, "phylo_debug_clade_patterns_of: NULL argument");
    if (!c->have_leaves) return fail(c, PHYLO_ESTATE, "phylo_debug_clade_patterns_of needs leaves");
    *eligible = (c->clade_ready && pat_on(c)) ? 1 : 0;
    *taken = c->run.plan.clade_pat ? 1 : 0;
    *bytes = c->clade_ready ? (int64_t)c->clade_layout.total : 0;
    return PHYLO_OK;
}

int phylo_debug_tree_plan(int N, int K, int G, int world, int64_t n_clades, int64_t n_topologies, int kept_whole, int force_wide,
                          int64_t summary_temp, int64_t branches_temp, int64_t* scalars, int64_t* summary_slab, int64_t* branches_slab,
                          int32_t* sort_bits, int32_t* launches) {
    if (K < 1 || G < 1 || K % G != 0 || N > PK_MAX_TAXA || world < 1 || summary_temp < 0 || branches_temp < 0 || !scalars || !summary_slab ||
        !branches_slab || !sort_bits || !launches)
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_tree_plan: bad arguments");
    char why[160];
    const pt_facts f{N, K, G, world};
    if (pt_refuses(f, why, sizeof why)) return fail(nullptr, PHYLO_EINVAL, "%s", why);
    const pb_facts fb{N, K, G, world, n_clades, n_topologies, kept_whole != 0, force_wide != 0};
    if (pb_refuses(fb, why, sizeof why)) return fail(nullptr, PHYLO_ESTATE, "%s", why);
    pt_plan p = pt_plan_form(f);
    pt_plan_slab(p, (size_t)summary_temp);
    pb_plan q = pb_plan_form(fb);
    pb_plan_slab(q, (size_t)branches_temp);
    unsigned bits[PT_MAX_WORDS + 9];
    const int n_sorts = pt_plan_sorts(p, bits);
    for (int i = 0; i < n_sorts; ++i) sort_bits[i] = (int32_t)bits[i];
    const int64_t sc[] = {p.R, p.L, p.W, p.E, p.Emax, p.Kg, q.cbits, q.tbits, q.wide, q.gather, n_sorts, pt_slab::NBUF, pb_slab::NBUF};
    memcpy(scalars, sc, sizeof sc);
    for (int i = 0; i < pt_slab::NBUF; ++i) { summary_slab[i] = (int64_t)p.slab.off[i]; summary_slab[pt_slab::NBUF + i] = (int64_t)p.slab.bytes[i]; }
    summary_slab[2 * pt_slab::NBUF] = (int64_t)p.slab.total;
    for (int i = 0; i < pb_slab::NBUF; ++i) { branches_slab[i] = (int64_t)q.slab.off[i]; branches_slab[pb_slab::NBUF + i] = (int64_t)q.slab.bytes[i]; }
    branches_slab[2 * pb_slab::NBUF] = (int64_t)q.slab.total;
    launches[0] = pt_plan_launches(p);
    launches[1] = pb_plan_launches(q);
    return PHYLO_OK;
}

int phylo_debug_scan_form(phylo_ctx* c, int Kg, int multi_min, int wanted) {
    if (Kg < 1) {
        (void)fail(c, PHYLO_EINVAL, "phylo_debug_scan_form: bad arguments");
        return -1;
    }
    return (int)sweep_scan_form_of(Kg, c ? c->env.scan_multi_min : multi_min, wanted != 0, k_sweep_limits);
}

int phylo_debug_persist_plan(int N, int K, int S, int G, uint32_t flags, uint32_t switches, int world, int transport, int n_cus,
                             int blocks_per_cu, int persist_wgs, int persist_nt, int64_t* out) {
    if (N < 1 || K < 1 || S < 1 || G < 1 || K % G != 0 || world < 1 || !out)
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_persist_plan: bad arguments");
    persist_facts f = persist_facts_flags(N, K, S, G, world, transport != 0, flags, (switches & 2) != 0, (switches & 1) != 0);
    f.n_cus = n_cus; f.blocks_per_cu = blocks_per_cu; f.persist_wgs = persist_wgs; f.persist_nt = persist_nt_of(persist_nt);
    const persist_grid p = persist_plan_of(f, k_persist_limits);
    out[0] = p.taken ? 1 : 0; out[1] = p.Wg; out[2] = p.m; out[3] = p.nt; out[4] = (int64_t)p.lds;
    return PHYLO_OK;
}

int phylo_debug_persist_of(phylo_ctx* c, int32_t* nt, int32_t* Wg, int32_t* m, int64_t* lds) {
    if (!c || !nt || !Wg || !m || !lds) return fail(c, PHYLO_EINVAL, "phylo_debug_persist_of: NULL argument");
    if (!c->last_persistent) return fail(c, PHYLO_ESTATE, "phylo_debug_persist_of: the last sweep was not a one-launch sweep");
    *nt = c->last_pp_nt; *Wg = c->last_pp_Wg; *m = c->last_pp_m; *lds = (int64_t)c->last_pp_lds;
    return PHYLO_OK;
}

int phylo_debug_tree_branches_of(phylo_ctx* c, int32_t* wide, int32_t* cbits, int32_t* tbits) {
    if (!c || !wide || !cbits || !tbits) return fail(c, PHYLO_EINVAL, "phylo_debug_tree_branches_of: NULL argument");
    if (c->tb_wide < 0) return fail(c, PHYLO_ESTATE, "phylo_debug_tree_branches_of: no phylo_tree_branches has run");
    *wide = c->tb_wide; *cbits = c->tb_cbits; *tbits = c->tb_tbits;
    return PHYLO_OK;
}

int phylo_debug_reverse_plan_batch(int N, int K, int G, int S, uint32_t switches, int64_t n_slow, int TS, int64_t coeff_wgs,
                                   int passes_in_flight, uint32_t* mask) {
    if (N < 2 || K < 1 || G < 1 || K % G != 0 || S < 1 || TS < 1 || n_slow < 0 || coeff_wgs < 0 || !mask)
        return fail(nullptr, PHYLO_EINVAL, "phylo_debug_reverse_plan_batch: bad arguments");
    pg_plan_in in{};
    in.N = N; in.K = K; in.K_local = K; in.S = S; in.world = 1;
    in.twist = false; in.marks = true;                      // (a batched sweep that keeps its graph: plain proposal, lazy)
    in.rev_host_lists = switches & 1; in.one_stream = switches & 2; in.two_streams = switches & 4;
    in.rows_chain = switches & 8; in.coeff_chain = switches & 16;
    in.dl_max_k = PG_DL_MAX_K;
    in.groups = G;
    pg_plan p = pg_plan_form(in);
    pg_plan_chains(p, (long)n_slow, TS, (long)coeff_wgs, passes_in_flight, N - 1);
    *mask = pg_plan_mask(p);
    return PHYLO_OK;
}

static int debug_device_lists_run(phylo_ctx* c, int32_t* lists, int64_t n_lists, int32_t* meta, int n_meta);

int phylo_debug_device_lists_of(phylo_ctx* c, const int64_t* ancestors, const int32_t* child, int32_t* lists, int64_t n_lists,
                                int32_t* meta, int n_meta) {
    CHK(bind(c));
    if (c->Kloc != c->K || c->K > PG_DL_MAX_K || !child || (c->N > 2 && !ancestors))
        return fail(c, PHYLO_EINVAL, "phylo_debug_device_lists_of: not sharded, K <= %d, ancestors and child given", PG_DL_MAX_K);
    CHK(ensure_sweep_state(c));
    CHK(ensure_graph_state(c));
    const int R = c->N - 1, K = c->K;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->swept = false; ++c->sweep_serial;   // the sweep's genealogy is overwritten: no reverse pass on it after this
    c->last_graph = false;
    if (R > 1) HIPCHK(c, hipMemcpy(c->d_anc, ancestors, (size_t)(R - 1) * K * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_child, child, (size_t)R * K * 2 * 4, hipMemcpyHostToDevice));
    return debug_device_lists_run(c, lists, n_lists, meta, n_meta);
}

int phylo_debug_device_lists(phylo_ctx* c, int32_t* lists, int64_t n_lists, int32_t* meta, int n_meta, int64_t* ancestors, int32_t* child) {
    CHK(bind(c));
    if (!c->swept || !c->last_graph || !c->last_graph_marks || c->last_graph_twist || c->Kloc != c->K || c->K / c->last_G > PG_DL_MAX_K)
        return fail(c, PHYLO_ESTATE, "phylo_debug_device_lists needs a preceding lazy sweep with PHYLO_KEEP_GRAPH and the plain proposal, not sharded, K <= %d", PG_DL_MAX_K);
    const int R = c->N - 1, K = c->K;
    CHK(debug_device_lists_run(c, lists, n_lists, meta, n_meta));
    if (ancestors && R > 1) memcpy(ancestors, c->h_anc_p, (size_t)(R - 1) * K * 8);   // the pinned copies the sweep left
    if (child) memcpy(child, c->h_child_p, (size_t)R * K * 2 * 4);
    return PHYLO_OK;
}

static int debug_device_lists_run(phylo_ctx* c, int32_t* lists, int64_t n_lists, int32_t* meta, int n_meta) {
    const int R = c->N - 1, K = c->K;
    const size_t ints = pg_lists_ints((size_t)R, (size_t)K);
    if (!lists || !meta || n_lists < (int64_t)ints || n_meta < 6 + 3 * (R + 1))
        return fail(c, PHYLO_EINVAL, "phylo_debug_device_lists: lists needs %zu ints, meta %d", ints, 6 + 3 * (R + 1));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_ad_off, 0xff, ints * 4, c->stream));        // (what the builders do not write stays -1)
    CHK(dev_lists_launch(c, c->stream, c->stream));
    pg_list_counts m;
    CHK(dev_lists_wait(c, m));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(lists, c->d_ad_off, ints * 4, hipMemcpyDeviceToHost));
    debug_lists_meta(m, pg_lists_cap((size_t)R, (size_t)K), R, meta);
    return PHYLO_OK;
}

// ---- tree posterior of the last sweep (phylo_trees.h; the form: phylo_trees_plan.h) --------------------
extern "C++" {
// (key, value) pairs of a stable sort and the buffers it may write: pt_sort leaves the sorted pairs in k / v again
template <typename KEY>
struct pt_pairs { KEY *k, *k_alt; uint32_t *v, *v_alt; };
// the run of a pass: the stages below read the plan and these, nothing else decides
struct ts_run {
    phylo_ctx* c; pt_plan plan; int launches;
    const int32_t* child;                // the children records [R][K][2]: the sweep's, or the gathered ones
    pt_pairs<unsigned long long> q;      // the current sort buffers
};
struct tb_run {
    phylo_ctx* c; pb_plan plan; int launches;
    const int32_t* child;
    const double *bl, *br;               // whole-K branch lengths [R][K]
    unsigned int* err;                   // this pass's error word: [3] of the summary's
    pb_seg_args a;
};
#define PT_LAUNCH(kern, n, ...)                                                                                       \
    do {                                                                                                              \
        hipLaunchKernelGGL(kern, dim3((unsigned)(((n) + PT_NT - 1) / PT_NT)), dim3(PT_NT), 0, p.c->stream, __VA_ARGS__); \
        CHK(launch_check(p.c, #kern));                                                                                \
        ++p.launches;                                                                                                 \
    } while (0)

// one stable LSD pass over n pairs on bits [0, bits)
template <typename KEY>
static int pt_sort(phylo_ctx* c, void* temp, size_t temp_bytes, pt_pairs<KEY>& q, long long n, unsigned bits, int& launches) {
    HIPCHK(c, rocprim::radix_sort_pairs(temp, temp_bytes, q.k, q.k_alt, q.v, q.v_alt, (size_t)n, 0u, bits, c->stream));
    std::swap(q.k, q.k_alt); std::swap(q.v, q.v_alt);
    ++launches;
    return PHYLO_OK;
}

// rocPRIM's temporary storage: the largest of what sorts of n32 / n64 pairs with 32- / 64-bit keys, inclusive scans of n_scan u32
// and u64 and an exclusive scan of n_excl counts need (0: not issued).  The queries launch nothing.
static int pt_temp_bytes(phylo_ctx* c, size_t n32, size_t n64, size_t n_scan, size_t n_excl, size_t& temp) {
    uint32_t* const v = nullptr;
    unsigned long long* const w = nullptr;
    size_t t[5] = {0, 0, 0, 0, 0};
    if (n32) HIPCHK(c, rocprim::radix_sort_pairs(nullptr, t[0], v, v, v, v, n32, 0u, 32u, c->stream));
    if (n64) HIPCHK(c, rocprim::radix_sort_pairs(nullptr, t[1], w, w, v, v, n64, 0u, 64u, c->stream));
    if (n_scan) HIPCHK(c, rocprim::inclusive_scan(nullptr, t[2], (const uint32_t*)v, v, n_scan, rocprim::plus<uint32_t>(), c->stream));
    if (n_scan) HIPCHK(c, rocprim::inclusive_scan(nullptr, t[3], (const unsigned long long*)w, w, n_scan, rocprim::plus<unsigned long long>(), c->stream));
    if (n_excl) HIPCHK(c, rocprim::exclusive_scan(nullptr, t[4], (const int32_t*)nullptr, v, 0u, n_excl, rocprim::plus<uint32_t>(), c->stream));
    temp = *std::max_element(t, t + 5);
    return PHYLO_OK;
}

// the slab of a pass from its scratch slot, its buffers' pointers from the plan's layout (BUFS: the list that made the layout)
#define PT_SLAB_CARVE(name, T, n) bufs.name = reinterpret_cast<T*>(base + slab.off[slab.name]);
#define PT_CARVE(BUFS, slot, bufs_)                             \
    do {                                                        \
        void* base_ = nullptr;                                  \
        CHK(scratch_get(p.c, slot, p.plan.slab.total, &base_)); \
        char* base = (char*)base_;                              \
        const auto& slab = p.plan.slab;                         \
        auto& bufs = bufs_;                                     \
        BUFS(PT_SLAB_CARVE)                                     \
    } while (0)

// Sharded: every rank's rows [R][Kloc][width] -> whole-K [R][K][width] in dst, by the host collective in chunks of 1 MiB per rank
// and call (within the host-mediated transport's slot).  A collective: every rank issues the same calls in the same order.
template <typename T>
static int pt_gather_rows(phylo_ctx* c, const T* src, T* dst, size_t width) {
    const size_t R = (size_t)c->N - 1, K = c->K, Kl = c->Kloc, P = c->world, row = Kl * width, mine_n = R * row;
    std::vector<T> mine(mine_n), all(P * mine_n), part, whole(R * K * width);
    HIPCHK(c, hipMemcpy(mine.data(), src, mine_n * sizeof(T), hipMemcpyDeviceToHost));
    const size_t chunk = ((size_t)1 << 20) / sizeof(T);
    for (size_t o = 0; o < mine_n; o += chunk) {
        const size_t n = std::min(chunk, mine_n - o);
        part.resize(n * P);
        const int rc = phylo_comm_allgather_host(c->comm, mine.data() + o, n * sizeof(T), part.data(), c->stream, &c->err);
        if (rc != PHYLO_OK) { g_last_error = c->err; return rc; }
        for (size_t q = 0; q < P; ++q) memcpy(all.data() + q * mine_n + o, part.data() + q * n, n * sizeof(T));
    }
    for (size_t r = 0; r < R; ++r)
        for (size_t q = 0; q < P; ++q) memcpy(whole.data() + (r * K + q * Kl) * width, all.data() + q * mine_n + r * row, row * sizeof(T));
    HIPCHK(c, hipMemcpy(dst, whole.data(), whole.size() * sizeof(T), hipMemcpyHostToDevice));
    return PHYLO_OK;
}

// the events of a pass (made at its first call) and the first one's record; its device time and launch count
static int pt_time_begin(phylo_ctx* c, hipEvent_t& e0, hipEvent_t& e1) {
    if (!e0) HIPCHK(c, hipEventCreate(&e0));
    if (!e1) HIPCHK(c, hipEventCreate(&e1));
    HIPCHK(c, hipEventRecord(e0, c->stream));
    return PHYLO_OK;
}
static int pt_perf(phylo_ctx* c, hipEvent_t e0, hipEvent_t e1, int launches, phylo_stats* perf) {
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, e0, e1));
    if (perf) { *perf = phylo_stats{}; perf->sweep_ms = ms; perf->n_launches = launches; }
    return PHYLO_OK;
}

// 1. check: the state, the refusals, the plan
static int ts_check(ts_run& p, const int64_t* n_clades, const int32_t* n_topologies) {
    phylo_ctx* c = p.c;
    CHK(bind(c));
    if (!n_clades || !n_topologies) return fail(c, PHYLO_EINVAL, "phylo_tree_summary: NULL count pointer");
    if (!c->swept) return fail(c, PHYLO_ESTATE, "phylo_tree_summary: no sweep has been run");
    if (c->run.active) return fail(c, PHYLO_ESTATE, "phylo_tree_summary: a sweep is being issued (phylo_sweep_finish first)");
    const pt_facts f{c->N, c->K, c->last_G, c->world};
    char why[160];
    if (pt_refuses(f, why, sizeof why)) return fail(c, PHYLO_EINVAL, "%s", why);
    p.plan = pt_plan_form(f);
    c->ts_done = c->tb_done = false;
    return PHYLO_OK;
}

// 2. carve: every buffer from one grow-only slab (scratch slot 12); 3. gather: sharded, the children records of all K particles
static int ts_carve_and_gather(ts_run& p) {
    phylo_ctx* c = p.c;
    size_t temp = 0;
    CHK(pt_temp_bytes(c, 0, (size_t)p.plan.Emax, (size_t)p.plan.Emax, 0, temp));
    pt_plan_slab(p.plan, temp);
    PT_CARVE(PT_SLAB_BUFS, 12, c->ts);
    p.child = c->d_child;
    if (p.plan.world > 1) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        CHK(pt_gather_rows(c, (const int32_t*)c->d_child, c->ts.child, 2));
        p.child = c->ts.child;
    }
    return PHYLO_OK;
}

// Keys -> stable sort: one pass over the n current pairs.  TS_WORD: an element's key is word `arg` of its clade's bitset (arg < 0:
// its group); TS_ORDER: pt_order_keys of mode `arg` (0 weight descending, 1 group, 2 representative).  fresh: the elements are
// 0 .. n-1 in order and the kernel writes the values; else it reads them.
enum ts_key { TS_WORD, TS_ORDER };
static int ts_sort_by(ts_run& p, long long n, ts_key kind, int arg, bool fresh, unsigned bits) {
    const pt_plan& m = p.plan;
    const pt_bufs& b = p.c->ts;
    const uint32_t* cur = fresh ? nullptr : p.q.v;
    uint32_t* ident = fresh ? p.q.v : nullptr;
    if (kind == TS_WORD)
        PT_LAUNCH(pt_clade_keys, n, (const unsigned long long*)b.bits, cur, n, m.K, m.W, arg, m.Kg, p.q.k, ident);
    else
        PT_LAUNCH(pt_order_keys, n, cur, n, arg, m.K, (const unsigned long long*)b.weight, (const uint32_t*)b.group,
                  (const uint32_t*)b.first, p.q.k, ident);
    return pt_sort(p.c, b.temp, m.temp_bytes, p.q, n, bits, p.launches);
}
// ... and, for a batch, the stable pass behind it that brings each group's elements together (by content / of an output order)
static int ts_group_pass(ts_run& p, long long n, bool order) {
    if (!p.plan.groups) return PHYLO_OK;
    return order ? ts_sort_by(p, n, TS_ORDER, 1, false, p.plan.order_group_bits) : ts_sort_by(p, n, TS_WORD, -1, false, p.plan.group_bits);
}

// Group equal keys: the n current pairs are sorted and a heads kernel has left every run's first element in flag, every element's
// weight in val.  Segment ids (own: per element), each segment's weight, count, group and first element; err[count_word] = segments.
static int ts_groups(ts_run& p, long long n, uint32_t* own, int count_word) {
    const pt_plan& m = p.plan;
    const pt_bufs& b = p.c->ts;
    size_t bytes = m.temp_bytes;
    HIPCHK(p.c, rocprim::inclusive_scan(b.temp, bytes, (const uint32_t*)b.flag, b.sid, (size_t)n, rocprim::plus<uint32_t>(), p.c->stream));
    HIPCHK(p.c, rocprim::inclusive_scan(b.temp, bytes, (const unsigned long long*)b.val, b.scan, (size_t)n, rocprim::plus<unsigned long long>(),
                                        p.c->stream));
    p.launches += 2;
    PT_LAUNCH(pt_seg_ids, n, (const uint32_t*)p.q.v, (const uint32_t*)b.flag, (const uint32_t*)b.sid, n, own, b.seg_start);
    PT_LAUNCH(pt_seg_sums, n, (const uint32_t*)p.q.v, (const uint32_t*)b.sid, (const uint32_t*)b.seg_start, (const unsigned long long*)b.scan,
              n, m.K, m.Kg, m.G, b.weight, b.count, b.group, b.first);
    HIPCHK(p.c, hipMemcpyAsync(b.err + count_word, b.sid + (n - 1), 4, hipMemcpyDeviceToDevice, p.c->stream));
    return PHYLO_OK;
}

// 4. - 7. the clade table
static int ts_clades(ts_run& p) {
    phylo_ctx* c = p.c;
    const pt_plan& m = p.plan;
    pt_bufs& b = c->ts;
    const long long E = m.E;
    // 4. weights and walk: integer weights of the particles; every tree walked into node slots and clade bitsets
    CHK(pt_time_begin(c, c->ev_ts0, c->ev_ts1));
    HIPCHK(c, hipMemsetAsync(b.err, 0, 16, c->stream));
    PT_LAUNCH(pt_weights, (long long)m.G * PT_NT, (const double*)(c->d_logw + (size_t)(m.R - 1) * m.K), m.Kg, b.u, b.U);   // (a workgroup per group)
    PT_LAUNCH(pt_walk, m.K, p.child, m.N, m.K, m.W, b.slot, b.bits, (unsigned int*)b.err);
    // 5. clade sort: stable passes over the bitset words, least significant first, then the group
    p.q = {b.kA, b.kB, b.vA, b.vB};
    for (int w = 0; w < m.W; ++w) CHK(ts_sort_by(p, E, TS_WORD, w, w == 0, m.word_bits[w]));
    CHK(ts_group_pass(p, E, false));
    // 6. clade groups: equal bitsets of a group are one clade (cid), with its weight
    PT_LAUNCH(pt_clade_heads, E, (const unsigned long long*)b.bits, (const uint32_t*)p.q.v, E, m.K, m.W, m.Kg, (const unsigned long long*)b.u,
              b.flag, b.val);
    CHK(ts_groups(p, E, b.cid, 1));
    // 7. clade order and output: weight descending (the segments are in bitset order already), then the group
    CHK(ts_sort_by(p, E, TS_ORDER, 0, true, m.weight_bits));
    CHK(ts_group_pass(p, E, true));
    b.cord = p.q.v;                                        // final here: vA or vB, by the number of passes so far
    PT_LAUNCH(pt_clade_out, E, b.cord, (const uint32_t*)b.sid, E, m.K, m.W, (const unsigned long long*)b.bits,
              (const unsigned long long*)b.weight, (const uint32_t*)b.group, (const uint32_t*)b.first, b.o_cbits, b.o_cw, b.o_cg);
    return PHYLO_OK;
}

// 8. - 10. the topology table.  Live across these stages: u, bits, cid and cord's buffer, which is why they sort their values in
// vC / vD; kA, kB and the segment arrays (flag .. first) are free again.  Live across the branch pass, which reads them: u, slot,
// cid, cord, o_tn, o_ptopo, child (sharded), and err[3], its own error word.
static int ts_topologies(ts_run& p) {
    const pt_plan& m = p.plan;
    const pt_bufs& b = p.c->ts;
    const long long K = m.K;
    // 8. in-particle sort and hash: each particle's clade ids ascending (the sorted keys stay in srt), the hash of that vector
    p.q = {b.kA, b.srt, b.vC, b.vD};
    PT_LAUNCH(pt_topo_pairs, m.E, (const uint32_t*)b.cid, m.E, m.K, p.q.k, p.q.v);
    CHK(pt_sort(p.c, b.temp, m.temp_bytes, p.q, m.E, m.cid_bits, p.launches));
    p.q = {b.kA, b.kB, b.vC, b.vD};
    PT_LAUNCH(pt_topo_hash, K, (const unsigned long long*)b.srt, m.K, m.L, p.q.k, p.q.v, b.hp);
    // 9. topology groups: the particles by (group, hash); equal vectors of a group are one topology (tid), with its weight
    CHK(pt_sort(p.c, b.temp, m.temp_bytes, p.q, K, m.weight_bits, p.launches));
    CHK(ts_group_pass(p, K, false));
    PT_LAUNCH(pt_topo_heads, K, (const unsigned long long*)b.hp, (const uint32_t*)p.q.v, (const unsigned long long*)b.srt, m.K, m.L, m.Kg,
              (const unsigned long long*)b.u, b.flag, b.val, (unsigned int*)b.err);
    CHK(ts_groups(p, K, b.tid, 2));
    // 10. topology order and output: representative ascending, then weight descending, then the group
    CHK(ts_sort_by(p, K, TS_ORDER, 2, true, m.rep_bits));
    CHK(ts_sort_by(p, K, TS_ORDER, 0, false, m.weight_bits));
    CHK(ts_group_pass(p, K, true));
    PT_LAUNCH(pt_topo_out, K, (const uint32_t*)p.q.v, (const uint32_t*)b.sid, m.K, m.Kg, (const unsigned long long*)b.weight,
              (const uint32_t*)b.count, (const uint32_t*)b.group, (const uint32_t*)b.first, b.o_tw, b.o_tn, b.o_trep, b.o_tg);
    PT_LAUNCH(pt_invert, K, (const uint32_t*)p.q.v, K, b.pos);
    PT_LAUNCH(pt_particle_topo, K, (const uint32_t*)b.tid, (const uint32_t*)b.pos, m.K, b.o_ptopo);
    return PHYLO_OK;
}

// 11. finish: the error words, the sweep's own timeout word, the counts
static int ts_finish(ts_run& p, int64_t* n_clades, int32_t* n_topologies, int32_t* n_groups, phylo_stats* perf) {
    phylo_ctx* c = p.c;
    HIPCHK(c, hipEventRecord(c->ev_ts1, c->stream));
    uint32_t hs[4] = {0, 0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(hs, c->ts.err, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned int tmo = 0;                                  // the summarised sweep's own timeout word (read, not cleared: the fetch reports it)
    if (c->last_graph && c->h_pub) tmo = c->h_pub[2];
    else HIPCHK(c, hipMemcpy(&tmo, c->d_counter + 1, sizeof tmo, hipMemcpyDeviceToHost));
    if (tmo) return fail(c, PHYLO_EHIP, "phylo_tree_summary: the sweep timed out in a bounded wait between workgroups; its results are invalid");
    if (hs[0] & PT_ERR_TREE) return fail(c, PHYLO_EHIP, "phylo_tree_summary: the sweep's children records do not form one tree per particle");
    if (hs[0] & PT_ERR_COLLISION)
        return fail(c, PHYLO_EHIP, "phylo_tree_summary: two different topologies share a 64-bit routing hash (not merged; summary refused)");
    CHK(pt_perf(c, c->ev_ts0, c->ev_ts1, p.launches, perf));
    *n_clades = c->ts_nc = hs[1];
    *n_topologies = c->ts_nt = (int)hs[2];
    c->ts_G = p.plan.G;
    if (n_groups) *n_groups = p.plan.G;
    c->ts_serial = c->sweep_serial;
    c->ts_done = true;
    return PHYLO_OK;
}

static int tree_summary_impl(phylo_ctx* c, int64_t* n_clades, int32_t* n_topologies, int32_t* n_groups, phylo_stats* perf) {
    ts_run p{c};
    CHK(ts_check(p, n_clades, n_topologies));
    CHK(ts_carve_and_gather(p));
    CHK(ts_clades(p));
    CHK(ts_topologies(p));
    return ts_finish(p, n_clades, n_topologies, n_groups, perf);
}

// ---- the branch pass over the last summary
// 1. check: the state (a new sweep makes the summary stale), the refusal, the plan
static int tb_check(tb_run& p) {
    phylo_ctx* c = p.c;
    CHK(bind(c));
    if (c->run.active) return fail(c, PHYLO_ESTATE, "phylo_tree_branches: a sweep is being issued (phylo_sweep_finish first)");
    if (!c->swept || !c->ts_done || c->ts_serial != c->sweep_serial)
        return fail(c, PHYLO_ESTATE, "phylo_tree_branches: no phylo_tree_summary of the last sweep (a new sweep needs a new summary)");
    const pb_facts f{c->N, c->K, c->ts_G, c->world, c->ts_nc, c->ts_nt, c->last_graph && c->d_gbl && c->d_gbr, c->env.tree_wide_keys};
    char why[160];
    if (pb_refuses(f, why, sizeof why)) return fail(c, PHYLO_ESTATE, "%s", why);
    p.plan = pb_plan_form(f);
    c->tb_done = false;
    return PHYLO_OK;
}

// 2. carve: every buffer from one grow-only slab (scratch slot 13); 3. gather: whole-K children records and branch lengths.  Sharded:
// the summary's gathered children and what a kept graph's graph_gather made whole already, or two collectives here (bl, then br)
static int tb_carve_and_gather(tb_run& p) {
    phylo_ctx* c = p.c;
    size_t temp = 0;
    CHK(pt_temp_bytes(c, (size_t)p.plan.E, p.plan.wide ? (size_t)p.plan.E : 0, 0, (size_t)p.plan.nt, temp));
    pb_plan_slab(p.plan, temp);
    PT_CARVE(PB_SLAB_BUFS, 13, c->tb);
    p.child = c->d_child; p.bl = c->d_bl; p.br = c->d_br;
    if (p.plan.world == 1) return PHYLO_OK;
    p.child = c->ts.child; p.bl = c->d_gbl; p.br = c->d_gbr;
    if (p.plan.gather) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        CHK(pt_gather_rows(c, (const double*)c->d_bl, c->tb.gbl, 1));
        CHK(pt_gather_rows(c, (const double*)c->d_br, c->tb.gbr, 1));
        p.bl = c->tb.gbl; p.br = c->tb.gbr;
    }
    return PHYLO_OK;
}

template <int family, typename KEY>
static int tb_seg_sums(tb_run& p, double* out, long long n_seg, const KEY* tkey) {
    p.a.out = out; p.a.n_seg = n_seg;
    hipLaunchKernelGGL((pb_seg_sums<family, KEY>), dim3((unsigned)((n_seg + PT_NT / 64 - 1) / (PT_NT / 64))), dim3(PT_NT), 0, p.c->stream, p.a,
                       tkey);
    CHK(launch_check(p.c, "pb_seg_sums"));
    ++p.launches;
    return PHYLO_OK;
}

// 4. - 6. the branch above every entry and leaf; the clade rows; the leaf rows
static int tb_clade_and_leaf_rows(tb_run& p) {
    phylo_ctx* c = p.c;
    const pb_plan& m = p.plan;
    const pt_bufs& b = c->ts;
    pb_bufs& t = c->tb;
    p.err = (unsigned int*)b.err + 3;                      // 4. walk
    CHK(pt_time_begin(c, c->ev_tb0, c->ev_tb1));
    HIPCHK(c, hipMemsetAsync(p.err, 0, 4, c->stream));
    PT_LAUNCH(pb_walk, m.K, p.child, (const int32_t*)b.slot, p.bl, p.br, m.N, m.K, t.ebr, t.lbr, p.err);
    // 5. clade rows: the entries sorted by their clade's output row (one narrow stable pass over ascending entries), then the sums
    PT_LAUNCH(pt_invert, m.E, b.cord, m.E, t.cpos);
    pt_pairs<uint32_t> q{t.kA, t.kB, t.vA, t.vB};
    PT_LAUNCH(pb_entry_keys<uint32_t>, m.E, (const uint32_t*)b.cid, (const uint32_t*)t.cpos, (const int32_t*)nullptr, m.E, m.K, m.L, 0, q.k, q.v);
    CHK(pt_sort(c, t.temp, m.temp_bytes, q, m.E, m.cbits, p.launches));
    t.cperm = q.v;
    PT_LAUNCH(pb_clade_starts, m.E, (const uint32_t*)q.k, m.E, (uint32_t)m.nc, t.cstart);
    pb_seg_args& a = p.a;
    a.u = b.u; a.ebr = t.ebr; a.lbr = t.lbr; a.cperm = t.cperm; a.cstart = t.cstart; a.toff = t.toff; a.tn = b.o_tn; a.o_tc = t.o_tc;
    a.N = m.N; a.K = m.K; a.Kg = m.Kg; a.cmask_bits = (int)m.cbits;
    CHK(tb_seg_sums<PB_CLADES>(p, t.o_cs, m.nc, (const uint32_t*)nullptr));
    // 6. leaf rows
    return tb_seg_sums<PB_LEAVES>(p, t.o_ls, (long long)m.G * m.N, (const uint32_t*)nullptr);
}

// the entries, particle-major, sorted by (topology row, clade row) keys of one width; tperm = the sorted entries
template <typename KEY>
static int tb_topo_sums(tb_run& p, pt_pairs<KEY> q) {
    const pb_plan& m = p.plan;
    pb_bufs& t = p.c->tb;
    PT_LAUNCH(pb_entry_keys<KEY>, m.E, (const uint32_t*)p.c->ts.cid, (const uint32_t*)t.cpos, (const int32_t*)p.c->ts.o_ptopo, m.E, m.K, m.L,
              (int)m.cbits, q.k, q.v);
    CHK(pt_sort(p.c, t.temp, m.temp_bytes, q, m.E, m.cbits + m.tbits, p.launches));
    t.tperm = p.a.tperm = q.v;
    return tb_seg_sums<PB_TOPOS>(p, t.o_ts, m.nt * m.nb, (const KEY*)q.k);
}

// 7. topology rows: row t's runs start at (N - 2) toff[t]
static int tb_topo_rows(tb_run& p) {
    const pb_plan& m = p.plan;
    pb_bufs& t = p.c->tb;
    size_t bytes = m.temp_bytes;
    HIPCHK(p.c, rocprim::exclusive_scan(t.temp, bytes, (const int32_t*)p.c->ts.o_tn, t.toff, 0u, (size_t)m.nt, rocprim::plus<uint32_t>(),
                                        p.c->stream));
    ++p.launches;
    // Buffers that are free by now take the sorted entries (tperm; cperm in vB stays): cpos in the narrow form, whose last reader is
    // the key kernel ahead of the sort; kA in the wide form, whose keys are in wA / wB.
    uint32_t* const tperm_narrow = t.cpos;
    uint32_t* const tperm_wide = t.kA;
    if (m.wide) return tb_topo_sums(p, pt_pairs<unsigned long long>{t.wA, t.wB, t.vA, tperm_wide});
    return tb_topo_sums(p, pt_pairs<uint32_t>{t.kA, t.kB, t.vA, tperm_narrow});
}

// 8. finish: the error word
static int tb_finish(tb_run& p, phylo_stats* perf) {
    phylo_ctx* c = p.c;
    HIPCHK(c, hipEventRecord(c->ev_tb1, c->stream));
    unsigned int herr = 0;
    HIPCHK(c, hipMemcpyAsync(&herr, p.err, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (herr & PT_ERR_TREE) return fail(c, PHYLO_EHIP, "phylo_tree_branches: the sweep's children records do not form one tree per particle");
    CHK(pt_perf(c, c->ev_tb0, c->ev_tb1, p.launches, perf));
    c->tb_done = true;
    c->tb_wide = p.plan.wide ? 1 : 0; c->tb_cbits = (int)p.plan.cbits; c->tb_tbits = (int)p.plan.tbits;
    return PHYLO_OK;
}

static int tree_branches_impl(phylo_ctx* c, phylo_stats* perf) {
    tb_run p{c};
    CHK(tb_check(p));
    CHK(tb_carve_and_gather(p));
    CHK(tb_clade_and_leaf_rows(p));
    CHK(tb_topo_rows(p));
    return tb_finish(p, perf);
}
#undef PT_CARVE
#undef PT_SLAB_CARVE
#undef PT_LAUNCH
}  // extern "C++"

int phylo_tree_summary(phylo_ctx* c, int64_t* n_clades, int32_t* n_topologies, int32_t* n_groups, phylo_stats* perf) {
    return tree_summary_impl(c, n_clades, n_topologies, n_groups, perf);
}

int phylo_tree_summary_fetch(phylo_ctx* c, uint64_t* clade_bits, uint64_t* clade_weight, int32_t* clade_group, uint64_t* topo_weight,
                             int32_t* topo_count, int32_t* topo_rep, int32_t* topo_group, int32_t* particle_topo, uint64_t* u, uint64_t* U) {
    CHK(bind(c));
    if (!c->ts_done) return fail(c, PHYLO_ESTATE, "phylo_tree_summary_fetch: no phylo_tree_summary has been run");
    const pt_bufs& b = c->ts;
    const size_t nc = (size_t)c->ts_nc, nt = (size_t)c->ts_nt, K = c->K, W = ((size_t)c->N + 63) / 64;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (clade_bits && nc) HIPCHK(c, hipMemcpy(clade_bits, b.o_cbits, nc * W * 8, hipMemcpyDeviceToHost));
    if (clade_weight && nc) HIPCHK(c, hipMemcpy(clade_weight, b.o_cw, nc * 8, hipMemcpyDeviceToHost));
    if (clade_group && nc) HIPCHK(c, hipMemcpy(clade_group, b.o_cg, nc * 4, hipMemcpyDeviceToHost));
    if (topo_weight) HIPCHK(c, hipMemcpy(topo_weight, b.o_tw, nt * 8, hipMemcpyDeviceToHost));
    if (topo_count) HIPCHK(c, hipMemcpy(topo_count, b.o_tn, nt * 4, hipMemcpyDeviceToHost));
    if (topo_rep) HIPCHK(c, hipMemcpy(topo_rep, b.o_trep, nt * 4, hipMemcpyDeviceToHost));
    if (topo_group) HIPCHK(c, hipMemcpy(topo_group, b.o_tg, nt * 4, hipMemcpyDeviceToHost));
    if (u) HIPCHK(c, hipMemcpy(u, b.u, K * 8, hipMemcpyDeviceToHost));
    if (U) HIPCHK(c, hipMemcpy(U, b.U, (size_t)c->ts_G * 8, hipMemcpyDeviceToHost));
    if (particle_topo) {                                   // rows counted from the first row of the particle's group
        std::vector<int32_t> tg(nt);
        HIPCHK(c, hipMemcpy(tg.data(), b.o_tg, nt * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(particle_topo, b.o_ptopo, K * 4, hipMemcpyDeviceToHost));
        std::vector<int32_t> start((size_t)c->ts_G, 0);
        for (size_t j = nt; j-- > 0;) start[(size_t)tg[j]] = (int32_t)j;   // (rows are group-major; every group has a row)
        const size_t Kg = K / (size_t)c->ts_G;
        for (size_t k = 0; k < K; ++k) particle_topo[k] -= start[k / Kg];
    }
    return PHYLO_OK;
}

int phylo_tree_branches(phylo_ctx* c, phylo_stats* perf) { return tree_branches_impl(c, perf); }

int phylo_tree_branches_fetch(phylo_ctx* c, double* clade_stats, double* leaf_stats, int32_t* topo_clades, double* topo_stats) {
    CHK(bind(c));
    if (!c->ts_done || !c->tb_done) return fail(c, PHYLO_ESTATE, "phylo_tree_branches_fetch: no phylo_tree_branches of the last summary");
    const pb_bufs& t = c->tb;
    const size_t nc = (size_t)c->ts_nc, nt = (size_t)c->ts_nt, N = c->N, L = N - 2, G = c->ts_G;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (clade_stats) HIPCHK(c, hipMemcpy(clade_stats, t.o_cs, nc * 32, hipMemcpyDeviceToHost));
    if (leaf_stats) HIPCHK(c, hipMemcpy(leaf_stats, t.o_ls, G * N * 32, hipMemcpyDeviceToHost));
    if (topo_stats) HIPCHK(c, hipMemcpy(topo_stats, t.o_ts, nt * (2 * N - 2) * 32, hipMemcpyDeviceToHost));
    if (topo_clades) {                                     // rows counted from the first clade row of the topology's group
        std::vector<int32_t> cg(nc), tg(nt);
        HIPCHK(c, hipMemcpy(cg.data(), c->ts.o_cg, nc * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(tg.data(), c->ts.o_tg, nt * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(topo_clades, t.o_tc, nt * L * 4, hipMemcpyDeviceToHost));
        std::vector<int32_t> start(G, 0);
        for (size_t j = nc; j-- > 0;) start[(size_t)cg[j]] = (int32_t)j;
        for (size_t j = 0; j < nt; ++j)
            for (size_t i = 0; i < L; ++i) topo_clades[j * L + i] -= start[(size_t)tg[j]];
    }
    return PHYLO_OK;
}

int phylo_math_probe(phylo_ctx* c, int op, const double* x, const double* y, int n, double* out) {
    CHK(bind(c));
    if (n < 0 || (n > 0 && (!x || !y || !out))) return fail(c, PHYLO_EINVAL, "bad arguments");
    if (n == 0) return PHYLO_OK;
    void *dx, *dy, *dout;
    CHK(scratch_get(c, 0, (size_t)n * 8, &dx));
    CHK(scratch_get(c, 1, (size_t)n * 8, &dy));
    CHK(scratch_get(c, 2, (size_t)n * 8, &dout));
    HIPCHK(c, hipMemcpyAsync(dx, x, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dy, y, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    if (op == 5) {                                         // the reverse pass's reciprocal (phylo_grad.h)
        hipLaunchKernelGGL(pg_probe_rcp, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, (const double*)dx, n, (double*)dout);
        CHK(launch_check(c, "pg_probe_rcp"));
    } else {
        hipLaunchKernelGGL(pk_math_probe, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, op, (const double*)dx, (const double*)dy, n,
                           (double*)dout);
        CHK(launch_check(c, "pk_math_probe"));
    }
    HIPCHK(c, hipMemcpyAsync(out, dout, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

int phylo_debug_frechet(phylo_ctx* c, int form, const double* A, const double* E, int n, double* L) {
    CHK(bind(c));
    if ((form != 0 && form != 1) || n < 0 || n > (1 << 24) || (n > 0 && (!A || !E || !L)))
        return fail(c, PHYLO_EINVAL, "phylo_debug_frechet: form 0 or 1, 0 <= n <= 2^24, A, E and L given");
    if (n == 0) return PHYLO_OK;
    const size_t bytes = (size_t)n * 16 * 8;
    void *dA, *dE, *dL;
    CHK(scratch_get(c, 0, bytes, &dA));
    CHK(scratch_get(c, 1, bytes, &dE));
    CHK(scratch_get(c, 2, bytes, &dL));
    HIPCHK(c, hipMemcpyAsync(dA, A, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dE, E, bytes, hipMemcpyHostToDevice, c->stream));
    if (form == 0) {
        hipLaunchKernelGGL(pg_probe_frechet, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, (const double*)dA, (const double*)dE, n, (double*)dL);
        CHK(launch_check(c, "pg_probe_frechet"));
    } else {                                               // whole workgroups: the quads past matrix n - 1 are padded by the kernel
        hipLaunchKernelGGL(pg_probe_frechet_row, dim3(cdiv((long)n * 4, 256)), dim3(256), 0, c->stream, (const double*)dA, (const double*)dE, n,
                           (double*)dL);
        CHK(launch_check(c, "pg_probe_frechet_row"));
    }
    HIPCHK(c, hipMemcpyAsync(L, dL, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

int phylo_debug_site_product(phylo_ctx* c, const double* p, const double* x1, const double* x2, int n, double* out_p, int32_t* out_E,
                             double* out_extra) {
    if (n < 0 || n > (1 << 22) || (n > 0 && (!p || !x1 || !x2 || !out_p || !out_E || !out_extra)))
        return fail(c, PHYLO_EINVAL, "phylo_debug_site_product: 0 <= n <= 2^22, inputs of n and outputs of 2 n values given");
    if (!c) {                                              // the host body: no device is touched
        for (int i = 0; i < n; ++i) pk_site_product_one(p[i], x1[i], x2[i], i, n, out_p, out_E, out_extra);
        return PHYLO_OK;
    }
    CHK(bind(c));
    if (n == 0) return PHYLO_OK;
    const size_t in = (size_t)n * 8;
    void *din, *dpx, *dE;
    CHK(scratch_get(c, 0, 3 * in, &din));
    CHK(scratch_get(c, 1, 4 * in, &dpx));                  // p' (2 n) | extra' (2 n)
    CHK(scratch_get(c, 2, (size_t)n * 2 * 4, &dE));
    double* d = static_cast<double*>(din);
    double* o = static_cast<double*>(dpx);
    HIPCHK(c, hipMemcpyAsync(d, p, in, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + n, x1, in, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d + 2 * (size_t)n, x2, in, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(pk_site_product_probe, dim3(cdiv(n, 256)), dim3(256), 0, c->stream, (const double*)d, (const double*)(d + n),
                       (const double*)(d + 2 * (size_t)n), n, o, (int32_t*)dE, o + 2 * (size_t)n);
    CHK(launch_check(c, "pk_site_product_probe"));
    HIPCHK(c, hipMemcpyAsync(out_p, o, 2 * in, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_extra, o + 2 * (size_t)n, 2 * in, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out_E, dE, (size_t)n * 2 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

// ---- multi-GPU --------------------------------------------------------------------------------
int phylo_comm_unique_id(char id[PHYLO_COMM_ID_BYTES]) {
    std::string err;
    int rc = phylo_comm_make_id(id, &err);
    if (rc != PHYLO_OK) g_last_error = err;
    return rc;
}

int phylo_comm_init(phylo_ctx* c, int rank, int world, const char id[PHYLO_COMM_ID_BYTES]) {
    CHK(bind(c));
    if (world < 1 || rank < 0 || rank >= world || !id) return fail(c, PHYLO_EINVAL, "bad rank/world");
    if (c->K % world != 0) return fail(c, PHYLO_EINVAL, "K = %d is not divisible by world = %d", c->K, world);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_sweep_state(c);                                   // peers may still map the old pool: drop it first
    int rc = phylo_comm_setup(&c->comm, rank, world, id, &c->err);
    if (rc != PHYLO_OK) { g_last_error = c->err; return rc; }
    c->rank = rank;
    c->world = world;
    c->Kloc = c->K / world;
    c->k0 = rank * c->Kloc;
    c->swept = false; ++c->sweep_serial;
    c->state_ready = false;
    CHK(alloc_sweep_state(c));                             // collective: every rank maps every peer's pool here
    CHK(refresh_leaf_ll(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

int phylo_comm_share(phylo_ctx* c, phylo_ctx* owner) {
    CHK(bind(c));
    if (!owner || owner == c) return fail(c, PHYLO_EINVAL, "phylo_comm_share needs another context as the owner");
    if (owner->comm.parent) return fail(c, PHYLO_EINVAL, "the owner must hold its own communicator (phylo_comm_init)");
    if (owner->device != c->device) return fail(c, PHYLO_EINVAL, "both contexts must live on the same device");
    if (c->K % owner->world != 0) return fail(c, PHYLO_EINVAL, "K = %d is not divisible by world = %d", c->K, owner->world);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_sweep_state(c);
    phylo_comm_destroy(&c->comm);
    if (owner->comm.transport == 1 && !owner->comm.cstream)
        HIPCHK(c, hipStreamCreateWithFlags(&owner->comm.cstream, hipStreamNonBlocking));
    c->comm.parent = &owner->comm;
    c->comm.rank = owner->comm.rank;
    c->comm.world = owner->comm.world;
    c->comm.transport = owner->comm.transport;
    c->rank = owner->rank;
    c->world = owner->world;
    c->Kloc = c->K / c->world;
    c->k0 = c->rank * c->Kloc;
    c->swept = false; ++c->sweep_serial;
    c->state_ready = false;
    CHK(alloc_sweep_state(c));                             // collective: every rank maps every peer's pool here
    CHK(refresh_leaf_ll(c));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PHYLO_OK;
}

int phylo_debug_remote_cache(phylo_ctx* c, int* used, int* cap) {
    CHK(bind(c));
    if (!used || !cap) return fail(c, PHYLO_EINVAL, "phylo_debug_remote_cache: NULL argument");
    *used = 0;
    *cap = c->cache_cap;
    if (c->d_mirror) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        int32_t n = 0;
        HIPCHK(c, hipMemcpy(&n, c->d_mirror + (size_t)(c->N - 1) * c->K, 4, hipMemcpyDeviceToHost));
        *used = n;
    }
    return PHYLO_OK;
}

int phylo_comm_exchange_kind(const phylo_ctx* c) {
    if (!c || c->comm.transport == 0) return 0;
    return c->p2p ? 3 : c->comm.transport;
}

int phylo_comm_max(phylo_ctx* c, double* value) {
    CHK(bind(c));
    if (!value) return fail(c, PHYLO_EINVAL, "value is NULL");
    return phylo_comm_allreduce_max(c->comm, value, c->stream, &c->err);
}

int phylo_comm_allgather(phylo_ctx* c, const void* mine, size_t bytes, void* all) {
    CHK(bind(c));
    if (!mine || !all || bytes == 0) return fail(c, PHYLO_EINVAL, "bad arguments to phylo_comm_allgather");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return phylo_comm_allgather_host(c->comm, mine, bytes, all, c->stream, &c->err);
}

int phylo_comm_barrier(phylo_ctx* c) {
    double v = 0.0;
    return phylo_comm_max(c, &v);
}

}  // extern "C"
