// phylo_revlists.h -- the integer lists of the reverse pass (phylo_sweep_backward), built on the HOST from the ancestors and the
// children that the sweep left: who adopted whom (per rank event, counting sort by ancestor) and which nodes have which parents
// (entries node * 2 + side grouped by child), plus what follows from them per node: heavy nodes cut into chunks, the nodes that go
// through pg_nodes_rows (flags, lists by rank event), the adopted particles of every rank event; the twisted proposal's look-ahead
// lists (pg_build_lookahead); and the form of the pass (pg_plan_form, pg_plan_chains).  Plain C++, no HIP: the same functions run
// under phylo_debug_reverse_lists, phylo_debug_lookahead_lists and phylo_debug_reverse_plan for the CPU tests
// (tests/test_revlists_cpu.py, tests/test_revplan_cpu.py check them against restatements in Python).  The layout of the slab is
// the one the device reads (pg_args in phylo_grad.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#define PG_PCHUNK 8                    // parents staged in LDS at a time; more parents than this = a heavy node
#define PG_HCHUNK 32                   // parents per chunk of a heavy node
// par_idx entry: (parent node * 2 + side) | PG_FREE_PARENT when the parent's adjoint row is the own term alone and is not stored
// (rows form: pg_nodes_free); the gather then recomputes it from alpha_parent
#define PG_FREE_PARENT (1 << 30)

struct pg_lists {
    int32_t *ad_off, *ad_idx;          // [R][K+1], [R][K]
    int32_t *par_off, *par_idx;        // [R K + 1], [2 R K]
    int32_t *heavy, *chunk_beg, *chunk_cnt;   // [R K], [cap], [cap]
    int32_t *slow_flag, *slow_idx;     // [R K] x 2
    int32_t* adp;                      // [R K]
    size_t cap;
};
inline size_t pg_lists_cap(size_t R, size_t K) { return 2 * R * K / 4 + 1; }
inline size_t pg_lists_ints(size_t R, size_t K) {
    return R * (K + 1) + R * K + (R * K + 1) + 2 * R * K + R * K + 2 * pg_lists_cap(R, K) + 3 * R * K;
}
inline pg_lists pg_lists_carve(int32_t* base, size_t R, size_t K) {
    const size_t nn = R * K;
    pg_lists L;
    L.cap = pg_lists_cap(R, K);
    L.ad_off = base;
    L.ad_idx = L.ad_off + R * (K + 1);
    L.par_off = L.ad_idx + nn;
    L.par_idx = L.par_off + nn + 1;
    L.heavy = L.par_idx + 2 * nn;
    L.chunk_beg = L.heavy + nn;
    L.chunk_cnt = L.chunk_beg + L.cap;
    L.slow_flag = L.chunk_cnt + L.cap;
    L.slow_idx = L.slow_flag + nn;
    L.adp = L.slow_idx + nn;
    return L;
}

// What the host needs of the lists, whoever built them (the builders below, or pg_dl_lists through its pinned meta block): the
// per-rank-event offsets and the totals.  Device-built lists number a heavy node's chunks globally: rank_chunk0 is all zeros and
// max_chunks 0 there.
struct pg_list_counts {
    std::vector<int32_t> ev_adp0;      // adopted particles of rank event r: adp[ev_adp0[r] .. ev_adp0[r + 1])
    std::vector<int32_t> ev_slow0;     // flagged nodes of rank event r: slow_idx[ev_slow0[r] .. ev_slow0[r + 1])
    std::vector<int32_t> rank_chunk0;  // first chunk of rank event r
    int32_t n_adp = 0, n_slow = 0, n_par = 0;   // adopted particles, flagged nodes, parent entries
    size_t n_chunks = 0, max_chunks = 0;        // chunks in all, most chunks of one rank event
};

// Clears what the builders count into (ad_off, ad_idx, par_off, slow_flag).  Between this and pg_build_parents the caller may set
// bit 1 of slow_flag[x] (twisted proposal: node x has look-ahead entries).
inline void pg_lists_clear(const pg_lists& L, int R, int K) {
    const size_t nn = (size_t)R * K;
    memset(L.ad_off, 0, ((size_t)R * (K + 1) + nn + nn + 1) * 4);      // ad_off, ad_idx, par_off
    memset(L.slow_flag, 0, nn * 4);
}

// Adopters of every particle at every rank event (anc[r-1][k'] = the particle k' adopted at rank event r, a GLOBAL index: the
// caller adds g K / G to the group-local ancestors of a batched sweep (pg_global_ancestors); ascending k' within a list), and the adopted particles (r * K + k), grouped by rank event: adp[ev_adp0[r] .. ev_adp0[r+1]); fills ev_adp0 and n_adp.
// A few ancestors take nearly all the draws, so counters and cursors are chains of store-to-load forwards on one address: the
// particles are taken as four contiguous quarters with a counter row each (four independent chains), whose prefix sums give
// every quarter its own cursor into an ancestor's list.
inline void pg_build_adopters(int R, int K, const int64_t* anc, const pg_lists& L, std::vector<int32_t>& cur, pg_list_counts& o) {
    std::vector<int32_t>& ev_adp0 = o.ev_adp0;
    ev_adp0.assign((size_t)R + 1, 0);
    int32_t n_adp = 0;
    const int Kq = K / 4;
    cur.assign((size_t)4 * K, 0);
    for (int r = 1; r < R; ++r) {
        int32_t* off = L.ad_off + (size_t)r * (K + 1);
        const int64_t* a = anc + (size_t)(r - 1) * K;
        int32_t* idx = L.ad_idx + (size_t)r * K;
        int32_t *c0 = cur.data(), *c1 = c0 + K, *c2 = c1 + K, *c3 = c2 + K;
        if (r > 1) memset(c0, 0, (size_t)4 * K * 4);
        for (int k = 0; k < Kq; ++k) {
            ++c0[a[k]]; ++c1[a[k + Kq]]; ++c2[a[k + 2 * Kq]]; ++c3[a[k + 3 * Kq]];
        }
        for (int k = 4 * Kq; k < K; ++k) ++c3[a[k]];       // (the last quarter takes the remainder)
        ev_adp0[r - 1] = n_adp;
        int32_t run = 0;
        for (int x = 0; x < K; ++x) {
            const int32_t t0 = c0[x], t1 = c1[x], t2 = c2[x], t3 = c3[x];
            off[x] = run;
            c0[x] = run; c1[x] = run + t0; c2[x] = run + t0 + t1; c3[x] = run + t0 + t1 + t2;
            const int32_t tot = (t0 + t1) + (t2 + t3);
            if (tot) L.adp[n_adp++] = (r - 1) * K + x;      // somebody adopts (r - 1, x) at rank event r
            run += tot;
        }
        off[K] = run;
        for (int k = 0; k < Kq; ++k) {
            idx[c0[a[k]]++] = k; idx[c1[a[k + Kq]]++] = k + Kq; idx[c2[a[k + 2 * Kq]]++] = k + 2 * Kq; idx[c3[a[k + 3 * Kq]]++] = k + 3 * Kq;
        }
        for (int k = 4 * Kq; k < K; ++k) idx[c3[a[k]]++] = k;
    }
    if (R >= 1) ev_adp0[R - 1] = n_adp;
    ev_adp0[R] = n_adp;
    if (R == 1) ev_adp0[0] = 0;
    o.n_adp = n_adp;
}

// The ancestors of a batched sweep are indices inside the adopter's group of Kg particles: as indices of the one K-particle genealogy.
inline void pg_global_ancestors(int R, int K, int Kg, const int64_t* anc, std::vector<int64_t>& out) {
    out.resize(R > 1 ? (size_t)(R - 1) * K : 0);
    for (int r = 0; r + 1 < R; ++r)
        for (int g = 0, k = 0; k < K; ++g)
            for (const int end = k + Kg; k < end; ++k) out[(size_t)r * K + k] = anc[(size_t)r * K + k] + (int64_t)g * Kg;
}

// Bit 2 of slow_flag for every node somebody adopted (r - 1, anc[r-1][k]): what pg_build_parents needs of the adopters when the early
// pg_nodes_free has skipped the adopted nodes -- one pass over the ancestors, so the parents' lists can be built (and the launch that
// needs them started) before the adopters' counting sorts.
inline void pg_mark_adopted(int R, int K, const int64_t* anc, const pg_lists& L) {
    for (int r = 1; r < R; ++r) {
        const int64_t* a = anc + (size_t)(r - 1) * K;
        int32_t* f = L.slow_flag + (size_t)(r - 1) * K;
        for (int k = 0; k < K; ++k) f[a[k]] |= 4;
    }
}

// (Tried on the builders, measured on a GPU box, not kept: four counter rows per child as in pg_build_adopters -- faster on synthetic
//  genealogies with many internal children, 0.18 -> 0.26 ms on primate.p's, whose later rank events still merge mostly leaves, because
//  of the four times larger cursor array; worker threads -- rank events in groups, quarters of the child entries on four cores --
//  0.6 -> 1.7 ms for DS1 at K = 4096 on the 16-core share of a box.)
// Parents: entries e = node * 2 + side grouped by child (ascending e).  One pass over the nodes turns the counts into offsets and
// decides everything per node: heavy nodes (more than PG_PCHUNK parents) get their list cut into chunks of PG_HCHUNK, numbered
// within the rank event (rank_chunk0); nodes with parents (bit 0), look-ahead entries (bit 1, set by the caller) or -- after the
// early pg_nodes_free -- adopters (bit 2) are flagged ((index in slow_idx) << 3 | bits) and listed by rank event (ev_slow0) for
// pg_nodes_rows; all the others: pg_nodes_free.  A parent that goes through pg_nodes_free never stores its adjoint row: its
// entries carry PG_FREE_PARENT (rows form only).  After the early pg_nodes_free the caller runs pg_mark_adopted first.
// Fills rank_chunk0, ev_slow0, n_chunks, max_chunks, n_slow and n_par.
inline void pg_build_parents(int N, int R, int K, const int32_t* child, bool rows_form, bool tail_flagged, const pg_lists& L,
                             std::vector<int32_t>& cur, pg_list_counts& o) {
    std::vector<int32_t>&rank_chunk0 = o.rank_chunk0, &ev_slow0 = o.ev_slow0;
    const size_t nn = (size_t)R * K;
    // (leaf or internal child is a coin toss in the later rank events: no branch on it -- a leaf counts into one of 64 dummies in
    //  turn: increments of one address are a chain of store-to-load forwards, 5 cycles each)
    int32_t dummy[64] = {0};
    const size_t e0 = 2 * (size_t)K;                        // (the children of rank event 0 are leaves: nothing to count)
    for (size_t e = e0; e < 2 * nn; ++e) {
        const int32_t ch = child[e];
        int32_t* p = ch >= N ? L.par_off + (size_t)(ch - N) + 1 : dummy + (e & 63);
        ++*p;
    }
    rank_chunk0.assign((size_t)R + 1, 0);
    ev_slow0.assign((size_t)R + 1, 0);
    size_t max_chunks = 0, n_chunks = 0;
    int32_t ns = 0, run = 0;
    for (int r = 0; r < R; ++r) {
        rank_chunk0[r] = (int32_t)n_chunks;
        ev_slow0[r] = ns;
        for (int k = 0; k < K; ++k) {
            const size_t x = (size_t)r * K + k;
            const int32_t np = L.par_off[x + 1];         // still the count: the offsets are written behind the read position
            L.par_off[x] = run;
            int32_t f = L.slow_flag[x];                  // (set by the caller: bit 1 look-ahead entries, bit 2 adopted -- pg_mark_adopted:
            if (np) f |= 1;                              //  the early launch skipped those; without parents they join the flagged ones)
            L.heavy[x] = -1;
            if (np > PG_PCHUNK) {
                L.heavy[x] = (int32_t)(n_chunks - rank_chunk0[r]);
                for (int32_t b = run; b < run + np; b += PG_HCHUNK) {
                    L.chunk_beg[n_chunks] = b;
                    L.chunk_cnt[n_chunks] = run + np - b < PG_HCHUNK ? run + np - b : PG_HCHUNK;
                    ++n_chunks;
                }
            }
            if (f) {
                f |= ns << 3;
                L.slow_idx[ns++] = (int32_t)x;
            }
            L.slow_flag[x] = f;
            run += np;
        }
        if (n_chunks - rank_chunk0[r] > max_chunks) max_chunks = n_chunks - rank_chunk0[r];
    }
    L.par_off[nn] = run;
    rank_chunk0[R] = (int32_t)n_chunks;
    ev_slow0[R] = ns;
    // scatter without a branch on leaf / internal (masks, not ?: -- the compiler made a branch of that, mispredicted every other
    // time in the later rank events): a leaf child advances one of 64 dummy cursors and writes into the tail of par_idx,
    // which is never used (the 2 K children of rank event 0 are all leaves).
    // tail_flagged (the plain reverse pass after the early pg_nodes_free): the entries of FREE parents (no flag: their adjoint is
    // recomputed from omega, nothing of the chain is needed) fill a child's
    // list from the front, ascending; the few entries of flagged parents from the back, so the list ends with them in descending
    // order -- pg_parent_chunks_all sums the free ones of every rank event in one launch, pg_nodes_rows walks the tail.
    cur.resize((tail_flagged ? 2 : 1) * (nn + 64));
    int32_t* front = cur.data();
    memcpy(front, L.par_off, nn * 4);
    memset(front + nn, 0, 64 * 4);                          // the 64 dummy cursors start from 0 at every call (their values are masked
    if (tail_flagged) {                                     //  out of the result; left alone they would count up from call to call)
        int32_t* back = front + nn + 64;                    // (the cursors from the back: the row behind the front cursors)
        for (size_t x = 0; x < nn; ++x) back[x] = L.par_off[x + 1] - 1;
        memset(back + nn, 0, 64 * 4);
    }
    const int32_t free_bit = rows_form ? PG_FREE_PARENT : 0;
    const int32_t tail = (int32_t)(2 * nn) - 1;
    int32_t tmask = 1;                                      // dummy slots: the last min(64, 2 K rounded down to a power of two)
    while (tmask * 2 <= 2 * K && tmask < 64) tmask *= 2;
    tmask -= 1;
    const ptrdiff_t rowlen = (ptrdiff_t)(nn + 64);
    for (size_t e = e0; e < 2 * nn; ++e) {                 // e = node * 2 + side, ascending
        const int32_t ch = child[e];
        const int32_t in = -(int32_t)(ch >= N);              // all ones: internal child
        const int32_t lane = (int32_t)(e & 63);
        const int32_t ci = ((ch - N) & in) | (((int32_t)nn + lane) & ~in);
        const int32_t fl = L.slow_flag[e >> 1] != 0;         // the parent is a flagged node
        const int32_t tob = fl & (tail_flagged ? 1 : 0);     // 1: from the back
        int32_t* cp = front + (ptrdiff_t)tob * rowlen + ci;
        const int32_t pos = *cp;
        *cp = pos + 1 - 2 * tob;
        const int32_t di = (pos & in) | ((tail - (lane & tmask)) & ~in);
        L.par_idx[di] = (int32_t)e | (fl ? 0 : free_bit);
    }
    o.n_chunks = n_chunks; o.max_chunks = max_chunks; o.n_slow = ns; o.n_par = run;
}

// pg_build_parents with tail_flagged fills a list's flagged entries from the back, which leaves them descending; the device builders
// (phylo_revlists_dev.h) leave them ascending, and pg_nodes_rows adds them in list order.  The reverse pass turns the host-built
// tails round, so that a gradient has the same bits whoever built its lists.  Only flagged nodes have parents: n_slow short walks.
// Both this and the marks of an eager sweep (rev_marks in phylo_hip.hip) apply above PG_KEPT_BITS_TAXA taxa only.  Up to there
// gradients existed before either, the forms with host-built lists or without marks agreed with the default to the last few bits
// (the tests hold them to 1e-12), and each keeps the bits it had; above, no reverse pass worked, and all forms give the same bits.
#define PG_KEPT_BITS_TAXA 65
inline void pg_flagged_tails_ascending(const pg_lists& L, int32_t n_slow) {
    for (int32_t i = 0; i < n_slow; ++i) {
        const size_t x = (size_t)L.slow_idx[i];
        int32_t *b = L.par_idx + L.par_off[x], *e = L.par_idx + L.par_off[x + 1];
        int32_t* t = e;
        while (t > b && !(t[-1] & PG_FREE_PARENT)) --t;
        for (int32_t* u = e - 1; t < u; ++t, --u) { const int32_t v = *t; *t = *u; *u = v; }
    }
}

// ---- twisted proposal: the look-ahead lists --------------------------------------------------------------------------------------
// The look-ahead merges of rank event r touch every internal node among the adopted roots (rad[r][k][slot], slots 0 .. N - r - 1;
// rank event 0 adopts leaves only).  Entries (adopter * N + slot) grouped by node (counting sort: ascending adopter, then slot),
// cut into chunks; per rank event the touched nodes with their chunks.  `image` receives what the device reads, for all rank
// events in one upload: xent | xchunk_node | xchunk_beg | xchunk_cnt | xchunk_part | xnode_id | xnode_chunk0 | xnode_nchunks (+ one
// spare int); the counts below are the offsets into it.  Sets bit 1 of slow_flag[x] for every touched node (before
// pg_build_parents: such a node goes through pg_nodes_rows).  xch_max: PG_XCH of phylo_grad.h.
struct pg_lookahead {
    std::vector<int32_t> ev_chunk0, ev_node0;   // [R + 1]: first chunk / first touched node of rank event r
    size_t n_xent = 0, n_xchunks = 0, n_xnodes = 0;
    size_t max_chunks = 0;                      // most chunks of one rank event
};
inline void pg_build_lookahead(int N, int K, int S, int xch_max, const int32_t* rad, int32_t* slow_flag, std::vector<int32_t>& image,
                               pg_lookahead& o) {
    const int R = N - 1;
    o.ev_chunk0.assign((size_t)R + 1, 0);
    o.ev_node0.assign((size_t)R + 1, 0);
    o.max_chunks = 0;
    std::vector<int32_t> xent, xc_node, xc_beg, xc_cnt, xc_part, xn_id, xn_c0, xn_nc;
    std::vector<int32_t> cnt, first;
    const long ts = (S + 255) / 256;
    for (int r = 0; r < R; ++r) {
        o.ev_chunk0[r] = (int32_t)xc_node.size();
        o.ev_node0[r] = (int32_t)xn_id.size();
        if (r == 0) continue;                                   // rank event 0 adopts leaves only
        const int n = N - r;
        const size_t nn_r = (size_t)r * K;                      // nodes that exist before rank event r
        cnt.assign(nn_r + 1, 0);
        const int32_t* tab = rad + (size_t)r * K * N;
        for (int k = 0; k < K; ++k)
            for (int i = 0; i < n; ++i) {
                const int x = tab[(size_t)k * N + i];
                if (x >= N) ++cnt[(size_t)(x - N) + 1];
            }
        for (size_t i = 0; i < nn_r; ++i) cnt[i + 1] += cnt[i];
        const size_t base = xent.size();
        xent.resize(base + (size_t)cnt[nn_r]);
        first.assign(cnt.begin(), cnt.end() - 1);
        for (int k = 0; k < K; ++k)
            for (int i = 0; i < n; ++i) {
                const int x = tab[(size_t)k * N + i];
                if (x >= N) xent[base + (size_t)first[x - N]++] = k * N + i;
            }
        // chunk shape of this rank event: enough workgroups to fill the GPU, not more rows than pg_twist_xsum should add per node.
        // Many entries (large K): up to PG_XCH entries per chunk, all partner slots.  Few entries (the K = 32..64 of the
        // reference's experiments): one entry per chunk and the n - 1 partner slots cut into slices, or a chunk is one thread's
        // walk over (n - 1) M merges per site, a few hundred microseconds with M = 10.
        const long total_ent = cnt[nn_r];
        const long target = 2048 / ts > 64 ? 2048 / ts : 64;
        int xch = (int)((total_ent + target - 1) / target);
        xch = xch < 1 ? 1 : (xch > xch_max ? xch_max : xch);
        int slices = 1;
        if (xch == 1 && total_ent > 0) {
            slices = (int)(target / total_ent);
            slices = slices < 1 ? 1 : (slices > n ? n : slices);
        }
        const int pw = (n + slices - 1) / slices;              // partner slots per slice
        for (size_t x = 0; x < nn_r; ++x) {
            const int m = cnt[x + 1] - cnt[x];
            if (m == 0) continue;
            xn_id.push_back((int32_t)(x + N));
            xn_c0.push_back((int32_t)xc_node.size());
            int nc = 0;
            for (int b = 0; b < m; b += xch)
                for (int p0 = 0; p0 < n; p0 += pw) {
                    xc_node.push_back((int32_t)(x + N));
                    xc_beg.push_back((int32_t)(base + cnt[x] + b));
                    xc_cnt.push_back(m - b < xch ? m - b : xch);
                    xc_part.push_back(p0 | ((p0 + pw < n ? p0 + pw : n) << 16));
                    ++nc;
                }
            xn_nc.push_back(nc);
        }
        const size_t nch = xc_node.size() - (size_t)o.ev_chunk0[r];
        if (nch > o.max_chunks) o.max_chunks = nch;
    }
    o.ev_chunk0[R] = (int32_t)xc_node.size();
    o.ev_node0[R] = (int32_t)xn_id.size();
    o.n_xent = xent.size(); o.n_xchunks = xc_node.size(); o.n_xnodes = xn_id.size();
    // the newest rank event that touches a node is launched first: its pg_twist_xsum starts the node's adjoint row (bit 30)
    // instead of adding to it, so nothing has to be cleared; such a node goes through pg_nodes_rows (flag bit 1)
    for (size_t i = o.n_xnodes; i-- > 0;) {
        int32_t& f = slow_flag[xn_id[i] - N];
        if (!(f & 2)) { f |= 2; xn_nc[i] |= 1 << 30; }
    }
    image.resize(o.n_xent + 4 * o.n_xchunks + 3 * o.n_xnodes + 1);
    int32_t* w = image.data();
    auto put = [&](const std::vector<int32_t>& v) { if (!v.empty()) memcpy(w, v.data(), v.size() * 4); w += v.size(); };
    put(xent); put(xc_node); put(xc_beg); put(xc_cnt); put(xc_part); put(xn_id); put(xn_c0); put(xn_nc);
}

// ---- the form of a reverse pass ---------------------------------------------------------------------------------------------------
// Every form computes the same bits (the tests assert that); which one is issued is decided here and nowhere else, at two points:
// pg_plan_form before anything is launched, pg_plan_chains once the lists' counts are known.  phylo_sweep_backward's driver reads
// the plan; phylo_debug_reverse_plan returns it as pg_plan_mask (tests/test_revplan_cpu.py restates the rules).
struct pg_plan_in {
    int N, K, K_local, S, world;       // the shape (K_local: this rank's particles; world: ranks of the context)
    bool twist, marks;                 // the last sweep: twisted proposal; lazy, left marks of the adopted nodes
    bool rev_host_lists, one_stream, two_streams, rows_chain, coeff_chain;   // the PHYLO_REV_HOST_LISTS / PHYLO_GRAD_* switches
    int dl_max_k;                      // PG_DL_MAX_K of phylo_revlists_dev.h
    int groups;                        // batched sweep: independent systems of K / groups particles in one genealogy (0 or 1: one sweep)
};
struct pg_plan {
    // pg_plan_form
    bool twist, rows_form, whole, early_free, dev_lists, sort_early, bg_free, two, parents_first;
    bool rows_chain, coeff_chain;      // (the two switches pg_plan_chains reads)
    // pg_plan_chains
    bool rows_all, rows_overlap, chunks_first, interleave, coeff_all;
};

inline void pg_plan_chains(pg_plan& p, long n_slow, long TS, long coeff_wgs, int passes_in_flight, int R);

inline pg_plan pg_plan_form(const pg_plan_in& in) {
    pg_plan p{};
    const size_t nn = (size_t)(in.N - 1) * (size_t)in.K;
    p.twist = in.twist;
    p.rows_chain = in.rows_chain; p.coeff_chain = in.coeff_chain;
    p.rows_form = in.S <= 4096;                            // pg_nodes_rows: one workgroup per node, one tile
    // sharded: the sweep made the per-rank records whole on every rank (graph_gather), node rows are read from their owners' pools,
    // and every rank runs the whole pass over that genealogy
    p.whole = in.world > 1;
    // a lazy sweep left marks: a node nobody adopted has no parents and alpha = omega, known without any list -- nearly all
    // nodes, done while the lists are built
    p.early_free = p.rows_form && !in.twist && in.marks;
    // After a lazy sweep with the plain proposal the lists are built by kernels (phylo_revlists_dev.h) and the host waits for a few
    // dozen integers; PHYLO_REV_HOST_LISTS keeps the host builders (the A/B switch, and what every other form uses).
    // (never on a sharded context: the device lists are what gates the one-launch chains, pg_coeff_all / pg_nodes_rows_all, which
    //  hand values between workgroups and assume nobody else on the GPU waits likewise -- sharded ranks sharing a GPU run their
    //  passes at once; a sharded pass takes the host lists and a launch per rank event)
    // (the one limit that is per group: pg_dl_adopters sorts a group's adopters of one rank event in one workgroup; everything else
    //  -- the node kernels, the parents' sort, the limits of the one-launch chains in pg_plan_chains -- sees the total K)
    const int Kg = in.groups > 1 ? in.K / in.groups : in.K;
    p.dev_lists = p.early_free && !p.whole && !in.rev_host_lists && in.K_local == in.K && Kg <= in.dl_max_k;
    // (the list kernels' sort goes to the second stream as soon as the host has seen the sweep end: queued there behind the lists'
    //  event, it neither waits for the host to read the counts nor holds up the coefficient chain on the context's stream)
    p.sort_early = p.dev_lists && !in.one_stream;
    // The early pg_nodes_free is 85 us of throughput work nothing waits for before pg_node_finish, while everything else is a chain
    // of small dependent launches: it runs on a stream of the lowest priority, in the background of the chains.
    // (Measured, K = 2048: reverse pass 0.539 -> 0.511 ms with all 898 sites; with 256 sites the launch is 25 us and the extra
    //  events and the fill launch cost more than they hide, 0.440 -> 0.473 ms: large sweeps only.)
    p.bg_free = p.early_free && !in.one_stream && (in.two_streams || nn * (size_t)in.S >= ((size_t)12 << 20));
    // Two chains of small dependent launches remain, both newest rank event first: the coefficients (on the context's stream) and
    // the adopted nodes' adjoints, which need the coefficients of their own and of later rank events only (ev_coeff[r]), on a
    // second stream.  After the early pg_nodes_free the parents' lists are built FIRST (they need of the adopters only who was
    // adopted: pg_mark_adopted), so that the one launch over all heavy nodes' free parents runs while the host sorts the adopters
    // and beside the coefficient chain; the adopted nodes' chain then follows the coefficients one rank event behind.
    // (Without that reordering and for small sweeps two streams gain nothing -- the host finishes the parents' lists only when the
    //  coefficient chain is over -- and the events cost 13 us: primate.p, K = 2048, 0.542 against 0.555 ms; DS1, K = 4096: 2.48 -> 2.16.)
    // (The reordering, measured, K = 2048: reverse pass 0.522 -> 0.476 ms with all 898 sites, 0.455 -> 0.466 with 256: large sweeps
    //  only, like the background launch -- it is taken exactly when that one is.)
    p.parents_first = p.bg_free || p.dev_lists;
    p.two = !in.one_stream && (in.two_streams || nn >= 65536 || p.parents_first);
    // Until the counts are known the chains are those of a pass without flagged nodes.  That is final wherever the parents' lists
    // come after the coefficient chain (!parents_first): no one-launch chain without dev_lists, and interleave reads no count.
    pg_plan_chains(p, 0, 1, 0, 0, in.N - 1);
    return p;
}

// n_slow: flagged nodes; TS: tiles of 256 sites per row; coeff_wgs: workgroups of all pg_coeff launches together (0: not known,
// host lists); passes_in_flight: reverse passes in flight in this process, this one included; R = N - 1.
inline void pg_plan_chains(pg_plan& p, long n_slow, long TS, long coeff_wgs, int passes_in_flight, int R) {
    // the adopted nodes' chain as ONE launch (pg_nodes_rows_all; the plain proposal with the lists built on the device): the
    // coefficient chain -- then the longest chain of the pass -- is issued first and in one go, the parents' sort and the chunk sums
    // behind it, and the one launch waits for the last coefficients
    p.rows_all = p.early_free && p.dev_lists && p.two && !p.rows_chain && n_slow > 0 && n_slow * TS <= 16384;
    // few enough workgroups to leave the coefficient chain room on every SIMD: the launch runs BESIDE that chain and waits, rank
    // event by rank event, for its completion words; else it is launched behind the chain's last event
    // (a launch that waits inside the GPU for another launch of its own pass assumes the two share the GPU with nobody who waits
    //  likewise: not with another pass of this process in flight)
    p.rows_overlap = p.rows_all && n_slow * TS <= 512 && passes_in_flight <= 1;
    // (the launch behind the coefficient chain: that chain is the longer one and is issued first; the launch beside it: the sort and
    //  the chunk sums first, so that the adopted nodes follow the coefficients rank event by rank event)
    p.chunks_first = !p.rows_all || p.rows_overlap;
    // With the parents' lists already there, the two chains are launched in turn, a rank event of each: the host needs ~3 us per
    // call, and the adopted nodes' chain queued behind all the coefficient launches would start ~70 us late.
    p.interleave = p.early_free && p.two && p.parents_first && !p.rows_all;
    // with the adopted nodes in one launch, the coefficient chain is one launch too (pg_coeff_all) when all of its workgroups
    // can be resident (pg_coeff_plan holds 66 rank events; beyond 65 taxa the coefficients run as a launch per rank event, which
    // ticks the same tickets and completion words for pg_nodes_rows_all -- DESIGN.md section 4b-taxa)
    p.coeff_all = p.rows_all && R - 1 <= 64 && coeff_wgs > 0 && coeff_wgs <= 2048 && !p.coeff_chain;
}

enum {
    PG_PLAN_ROWS_FORM = 1 << 0, PG_PLAN_WHOLE = 1 << 1, PG_PLAN_EARLY_FREE = 1 << 2, PG_PLAN_DEV_LISTS = 1 << 3,
    PG_PLAN_SORT_EARLY = 1 << 4, PG_PLAN_BG_FREE = 1 << 5, PG_PLAN_TWO = 1 << 6, PG_PLAN_PARENTS_FIRST = 1 << 7,
    PG_PLAN_ROWS_ALL = 1 << 8, PG_PLAN_ROWS_OVERLAP = 1 << 9, PG_PLAN_CHUNKS_FIRST = 1 << 10, PG_PLAN_INTERLEAVE = 1 << 11,
    PG_PLAN_COEFF_ALL = 1 << 12
};
inline uint32_t pg_plan_mask(const pg_plan& p) {
    return (p.rows_form ? PG_PLAN_ROWS_FORM : 0) | (p.whole ? PG_PLAN_WHOLE : 0) | (p.early_free ? PG_PLAN_EARLY_FREE : 0) |
           (p.dev_lists ? PG_PLAN_DEV_LISTS : 0) | (p.sort_early ? PG_PLAN_SORT_EARLY : 0) | (p.bg_free ? PG_PLAN_BG_FREE : 0) |
           (p.two ? PG_PLAN_TWO : 0) | (p.parents_first ? PG_PLAN_PARENTS_FIRST : 0) | (p.rows_all ? PG_PLAN_ROWS_ALL : 0) |
           (p.rows_overlap ? PG_PLAN_ROWS_OVERLAP : 0) | (p.chunks_first ? PG_PLAN_CHUNKS_FIRST : 0) |
           (p.interleave ? PG_PLAN_INTERLEAVE : 0) | (p.coeff_all ? PG_PLAN_COEFF_ALL : 0);
}
