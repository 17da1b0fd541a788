// phylo_treenni_rates.h -- phylo_trees_nni_rates: the change of the MIXTURE log-likelihood of many explicit trees under every
// nearest-neighbour interchange, at the trees' current branch lengths, under C rate categories.  Host: the
// plan of a call (chunk of trees, slab layout, capped grid, LDS of a launch).  Device: ptnr_updown (ptgr_updown's upward pass,
// categories outermost, every category's nodes kept in its own plane of the node store; then ptn_updown's moves with the
// categories INNERMOST per move, so that the neighbour's site value is complete inside a site before its log is taken) and
// ptnr_finish.  A sibling of phylo_treenni.h and phylo_treegrad_rates.h over their device functions: pt2_prune*, ptg_updown*,
// ptgr_updown*, ptn_updown and ptn_finish keep their code objects.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "phylo_treegrad_rates.h"
#include "phylo_treenni.h"

// ------------------------------------------------------------------------------------------------
// host: the plan of one call -- no HIP (tests/treenni_rates_asan_main.cpp runs it under sanitizers)
// ------------------------------------------------------------------------------------------------
struct ptnr_plan {
    int chunk = 0;                 // trees per chunk
    int grid = 0;                  // workgroups of ptnr_updown for a full chunk (a shorter last chunk launches min(grid, its items))
    size_t per_tree = 0, wg_store = 0;
    // byte offsets into the slab (all multiples of 256)
    size_t o_prior = 0, o_w = 0, o_ops = 0, o_dops = 0, o_nops = 0, o_P = 0, o_t = 0, o_gap = 0, o_tilev = 0, o_out = 0, o_dtile = 0, o_dout = 0,
           o_store = 0, total = 0;
};

// dynamic LDS of a launch: the stack of the upward pass | acc [2 (N-1)]
inline size_t ptnr_lds_bytes(int N, int depth) { return (size_t)depth * PTG_U * PTG_SLOT_BYTES + 2 * ((size_t)N - 1) * 8; }

// the slab in slab order: prior | weights | ops | downward ops | children's ops | per category: M, lengths, gap rows of M | tile values |
// loglik | delta tiles | delta
inline int ptnr_regions(int N, int ntiles, int C, bool coded, ptnr_plan& q, pts_region* r) {
    const size_t R = (size_t)N - 1, nt = (size_t)ntiles, nc = (size_t)C;
    int k = 0;
    r[k++] = {PTS_FIXED, 32, true, &q.o_prior};
    r[k++] = {PTS_TREE, nc * 8, true, &q.o_w};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_ops};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_dops};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_nops};
    r[k++] = {PTS_TREE, nc * R * 256, true, &q.o_P};
    r[k++] = {PTS_TREE, nc * R * 16, true, &q.o_t};
    r[k++] = {PTS_TREE, nc * R * 64, coded, &q.o_gap};
    r[k++] = {PTS_TREE, nt * 8, true, &q.o_tilev};
    r[k++] = {PTS_TREE, 8, true, &q.o_out};
    r[k++] = {PTS_TREE, nt * 2 * R * 8, true, &q.o_dtile};
    r[k++] = {PTS_TREE, 2 * R * 8, true, &q.o_dout};
    return k;
}

// 0: fine.  T trees of N taxa under C categories, ntiles site tiles, n_cus compute units; env_chunk > 0 caps the chunk
// (PHYLO_TREES_CHUNK).  The grid is ptgr_make_plan's: min(items, 8 per compute unit, 256 MiB of node stores), at least 1.
inline int ptnr_make_plan(int N, int ntiles, int T, int C, bool coded, int n_cus, int env_chunk, ptnr_plan* p) {
    if (N < 2 || ntiles < 1 || T < 1 || n_cus < 1 || C < 1 || C > PTGR_MAX_CATS) return 1;
    ptnr_plan q;
    q.wg_store = (size_t)C * ((size_t)N - 1) * PTG_U * PTG_SLOT_BYTES;
    pts_region r[PTS_MAX_REGIONS];
    ptg_finish_plan(q, r, ptnr_regions(N, ntiles, C, coded, q, r), ntiles, T, n_cus, env_chunk, 0, 0);
    *p = q;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

struct ptnr_args {
    pt2_args a;                      // ops, leaves, codes, prior, tilev, N, S, T, ntiles as pt2_prune takes them; P [trees][C][N-1][2][16] (M),
                                     // gap [trees][C][N-1][2][4]; site_lik unused
    const int32_t* dops;             // [trees][N-1][4] downward operations (ptg_down_ops)
    const int32_t* nops;             // [trees][N-1][4] the children's operations (ptn_nni_ops)
    const double* w;                 // [trees][C] the tree's weights: indexed by tree, so a mixture per tree costs nothing
    double* dtile;                   // [trees][ntiles][2 (N-1)] per-move tile sums, by the schedule index of the move's node v
    pk_d2* store;                    // [grid][C][N-1][U][2][64] node stores
    int n_items, depth, C;
};

// One neighbour in one category: ptn_move's x_p' (below the moved branch mz * mc, above it (x' . Mv) * my) and its factor against
// the outer partial av, folded into the neighbour's site value: w f' at the first category, fma(w, f', m') after it.
template <int U>
__device__ __forceinline__ void ptnr_fold(const double (&av)[U][4], const double (&mz)[U][4], const double (&mc)[U][4], const double (&my)[U][4],
                                          const double (&Mv)[16], double w, bool first, double (&mp)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        double xv[4], t[4], xp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = mz[u][j] * mc[u][j];
        pt2_row_times(xv, Mv, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) xp[j] = t[j] * my[u][j];
        const double f = pk_site_lik(av[u], xp);
        mp[u] = first ? w * f : pm_fma(w, f, mp[u]);
    }
}

// d = log(m' / m) of a finished neighbour: the step's 64 sites reduced by the wave's tree and added by lane 0 into the move's entry
template <int U>
__device__ __forceinline__ void ptnr_put(const double (&mp)[U], const double (&inv)[U], const bool (&live)[U], int lane, double* entry) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const double d = pm_log(mp[u] * inv[u]);
        const double tot = pk_wave_tree_sum(live[u] ? d : 0.0);
        if (lane == 0) *entry = *entry + tot;
    }
}

// the outer partial of a child: M (abar_p * sibling's message), ptg_updown's terms, into the child's slot of the category's plane
template <int U>
__device__ __forceinline__ void ptnr_outer(const double (&av)[U][4], const double (&ec)[U][4], const double (&m)[16], pk_d2* dst) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        double q[4], ac[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) q[j] = av[u][j] * ec[u][j];
#pragma unroll
        for (int k = 0; k < 4; ++k) ac[k] = ((m[4 * k] * q[0] + m[4 * k + 1] * q[1]) + m[4 * k + 2] * q[2]) + m[4 * k + 3] * q[3];
        const pk_d2 lo = {ac[0], ac[1]}, hi = {ac[2], ac[3]};
        dst[u * 128] = lo;
        dst[u * 128 + 64] = hi;
    }
}

// One wave (= one workgroup) per work item (tree, site tile), lane = column; workgroup w takes items w, w + grid, ...  Per strip of
// 64 U sites: ptgr_updown's upward pass (categories outermost over one LDS stack, the site value m in registers: the tile value is
// phylo_trees_loglik_rates' bits; every non-root node of category c kept in plane c of the workgroup's node store) and its 1 / m.
// Then the moves, and for every move the categories in ascending order INSIDE it: two per-lane accumulators m'[side][U], one per
// neighbour, take w_0 f'_0 and then fma(w_c, f'_c, m'); after the last category one pm_log(m' / m) and one wave sum per move and
// step.  First the two interchanges across the root's edge (both root children internal; every plane still holds partials).  Then
// the schedule in reverse, and at the operation of p one internal child v at a time: per category the outer partial of p from plane
// c (the prior at the root), the sibling's message and the messages of v's children under v's own matrices of category c (their
// slots hold partials in EVERY plane: v's operation comes later in this walk, ptn_nni_ops' guarantee), both neighbours' factors.
// The outer partials of p's internal children replace their partials in plane c in the pass of p's LAST internal child only: with
// two internal children the second child's moves still read the first child's partial as their sibling's message.
// A move's entry of the LDS array acc[2 (N-1)] is 2 (operation of v) + side.  Launched with ptnr_lds_bytes of dynamic LDS.
template <int U, bool CODED>
__global__ __launch_bounds__(64) void ptnr_updown(const ptnr_args g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ptnr_lds[];
    const pt2_args& a = g.a;
    const int lane = threadIdx.x;
    const int R = a.N - 1, C = g.C;
    pk_d2* stack = reinterpret_cast<pk_d2*>(ptnr_lds);
    double* acc = reinterpret_cast<double*>(ptnr_lds + (size_t)g.depth * U * PT2_SLOT_BYTES);
    const size_t plane = (size_t)R * U * 128;               // pk_d2 entries of one category's nodes
    pk_d2* store = g.store + (size_t)blockIdx.x * C * plane + lane;
#pragma unroll 1
    for (int item = blockIdx.x; item < g.n_items; item += gridDim.x) {     // item: wave-uniform
        const int tree = item / a.ntiles, tile = item - tree * a.ntiles;
        const int s0 = tile * a.T, s1 = s0 + a.T < a.S ? s0 + a.T : a.S;
        pt2_ci4* ops = (pt2_ci4*)(a.ops + (size_t)tree * R * 4);
        pt2_ci4* dops = (pt2_ci4*)(g.dops + (size_t)tree * R * 4);
        pt2_ci4* nops = (pt2_ci4*)(g.nops + (size_t)tree * R * 4);
        const double* Pt = a.P + (size_t)tree * C * R * 32;
        const double* Gt = CODED ? a.gap + (size_t)tree * C * R * 8 : nullptr;
        pt2_cd* wt = (pt2_cd*)(g.w + (size_t)tree * C);
        pt2_cd* prc = (pt2_cd*)a.prior;
        for (int j = lane; j < 2 * R; j += 64) acc[j] = 0.0;
        __syncthreads();
        pm_lp col = pm_lp_init();
#pragma unroll 1
        for (int base = s0; base < s1; base += 64 * U) {   // base: wave-uniform
            unsigned int sc[U];                             // a site past the end re-reads the last one; it contributes +0.0
            double m[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = base + 64 * u + lane;
                sc[u] = (unsigned int)(s < s1 ? s : s1 - 1);
                m[u] = 0.0;
            }
#pragma unroll 1
            for (int c = 0; c < C; ++c) {                   // upward: ptgr_updown's loops, and the nodes kept
                const double* P = Pt + (size_t)c * R * 32;
                const double* G = CODED ? Gt + (size_t)c * R * 8 : nullptr;
                pk_d2* pl = store + (size_t)c * plane;
                double o[U][4];
#pragma unroll 1
                for (int i = 0; i < R; ++i) {
                    const pt2_i4 op = ops[i];
                    double l[U][4], r[U][4];
                    pt2_side<U, CODED>(a, op.y, P + (size_t)i * 32, CODED ? G + (size_t)i * 8 : nullptr, stack, sc, lane, l);
                    pt2_side<U, CODED>(a, op.z, P + (size_t)i * 32 + 16, CODED ? G + (size_t)i * 8 + 4 : nullptr, stack, sc, lane, r);
                    pk_d2* dst = stack + (size_t)op.x * U * 128 + lane;
                    pk_d2* keep = pl + (size_t)op.w * U * 128;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) o[u][j] = l[u][j] * r[u][j];
                        const pk_d2 lo = {o[u][0], o[u][1]}, hi = {o[u][2], o[u][3]};
                        dst[u * 128] = lo;
                        dst[u * 128 + 64] = hi;
                        if (i < R - 1) {                    // wave-uniform; the root's slot of the store is never read
                            keep[u * 128] = lo;
                            keep[u * 128 + 64] = hi;
                        }
                    }
                }
                const double pr[4] = {prc[0], prc[1], prc[2], prc[3]};
                const double w = wt[c];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (base + 64 * u < s1) {               // wave-uniform
                        const double f = pk_site_lik(pr, o[u]);
                        m[u] = c ? pm_fma(w, f, m[u]) : w * f;
                    }
            }
            double inv[U];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = base + 64 * u + lane;
                live[u] = s < s1;
                inv[u] = 0.0;
                if (base + 64 * u < s1) {                   // wave-uniform
                    inv[u] = m[u] >= PTG_LIK_FLOOR && m[u] < pm_inf() ? 1.0 / m[u] : pm_nan();     // ptgr_updown's rule
                    if (s < s1) pm_lp_mul(col, m[u]);
                }
            }
            {                                               // across the root's edge: v = (a, b), c = (d, e) exchange b with d, with e
                const pt2_i4 dop = dops[R - 1], nop = nops[R - 1];
                if (dop.x < 0 && dop.y < 0) {               // wave-uniform
                    const pt2_i4 vd = dops[nop.x], cd = dops[nop.y];
                    double mp[2][U] = {};
#pragma unroll 1
                    for (int c = 0; c < C; ++c) {
                        const pk_d2* pl = store + (size_t)c * plane;
                        const double* Pc = Pt + (size_t)c * R * 32;
                        const double* Mv = Pc + (size_t)nop.x * 32;
                        const double* Mc = Pc + (size_t)nop.y * 32;
                        double ma[U][4], mb[U][4], md[U][4], me[U][4];
                        ptn_msg<U, CODED>(a, vd.x, Mv, pl, sc, ma);
                        ptn_msg<U, CODED>(a, vd.y, Mv + 16, pl, sc, mb);
                        ptn_msg<U, CODED>(a, cd.x, Mc, pl, sc, md);
                        ptn_msg<U, CODED>(a, cd.y, Mc + 16, pl, sc, me);
                        double mv[16], mc[16];
                        pt2_uniform16(Pc + (size_t)(R - 1) * 32, mv);
                        pt2_uniform16(Pc + (size_t)(R - 1) * 32 + 16, mc);
                        const double pr[4] = {prc[0], prc[1], prc[2], prc[3]};
                        const double w = wt[c];
#pragma unroll
                        for (int sd = 0; sd < 2; ++sd) {
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const double (&in)[4] = sd ? me[u] : md[u];      // joins a under v
                                const double (&st)[4] = sd ? md[u] : me[u];      // stays under c, joined by b
                                double xv[4], xc[4], tv[4], tc[4], xr[4];
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    xv[j] = ma[u][j] * in[j];
                                    xc[j] = st[j] * mb[u][j];
                                }
                                pt2_row_times(xv, mv, tv);
                                pt2_row_times(xc, mc, tc);
#pragma unroll
                                for (int j = 0; j < 4; ++j) xr[j] = tv[j] * tc[j];
                                const double f = pk_site_lik(pr, xr);
                                mp[sd][u] = c ? pm_fma(w, f, mp[sd][u]) : w * f;
                            }
                        }
                    }
                    ptnr_put<U>(mp[0], inv, live, lane, acc + 2 * (R - 1));
                    ptnr_put<U>(mp[1], inv, live, lane, acc + 2 * (R - 1) + 1);
                }
            }
#pragma unroll 1
            for (int i = R - 1; i >= 0; --i) {              // downward
                const pt2_i4 dop = dops[i];                 // x, y: left and right child; z: the node's row
                const pt2_i4 nop = nops[i];                 // x, y: the operations of the children
                if (dop.x >= 0 && dop.y >= 0) continue;     // wave-uniform: two leaves below, no move and no outer partial to leave
                const int last = dop.y < 0 ? 1 : 0;         // the pass that leaves the outer partials
#pragma unroll 1
                for (int sd = 0; sd < 2; ++sd) {
                    const int src = sd ? dop.y : dop.x;
                    if (src >= 0) continue;                 // wave-uniform: an internal child v, one at a time
                    const int sib = sd ? dop.x : dop.y;
                    const int jv = sd ? nop.y : nop.x;
                    const pt2_i4 vd = dops[jv];
                    double mp[2][U] = {};
#pragma unroll 1
                    for (int c = 0; c < C; ++c) {
                        pk_d2* pl = store + (size_t)c * plane;
                        const double* Pc = Pt + (size_t)c * R * 32;
                        const double* Mi = Pc + (size_t)i * 32;
                        const double* Mj = Pc + (size_t)jv * 32;
                        double av[U][4];
                        if (i == R - 1) {
#pragma unroll
                            for (int u = 0; u < U; ++u)
#pragma unroll
                                for (int j = 0; j < 4; ++j) av[u][j] = prc[j];
                        } else {
                            const pk_d2* sl = pl + (size_t)dop.z * U * 128;
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const pk_d2 lo = sl[u * 128], hi = sl[u * 128 + 64];
                                av[u][0] = lo.x; av[u][1] = lo.y; av[u][2] = hi.x; av[u][3] = hi.y;
                            }
                        }
                        double ec[U][4];                    // the sibling's message again: the chain of the upward pass
                        ptn_msg<U, CODED>(a, sib, Mi + (1 - sd) * 16, pl, sc, ec);
                        double mm[16];
                        pt2_uniform16(Mi + sd * 16, mm);    // the branch above v
                        {
                            double ma[U][4], mb[U][4];      // v's children under v's matrices (their slots still hold partials)
                            ptn_msg<U, CODED>(a, vd.x, Mj, pl, sc, ma);
                            ptn_msg<U, CODED>(a, vd.y, Mj + 16, pl, sc, mb);
                            const double w = wt[c];
                            ptnr_fold<U>(av, mb, ec, ma, mm, w, c == 0, mp[0]);        // side 0: a and the sibling change places
                            ptnr_fold<U>(av, ma, ec, mb, mm, w, c == 0, mp[1]);        // side 1: b and the sibling
                        }
                        if (sd == last) {                   // wave-uniform: every read of the children's partials in plane c is done
                            if (sib < 0) {                  // (sd = 1, both internal) the sibling's outer partial, from v's message
                                double ev[U][4], ms[16];
                                ptn_msg<U, CODED>(a, src, Mi + sd * 16, pl, sc, ev);
                                pt2_uniform16(Mi + (1 - sd) * 16, ms);
                                ptnr_outer<U>(av, ev, ms, pl + (size_t)(~sib) * U * 128);
                            }
                            ptnr_outer<U>(av, ec, mm, pl + (size_t)(~src) * U * 128);
                        }
                    }
                    ptnr_put<U>(mp[0], inv, live, lane, acc + 2 * jv);
                    ptnr_put<U>(mp[1], inv, live, lane, acc + 2 * jv + 1);
                }
            }
        }
        const double t = pk_wave_tree_sum(pm_lp_finish(col));
        if (lane == 0) a.tilev[item] = t;                   // [tree][tile]
        __syncthreads();                                    // lane 0's sums, read by every lane
        double* out = g.dtile + (size_t)item * 2 * R;
        for (int j = lane; j < 2 * R; j += 64) out[j] = acc[j];
        __syncthreads();                                    // ... before the next item clears them
    }
}

// Per (tree, move): the tiles added left to right; written to the caller's row (op.w of the operation of v) and side.  A tree
// whose log-likelihood is not finite gets NaN in every entry (one with a site value below PTG_LIK_FLOOR already carries it); so
// do the two entries of the root's row when one of the root's children is a leaf: those moves do not exist.  out [trees][N-1][2].
__global__ __launch_bounds__(256) void ptnr_finish(const double* __restrict__ dtile, const int32_t* __restrict__ ops, const double* __restrict__ loglik,
                                                   int ntiles, int trees, int R, double* __restrict__ out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = 2L * R;
    if (idx >= trees * per) return;
    const long tree = idx / per;
    const int b = (int)(idx - tree * per);
    const double* tv = dtile + (size_t)tree * ntiles * per + b;
    double tot = tv[0];
    for (int i = 1; i < ntiles; ++i) tot = tot + tv[(size_t)i * per];
    const int32_t* top = ops + (size_t)tree * R * 4;
    const double ll = loglik[tree];
    if (pm_isnan(ll) || ll == pm_inf() || ll == -pm_inf()) tot = pm_nan();
    if ((b >> 1) == R - 1 && (top[4 * (R - 1) + 1] >= 0 || top[4 * (R - 1) + 2] >= 0)) tot = pm_nan();
    const int row = top[4 * (b >> 1) + 3];
    out[(size_t)tree * per + 2 * row + (b & 1)] = tot;
}

inline void ptnr_launch(const ptnr_args& g, int grid, bool coded, hipStream_t s) {
    const size_t lds = ptnr_lds_bytes(g.a.N, g.depth);
    if (coded) hipLaunchKernelGGL((ptnr_updown<PTG_U, true>), dim3((unsigned)grid), dim3(64), lds, s, g);
    else hipLaunchKernelGGL((ptnr_updown<PTG_U, false>), dim3((unsigned)grid), dim3(64), lds, s, g);
}
#endif  // __HIPCC__
