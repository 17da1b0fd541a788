// phylo_treegrad_rates.h -- phylo_trees_grad_rates: the derivatives of the MIXTURE log-likelihood of many explicit trees under C
// rate categories with respect to each of their 2 (N-1) branch lengths, their own second derivatives, and
// the derivatives with respect to every category's rate and weight.  Host: the plan of a call (chunk of trees, slab layout, capped
// grid, LDS of a launch).  Device: ptgr_updown (the upward pass of pt2_prune_rates, categories outermost, every category's nodes
// kept in its own plane of the node store; then the schedule in reverse with the categories innermost per operation, so that the
// sum over the categories is complete inside a site before it is divided by the site value and squared) and ptgr_finish.  A
// sibling of phylo_treegrad.h over its device functions: ptg_updown, ptg_dmats, ptg_finish, pt2_prune and pt2_prune_rates keep
// their code objects.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>
#include <cstdio>

#include "phylo_treegrad.h"

#define PTGR_MAX_CATS 16                          // PT2_MAX_CATS
#define PTGR_MAX_LDS ((size_t)64 << 10)           // dynamic LDS of a launch without raising the function's maximum

// ------------------------------------------------------------------------------------------------
// host: the plan of one call -- no HIP (tests/treegrad_rates_asan_main.cpp runs it under sanitizers)
// ------------------------------------------------------------------------------------------------
struct ptgr_plan {
    int chunk = 0;                 // trees per chunk
    int grid = 0;                  // workgroups of ptgr_updown for a full chunk
    int nq = 1;                    // 1: gradient; 2: gradient and curvature
    int np = 0;                    // 0: no rate and weight sums; 2: both
    int ncoef = 0;                 // doubles of a tree's coefficient block: w | u = w r | v = u r
    size_t per_tree = 0, wg_store = 0;
    // byte offsets into the slab (all multiples of 256)
    size_t o_prior = 0, o_coef = 0, o_ops = 0, o_dops = 0, o_P = 0, o_t = 0, o_b = 0, o_gap = 0, o_tilev = 0, o_out = 0, o_dtile = 0, o_dout = 0, o_ptile = 0,
           o_pout = 0, o_store = 0, total = 0;
};

// dynamic LDS of a launch: the stack of the upward pass | acc [nq][2 (N-1)] | (params) rate sums [C][64] | weight sums [C]
inline size_t ptgr_lds_bytes(int N, int depth, int C, bool curv, bool params) {
    return (size_t)depth * PTG_U * PTG_SLOT_BYTES + (size_t)(curv ? 2 : 1) * 2 * ((size_t)N - 1) * 8 + (params ? (size_t)C * 65 * 8 : 0);
}

// the slab in slab order: prior | coefficients | ops | downward ops | per category: M, M', M'' | scaled lengths | given lengths | gap rows of
// M | tile values | loglik | derivative tiles | derivatives | rate and weight tiles | rate and weight sums
inline int ptgr_regions(int N, int ntiles, int C, bool coded, ptgr_plan& q, pts_region* r) {
    const size_t R = (size_t)N - 1, nt = (size_t)ntiles, nc = (size_t)C, nq = (size_t)q.nq, np = (size_t)q.np;
    int k = 0;
    r[k++] = {PTS_FIXED, 32, true, &q.o_prior};
    r[k++] = {PTS_TREE, (size_t)q.ncoef * 8, true, &q.o_coef};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_ops};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_dops};
    r[k++] = {PTS_TREE, nc * 3 * R * 256, true, &q.o_P};
    r[k++] = {PTS_TREE, nc * R * 16, true, &q.o_t};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_b};
    r[k++] = {PTS_TREE, nc * R * 64, coded, &q.o_gap};
    r[k++] = {PTS_TREE, nt * 8, true, &q.o_tilev};
    r[k++] = {PTS_TREE, 8, true, &q.o_out};
    r[k++] = {PTS_TREE, nt * nq * 2 * R * 8, true, &q.o_dtile};
    r[k++] = {PTS_TREE, nq * 2 * R * 8, true, &q.o_dout};
    r[k++] = {PTS_TREE, nt * np * nc * 8, np > 0, &q.o_ptile};
    r[k++] = {PTS_TREE, np * nc * 8, np > 0, &q.o_pout};
    return k;
}

// 0: fine.  T trees of N taxa under C categories, ntiles site tiles, n_cus compute units; env_chunk > 0 caps the chunk.
inline int ptgr_make_plan(int N, int ntiles, int T, int C, bool coded, bool curv, bool params, int n_cus, int env_chunk, ptgr_plan* p) {
    if (N < 2 || ntiles < 1 || T < 1 || n_cus < 1 || C < 1 || C > PTGR_MAX_CATS) return 1;
    ptgr_plan q;
    q.nq = curv ? 2 : 1;
    q.np = params ? 2 : 0;
    q.ncoef = 3 * C;
    q.wg_store = (size_t)C * ((size_t)N - 1) * PTG_U * PTG_SLOT_BYTES;
    pts_region r[PTS_MAX_REGIONS];
    ptg_finish_plan(q, r, ptgr_regions(N, ntiles, C, coded, q, r), ntiles, T, n_cus, env_chunk, 0, 0);
    *p = q;
    return 0;
}

// The mixture of one tree: every rate and weight a finite number >= 0, every scaled length finite.  0: fine; else a message that
// names row and category (the caller names the tree).
inline int ptgr_check_mixture(int N, const double* blen, int C, const double* rate, const double* weight, char* msg, size_t nmsg) {
    for (int k = 0; k < C; ++k) {
        if (!(rate[k] >= 0.0) || !std::isfinite(rate[k])) {
            snprintf(msg, nmsg, "rate %g of category %d is not a finite number >= 0", rate[k], k);
            return 1;
        }
        if (!(weight[k] >= 0.0) || !std::isfinite(weight[k])) {
            snprintf(msg, nmsg, "weight %g of category %d is not a finite number >= 0", weight[k], k);
            return 1;
        }
    }
    for (int k = 0; k < C; ++k)
        for (int i = 0; i < 2 * (N - 1); ++i)
            if (!std::isfinite(rate[k] * blen[i])) {
                snprintf(msg, nmsg, "row %d, category %d: branch length %g at rate %g is not finite", i / 2, k, blen[i], rate[k]);
                return 1;
            }
    return 0;
}

// A tree's coefficient block: w | u = w r | v = u r (one multiply each)
inline void ptgr_coefficients(int C, const double* rate, const double* weight, double* coef) {
    for (int k = 0; k < C; ++k) {
        const double u = weight[k] * rate[k];
        coef[k] = weight[k];
        coef[C + k] = u;
        coef[2 * C + k] = u * rate[k];
    }
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

struct ptgr_args {
    pt2_args a;                      // ops, leaves, codes, tilev, N, S, T, ntiles as pt2_prune takes them; P [trees][C][N-1][2][16] (M),
                                     // gap [trees][C][N-1][2][4]; site_lik unused
    const int32_t* dops;             // [trees][N-1][4] downward operations (ptg_down_ops)
    const double* coef;              // [trees][3 C] w | u | v: indexed by tree, so a mixture per tree costs nothing
    const double* blen;              // [trees][N-1][2] the GIVEN lengths in schedule order (the rate sums multiply by them)
    double* dtile;                   // [trees][ntiles][nq][2 (N-1)] per-branch tile sums, in schedule order
    double* ptile;                   // [trees][ntiles][2][C] rate and weight tile sums, or NULL
    pk_d2* store;                    // [grid][C][N-1][U][2][64] node stores
    long mat_plane;                  // doubles from M to M' (and from M' to M'')
    int n_items, depth, C;
};

// One wave (= one workgroup) per work item (tree, site tile), lane = column; workgroup w takes items w, w + grid, ...  Per strip
// of 64 U sites: the upward pass of pt2_prune_rates<2> (categories outermost over one LDS stack, the site value m held in
// registers: the tile value is its bits), every non-root node of category c also stored to plane c of the workgroup's node store;
// then the schedule in reverse, and per operation the categories in ascending order: the outer partial of the node in category c
// (the prior at the root), both children's partials, both messages again, g, D1 (and D2) of both branches by ptg_xDg, added as
// a1 = a1 + u_c D1 (a2 = a2 + v_c D2) from +0.0; the child's outer partial takes the child's slot of plane c.  After the last
// category a1 / m (and a2 / m - (a1 / m)^2) go through pk_wave_tree_sum and lane 0 adds them into the LDS array acc as ptg_updown
// does.  PARAMS: every lane adds (blen_b w_c) D1_c / m into its own entry of the LDS array dr [C][64] (an own-lane
// read-add-write: no conflict, no barrier), reduced by the wave tree once per item; at the root operation f_c is made again from
// its two messages and f_c / m goes through the wave tree into dw [C], steps ascending.
// Launched with ptgr_lds_bytes of dynamic LDS.
template <int U, bool CODED, bool CURV, bool PARAMS>
__global__ __launch_bounds__(64) void ptgr_updown(const ptgr_args g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ptgr_lds[];
    constexpr int NQ = CURV ? 2 : 1;
    const pt2_args& a = g.a;
    const int lane = threadIdx.x;
    const int R = a.N - 1, C = g.C;
    pk_d2* stack = reinterpret_cast<pk_d2*>(ptgr_lds);
    double* acc = reinterpret_cast<double*>(ptgr_lds + (size_t)g.depth * U * PT2_SLOT_BYTES);
    double* dr = acc + NQ * 2 * R;                          // [C][64]
    double* dw = dr + C * 64;                               // [C]
    const size_t plane = (size_t)R * U * 128;               // pk_d2 entries of one category's nodes
    pk_d2* store = g.store + (size_t)blockIdx.x * C * plane + lane;
#pragma unroll 1
    for (int item = blockIdx.x; item < g.n_items; item += gridDim.x) {     // item: wave-uniform
        const int tree = item / a.ntiles, tile = item - tree * a.ntiles;
        const int s0 = tile * a.T, s1 = s0 + a.T < a.S ? s0 + a.T : a.S;
        pt2_ci4* ops = (pt2_ci4*)(a.ops + (size_t)tree * R * 4);
        pt2_ci4* dops = (pt2_ci4*)(g.dops + (size_t)tree * R * 4);
        const double* Pt = a.P + (size_t)tree * C * R * 32;
        const double* Gt = CODED ? a.gap + (size_t)tree * C * R * 8 : nullptr;
        pt2_cd* cf = (pt2_cd*)(g.coef + (size_t)tree * 3 * C);
        pt2_cd* prc = (pt2_cd*)a.prior;
        pt2_cd* bt = (pt2_cd*)(g.blen + (size_t)tree * R * 2);
        for (int j = lane; j < NQ * 2 * R; j += 64) acc[j] = 0.0;
        if constexpr (PARAMS) {
            for (int c = 0; c < C; ++c) dr[c * 64 + lane] = 0.0;
            if (lane < C) dw[lane] = 0.0;
        }
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
            for (int c = 0; c < C; ++c) {                   // upward: pt2_prune_rates' loops, and the nodes kept
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
                const double w = cf[c];
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
                    // below the floor 1 / m overflows or is made from a subnormal's few bits: NaN, which the wave reductions
                    // carry into every sum of the tile and ptgr_finish into every entry of the tree
                    inv[u] = m[u] >= PTG_LIK_FLOOR && m[u] < pm_inf() ? 1.0 / m[u] : pm_nan();
                    if (s < s1) pm_lp_mul(col, m[u]);
                }
            }
#pragma unroll 1
            for (int i = R - 1; i >= 0; --i) {              // downward
                const pt2_i4 dop = dops[i];                 // x, y: left and right child; z: the node's row
                double a1[2][U], a2[2][U];
#pragma unroll
                for (int sd = 0; sd < 2; ++sd)
#pragma unroll
                    for (int u = 0; u < U; ++u) a1[sd][u] = a2[sd][u] = 0.0;
#pragma unroll 1
                for (int c = 0; c < C; ++c) {
                    pk_d2* pl = store + (size_t)c * plane;
                    const double* Mi = Pt + ((size_t)c * R + i) * 32;
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
                    double x[2][U][4], gg[2][U][4];         // the children's partials; g of the left branch = outer partial x right
                    ptg_child<U, CODED>(a, dop.x, pl, sc, x[0]);
                    ptg_child<U, CODED>(a, dop.y, pl, sc, x[1]);
                    {
                        double ml[16], mr[16];
                        pt2_uniform16(Mi, ml);
                        pt2_uniform16(Mi + 16, mr);
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            double el[4], er[4];            // the messages again: the chain of the upward pass
                            pt2_row_times(x[0][u], ml, el);
                            pt2_row_times(x[1][u], mr, er);
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                gg[0][u][j] = av[u][j] * er[j];
                                gg[1][u][j] = av[u][j] * el[j];
                            }
                            if constexpr (PARAMS) {
                                if (i == R - 1) {           // wave-uniform: f_c again, from the root's two messages
                                    double o[4];
#pragma unroll
                                    for (int j = 0; j < 4; ++j) o[j] = el[j] * er[j];
                                    const double pr[4] = {prc[0], prc[1], prc[2], prc[3]};
                                    const double tot = pk_wave_tree_sum(live[u] ? pk_site_lik(pr, o) * inv[u] : 0.0);
                                    if (lane == 0) dw[c] = dw[c] + tot;
                                }
                            }
                        }
                    }
                    const double uc = cf[C + c], vc = cf[2 * C + c];
#pragma unroll
                    for (int sd = 0; sd < 2; ++sd) {
                        const int src = sd ? dop.y : dop.x;
                        {
                            double d[16];
                            pt2_uniform16(Mi + g.mat_plane + sd * 16, d);
                            double bw = 0.0;
                            if constexpr (PARAMS) bw = bt[2 * i + sd] * cf[c];
                            double part = 0.0;
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const double d1 = ptg_xDg(x[sd][u], d, gg[sd][u]);
                                a1[sd][u] = a1[sd][u] + uc * d1;
                                if constexpr (PARAMS) part = part + (live[u] ? (bw * d1) * inv[u] : 0.0);
                            }
                            if constexpr (PARAMS) dr[c * 64 + lane] = dr[c * 64 + lane] + part;
                        }
                        if constexpr (CURV) {
                            double d[16];
                            pt2_uniform16(Mi + 2 * g.mat_plane + sd * 16, d);
#pragma unroll
                            for (int u = 0; u < U; ++u) a2[sd][u] = a2[sd][u] + vc * ptg_xDg(x[sd][u], d, gg[sd][u]);
                        }
                        if (src < 0) {                      // wave-uniform: the child's outer partial takes the child's slot
                            double mm[16];
                            pt2_uniform16(Mi + sd * 16, mm);
                            pk_d2* dst = pl + (size_t)(~src) * U * 128;
#pragma unroll
                            for (int u = 0; u < U; ++u) {
                                const double (&q)[4] = gg[sd][u];
                                double ac[4];
#pragma unroll
                                for (int k = 0; k < 4; ++k) ac[k] = ((mm[4 * k] * q[0] + mm[4 * k + 1] * q[1]) + mm[4 * k + 2] * q[2]) + mm[4 * k + 3] * q[3];
                                const pk_d2 lo = {ac[0], ac[1]}, hi = {ac[2], ac[3]};
                                dst[u * 128] = lo;
                                dst[u * 128 + 64] = hi;
                            }
                        }
                    }
                }
#pragma unroll
                for (int sd = 0; sd < 2; ++sd)
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const double r1 = a1[sd][u] * inv[u];
                        const double tot = pk_wave_tree_sum(live[u] ? r1 : 0.0);
                        if (lane == 0) acc[2 * i + sd] = acc[2 * i + sd] + tot;
                        if constexpr (CURV) {
                            const double cv = a2[sd][u] * inv[u] - r1 * r1;
                            const double tc = pk_wave_tree_sum(live[u] ? cv : 0.0);
                            if (lane == 0) acc[2 * R + 2 * i + sd] = acc[2 * R + 2 * i + sd] + tc;
                        }
                    }
            }
        }
        const double t = pk_wave_tree_sum(pm_lp_finish(col));
        if (lane == 0) a.tilev[item] = t;                   // [tree][tile]
        __syncthreads();                                    // lane 0's sums, read by every lane
        double* out = g.dtile + (size_t)item * NQ * 2 * R;
        for (int j = lane; j < NQ * 2 * R; j += 64) out[j] = acc[j];
        if constexpr (PARAMS) {
            double* po = g.ptile + (size_t)item * 2 * C;
#pragma unroll 1
            for (int c = 0; c < C; ++c) {
                const double tot = pk_wave_tree_sum(dr[c * 64 + lane]);
                if (lane == 0) po[c] = tot;
            }
            if (lane < C) po[C + lane] = dw[lane];
        }
        __syncthreads();                                    // ... before the next item clears them
    }
}

// The branch sums as ptg_finish gives them (tiles left to right, the caller's row and side; out [nq][trees][N-1][2]) and, with
// np = 2, the rate and weight sums (pout [2][trees][C]).  A tree whose log-likelihood is not finite gets NaN in every entry (one
// with a site value below PTG_LIK_FLOOR already carries it).
__global__ __launch_bounds__(256) void ptgr_finish(const double* __restrict__ dtile, const double* __restrict__ ptile, const int32_t* __restrict__ ops,
                                                   const double* __restrict__ loglik, int ntiles, int trees, int R, int nq, int np, int C,
                                                   double* __restrict__ out, double* __restrict__ pout) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)nq * 2 * R, pper = (long)np * C;
    if (idx >= trees * (per + pper)) return;
    if (idx < trees * per) {
        const long tree = idx / per, rem = idx - tree * per;
        const int q = (int)(rem / (2 * R)), b = (int)(rem - (long)q * 2 * R);
        const double* tv = dtile + (size_t)tree * ntiles * per + rem;
        double tot = tv[0];
        for (int i = 1; i < ntiles; ++i) tot = tot + tv[(size_t)i * per];
        const double ll = loglik[tree];
        if (pm_isnan(ll) || ll == pm_inf() || ll == -pm_inf()) tot = pm_nan();
        const int row = ops[((size_t)tree * R + (b >> 1)) * 4 + 3];
        out[((size_t)q * trees + tree) * 2 * R + 2 * row + (b & 1)] = tot;
    } else {
        const long k = idx - trees * per;
        const long tree = k / pper, rem = k - tree * pper;
        const int q = (int)(rem / C), c = (int)(rem - (long)q * C);
        const double* tv = ptile + (size_t)tree * ntiles * pper + rem;
        double tot = tv[0];
        for (int i = 1; i < ntiles; ++i) tot = tot + tv[(size_t)i * pper];
        const double ll = loglik[tree];
        if (pm_isnan(ll) || ll == pm_inf() || ll == -pm_inf()) tot = pm_nan();
        pout[((size_t)q * trees + tree) * C + c] = tot;
    }
}

template <bool CODED, bool CURV, bool PARAMS>
inline void ptgr_launch_as(const ptgr_args& g, int grid, hipStream_t s) {
    const size_t lds = ptgr_lds_bytes(g.a.N, g.depth, g.C, CURV, PARAMS);
    hipLaunchKernelGGL((ptgr_updown<PTG_U, CODED, CURV, PARAMS>), dim3((unsigned)grid), dim3(64), lds, s, g);
}
inline void ptgr_launch(const ptgr_args& g, int grid, bool coded, bool curv, bool params, hipStream_t s) {
    const int form = (coded ? 4 : 0) | (curv ? 2 : 0) | (params ? 1 : 0);
    switch (form) {
        case 0: ptgr_launch_as<false, false, false>(g, grid, s); break;
        case 1: ptgr_launch_as<false, false, true>(g, grid, s); break;
        case 2: ptgr_launch_as<false, true, false>(g, grid, s); break;
        case 3: ptgr_launch_as<false, true, true>(g, grid, s); break;
        case 4: ptgr_launch_as<true, false, false>(g, grid, s); break;
        case 5: ptgr_launch_as<true, false, true>(g, grid, s); break;
        case 6: ptgr_launch_as<true, true, false>(g, grid, s); break;
        default: ptgr_launch_as<true, true, true>(g, grid, s); break;
    }
}
#endif  // __HIPCC__
