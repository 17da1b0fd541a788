// phylo_treegrad_model.h -- phylo_trees_grad_model: the derivatives of the log-likelihood of many explicit trees along P directions
// in the space of generators, and with respect to the root distribution.  Host: the plan of a call (chunk
// of trees, slab layout, capped grid, LDS of a launch).  Device: ptm_dirmats (D_{p,b} = L(Q t_b, E_p t_b), the Frechet derivative
// of expm, for every branch and direction of a chunk), ptm_updown (ptg_updown's upward pass, node store and downward recursion,
// with the sum over ALL branches of x_child . D_{p,b} . g_b / L_s kept per lane and direction beside section 13's per-branch
// sums) and ptm_finish.  A sibling of phylo_treegrad.h over its device functions: ptg_updown, ptg_dmats, ptg_finish and the
// ptgr kernels keep their code objects.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "phylo_treegrad.h"

#define PTM_MAX_DIRS 16                           // directions of one call
#define PTM_MAX_LDS ((size_t)64 << 10)            // dynamic LDS of a launch without raising the function's maximum

// ------------------------------------------------------------------------------------------------
// host: the plan of one call -- no HIP (tests/treegrad_model_asan_main.cpp runs it under sanitizers)
// ------------------------------------------------------------------------------------------------
struct ptm_plan {
    int chunk = 0;                 // trees per chunk
    int grid = 0;                  // workgroups of ptm_updown for a full chunk (a shorter last chunk launches min(grid, its items))
    int nm = 0;                    // doubles of an item's model sums: P directions | 4 prior entries
    size_t per_tree = 0, wg_store = 0;
    // byte offsets into the slab (all multiples of 256)
    size_t o_prior = 0, o_dirs = 0, o_ops = 0, o_dops = 0, o_P = 0, o_D = 0, o_t = 0, o_gap = 0, o_tilev = 0, o_out = 0, o_dtile = 0, o_dout = 0,
           o_mtile = 0, o_mout = 0, o_store = 0, total = 0;
};

// dynamic LDS of a launch: the stack of the upward pass | (grad) acc [2 (N-1)] | direction sums [P][64]
inline size_t ptm_lds_bytes(int N, int depth, int P, bool grad) {
    return (size_t)depth * PTG_U * PTG_SLOT_BYTES + (grad ? 2 * ((size_t)N - 1) * 8 : 0) + (size_t)P * 64 * 8;
}

// the slab in slab order: prior | directions | ops | downward ops | M (and M') | D | lengths | gap rows of M | tile values | loglik |
// branch tiles | branch sums | model tiles | model sums
inline int ptm_regions(int N, int ntiles, int P, bool coded, bool grad, ptm_plan& q, pts_region* r) {
    const size_t R = (size_t)N - 1, nt = (size_t)ntiles, np = (size_t)P, nm = (size_t)q.nm;
    int k = 0;
    r[k++] = {PTS_FIXED, 32, true, &q.o_prior};
    r[k++] = {PTS_FIXED, np * 128, true, &q.o_dirs};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_ops};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_dops};
    r[k++] = {PTS_TREE, (grad ? 2 : 1) * R * 256, true, &q.o_P};
    r[k++] = {PTS_TREE, 2 * R * np * 128, true, &q.o_D};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_t};
    r[k++] = {PTS_TREE, R * 64, coded, &q.o_gap};
    r[k++] = {PTS_TREE, nt * 8, true, &q.o_tilev};
    r[k++] = {PTS_TREE, 8, true, &q.o_out};
    r[k++] = {PTS_TREE, nt * 2 * R * 8, grad, &q.o_dtile};
    r[k++] = {PTS_TREE, 2 * R * 8, grad, &q.o_dout};
    r[k++] = {PTS_TREE, nt * nm * 8, true, &q.o_mtile};
    r[k++] = {PTS_TREE, nm * 8, true, &q.o_mout};
    return k;
}

// 0: fine.  T trees of N taxa along P directions, ntiles site tiles, n_cus compute units; env_chunk > 0 caps the chunk.
inline int ptm_make_plan(int N, int ntiles, int T, int P, bool coded, bool grad, int n_cus, int env_chunk, ptm_plan* p) {
    if (N < 2 || ntiles < 1 || T < 1 || n_cus < 1 || P < 1 || P > PTM_MAX_DIRS) return 1;
    ptm_plan q;
    q.nm = P + 4;
    q.wg_store = ((size_t)N - 1) * PTG_U * PTG_SLOT_BYTES;
    pts_region r[PTS_MAX_REGIONS];
    ptg_finish_plan(q, r, ptm_regions(N, ntiles, P, coded, grad, q, r), ntiles, T, n_cus, env_chunk, 0, 0);
    *p = q;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

// D_{p,b} = L(Q_eff t_b, E_p t_b), one lane per (matrix, direction): A[i] = Q_eff[i] t_b and E[i] = dirs[p][i] t_b, one multiply
// each, then pg_expm4_frechet.  jc: the generator pm_jc69 implies (1/4, diagonal -3/4).  t [n_mat] in schedule order (left, right);
// D [n_mat][P][16], indexed like M.  A zero length gives A = E = 0 and every term of the series 0: D = 0.
__global__ __launch_bounds__(64) void ptm_dirmats(const double* __restrict__ Q, int jc, const double* __restrict__ dirs, int P,
                                                  const double* __restrict__ t, long n_mat, double* __restrict__ D) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_mat * P) return;
    const long m = idx / P;
    const int p = (int)(idx - m * P);
    const double tb = t[m];
    double A[16], E[16], L[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        A[e] = (jc ? (e % 5 == 0 ? -0.75 : 0.25) : Q[e]) * tb;
        E[e] = dirs[p * 16 + e] * tb;
    }
    pg_expm4_frechet(A, E, L);
#pragma unroll
    for (int e = 0; e < 16; ++e) D[idx * 16 + e] = L[e];
}

struct ptm_args {
    ptg_args g;                      // as ptg_updown takes them; dtile unused (NULL) without GRAD, mat_plane the doubles from M to M'
    const double* D;                 // [trees][N-1][2][P][16] direction matrices in schedule order (ptm_dirmats)
    double* mtile;                   // [trees][ntiles][P + 4] direction sums | prior sums of an item
    int P;
};

// ptg_updown (CURV = false) with the model sums beside it: the same upward pass, node store, site factors and downward recursion,
// and under GRAD the same per-branch sums in the same order (grad is ptg_updown's bits).  Per operation and side, after the
// per-branch term, the directions in ascending order: D_{p,b} as 16 wave-uniform scalars (one matrix at a time), ptg_xDg for the
// U steps, times 1 / L_s, a step past the end +0.0, the U terms added in ascending order from +0.0 and that sum added by the lane
// into ITS entry of the LDS array dth [P][64] (an own-lane read-add-write: no conflict, no barrier).  The prior sums: four
// register accumulators per lane, x_root[j] / L_s added after the upward pass of each strip, steps ascending.  Per item P + 4 wave
// reductions (pk_wave_tree_sum), lane 0 writes mtile [item][P + 4].
// Launched with ptm_lds_bytes of dynamic LDS.
template <int U, bool CODED, bool GRAD>
__global__ __launch_bounds__(64) void ptm_updown(const ptm_args m) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ptm_lds[];
    const ptg_args& g = m.g;
    const pt2_args& a = g.a;
    const int lane = threadIdx.x;
    const int R = a.N - 1, NP = m.P;
    pk_d2* stack = reinterpret_cast<pk_d2*>(ptm_lds);
    double* acc = reinterpret_cast<double*>(ptm_lds + (size_t)g.depth * U * PT2_SLOT_BYTES);
    double* dth = acc + (GRAD ? 2 * R : 0) + lane;         // [P][64], this lane's column
    pk_d2* store = g.store + (size_t)blockIdx.x * R * U * 128 + lane;
#pragma unroll 1
    for (int item = blockIdx.x; item < g.n_items; item += gridDim.x) {     // item: wave-uniform
        const int tree = item / a.ntiles, tile = item - tree * a.ntiles;
        const int s0 = tile * a.T, s1 = s0 + a.T < a.S ? s0 + a.T : a.S;
        pt2_ci4* ops = (pt2_ci4*)(a.ops + (size_t)tree * R * 4);
        pt2_ci4* dops = (pt2_ci4*)(g.dops + (size_t)tree * R * 4);
        const double* P = a.P + (size_t)tree * R * 32;
        const double* G = CODED ? a.gap + (size_t)tree * R * 8 : nullptr;
        const double* Dt = m.D + (size_t)tree * R * 2 * NP * 16;
        if constexpr (GRAD)
            for (int j = lane; j < 2 * R; j += 64) acc[j] = 0.0;
        for (int p = 0; p < NP; ++p) dth[p * 64] = 0.0;
        double dp[4] = {0.0, 0.0, 0.0, 0.0};
        __syncthreads();
        pm_lp col = pm_lp_init();
#pragma unroll 1
        for (int base = s0; base < s1; base += 64 * U) {   // base: wave-uniform
            unsigned int sc[U];                             // a site past the end re-reads the last one; it contributes +0.0
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = base + 64 * u + lane;
                sc[u] = (unsigned int)(s < s1 ? s : s1 - 1);
            }
            double o[U][4];
#pragma unroll 1
            for (int i = 0; i < R; ++i) {                   // upward: pt2_prune's loop, and the node kept
                const pt2_i4 op = ops[i];
                double l[U][4], r[U][4];
                pt2_side<U, CODED>(a, op.y, P + (size_t)i * 32, CODED ? G + (size_t)i * 8 : nullptr, stack, sc, lane, l);
                pt2_side<U, CODED>(a, op.z, P + (size_t)i * 32 + 16, CODED ? G + (size_t)i * 8 + 4 : nullptr, stack, sc, lane, r);
                pk_d2* dst = stack + (size_t)op.x * U * 128 + lane;
                pk_d2* keep = store + (size_t)op.w * U * 128;
#pragma unroll
                for (int u = 0; u < U; ++u) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[u][j] = l[u][j] * r[u][j];
                    const pk_d2 lo = {o[u][0], o[u][1]}, hi = {o[u][2], o[u][3]};
                    dst[u * 128] = lo;
                    dst[u * 128 + 64] = hi;
                    if (i < R - 1) {                        // wave-uniform; the root's slot of the store is never read
                        keep[u * 128] = lo;
                        keep[u * 128 + 64] = hi;
                    }
                }
            }
            pt2_cd* prc = (pt2_cd*)a.prior;
            const double pr[4] = {prc[0], prc[1], prc[2], prc[3]};
            double inv[U];
            bool live[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = base + 64 * u + lane;
                live[u] = s < s1;
                inv[u] = 0.0;
                if (base + 64 * u < s1) {                   // wave-uniform
                    const double lik = pk_site_lik(pr, o[u]);
                    // ptg_updown's rule: NaN below the floor, carried by the wave reductions into every sum of the tile
                    inv[u] = lik >= PTG_LIK_FLOOR && lik < pm_inf() ? 1.0 / lik : pm_nan();
                    if (s < s1) pm_lp_mul(col, lik);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) dp[j] = dp[j] + (live[u] ? o[u][j] * inv[u] : 0.0);
            }
#pragma unroll 1
            for (int i = R - 1; i >= 0; --i) {              // downward
                const pt2_i4 dop = dops[i];                 // x, y: left and right child; z: the node's row
                double av[U][4];
                if (i == R - 1) {
#pragma unroll
                    for (int u = 0; u < U; ++u)
#pragma unroll
                        for (int j = 0; j < 4; ++j) av[u][j] = pr[j];
                } else {
                    const pk_d2* sl = store + (size_t)dop.z * U * 128;
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const pk_d2 lo = sl[u * 128], hi = sl[u * 128 + 64];
                        av[u][0] = lo.x; av[u][1] = lo.y; av[u][2] = hi.x; av[u][3] = hi.y;
                    }
                }
                const double* Mi = P + (size_t)i * 32;
                double x[2][U][4], gg[2][U][4];             // the children's partials; g of the left branch = outer partial x right
                ptg_child<U, CODED>(a, dop.x, store, sc, x[0]);
                ptg_child<U, CODED>(a, dop.y, store, sc, x[1]);
                {
                    double ml[16], mr[16];
                    pt2_uniform16(Mi, ml);
                    pt2_uniform16(Mi + 16, mr);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        double el[4], er[4];                // the messages again: the chain of the upward pass
                        pt2_row_times(x[0][u], ml, el);
                        pt2_row_times(x[1][u], mr, er);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            gg[0][u][j] = av[u][j] * er[j];
                            gg[1][u][j] = av[u][j] * el[j];
                        }
                    }
                }
#pragma unroll
                for (int sd = 0; sd < 2; ++sd) {
                    const int src = sd ? dop.y : dop.x;
                    if constexpr (GRAD) {
                        double d[16];
                        pt2_uniform16(Mi + g.mat_plane + sd * 16, d);
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const double r1 = ptg_xDg(x[sd][u], d, gg[sd][u]) * inv[u];
                            const double tot = pk_wave_tree_sum(live[u] ? r1 : 0.0);
                            if (lane == 0) acc[2 * i + sd] = acc[2 * i + sd] + tot;
                        }
                    }
                    const double* Db = Dt + ((size_t)i * 2 + sd) * NP * 16;
#pragma unroll 1
                    for (int p = 0; p < NP; ++p) {          // one D at a time: 32 scalar registers
                        double d[16];
                        pt2_uniform16(Db + (size_t)p * 16, d);
                        double part = 0.0;
#pragma unroll
                        for (int u = 0; u < U; ++u) part = part + (live[u] ? ptg_xDg(x[sd][u], d, gg[sd][u]) * inv[u] : 0.0);
                        dth[p * 64] = dth[p * 64] + part;
                    }
                    if (src < 0) {                          // wave-uniform: the child's outer partial takes the child's slot
                        double mm[16];
                        pt2_uniform16(Mi + sd * 16, mm);
                        pk_d2* dst = store + (size_t)(~src) * U * 128;
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
        }
        const double t = pk_wave_tree_sum(pm_lp_finish(col));
        if (lane == 0) a.tilev[item] = t;                   // [tree][tile]
        __syncthreads();                                    // lane 0's sums, read by every lane
        if constexpr (GRAD) {
            double* out = g.dtile + (size_t)item * 2 * R;
            for (int j = lane; j < 2 * R; j += 64) out[j] = acc[j];
        }
        double* mo = m.mtile + (size_t)item * (NP + 4);
#pragma unroll 1
        for (int p = 0; p < NP; ++p) {
            const double tot = pk_wave_tree_sum(dth[p * 64]);
            if (lane == 0) mo[p] = tot;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double tot = pk_wave_tree_sum(dp[j]);
            if (lane == 0) mo[NP + j] = tot;
        }
        __syncthreads();                                    // ... before the next item clears them
    }
}

// Per (tree, model sum): the tiles added left to right.  A tree whose log-likelihood is not finite gets NaN in every entry (one
// with a site factor below PTG_LIK_FLOOR already carries it).  dtheta [trees][P], dprior [trees][4].
__global__ __launch_bounds__(256) void ptm_finish(const double* __restrict__ mtile, const double* __restrict__ loglik, int ntiles, int trees, int P,
                                                  double* __restrict__ dtheta, double* __restrict__ dprior) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = P + 4;
    if (idx >= trees * per) return;
    const long tree = idx / per;
    const int q = (int)(idx - tree * per);
    const double* tv = mtile + (size_t)tree * ntiles * per + q;
    double tot = tv[0];
    for (int i = 1; i < ntiles; ++i) tot = tot + tv[(size_t)i * per];
    const double ll = loglik[tree];
    if (pm_isnan(ll) || ll == pm_inf() || ll == -pm_inf()) tot = pm_nan();
    if (q < P) dtheta[tree * P + q] = tot;
    else dprior[tree * 4 + (q - P)] = tot;
}

template <bool CODED, bool GRAD>
inline void ptm_launch_as(const ptm_args& m, int grid, hipStream_t s) {
    const size_t lds = ptm_lds_bytes(m.g.a.N, m.g.depth, m.P, GRAD);
    hipLaunchKernelGGL((ptm_updown<PTG_U, CODED, GRAD>), dim3((unsigned)grid), dim3(64), lds, s, m);
}
inline void ptm_launch(const ptm_args& m, int grid, bool coded, bool grad, hipStream_t s) {
    if (coded) {
        if (grad) ptm_launch_as<true, true>(m, grid, s);
        else ptm_launch_as<true, false>(m, grid, s);
    } else {
        if (grad) ptm_launch_as<false, true>(m, grid, s);
        else ptm_launch_as<false, false>(m, grid, s);
    }
}
#endif  // __HIPCC__
