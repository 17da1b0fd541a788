// phylo_treegrad.h -- phylo_trees_grad: the derivatives of the log-likelihood of MANY explicit trees with respect to each of their
// 2 (N-1) branch lengths, and their own second derivatives.  Host: the plan of a call (chunk of trees, slab
// layout, capped grid) and the downward operations of a scheduled tree; device: ptg_dmats (M' = M Q, M'' = M' Q), ptg_updown (the
// upward pass of pt2_prune with every internal node's partial kept in a node store in device memory, then the schedule walked in
// reverse with the outer partials) and ptg_finish (tiles added left to right, rows back in the caller's order).  A sibling of
// phylo_treeset.h: pt2_prune and pt2_prune_rates keep their code objects.  The downward pass follows the contract's order of
// operations term by term, without fma, so that a plain restatement (tests/treegrad_ref.py) gives every site's terms bit for bit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "phylo_treeset_plan.h"

#define PTG_U 2                                   // site steps per pass: an operation of the downward pass holds the outer partial, two messages and two g
#define PTG_SLOT_BYTES 2048                       // one node of one site step: 64 lanes x 4 doubles (PT2_SLOT_BYTES)
#define PTG_CHUNK_BYTES ((size_t)64 << 20)        // device scratch of one chunk of trees, the node store apart
#define PTG_STORE_BYTES ((size_t)256 << 20)       // the node stores of all resident workgroups
#define PTG_WG_PER_CU 8                           // workgroups (= waves) per compute unit the grid is capped at
#define PTG_LIK_FLOOR 0x1p-1020                   // a site factor below this (or not finite) has no usable reciprocal: NaN derivatives

// ------------------------------------------------------------------------------------------------
// host: the plan of one call -- no HIP, so that a plain host program can run it under sanitizers (tests/treegrad_asan_main.cpp)
// ------------------------------------------------------------------------------------------------
struct ptg_plan {
    int chunk = 0;                 // trees per chunk
    int grid = 0;                  // workgroups of ptg_updown for a full chunk (a shorter last chunk launches min(grid, its items))
    int nq = 1;                    // 1: gradient; 2: gradient and curvature
    size_t per_tree = 0, wg_store = 0;
    // byte offsets into the slab (all multiples of 256)
    size_t o_prior = 0, o_ops = 0, o_dops = 0, o_P = 0, o_t = 0, o_gap = 0, o_tilev = 0, o_out = 0, o_dtile = 0, o_dout = 0, o_store = 0, total = 0;
};

// the slab in slab order: prior | ops | downward ops | M, M', M'' | lengths | gap rows of M | tile values | loglik | derivative tiles | derivatives
inline int ptg_regions(int N, int ntiles, bool coded, ptg_plan& q, pts_region* r) {
    const size_t R = (size_t)N - 1, nt = (size_t)ntiles, nq = (size_t)q.nq;
    int k = 0;
    r[k++] = {PTS_FIXED, 32, true, &q.o_prior};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_ops};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_dops};
    r[k++] = {PTS_TREE, 3 * R * 256, true, &q.o_P};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_t};
    r[k++] = {PTS_TREE, R * 64, coded, &q.o_gap};
    r[k++] = {PTS_TREE, nt * 8, true, &q.o_tilev};
    r[k++] = {PTS_TREE, 8, true, &q.o_out};
    r[k++] = {PTS_TREE, nt * nq * 2 * R * 8, true, &q.o_dtile};
    r[k++] = {PTS_TREE, nq * 2 * R * 8, true, &q.o_dout};
    return k;
}

// What every plan with a node store does once its regions are stated: bytes per tree, chunk, grid, offsets, total.  P: a plan struct
// with chunk, grid, per_tree, wg_store, o_store, total; out_region / out_tree: the staging of the ancestral calls, else 0.
template <class P>
inline void ptg_finish_plan(P& q, const pts_region* r, int nr, int ntiles, int T, int n_cus, int env_chunk, size_t out_region, size_t out_tree) {
    q.per_tree = pts_sum(r, nr, PTS_TREE);
    q.chunk = pts_chunk(q.per_tree, ntiles, T, env_chunk, PTG_CHUNK_BYTES, out_region, out_tree);
    q.grid = pts_grid((size_t)q.chunk * (size_t)ntiles, q.wg_store, n_cus, PTG_STORE_BYTES, PTG_WG_PER_CU);
    q.total = pts_lay_out(r, nr, (size_t)q.chunk, (size_t)q.grid * q.wg_store, &q.o_store);
}

// the same plan as pts_check_plan wants to see it
template <class P>
inline pts_plan_facts ptg_plan_facts(const P& q, int ntiles, int T, int n_cus, int env_chunk, size_t out_region) {
    return {q.chunk, q.grid, q.per_tree, q.wg_store, q.o_store, q.total, ntiles, T, n_cus, env_chunk, PTG_CHUNK_BYTES, PTG_STORE_BYTES, PTG_WG_PER_CU,
            out_region};
}

// 0: fine.  T trees of N taxa, ntiles site tiles, n_cus compute units; env_chunk > 0 caps the chunk (PHYLO_TREES_CHUNK).
inline int ptg_make_plan(int N, int ntiles, int T, bool coded, bool curv, int n_cus, int env_chunk, ptg_plan* p) {
    if (N < 2 || ntiles < 1 || T < 1 || n_cus < 1) return 1;
    ptg_plan q;
    q.nq = curv ? 2 : 1;
    q.wg_store = ((size_t)N - 1) * PTG_U * PTG_SLOT_BYTES;
    pts_region r[PTS_MAX_REGIONS];
    ptg_finish_plan(q, r, ptg_regions(N, ntiles, coded, q, r), ntiles, T, n_cus, env_chunk, 0, 0);
    *p = q;
    return 0;
}

// The downward operations of a checked tree whose schedule is ops (pt2_schedule): dops[i] = {left, right, row, 0} of operation i,
// a child >= 0 a leaf, a child < 0 the ROW ~child of an internal child (the node store is indexed by row, the LDS stack of the
// upward pass by slot).  0: fine; 1: ops and child do not fit one another (never, after pt2_check_tree and pt2_schedule).
inline int ptg_down_ops(int N, const int32_t* child, const int32_t* ops, int32_t* dops) {
    const int R = N - 1;
    for (int i = 0; i < R; ++i) {
        const int row = ops[4 * i + 3];
        if (row < 0 || row >= R || (i == R - 1 && row != R - 1)) return 1;
        for (int sd = 0; sd < 2; ++sd) {
            const int ch = child[2 * row + sd];
            if (ch < 0 || ch >= N + row) return 1;
            if ((ch < N) != (ops[4 * i + 1 + sd] >= 0)) return 1;
            dops[4 * i + sd] = ch < N ? ch : ~(ch - N);
        }
        dops[4 * i + 2] = row;
        dops[4 * i + 3] = 0;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "phylo_treeset.h"

// M' = M Q and M'' = M' Q, one thread per matrix entry (k, j): M'[k][j] = ((M[k][0] Q[0][j] + M[k][1] Q[1][j]) + M[k][2] Q[2][j]) +
// M[k][3] Q[3][j], every product and sum rounded on its own (no fma: a plain restatement reproduces the bits); M''[k][j] is the
// same sum over row k of M', which the thread computes for itself.  jc: the generator pm_jc69 implies (1/4, diagonal -3/4).
__global__ __launch_bounds__(256) void ptg_dmats(const double* __restrict__ Q, int jc, const double* __restrict__ M, long n_mat,
                                                 double* __restrict__ M1, double* __restrict__ M2) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_mat * 16) return;
    const double* m = M + (t >> 4) * 16 + ((t >> 2) & 3) * 4;
    const int j = (int)(t & 3);
    double q[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) q[e] = jc ? (e % 5 == 0 ? -0.75 : 0.25) : Q[e];
    double r1[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) r1[jj] = ((m[0] * q[jj] + m[1] * q[4 + jj]) + m[2] * q[8 + jj]) + m[3] * q[12 + jj];
    M1[t] = r1[j];
    M2[t] = ((r1[0] * q[j] + r1[1] * q[4 + j]) + r1[2] * q[8 + j]) + r1[3] * q[12 + j];
}

struct ptg_args {
    pt2_args a;                      // ops, P (M), gap (of M), leaves, codes, prior, tilev, N, S, T, ntiles as pt2_prune takes them (site_lik unused)
    const int32_t* dops;             // [trees][N-1][4] downward operations (ptg_down_ops)
    double* dtile;                   // [trees][ntiles][nq][2 (N-1)] per-branch tile sums, in schedule order
    pk_d2* store;                    // [grid][N-1][U][2][64] node stores
    long mat_plane;                  // doubles from M to M' (and from M' to M'')
    int n_items, depth;
};

// The partial of one child for the wave's U site steps: a coded leaf's indicator row (code 4, a gap: all ones), a generic leaf's
// resident row, an internal child's entry of the node store.  src is wave-uniform.
template <int U, bool CODED>
__device__ __forceinline__ void ptg_child(const pt2_args& a, int src, const pk_d2* store, const unsigned int (&sc)[U], double (&x)[U][4]) {
    if (src >= 0) {
        if constexpr (CODED) {
            const uint8_t* cd = a.codes + (size_t)src * a.S;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned int c = *(pk_gu8c*)(cd + sc[u]);
#pragma unroll
                for (int k = 0; k < 4; ++k) x[u][k] = (c == (unsigned int)k || c >= 4u) ? 1.0 : 0.0;
            }
        } else {
            const double* rows = a.leaves + (size_t)src * a.S * 4;
#pragma unroll
            for (int u = 0; u < U; ++u) pk_load4(rows + (size_t)sc[u] * 4, x[u]);
        }
    } else {
        const pk_d2* sl = store + (size_t)(~src) * U * 128;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const pk_d2 lo = sl[u * 128], hi = sl[u * 128 + 64];
            x[u][0] = lo.x; x[u][1] = lo.y; x[u][2] = hi.x; x[u][3] = hi.y;
        }
    }
}

// sum_k x[k] sum_j D[k][j] g[j] in the contract's order: j ascending inside, k ascending outside, every product and sum rounded on
// its own (a plain restatement reproduces the bits).  D wave-uniform.
__device__ __forceinline__ double ptg_xDg(const double (&x)[4], const double (&D)[16], const double (&g)[4]) {
    double t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = ((D[4 * k] * g[0] + D[4 * k + 1] * g[1]) + D[4 * k + 2] * g[2]) + D[4 * k + 3] * g[3];
    return ((x[0] * t[0] + x[1] * t[1]) + x[2] * t[2]) + x[3] * t[3];
}

// One wave (= one workgroup) per work item (tree, site tile), lane = column; workgroup w takes items w, w + grid, ...  Per strip
// of 64 U sites: the upward pass of pt2_prune (same schedule, same LDS stack, same chains: the root and the site factor are its
// bits) with every non-root node also stored to the workgroup's node store [row][site step][half][lane]; then the schedule in
// reverse: the outer partial of the node (the prior at the root, else what its parent left in the node's slot), both children's
// partials (ptg_child) and both messages again (the upward chain), g, and per branch L' / L (and L'' / L - (L' / L)^2) in the
// contract's order (ptg_xDg; M' and M'' wave-uniform; 1 / L is NaN where L lies below PTG_LIK_FLOOR or is not finite), reduced
// over the wave by pk_wave_tree_sum and added by lane 0 into its
// entry of the LDS array acc[nq][2 (N-1)]; the outer partial of an internal child overwrites the child's partial.  A lane only
// ever touches its own column of the store, and lane 0 alone the array: neither needs a fence inside an item.
// Launched with depth * U * 2048 + nq * 2 (N-1) * 8 bytes of dynamic LDS.
template <int U, bool CODED, bool CURV>
__global__ __launch_bounds__(64) void ptg_updown(const ptg_args g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ptg_lds[];
    constexpr int NQ = CURV ? 2 : 1;
    const pt2_args& a = g.a;
    pk_d2* stack = reinterpret_cast<pk_d2*>(ptg_lds);
    double* acc = reinterpret_cast<double*>(ptg_lds + (size_t)g.depth * U * PT2_SLOT_BYTES);
    const int lane = threadIdx.x;
    const int R = a.N - 1;
    pk_d2* store = g.store + (size_t)blockIdx.x * R * U * 128 + lane;
#pragma unroll 1
    for (int item = blockIdx.x; item < g.n_items; item += gridDim.x) {     // item: wave-uniform
        const int tree = item / a.ntiles, tile = item - tree * a.ntiles;
        const int s0 = tile * a.T, s1 = s0 + a.T < a.S ? s0 + a.T : a.S;
        pt2_ci4* ops = (pt2_ci4*)(a.ops + (size_t)tree * R * 4);
        pt2_ci4* dops = (pt2_ci4*)(g.dops + (size_t)tree * R * 4);
        const double* P = a.P + (size_t)tree * R * 32;
        const double* G = CODED ? a.gap + (size_t)tree * R * 8 : nullptr;
        for (int j = lane; j < NQ * 2 * R; j += 64) acc[j] = 0.0;
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
                    // below the floor 1 / lik overflows (lik < 2^-1024) or is made from a subnormal's few bits: NaN, which the
                    // wave reduction carries into every sum of the tile and ptg_finish into every entry of the tree
                    inv[u] = lik >= PTG_LIK_FLOOR && lik < pm_inf() ? 1.0 / lik : pm_nan();
                    if (s < s1) pm_lp_mul(col, lik);
                }
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
                ptg_child<U, CODED>(a, dop.x, store, sc, x[0]);     // message, and the reverse
                ptg_child<U, CODED>(a, dop.y, store, sc, x[1]);
                {
                    double ml[16], mr[16];
                    pt2_uniform16(Mi, ml);
                    pt2_uniform16(Mi + 16, mr);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        double el[4], er[4];                // the messages again: the chain of the upward pass (a coded leaf's
                        pt2_row_times(x[0][u], ml, el);     // table row IS this chain over its indicator row)
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
                    double r1[U];
                    {
                        double d[16];
                        pt2_uniform16(Mi + g.mat_plane + sd * 16, d);
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            r1[u] = ptg_xDg(x[sd][u], d, gg[sd][u]) * inv[u];
                            const double tot = pk_wave_tree_sum(live[u] ? r1[u] : 0.0);
                            if (lane == 0) acc[2 * i + sd] = acc[2 * i + sd] + tot;
                        }
                    }
                    if constexpr (CURV) {
                        double d[16];
                        pt2_uniform16(Mi + 2 * g.mat_plane + sd * 16, d);
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const double c = ptg_xDg(x[sd][u], d, gg[sd][u]) * inv[u] - r1[u] * r1[u];
                            const double tot = pk_wave_tree_sum(live[u] ? c : 0.0);
                            if (lane == 0) acc[2 * R + 2 * i + sd] = acc[2 * R + 2 * i + sd] + tot;
                        }
                    }
                    if (src < 0) {                          // wave-uniform: the child's outer partial takes the child's slot
                        double m[16];
                        pt2_uniform16(Mi + sd * 16, m);
                        pk_d2* dst = store + (size_t)(~src) * U * 128;
#pragma unroll
                        for (int u = 0; u < U; ++u) {
                            const double (&q)[4] = gg[sd][u];
                            double ac[4];
#pragma unroll
                            for (int k = 0; k < 4; ++k) ac[k] = ((m[4 * k] * q[0] + m[4 * k + 1] * q[1]) + m[4 * k + 2] * q[2]) + m[4 * k + 3] * q[3];
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
        double* out = g.dtile + (size_t)item * NQ * 2 * R;
        for (int j = lane; j < NQ * 2 * R; j += 64) out[j] = acc[j];
        __syncthreads();                                    // ... before the next item clears them
    }
}

// Per (tree, quantity, branch of the schedule): the tiles added left to right; written to the caller's row (op.w) and side.  A tree
// whose log-likelihood is not finite gets NaN in every entry (one with a site factor below PTG_LIK_FLOOR already carries it).
// out [nq][trees][N-1][2].
__global__ __launch_bounds__(256) void ptg_finish(const double* __restrict__ dtile, const int32_t* __restrict__ ops, const double* __restrict__ loglik,
                                                  int ntiles, int trees, int R, int nq, double* __restrict__ out) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long per = (long)nq * 2 * R;
    if (idx >= trees * per) return;
    const long tree = idx / per, rem = idx - tree * per;
    const int q = (int)(rem / (2 * R)), b = (int)(rem - (long)q * 2 * R);
    const double* tv = dtile + (size_t)tree * ntiles * per + rem;
    double tot = tv[0];
    for (int i = 1; i < ntiles; ++i) tot = tot + tv[(size_t)i * per];
    const double ll = loglik[tree];
    if (pm_isnan(ll) || ll == pm_inf() || ll == -pm_inf()) tot = pm_nan();
    const int row = ops[((size_t)tree * R + (b >> 1)) * 4 + 3];
    out[((size_t)q * trees + tree) * 2 * R + 2 * row + (b & 1)] = tot;
}

template <bool CODED, bool CURV>
inline void ptg_launch_as(const ptg_args& g, int grid, hipStream_t s) {
    const size_t lds = (size_t)g.depth * PTG_U * PT2_SLOT_BYTES + (size_t)(CURV ? 2 : 1) * 2 * (g.a.N - 1) * 8;
    hipLaunchKernelGGL((ptg_updown<PTG_U, CODED, CURV>), dim3((unsigned)grid), dim3(64), lds, s, g);
}
inline void ptg_launch(const ptg_args& g, int grid, bool coded, bool curv, hipStream_t s) {
    if (coded) {
        if (curv) ptg_launch_as<true, true>(g, grid, s);
        else ptg_launch_as<true, false>(g, grid, s);
    } else {
        if (curv) ptg_launch_as<false, true>(g, grid, s);
        else ptg_launch_as<false, false>(g, grid, s);
    }
}
#endif  // __HIPCC__
