// phylo_treeanc.h -- phylo_trees_ancestral: the marginal posterior of every state at every internal node and site of MANY explicit
// trees, the most probable state and its posterior.  Host: the plan of a call (chunk of trees, slab layout,
// staging of the requested outputs, capped grid); device: pta_updown, a sibling of ptg_updown over the same helpers -- the upward
// pass with every node kept, then the schedule in reverse with the outer partials, and per node the three products of the contract
// written straight to the staging region.  No sum over sites: no wave reduction, no LDS beyond the stack.  ptg_updown and its
// siblings keep their code objects.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "phylo_treegrad.h"

#define PTA_NOSTATE 255                           // PHYLO_ANC_NOSTATE: a site without a most probable state
#define PTA_OUT_BYTES ((size_t)256 << 20)         // staging of a chunk's requested outputs; grows to one tree's need
#define PTA_OUT_MAX ((size_t)1 << 30)             // a single tree that needs more is refused
#define PTA_POST 1u                               // bits of `outs`
#define PTA_STATE 2u
#define PTA_PMAX 4u

// ------------------------------------------------------------------------------------------------
// host: the plan of one call -- no HIP, so that a plain host program can run it under sanitizers (tests/treeanc_asan_main.cpp)
// ------------------------------------------------------------------------------------------------
struct pta_plan {
    int chunk = 0;                 // trees per chunk: the smallest of what the slab holds, what the staging holds and the caller's cap
    int grid = 0;                  // workgroups of pta_updown for a full chunk (ptg_make_plan's cap)
    size_t per_tree = 0, wg_store = 0;
    size_t out_tree = 0;           // bytes of the requested outputs of one tree: R S (32 + 1 + 8) over those asked for
    size_t out_region = 0;         // bytes of the staging region: PTA_OUT_BYTES, or out_tree where that is more
    // byte offsets into the slab (all multiples of 256)
    size_t o_prior = 0, o_ops = 0, o_dops = 0, o_P = 0, o_t = 0, o_gap = 0, o_tilev = 0, o_out = 0, o_post = 0, o_state = 0, o_pmax = 0,
           o_store = 0, total = 0;
};

// the slab in slab order: prior | ops | downward ops | M | lengths | gap rows of M | tile values | loglik | staging of post, state, pmax
inline int pta_regions(int N, int S, int ntiles, bool coded, unsigned outs, pta_plan& q, pts_region* r) {
    const size_t R = (size_t)N - 1, nt = (size_t)ntiles, cells = R * (size_t)S;
    int k = 0;
    r[k++] = {PTS_FIXED, 32, true, &q.o_prior};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_ops};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_dops};
    r[k++] = {PTS_TREE, R * 256, true, &q.o_P};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_t};
    r[k++] = {PTS_TREE, R * 64, coded, &q.o_gap};
    r[k++] = {PTS_TREE, nt * 8, true, &q.o_tilev};
    r[k++] = {PTS_TREE, 8, true, &q.o_out};
    r[k++] = {PTS_STAGED, cells * 32, (outs & PTA_POST) != 0, &q.o_post};
    r[k++] = {PTS_STAGED, cells, (outs & PTA_STATE) != 0, &q.o_state};
    r[k++] = {PTS_STAGED, cells * 8, (outs & PTA_PMAX) != 0, &q.o_pmax};
    return k;
}

// 0: fine; 1: no plan for these numbers; 2: one tree's outputs exceed PTA_OUT_MAX (p->out_tree says by how much).
// T trees of N taxa and S sites in ntiles site tiles; outs: which outputs are asked for; env_chunk > 0 caps the chunk.
inline int pta_make_plan(int N, int S, int ntiles, int T, bool coded, unsigned outs, int n_cus, int env_chunk, pta_plan* p) {
    if (N < 2 || S < 1 || ntiles < 1 || T < 1 || n_cus < 1 || !(outs & 7u) || (outs & ~7u)) return 1;
    pta_plan q;
    pts_region r[PTS_MAX_REGIONS];
    const int nr = pta_regions(N, S, ntiles, coded, outs, q, r);
    q.per_tree = pts_sum(r, nr, PTS_TREE);
    q.out_tree = pts_sum(r, nr, PTS_STAGED);
    if (q.out_tree > PTA_OUT_MAX) {
        *p = q;
        return 2;
    }
    q.out_region = q.out_tree > PTA_OUT_BYTES ? q.out_tree : PTA_OUT_BYTES;
    q.wg_store = ((size_t)N - 1) * PTG_U * PTG_SLOT_BYTES;
    ptg_finish_plan(q, r, nr, ntiles, T, n_cus, env_chunk, q.out_region, q.out_tree);
    *p = q;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

struct pta_args {
    pt2_args a;                      // ops, P (M), gap (of M), leaves, codes, prior, tilev, N, S, T, ntiles as pt2_prune takes them (site_lik unused)
    const int32_t* dops;             // [trees][N-1][4] downward operations (ptg_down_ops)
    pk_d2* store;                    // [grid][N-1][U][2][64] node stores
    double* post;                    // [trees][N-1][S][4] or NULL   (rows in the caller's order: the row of an operation is dop.z)
    uint8_t* state;                  // [trees][N-1][S] or NULL
    double* pmax;                    // [trees][N-1][S] or NULL
    int n_items, depth;
};

// One wave (= one workgroup) per work item (tree, site tile), lane = column; workgroup w takes items w, w + grid, ...  Per strip of
// 64 U sites the upward pass, the node store and 1 / L are ptg_updown's line by line (the root and the site factor are pt2_prune's
// bits).  Then the schedule in reverse: the outer partial of the node (the prior at the root, else what its parent left in the
// node's slot), both children's partials and both messages again (the upward chain), and
//     post[j] = (abar[j] * (msg_l[j] * msg_r[j])) * inv         three products, each rounded on its own; not renormalised
//     state   = the lowest j whose post is the largest of the four; PTA_NOSTATE if any of them is NaN;  pmax = post[state] or NaN
// written for live lanes only: a lane's 32 bytes of post are adjacent, so the wave's two 16-byte stores fill one contiguous 2 KiB;
// state is 64 contiguous bytes per wave and pmax 512.  1 / L is NaN where L lies below PTG_LIK_FLOOR or is not finite: that
// site's column is NaN / PTA_NOSTATE at every node, and no other site sees it.  The outer partial of an internal child overwrites
// the child's partial in the node store, as in ptg_updown.  Which outputs exist is a wave-uniform kernel argument.
// Launched with depth * U * 2048 bytes of dynamic LDS (the stack; a lane only ever touches its own column: no barrier).
template <int U, bool CODED>
__global__ __launch_bounds__(64) void pta_updown(const pta_args g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pta_lds[];
    const pt2_args& a = g.a;
    pk_d2* stack = reinterpret_cast<pk_d2*>(pta_lds);
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
        pm_lp col = pm_lp_init();
#pragma unroll 1
        for (int base = s0; base < s1; base += 64 * U) {   // base: wave-uniform
            unsigned int sc[U];                             // a site past the end re-reads the last one; it writes nothing
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
                ptg_child<U, CODED>(a, dop.x, store, sc, x[0]);
                ptg_child<U, CODED>(a, dop.y, store, sc, x[1]);
                const size_t cell0 = ((size_t)tree * R + (size_t)dop.z) * (size_t)a.S;    // the node's row of the outputs
                {
                    double ml[16], mr[16];
                    pt2_uniform16(Mi, ml);
                    pt2_uniform16(Mi + 16, mr);
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        double el[4], er[4];                // the messages again: the chain of the upward pass
                        pt2_row_times(x[0][u], ml, el);
                        pt2_row_times(x[1][u], mr, er);
                        double po[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            gg[0][u][j] = av[u][j] * er[j];
                            gg[1][u][j] = av[u][j] * el[j];
                            po[j] = (av[u][j] * (el[j] * er[j])) * inv[u];
                        }
                        if (live[u]) {                      // a site past the tile's end writes nothing
                            const size_t cell = cell0 + (size_t)(base + 64 * u + lane);
                            if (g.post) {                   // wave-uniform
                                pk_d2* pp = (pk_d2*)(g.post + cell * 4);
                                const pk_d2 lo = {po[0], po[1]}, hi = {po[2], po[3]};
                                pp[0] = lo;
                                pp[1] = hi;
                            }
                            if (g.state || g.pmax) {        // wave-uniform
                                const bool nan = pm_isnan(po[0]) || pm_isnan(po[1]) || pm_isnan(po[2]) || pm_isnan(po[3]);
                                int best = 0;
                                double pb = po[0];
#pragma unroll
                                for (int j = 1; j < 4; ++j)
                                    if (po[j] > pb) {       // strictly larger: the lowest j among equals
                                        pb = po[j];
                                        best = j;
                                    }
                                if (g.state) g.state[cell] = (uint8_t)(nan ? PTA_NOSTATE : best);
                                if (g.pmax) g.pmax[cell] = nan ? pm_nan() : pb;
                            }
                        }
                    }
                }
#pragma unroll
                for (int sd = 0; sd < 2; ++sd) {
                    const int src = sd ? dop.y : dop.x;
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
    }
}

template <bool CODED>
inline void pta_launch_as(const pta_args& g, int grid, hipStream_t s) {
    hipLaunchKernelGGL((pta_updown<PTG_U, CODED>), dim3((unsigned)grid), dim3(64), (size_t)g.depth * PTG_U * PT2_SLOT_BYTES, s, g);
}
inline void pta_launch(const pta_args& g, int grid, bool coded, hipStream_t s) {
    if (coded) pta_launch_as<true>(g, grid, s);
    else pta_launch_as<false>(g, grid, s);
}
#endif  // __HIPCC__
