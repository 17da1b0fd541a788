// phylo_treeanc_rates.h -- phylo_trees_ancestral_rates: the marginal posterior of every state at every internal node and site of
// MANY explicit trees under a mixture of C rate categories, the most probable state and its posterior, and beside them the
// posterior of every category at every site and the posterior mean rate of the site.  Host: the plan of a
// call (chunk of trees, slab layout, staging of the requested outputs, capped grid); device: ptar_updown, a sibling of pta_updown
// and ptgr_updown over the same helpers -- the upward pass of pt2_prune_rates with every category's nodes kept in its own plane of
// the node store, then the schedule in reverse with the categories innermost per operation, so that the sum over the categories is
// complete inside a node before it is multiplied by 1 / m.  No M', no M'', no sum over sites: no LDS beyond the stack, no barrier.
// pta_updown, ptgr_updown and their siblings keep their code objects.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "phylo_treeanc.h"
#include "phylo_treegrad_rates.h"

#define PTAR_POST PTA_POST                        // bits of `outs`: the first three are phylo_trees_ancestral's
#define PTAR_STATE PTA_STATE
#define PTAR_PMAX PTA_PMAX
#define PTAR_CATPOST 8u
#define PTAR_SITERATE 16u
#define PTAR_ALL 31u

// ------------------------------------------------------------------------------------------------
// host: the plan of one call -- no HIP, so that a plain host program can run it under sanitizers (tests/treeanc_rates_asan_main.cpp)
// ------------------------------------------------------------------------------------------------
struct ptar_plan {
    int chunk = 0;                 // trees per chunk: the smallest of what the slab holds, what the staging holds and the caller's cap
    int grid = 0;                  // workgroups of ptar_updown for a full chunk (ptgr_make_plan's cap)
    int ncoef = 0;                 // doubles of a tree's coefficient block: w | r
    size_t per_tree = 0, wg_store = 0;
    size_t out_tree = 0;           // bytes of the requested outputs of one tree: R S (32 + 1 + 8) + S (8 C + 8) over those asked for
    size_t out_region = 0;         // bytes of the staging region: PTA_OUT_BYTES, or out_tree where that is more
    // byte offsets into the slab (all multiples of 256)
    size_t o_prior = 0, o_coef = 0, o_ops = 0, o_dops = 0, o_P = 0, o_t = 0, o_gap = 0, o_tilev = 0, o_out = 0, o_post = 0, o_state = 0,
           o_pmax = 0, o_cat = 0, o_rate = 0, o_store = 0, total = 0;
};

// the slab in slab order: prior | coefficients | ops | downward ops | per category: M, lengths, gap rows of M | tile values | loglik |
// staging of post, state, pmax, catpost, siterate
inline int ptar_regions(int N, int S, int ntiles, int C, bool coded, unsigned outs, ptar_plan& q, pts_region* r) {
    const size_t R = (size_t)N - 1, nt = (size_t)ntiles, nc = (size_t)C, cells = R * (size_t)S;
    int k = 0;
    r[k++] = {PTS_FIXED, 32, true, &q.o_prior};
    r[k++] = {PTS_TREE, (size_t)q.ncoef * 8, true, &q.o_coef};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_ops};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_dops};
    r[k++] = {PTS_TREE, nc * R * 256, true, &q.o_P};
    r[k++] = {PTS_TREE, nc * R * 16, true, &q.o_t};
    r[k++] = {PTS_TREE, nc * R * 64, coded, &q.o_gap};
    r[k++] = {PTS_TREE, nt * 8, true, &q.o_tilev};
    r[k++] = {PTS_TREE, 8, true, &q.o_out};
    r[k++] = {PTS_STAGED, cells * 32, (outs & PTAR_POST) != 0, &q.o_post};
    r[k++] = {PTS_STAGED, cells, (outs & PTAR_STATE) != 0, &q.o_state};
    r[k++] = {PTS_STAGED, cells * 8, (outs & PTAR_PMAX) != 0, &q.o_pmax};
    r[k++] = {PTS_STAGED, nc * (size_t)S * 8, (outs & PTAR_CATPOST) != 0, &q.o_cat};
    r[k++] = {PTS_STAGED, (size_t)S * 8, (outs & PTAR_SITERATE) != 0, &q.o_rate};
    return k;
}

// 0: fine; 1: no plan for these numbers; 2: one tree's outputs exceed PTA_OUT_MAX (p->out_tree says by how much).
// T trees of N taxa and S sites in ntiles site tiles under C categories; outs: which outputs are asked for; env_chunk > 0 caps the chunk.
inline int ptar_make_plan(int N, int S, int ntiles, int T, int C, bool coded, unsigned outs, int n_cus, int env_chunk, ptar_plan* p) {
    if (N < 2 || S < 1 || ntiles < 1 || T < 1 || n_cus < 1 || C < 1 || C > PTGR_MAX_CATS || !(outs & PTAR_ALL) || (outs & ~PTAR_ALL)) return 1;
    ptar_plan q;
    q.ncoef = 2 * C;
    pts_region r[PTS_MAX_REGIONS];
    const int nr = ptar_regions(N, S, ntiles, C, coded, outs, q, r);
    q.per_tree = pts_sum(r, nr, PTS_TREE);
    q.out_tree = pts_sum(r, nr, PTS_STAGED);
    if (q.out_tree > PTA_OUT_MAX) {
        *p = q;
        return 2;
    }
    q.out_region = q.out_tree > PTA_OUT_BYTES ? q.out_tree : PTA_OUT_BYTES;
    q.wg_store = (size_t)C * ((size_t)N - 1) * PTG_U * PTG_SLOT_BYTES;
    ptg_finish_plan(q, r, nr, ntiles, T, n_cus, env_chunk, q.out_region, q.out_tree);
    *p = q;
    return 0;
}

// A tree's coefficient block: w | r
inline void ptar_coefficients(int C, const double* rate, const double* weight, double* coef) {
    for (int k = 0; k < C; ++k) {
        coef[k] = weight[k];
        coef[C + k] = rate[k];
    }
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

struct ptar_args {
    pt2_args a;                      // ops, leaves, codes, prior, tilev, N, S, T, ntiles as pt2_prune takes them; P [trees][C][N-1][2][16] (M),
                                     // gap [trees][C][N-1][2][4]; site_lik unused
    const int32_t* dops;             // [trees][N-1][4] downward operations (ptg_down_ops)
    const double* coef;              // [trees][2 C] w | r: indexed by tree, so a mixture per tree costs nothing
    pk_d2* store;                    // [grid][C][N-1][U][2][64] node stores
    double* post;                    // [trees][N-1][S][4] or NULL   (rows in the caller's order: the row of an operation is dop.z)
    uint8_t* state;                  // [trees][N-1][S] or NULL
    double* pmax;                    // [trees][N-1][S] or NULL
    double* catpost;                 // [trees][C][S] or NULL
    double* siterate;                // [trees][S] or NULL
    int n_items, depth, C;
};

// One wave (= one workgroup) per work item (tree, site tile), lane = column; workgroup w takes items w, w + grid, ...  Per strip of
// 64 U sites the upward pass, the node store's planes and 1 / m are ptgr_updown's line by line (the tile value is
// pt2_prune_rates' bits).  Then the schedule in reverse, and per operation the categories in ascending order: the outer partial of
// the node in category c (the prior at the root, else what its parent left in the node's slot of plane c), both children's
// partials and both messages again (the upward chain), and
//     q[j] = abar_c[j] * (msg_l,c[j] * msg_r,c[j]);   acc[j] = acc[j] + w_c * q[j]   from +0.0, product and sum rounded on their own
// the child's outer partial takes the child's slot of plane c.  After the last category
//     post[j] = acc[j] * inv        not renormalised;  state and pmax by pta_updown's rule from those bits
// written for live lanes only, with pta_updown's stores.  At the root operation f_c is made again from the root's two messages (as
// ptgr_updown's PARAMS form does) and
//     catpost_c = (w_c * f_c) * inv      one contiguous 512-byte store per wave and category
//     e = e + r_c * catpost_c            from +0.0: the posterior mean rate of the site, written after the last category
// 1 / m is NaN where m lies below PTG_LIK_FLOOR or is not finite: that site's column is NaN / PTA_NOSTATE in every output, and no
// other site sees it.  Which outputs exist is a wave-uniform kernel argument.  The coefficient block is read through the constant
// address space.  Launched with depth * U * 2048 bytes of dynamic LDS (the stack; a lane only ever touches its own column: no
// barrier).
template <int U, bool CODED>
__global__ __launch_bounds__(64) void ptar_updown(const ptar_args g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ptar_lds[];
    const pt2_args& a = g.a;
    pk_d2* stack = reinterpret_cast<pk_d2*>(ptar_lds);
    const int lane = threadIdx.x;
    const int R = a.N - 1, C = g.C;
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
        pt2_cd* cf = (pt2_cd*)(g.coef + (size_t)tree * 2 * C);
        pt2_cd* prc = (pt2_cd*)a.prior;
        pm_lp col = pm_lp_init();
#pragma unroll 1
        for (int base = s0; base < s1; base += 64 * U) {   // base: wave-uniform
            unsigned int sc[U];                             // a site past the end re-reads the last one; it writes nothing
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
                    inv[u] = m[u] >= PTG_LIK_FLOOR && m[u] < pm_inf() ? 1.0 / m[u] : pm_nan();     // ptgr_updown's rule
                    if (s < s1) pm_lp_mul(col, m[u]);
                }
            }
#pragma unroll 1
            for (int i = R - 1; i >= 0; --i) {              // downward
                const pt2_i4 dop = dops[i];                 // x, y: left and right child; z: the node's row
                double acc[U][4], e[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    e[u] = 0.0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[u][j] = 0.0;
                }
#pragma unroll 1
                for (int c = 0; c < C; ++c) {
                    pk_d2* pl = store + (size_t)c * plane;
                    const double* Mi = Pt + ((size_t)c * R + i) * 32;
                    const double w = cf[c];
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
                            double el[4], er[4], xv[4];     // the messages again: the chain of the upward pass
                            pt2_row_times(x[0][u], ml, el);
                            pt2_row_times(x[1][u], mr, er);
#pragma unroll
                            for (int j = 0; j < 4; ++j) {
                                gg[0][u][j] = av[u][j] * er[j];
                                gg[1][u][j] = av[u][j] * el[j];
                                xv[j] = el[j] * er[j];
                                const double q = av[u][j] * xv[j];
                                const double wq = w * q;
                                acc[u][j] = acc[u][j] + wq;
                            }
                            if (i == R - 1 && (g.catpost || g.siterate)) {     // wave-uniform: f_c again, from the root's two messages
                                const double pr[4] = {prc[0], prc[1], prc[2], prc[3]};
                                const double wf = w * pk_site_lik(pr, xv);
                                const double cp = wf * inv[u];
                                const double rc = cf[C + c] * cp;
                                e[u] = e[u] + rc;
                                if (g.catpost && live[u])
                                    g.catpost[((size_t)tree * C + c) * (size_t)a.S + (size_t)(base + 64 * u + lane)] = cp;
                            }
                        }
                    }
#pragma unroll
                    for (int sd = 0; sd < 2; ++sd) {
                        const int src = sd ? dop.y : dop.x;
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
                const size_t cell0 = ((size_t)tree * R + (size_t)dop.z) * (size_t)a.S;    // the node's row of the outputs
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (!live[u]) continue;                 // a site past the tile's end writes nothing
                    const size_t site = (size_t)(base + 64 * u + lane);
                    const size_t cell = cell0 + site;
                    double po[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) po[j] = acc[u][j] * inv[u];
                    if (g.post) {                           // wave-uniform
                        pk_d2* pp = (pk_d2*)(g.post + cell * 4);
                        const pk_d2 lo = {po[0], po[1]}, hi = {po[2], po[3]};
                        pp[0] = lo;
                        pp[1] = hi;
                    }
                    if (g.state || g.pmax) {                // wave-uniform
                        const bool nan = pm_isnan(po[0]) || pm_isnan(po[1]) || pm_isnan(po[2]) || pm_isnan(po[3]);
                        int best = 0;
                        double pb = po[0];
#pragma unroll
                        for (int j = 1; j < 4; ++j)
                            if (po[j] > pb) {               // strictly larger: the lowest j among equals
                                pb = po[j];
                                best = j;
                            }
                        if (g.state) g.state[cell] = (uint8_t)(nan ? PTA_NOSTATE : best);
                        if (g.pmax) g.pmax[cell] = nan ? pm_nan() : pb;
                    }
                    if (i == R - 1 && g.siterate) g.siterate[(size_t)tree * (size_t)a.S + site] = e[u];     // wave-uniform
                }
            }
        }
        const double t = pk_wave_tree_sum(pm_lp_finish(col));
        if (lane == 0) a.tilev[item] = t;                   // [tree][tile]
    }
}

template <bool CODED>
inline void ptar_launch_as(const ptar_args& g, int grid, hipStream_t s) {
    hipLaunchKernelGGL((ptar_updown<PTG_U, CODED>), dim3((unsigned)grid), dim3(64), (size_t)g.depth * PTG_U * PT2_SLOT_BYTES, s, g);
}
inline void ptar_launch(const ptar_args& g, int grid, bool coded, hipStream_t s) {
    if (coded) ptar_launch_as<true>(g, grid, s);
    else ptar_launch_as<false>(g, grid, s);
}
#endif  // __HIPCC__
