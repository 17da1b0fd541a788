// phylo_treenni.h -- phylo_trees_nni: for MANY explicit trees, the change of the log-likelihood under every nearest-neighbour
// interchange (NNI) at the tree's current branch lengths.  Host: the plan of a call (chunk of trees, slab
// layout, capped grid: ptg_make_plan's rules over other per-tree bytes) and, per operation of a schedule, where the operations of
// its children stand; device: ptn_updown (ptg_updown's upward pass and outer-partial recursion, nothing of its derivatives, and at
// the operation of a node p the two interchanges across the branch to each internal child v, at the root's operation the two across
// the root's edge) and ptn_finish (tiles added left to right, entries back in the caller's rows, NaN where a move does not exist).
// A sibling of phylo_treegrad.h: pt2_prune and ptg_updown keep their code objects.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "phylo_treegrad.h"

// ------------------------------------------------------------------------------------------------
// host: the plan of one call -- no HIP, so that a plain host program can run it under sanitizers (tests/treenni_asan_main.cpp)
// ------------------------------------------------------------------------------------------------
struct ptn_plan {
    int chunk = 0;                 // trees per chunk
    int grid = 0;                  // workgroups of ptn_updown for a full chunk (a shorter last chunk launches min(grid, its items))
    size_t per_tree = 0, wg_store = 0;
    // byte offsets into the slab (all multiples of 256)
    size_t o_prior = 0, o_ops = 0, o_dops = 0, o_nops = 0, o_P = 0, o_t = 0, o_gap = 0, o_tilev = 0, o_out = 0, o_dtile = 0, o_dout = 0, o_store = 0,
           total = 0;
};

// the slab in slab order: prior | ops | downward ops | children's ops | M | lengths | gap rows of M | tile values | loglik | delta tiles | delta
inline int ptn_regions(int N, int ntiles, bool coded, ptn_plan& q, pts_region* r) {
    const size_t R = (size_t)N - 1, nt = (size_t)ntiles;
    int k = 0;
    r[k++] = {PTS_FIXED, 32, true, &q.o_prior};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_ops};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_dops};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_nops};
    r[k++] = {PTS_TREE, R * 256, true, &q.o_P};
    r[k++] = {PTS_TREE, R * 16, true, &q.o_t};
    r[k++] = {PTS_TREE, R * 64, coded, &q.o_gap};
    r[k++] = {PTS_TREE, nt * 8, true, &q.o_tilev};
    r[k++] = {PTS_TREE, 8, true, &q.o_out};
    r[k++] = {PTS_TREE, nt * 2 * R * 8, true, &q.o_dtile};
    r[k++] = {PTS_TREE, 2 * R * 8, true, &q.o_dout};
    return k;
}

// 0: fine.  T trees of N taxa, ntiles site tiles, n_cus compute units; env_chunk > 0 caps the chunk (PHYLO_TREES_CHUNK).
inline int ptn_make_plan(int N, int ntiles, int T, bool coded, int n_cus, int env_chunk, ptn_plan* p) {
    if (N < 2 || ntiles < 1 || T < 1 || n_cus < 1) return 1;
    ptn_plan q;
    q.wg_store = ((size_t)N - 1) * PTG_U * PTG_SLOT_BYTES;
    pts_region r[PTS_MAX_REGIONS];
    ptg_finish_plan(q, r, ptn_regions(N, ntiles, coded, q, r), ntiles, T, n_cus, env_chunk, 0, 0);
    *p = q;
    return 0;
}

// Where the operations of an operation's children stand: nops[i] = {left, right, 0, 0}, the schedule index of that child's own
// operation, -1 for a leaf.  ops the schedule (pt2_schedule), dops its downward operations (ptg_down_ops).  At the operation of p
// the kernel needs the children of p's internal child v and their matrices, which live at v's operation.  0: fine; 1: a child's
// operation does not stand before its parent's, or a row has two operations (never, after pt2_schedule and ptg_down_ops).
inline int ptn_nni_ops(int N, const int32_t* ops, const int32_t* dops, int32_t* nops) {
    const int R = N - 1;
    std::vector<int32_t> at((size_t)R, -1);
    for (int i = 0; i < R; ++i) {
        const int row = ops[4 * i + 3];
        if (row < 0 || row >= R || at[row] >= 0) return 1;
        at[row] = i;
        for (int sd = 0; sd < 2; ++sd) {
            const int d = dops[4 * i + sd];
            int j = -1;
            if (d < 0) {
                if (~d >= R) return 1;
                j = at[~d];
                if (j < 0) return 1;                        // (an earlier operation: at[] holds those only)
            }
            nops[4 * i + sd] = j;
        }
        nops[4 * i + 2] = 0;
        nops[4 * i + 3] = 0;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

struct ptn_args {
    pt2_args a;                      // ops, P (M), gap (of M), leaves, codes, prior, tilev, N, S, T, ntiles as pt2_prune takes them (site_lik unused)
    const int32_t* dops;             // [trees][N-1][4] downward operations (ptg_down_ops)
    const int32_t* nops;             // [trees][N-1][4] the children's operations (ptn_nni_ops)
    double* dtile;                   // [trees][ntiles][2 (N-1)] per-move tile sums, by the schedule index of the move's node v
    pk_d2* store;                    // [grid][N-1][U][2][64] node stores
    int n_items, depth;
};

// the message of one child for the wave's U site steps: its partial (ptg_child) through the upward pass's chain.  src, M wave-uniform.
template <int U, bool CODED>
__device__ __forceinline__ void ptn_msg(const pt2_args& a, int src, const double* M, const pk_d2* store, const unsigned int (&sc)[U], double (&out)[U][4]) {
    double x[U][4], m[16];
    ptg_child<U, CODED>(a, src, store, sc, x);
    pt2_uniform16(M, m);
#pragma unroll
    for (int u = 0; u < U; ++u) pt2_row_times(x[u], m, out[u]);
}

// One neighbour: below the moved branch x' = mz * mc, above it (x' . Mv) * my, its site likelihood against the outer partial av,
// d = log(L' / L); the step's 64 sites reduced by the wave's tree and added by lane 0 into the move's entry.
template <int U>
__device__ __forceinline__ void ptn_move(const double (&av)[U][4], const double (&mz)[U][4], const double (&mc)[U][4], const double (&my)[U][4],
                                         const double (&Mv)[16], const double (&inv)[U], const bool (&live)[U], int lane, double* entry) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
        double xv[4], t[4], xp[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[j] = mz[u][j] * mc[u][j];
        pt2_row_times(xv, Mv, t);
#pragma unroll
        for (int j = 0; j < 4; ++j) xp[j] = t[j] * my[u][j];
        const double d = pm_log(pk_site_lik(av[u], xp) * inv[u]);
        const double tot = pk_wave_tree_sum(live[u] ? d : 0.0);
        if (lane == 0) *entry = *entry + tot;
    }
}

// One wave (= one workgroup) per work item (tree, site tile), lane = column; workgroup w takes items w, w + grid, ...  Per strip of
// 64 U sites: ptg_updown's upward pass (pt2_prune's schedule, stack and chains: the root and the site factor are its bits; every
// non-root node kept in the workgroup's node store), 1 / L as ptg_updown forms it, the two interchanges across the root's edge
// (both root children internal), then the schedule in reverse: the outer partial of the node, both children's messages again, and
// for each internal child v, one at a time, the messages of v's children under v's own matrices (their slots still hold partials:
// v's operation comes later in this walk), the two interchanges of v with its sibling, and v's outer partial into v's slot.
// A move's entry of the LDS array acc[2 (N-1)] is 2 (operation of v) + side.  Launched with depth * U * 2048 + 2 (N-1) * 8 bytes
// of dynamic LDS.
template <int U, bool CODED>
__global__ __launch_bounds__(64) void ptn_updown(const ptn_args g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ptn_lds[];
    const pt2_args& a = g.a;
    pk_d2* stack = reinterpret_cast<pk_d2*>(ptn_lds);
    double* acc = reinterpret_cast<double*>(ptn_lds + (size_t)g.depth * U * PT2_SLOT_BYTES);
    const int lane = threadIdx.x;
    const int R = a.N - 1;
    pk_d2* store = g.store + (size_t)blockIdx.x * R * U * 128 + lane;
#pragma unroll 1
    for (int item = blockIdx.x; item < g.n_items; item += gridDim.x) {     // item: wave-uniform
        const int tree = item / a.ntiles, tile = item - tree * a.ntiles;
        const int s0 = tile * a.T, s1 = s0 + a.T < a.S ? s0 + a.T : a.S;
        pt2_ci4* ops = (pt2_ci4*)(a.ops + (size_t)tree * R * 4);
        pt2_ci4* dops = (pt2_ci4*)(g.dops + (size_t)tree * R * 4);
        pt2_ci4* nops = (pt2_ci4*)(g.nops + (size_t)tree * R * 4);
        const double* P = a.P + (size_t)tree * R * 32;
        const double* G = CODED ? a.gap + (size_t)tree * R * 8 : nullptr;
        for (int j = lane; j < 2 * R; j += 64) acc[j] = 0.0;
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
            for (int i = 0; i < R; ++i) {                   // upward: ptg_updown's loop
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
                    inv[u] = lik >= PTG_LIK_FLOOR && lik < pm_inf() ? 1.0 / lik : pm_nan();     // ptg_updown's rule
                    if (s < s1) pm_lp_mul(col, lik);
                }
            }
            {                                               // across the root's edge: v = (a, b), c = (d, e) exchange b with d, with e
                const pt2_i4 dop = dops[R - 1], nop = nops[R - 1];
                if (dop.x < 0 && dop.y < 0) {               // wave-uniform
                    const pt2_i4 vd = dops[nop.x], cd = dops[nop.y];
                    const double* Mv = P + (size_t)nop.x * 32;
                    const double* Mc = P + (size_t)nop.y * 32;
                    double ma[U][4], mb[U][4], md[U][4], me[U][4];
                    ptn_msg<U, CODED>(a, vd.x, Mv, store, sc, ma);
                    ptn_msg<U, CODED>(a, vd.y, Mv + 16, store, sc, mb);
                    ptn_msg<U, CODED>(a, cd.x, Mc, store, sc, md);
                    ptn_msg<U, CODED>(a, cd.y, Mc + 16, store, sc, me);
                    double mv[16], mc[16];
                    pt2_uniform16(P + (size_t)(R - 1) * 32, mv);
                    pt2_uniform16(P + (size_t)(R - 1) * 32 + 16, mc);
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
                            const double d = pm_log(pk_site_lik(pr, xr) * inv[u]);
                            const double tot = pk_wave_tree_sum(live[u] ? d : 0.0);
                            if (lane == 0) acc[2 * (R - 1) + sd] = acc[2 * (R - 1) + sd] + tot;
                        }
                    }
                }
            }
#pragma unroll 1
            for (int i = R - 1; i >= 0; --i) {              // downward
                const pt2_i4 dop = dops[i];                 // x, y: left and right child; z: the node's row
                const pt2_i4 nop = nops[i];                 // x, y: the operations of the children
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
                if (dop.x >= 0 && dop.y >= 0) continue;     // wave-uniform: two leaves below, no move and no outer partial to leave
                const double* Mi = P + (size_t)i * 32;
                double e[2][U][4];                          // the children's messages again: the chain of the upward pass
                ptn_msg<U, CODED>(a, dop.x, Mi, store, sc, e[0]);
                ptn_msg<U, CODED>(a, dop.y, Mi + 16, store, sc, e[1]);
#pragma unroll
                for (int sd = 0; sd < 2; ++sd) {
                    const int src = sd ? dop.y : dop.x;
                    if (src < 0) {                          // wave-uniform: an internal child v, one at a time
                        const int jv = sd ? nop.y : nop.x;
                        const pt2_i4 vd = dops[jv];
                        const double* Mj = P + (size_t)jv * 32;
                        double ma[U][4], mb[U][4];          // v's children under v's matrices (their slots still hold partials)
                        ptn_msg<U, CODED>(a, vd.x, Mj, store, sc, ma);
                        ptn_msg<U, CODED>(a, vd.y, Mj + 16, store, sc, mb);
                        double m[16];
                        pt2_uniform16(Mi + sd * 16, m);     // the branch above v
                        const double (&ec)[U][4] = e[1 - sd];    // the sibling's message
                        ptn_move<U>(av, mb, ec, ma, m, inv, live, lane, acc + 2 * jv);          // side 0: a and the sibling change places
                        ptn_move<U>(av, ma, ec, mb, m, inv, live, lane, acc + 2 * jv + 1);      // side 1: b and the sibling
                        pk_d2* dst = store + (size_t)(~src) * U * 128;     // v's outer partial takes v's slot (ptg_updown's terms)
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
// whose log-likelihood is not finite gets NaN in every entry (one with a site factor below PTG_LIK_FLOOR already carries it); so
// do the two entries of the root's row when one of the root's children is a leaf: those moves do not exist.  out [trees][N-1][2].
__global__ __launch_bounds__(256) void ptn_finish(const double* __restrict__ dtile, const int32_t* __restrict__ ops, const double* __restrict__ loglik,
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

inline void ptn_launch(const ptn_args& g, int grid, bool coded, hipStream_t s) {
    const size_t lds = (size_t)g.depth * PTG_U * PT2_SLOT_BYTES + (size_t)2 * (g.a.N - 1) * 8;
    if (coded) hipLaunchKernelGGL((ptn_updown<PTG_U, true>), dim3((unsigned)grid), dim3(64), lds, s, g);
    else hipLaunchKernelGGL((ptn_updown<PTG_U, false>), dim3((unsigned)grid), dim3(64), lds, s, g);
}
#endif  // __HIPCC__
