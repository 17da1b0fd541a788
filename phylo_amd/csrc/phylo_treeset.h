// phylo_treeset.h -- phylo_trees_loglik: the log-likelihood of MANY explicit rooted binary trees over the context's resident
// alignment.  Host: validation and the slot schedule of one tree; device: the pruning kernel that walks
// a tree's schedule with the partials of the subtrees in flight in an LDS stack (no partial ever reaches HBM), and the kernel
// that adds a tree's tile values left to right.  All arithmetic is phylo_math.h's and pk_merge_site's: the bits are those of
// phylo_tree_loglik (pk_tree_prune + pk_row_loglik) and of the C oracle.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "phylo_treeset_plan.h"

#if defined(__HIPCC__)
#include "phylo_kernels.h"
#endif

#define PT2_MAX_DEPTH 10                          // floor(log2 PK_MAX_TAXA) + 1 slots
#define PT2_SLOT_BYTES 2048                       // one slot of one site step: 64 lanes x 4 doubles
#define PT2_WAVE_LDS (20 * 1024)                  // four site steps per pass while the stack stays within this, else two
#define PT2_MAX_CATS 16                           // rate categories of phylo_trees_loglik_rates
#define PT2_SCRATCH_BYTES ((size_t)64 << 20)      // device scratch of one chunk of trees (phylo_trees_loglik cuts T to fit)
// The domain of pm_expm4: its entrywise relative error is at most 2^s (8 E + 4) u after s squarings, E = 116
// the worst error (in u = 2^-53) of a plain restatement of the algorithm without squarings, over the generators of
// tests/expm_cases.py.  PT2_EXPM_S_MAX is the largest s at which that bound is still <= 2^-20; a length with ||Q||_1 t above
// theta_13 2^s_max is refused, not answered with a matrix that has lost its digits (and, from 1e100 on, all of them: a zero matrix).
#define PT2_EXPM_S_MAX 23
#define PT2_EXPM_NORM_MAX (5.371920351148152 * 8388608.0)   // theta_13 * 2^PT2_EXPM_S_MAX = 4.5063e7

// ------------------------------------------------------------------------------------------------
// host: one tree = child[N-1][2], blen[N-1][2]; leaves 0 .. N-1, row i = internal node N + i, children from earlier rows
// ------------------------------------------------------------------------------------------------
// 0: fine; otherwise the offending row in *bad_row and a message
inline int pt2_check_tree(int N, const int32_t* child, const double* blen, int* bad_row, char* msg, size_t nmsg) {
    const int R = N - 1;
    std::vector<unsigned char> used((size_t)N + R, 0);
    for (int i = 0; i < R; ++i)
        for (int sd = 0; sd < 2; ++sd) {
            const int ch = child[2 * i + sd];
            const double b = blen[2 * i + sd];
            *bad_row = i;
            if (ch < 0 || ch >= N + i) {
                snprintf(msg, nmsg, "child %d is neither a leaf nor a node of an earlier row (N = %d)", ch, N);
                return 1;
            }
            if (used[ch]) {
                snprintf(msg, nmsg, "%s %d is a child twice", ch < N ? "leaf" : "node", ch);
                return 1;
            }
            used[ch] = 1;
            if (!(b >= 0.0) || !std::isfinite(b)) {
                snprintf(msg, nmsg, "branch length %g above child %d is not a finite number >= 0", b, ch);
                return 1;
            }
        }
    // 2 (N-1) distinct children out of the 2 N - 2 nodes below the root: every one of them exactly once
    return 0;
}

// ||Q||_1 the way pm_expm4 takes the norm of Q t: the largest column sum of |q_ij|, rows added in ascending order
inline double pt2_q_norm1(const double* Q16) {
    double norm = 0.0;
    for (int j = 0; j < 4; ++j) {
        double cs = 0.0;
        for (int i = 0; i < 4; ++i) cs = cs + std::fabs(Q16[i * 4 + j]);
        if (cs > norm) norm = cs;
    }
    return norm;
}

// Are the n lengths rate * t[i] inside the domain of pm_expm4 under a generator of 1-norm q_norm1: fl(q_norm1 * |fl(rate * t[i])|) <=
// PT2_EXPM_NORM_MAX?  0: all are; otherwise the first offender's index in *bad and a message that names its length and the limit
// (a NaN product offends: the comparison is false).  q_norm1 = 0 asks for no limit: the callers pass it under jc69_closed_form,
// whose pm_jc69 is right at every length.  No HIP: tests/expm_range_asan_main.cpp runs it under the host compiler's sanitizers.
inline int pt2_check_expm_range(double q_norm1, int n, const double* t, double rate, int* bad, char* msg, size_t nmsg) {
    if (q_norm1 == 0.0) return 0;
    for (int i = 0; i < n; ++i) {
        const double len = rate * t[i];
        const double a = q_norm1 * std::fabs(len);
        if (a <= PT2_EXPM_NORM_MAX) continue;
        *bad = i;
        if (rate == 1.0)
            snprintf(msg, nmsg, "length %g gives ||Q t||_1 = %g, above %g (theta_13 2^%d), the limit of the matrix exponential", t[i], a,
                     PT2_EXPM_NORM_MAX, PT2_EXPM_S_MAX);
        else
            snprintf(msg, nmsg, "length %g at rate %g gives ||Q t||_1 = %g, above %g (theta_13 2^%d), the limit of the matrix exponential",
                     t[i], rate, a, PT2_EXPM_NORM_MAX, PT2_EXPM_S_MAX);
        return 1;
    }
    return 0;
}

// the slots every row's subtree needs (Sethi-Ullman); need[N-2], the root's, is the depth pt2_schedule returns
// (no schedule holds fewer, and pt2_schedule's holds no more: DESIGN.md section 11)
inline void pt2_needs(int N, const int32_t* child, std::vector<int>& need) {
    const int R = N - 1;
    need.resize((size_t)R);
    for (int i = 0; i < R; ++i) {
        const int a = child[2 * i], b = child[2 * i + 1];
        int na = a < N ? 0 : need[a - N], nb = b < N ? 0 : need[b - N];
        if (na < nb) { const int t = na; na = nb; nb = t; }
        const int m = nb + (na > 0 ? 1 : 0);
        need[i] = na > m ? na : (m > 1 ? m : 1);
    }
}

// The schedule of a checked tree: N-1 operations {destination slot, left source, right source, row}; a source >= 0 is a leaf,
// a source < 0 the slot ~source.  Children-first, the child with the larger slot need first (Sethi-Ullman), the destination
// takes over the slot of an internal child: a tree of N leaves never holds more than floor(log2 N) + 1 slots.  Returns the depth.
inline int pt2_schedule(int N, const int32_t* child, int32_t* ops /*[N-1][4]*/) {
    const int R = N - 1;
    std::vector<int> need, slot_of((size_t)R, -1), stack, free_slots;
    pt2_needs(N, child, need);
    std::vector<unsigned char> state((size_t)R, 0);
    int n_ops = 0, depth = 0, next_slot = 0;
    stack.push_back(R - 1);
    while (!stack.empty()) {
        const int i = stack.back();
        const int a = child[2 * i], b = child[2 * i + 1];
        if (state[i] == 0) {
            state[i] = 1;
            const int na = a < N ? 0 : need[a - N], nb = b < N ? 0 : need[b - N];
            // (pushed last = visited first: the larger need; ties: the left child)
            if (na >= nb) { if (b >= N) stack.push_back(b - N); if (a >= N) stack.push_back(a - N); }
            else { if (a >= N) stack.push_back(a - N); if (b >= N) stack.push_back(b - N); }
            continue;
        }
        stack.pop_back();
        const int sa = a < N ? -1 : slot_of[a - N], sb = b < N ? -1 : slot_of[b - N];
        int dst;
        if (sa >= 0) { dst = sa; if (sb >= 0) free_slots.push_back(sb); }
        else if (sb >= 0) dst = sb;
        else if (!free_slots.empty()) {                   // the lowest free slot
            size_t best = 0;
            for (size_t j = 1; j < free_slots.size(); ++j) if (free_slots[j] < free_slots[best]) best = j;
            dst = free_slots[best];
            free_slots.erase(free_slots.begin() + (long)best);
        } else dst = next_slot++;
        slot_of[i] = dst;
        if (dst + 1 > depth) depth = dst + 1;
        int32_t* o = ops + 4 * (size_t)n_ops++;
        o[0] = dst; o[1] = sa >= 0 ? ~sa : a; o[2] = sb >= 0 ? ~sb : b; o[3] = i;
    }
    return depth;
}

// Site steps a wave carries through one pass over the schedule (operations and matrices are read once per pass): four while the
// stack stays within PT2_WAVE_LDS (depth <= 2: caterpillar-like trees), else two -- at most 40 KiB per wave at depth 10.  (One
// step per pass holds both matrices and all pointers in scalar registers at once and spills two of them: not built.)
inline int pt2_unroll(int depth) { return depth * 4 * PT2_SLOT_BYTES <= PT2_WAVE_LDS ? 4 : 2; }

// The plan of phylo_trees_loglik and phylo_trees_loglik_rates: one chunk of trees in device scratch, no node store.
struct pt2_plan {
    int chunk = 0;                 // trees per chunk
    bool sites = false;            // the row of site values is carried (asked for, or a chunk's four-step kernel needs it)
    size_t per_tree = 0;
    // byte offsets into the slab (all multiples of 256)
    size_t o_prior = 0, o_ops = 0, o_P = 0, o_t = 0, o_gap = 0, o_tilev = 0, o_out = 0, o_site = 0, o_cat = 0, total = 0;
};

// the slab in slab order: prior and weights | ops | matrices | lengths | gap rows | tile values | loglik | site values | category factors
inline int pt2_regions(int N, int S, int ntiles, int nc, bool coded, bool sites, bool cat, pt2_plan& q, pts_region* r) {
    const size_t R = (size_t)N - 1, c = (size_t)nc;
    int k = 0;
    r[k++] = {PTS_FIXED, 32 + PT2_MAX_CATS * 8, true, &q.o_prior};     // the prior, then the weights: one pointer for pt2_prune_rates
    r[k++] = {PTS_TREE, R * 16, true, &q.o_ops};
    r[k++] = {PTS_TREE, c * R * 256, true, &q.o_P};
    r[k++] = {PTS_TREE, c * R * 16, true, &q.o_t};
    r[k++] = {PTS_TREE, c * R * 64, coded, &q.o_gap};
    r[k++] = {PTS_TREE, (size_t)ntiles * 8, true, &q.o_tilev};
    r[k++] = {PTS_TREE, 8, true, &q.o_out};
    r[k++] = {PTS_TREE, (size_t)S * 8, sites, &q.o_site};
    r[k++] = {PTS_TREE, c * (size_t)S * 8, cat, &q.o_cat};
    return k;
}

// 0: fine.  T trees of N taxa and S sites in ntiles tiles, nc sets of lengths per tree (mix: the rates call, C = nc).  The rates
// call's four-step kernels keep the site values in their row between categories (pt2_prune_rates), so the row is there, asked for
// or not, when a chunk is that shallow: a chunk's depth is its deepest tree's (depth_of[T], pt2_needs' depths; read when mix and
// the row is not asked for).  Carrying the row makes the chunk smaller, so the chunks are looked at again with it.
inline int pt2_make_plan(int N, int S, int ntiles, int T, int nc, bool mix, bool coded, bool want_sites, bool want_cat, int env_chunk,
                         const int* depth_of, pt2_plan* p) {
    if (N < 2 || S < 1 || ntiles < 1 || T < 1 || nc < 1 || nc > PT2_MAX_CATS || (mix && !want_sites && !depth_of)) return 1;
    pt2_plan q;
    pts_region r[PTS_MAX_REGIONS];
    int nr = 0;
    q.sites = want_sites;
    for (;;) {
        nr = pt2_regions(N, S, ntiles, nc, coded, q.sites, want_cat, q, r);
        q.per_tree = pts_sum(r, nr, PTS_TREE);
        q.chunk = pts_chunk(q.per_tree, ntiles, T, env_chunk, PT2_SCRATCH_BYTES, 0, 0);
        if (!mix || q.sites) break;
        for (int t0 = 0; t0 < T && !q.sites; t0 += q.chunk)  // the chunks without the row: is one of them that shallow?
            q.sites = pt2_unroll(*std::max_element(depth_of + t0, depth_of + std::min(T, t0 + q.chunk))) == 4;
        if (!q.sites) break;
    }
    q.total = pts_lay_out(r, nr, (size_t)q.chunk, 0, nullptr);
    *p = q;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
#if defined(__HIPCC__)

struct pt2_args {
    const int32_t* ops;              // [trees][N-1][4] schedule (wave-uniform)
    const double* P;                 // [trees][N-1][2][16] matrices in schedule order, left then right
    const double* gap;               // [trees][N-1][2][4] row 4 of every matrix's leaf table (coded leaves), else NULL
    const double* leaves;            // [N][S][4]
    const uint8_t* codes;            // [N][S]
    const double* prior;             // [4]
    double* tilev;                   // [trees][ntiles]
    double* site_lik;                // [trees][S] or NULL
    int N, S, T, ntiles;
};

// row 4 of the 5 x 4 leaf table of every matrix (the fma chain over an all-ones row, pk_build_leaf_table); rows 0 .. 3 of the
// table are the matrix's own rows and are read in place
__global__ __launch_bounds__(256) void pt2_gap_rows(const double* __restrict__ P, long n_mat, double* __restrict__ gap) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_mat * 4) return;
    const double* p = P + (t >> 2) * 16;
    const int j = (int)(t & 3);
    gap[t] = pm_fma(1.0, p[12 + j], pm_fma(1.0, p[8 + j], pm_fma(1.0, p[4 + j], 1.0 * p[j])));
}

// Wave-uniform data the launch only reads (operations, matrices, prior) is read through the constant address space: the kernel
// also stores (site factors, tile values), after which hipcc would no longer prove a plain uniform load invariant and would
// fetch every matrix once per LANE.
typedef __attribute__((address_space(4))) const double pt2_cd;
typedef int pt2_i4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(4))) const pt2_i4 pt2_ci4;
__device__ __forceinline__ void pt2_uniform16(const double* M, double (&m)[16]) {
    pt2_cd* q = (pt2_cd*)M;
#pragma unroll
    for (int j = 0; j < 16; ++j) m[j] = q[j];
}

// (row . M)[j], the chain of pk_merge_site
__device__ __forceinline__ void pt2_row_times(const double (&x)[4], const double (&M)[16], double (&out)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double v = x[0] * M[j];
        v = pm_fma(x[1], M[4 + j], v);
        v = pm_fma(x[2], M[8 + j], v);
        out[j] = pm_fma(x[3], M[12 + j], v);
    }
}

// One side of one operation for the wave's U site steps: (child row . M) from a coded leaf (table look-up), a generic leaf
// (resident row) or a slot of the LDS stack.  src and M are wave-uniform.
template <int U, bool CODED>
__device__ __forceinline__ void pt2_side(const pt2_args& a, int src, const double* __restrict__ M, const double* __restrict__ gap,
                                         const pk_d2* stack, const unsigned int (&sc)[U], int lane, double (&out)[U][4]) {
    if (src >= 0) {
        if constexpr (CODED) {
            const uint8_t* cd = a.codes + (size_t)src * a.S;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned int c = *(pk_gu8c*)(cd + sc[u]);
                const double* row = c < 4u ? M + 4u * c : gap;
                pk_load4(row, out[u]);
            }
        } else {
            const double* rows = a.leaves + (size_t)src * a.S * 4;
            double m[16];
            pt2_uniform16(M, m);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                double x[4];
                pk_load4(rows + (size_t)sc[u] * 4, x);
                pt2_row_times(x, m, out[u]);
            }
        }
    } else {
        const pk_d2* sl = stack + (size_t)(~src) * U * 128 + lane;
        double m[16];
        pt2_uniform16(M, m);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const pk_d2 lo = sl[u * 128], hi = sl[u * 128 + 64];
            const double x[4] = {lo.x, lo.y, hi.x, hi.y};
            pt2_row_times(x, m, out[u]);
        }
    }
}

// One wave per (tree, site tile), lane = column of the tile, sites in increasing order.  Stack layout: slot d, site step u, half h
// (states 0,1 | 2,3), lane: 16 bytes each, so a wave's access is one contiguous kilobyte; a lane only ever touches its own
// column, so the stack needs no fence.  Launched with depth * U * 2048 bytes of dynamic LDS.
template <int U, bool CODED>
__global__ __launch_bounds__(64) void pt2_prune(const pt2_args a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pt2_lds[];
    pk_d2* stack = reinterpret_cast<pk_d2*>(pt2_lds);
    const int lane = threadIdx.x;
    const int tree = blockIdx.x / a.ntiles, tile = blockIdx.x - tree * a.ntiles;
    const int R = a.N - 1;
    const int s0 = tile * a.T, s1 = s0 + a.T < a.S ? s0 + a.T : a.S;
    pt2_ci4* ops = (pt2_ci4*)(a.ops + (size_t)tree * R * 4);
    const double* P = a.P + (size_t)tree * R * 32;
    const double* G = CODED ? a.gap + (size_t)tree * R * 8 : nullptr;
    pm_lp col = pm_lp_init();
#pragma unroll 1
    for (int base = s0; base < s1; base += 64 * U) {       // base: wave-uniform
        unsigned int sc[U];                                 // a site past the end re-reads the last one; its factor is dropped
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int s = base + 64 * u + lane;
            sc[u] = (unsigned int)(s < s1 ? s : s1 - 1);
        }
        double o[U][4];
#pragma unroll 1
        for (int i = 0; i < R; ++i) {
            const pt2_i4 op = ops[i];
            double l[U][4], r[U][4];
            pt2_side<U, CODED>(a, op.y, P + (size_t)i * 32, CODED ? G + (size_t)i * 8 : nullptr, stack, sc, lane, l);
            pt2_side<U, CODED>(a, op.z, P + (size_t)i * 32 + 16, CODED ? G + (size_t)i * 8 + 4 : nullptr, stack, sc, lane, r);
            pk_d2* dst = stack + (size_t)op.x * U * 128 + lane;
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int j = 0; j < 4; ++j) o[u][j] = l[u][j] * r[u][j];
                const pk_d2 lo = {o[u][0], o[u][1]}, hi = {o[u][2], o[u][3]};
                dst[u * 128] = lo;
                dst[u * 128 + 64] = hi;
            }
        }
        pt2_cd* prc = (pt2_cd*)a.prior;                      // (read here, not ahead of the loops: eight scalar registers fewer across them)
        const double pr[4] = {prc[0], prc[1], prc[2], prc[3]};
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int s = base + 64 * u + lane;
            if (base + 64 * u < s1) {                       // wave-uniform
                const double lik = pk_site_lik(pr, o[u]);
                if (s < s1) {
                    if (a.site_lik) a.site_lik[(size_t)tree * a.S + s] = lik;
                    pm_lp_mul(col, lik);
                }
            }
        }
    }
    const double t = pk_wave_tree_sum(pm_lp_finish(col));
    if (lane == 0) a.tilev[(size_t)tree * a.ntiles + tile] = t;
}

// The rates form: C categories of one tree in one wave.  Matrices and gap rows of a tree are laid out
// [category][op][left|right] (the host scaled the lengths: rate[c] * blen, so the kernel reads no rate), the schedule is the
// tree's one schedule, read once per category and pass.  Inside a pass the categories run outermost over the same LDS stack; a
// lane keeps U site values m[u] = weight[0] f_0, then pm_fma(weight[c], f_c, m[u]) in ascending c (in registers at U = 2, in its
// own entries of site_lik at U = 4: see the kernel), which enter pm_lp_mul where pt2_prune's lik does.  A sibling of pt2_prune over the same pt2_side, so that pt2_prune's code objects stay what they are.
struct pt2_rates_args {
    pt2_args a;                      // P [trees][C][N-1][2][16], gap [trees][C][N-1][2][4]; site_lik the mixed value (NULL only at U = 2);
                                     // prior [4 + C]: the prior, then the weights (wave-uniform, one pointer for both)
    double* cat_lik;                 // [trees][C][S] the factor of every category, or NULL
    int C;
};

// The kernel's own arguments, read again where they are used: what a category's tail and a pass's tail need (prior, weights and
// the three output pointers) is fetched there by scalar loads from the kernel-argument segment, not held in scalar registers
// across the operation loop, which already fills them with two matrices (pt2_prune sits at 93 .. 106 of 106).
typedef __attribute__((address_space(4))) const struct pt2_rates_args pt2_ckarg;
__device__ __forceinline__ pt2_ckarg* pt2_kernarg_here() {
    pt2_ckarg* k = (pt2_ckarg*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(k));                             // (a load through k stays below this point)
    return k;
}

template <int U, bool CODED>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(U == 4 ? 4 : (CODED ? 7 : 5)))) void pt2_prune_rates(const pt2_rates_args ra) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pt2_lds[];
    pk_d2* stack = reinterpret_cast<pk_d2*>(pt2_lds);
    const pt2_args& a = ra.a;
    const int lane = threadIdx.x;
    const int tree = blockIdx.x / a.ntiles, tile = blockIdx.x - tree * a.ntiles;
    const int R = a.N - 1;
    const int s0 = tile * a.T, s1 = s0 + a.T < a.S ? s0 + a.T : a.S;
    pt2_ci4* ops = (pt2_ci4*)(a.ops + (size_t)tree * R * 4);
    const double* P = a.P + (size_t)tree * ra.C * R * 32;   // category c's matrices and gap rows: stepped, and stepped back per pass
    const double* G = CODED ? a.gap + (size_t)tree * ra.C * R * 8 : nullptr;
    // The site values m[u] live in registers across the categories at two site steps.  At four, pt2_prune stands at 116 (coded)
    // and 128 (generic) VGPRs and 8 more cost a wave per SIMD (130 and 136) or, held to 128, a spill: there a lane keeps them in
    // its own entries of site_lik (which the host then provides, asked for or not), one 8-byte load and store per site and
    // category beside N-1 operations.  The bits are the same: a double goes through memory unchanged.
    constexpr bool VIA_SITE = U == 4;
    pm_lp col = pm_lp_init();
#pragma unroll 1
    for (int base = s0; base < s1; base += 64 * U) {       // base: wave-uniform
        unsigned int sc[U];                                 // a site past the end re-reads the last one; its factors are dropped
        double m[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int s = base + 64 * u + lane;
            sc[u] = (unsigned int)(s < s1 ? s : s1 - 1);
            m[u] = 0.0;
        }
#pragma unroll 1
        for (int c = 0;;) {                                 // c: wave-uniform, C >= 1
            double o[U][4];
#pragma unroll 1
            for (int i = 0; i < R; ++i) {
                const pt2_i4 op = ops[i];
                double l[U][4], r[U][4];
                pt2_side<U, CODED>(a, op.y, P + (size_t)i * 32, CODED ? G + (size_t)i * 8 : nullptr, stack, sc, lane, l);
                pt2_side<U, CODED>(a, op.z, P + (size_t)i * 32 + 16, CODED ? G + (size_t)i * 8 + 4 : nullptr, stack, sc, lane, r);
                pk_d2* dst = stack + (size_t)op.x * U * 128 + lane;
#pragma unroll
                for (int u = 0; u < U; ++u) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) o[u][j] = l[u][j] * r[u][j];
                    const pk_d2 lo = {o[u][0], o[u][1]}, hi = {o[u][2], o[u][3]};
                    dst[u * 128] = lo;
                    dst[u * 128 + 64] = hi;
                }
            }
            pt2_ckarg* k = pt2_kernarg_here();
            const int C = k->C;
            int e1 = __builtin_amdgcn_readfirstlane(s1);    // (the tail's tests are made here, not kept as masks across the loops)
            asm volatile("" : "+s"(e1));
            pt2_cd* prc = (pt2_cd*)k->a.prior;
            const double pr[4] = {prc[0], prc[1], prc[2], prc[3]};
            const double w = prc[4 + c];
            double* F = k->cat_lik;
            if (F) F += ((size_t)tree * C + c) * a.S;
            double* sl = k->a.site_lik + (size_t)tree * a.S;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = base + 64 * u + lane;
                if (base + 64 * u < e1) {                   // wave-uniform
                    const double f = pk_site_lik(pr, o[u]);
                    if (F && s < e1) F[s] = f;
                    if constexpr (VIA_SITE) {
                        if (s < e1) sl[s] = c ? pm_fma(w, f, sl[s]) : w * f;
                    } else m[u] = c ? pm_fma(w, f, m[u]) : w * f;
                }
            }
            P += (size_t)R * 32;
            if (CODED) G += (size_t)R * 8;
            if (++c == C) {
                P -= (size_t)C * R * 32;
                if (CODED) G -= (size_t)C * R * 8;
                break;
            }
        }
        double* sl = pt2_kernarg_here()->a.site_lik;
        if (sl) sl += (size_t)tree * a.S;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int s = base + 64 * u + lane;
            if (s < s1) {
                if constexpr (VIA_SITE) m[u] = sl[s];
                else if (sl) sl[s] = m[u];
                pm_lp_mul(col, m[u]);
            }
        }
    }
    const double t = pk_wave_tree_sum(pm_lp_finish(col));
    pt2_ckarg* k = pt2_kernarg_here();
    if (lane == 0) k->a.tilev[(size_t)blockIdx.x] = t;       // [tree][tile]: the workgroup's own index
}

template <int U, bool CODED>
inline void pt2_launch_rates_as(const pt2_rates_args& ra, int trees, int depth, hipStream_t s) {
    hipLaunchKernelGGL((pt2_prune_rates<U, CODED>), dim3((unsigned)trees * ra.a.ntiles), dim3(64), (size_t)depth * U * PT2_SLOT_BYTES, s, ra);
}
inline void pt2_launch_rates(const pt2_rates_args& ra, int trees, int depth, bool coded, hipStream_t s) {
    const int U = pt2_unroll(depth);
    if (coded) {
        if (U == 4) pt2_launch_rates_as<4, true>(ra, trees, depth, s);
        else pt2_launch_rates_as<2, true>(ra, trees, depth, s);
    } else {
        if (U == 4) pt2_launch_rates_as<4, false>(ra, trees, depth, s);
        else pt2_launch_rates_as<2, false>(ra, trees, depth, s);
    }
}

// a tree's tile values, added left to right (as pk_tile_epilogue and pk_row_loglik add them)
__global__ __launch_bounds__(256) void pt2_finish(const double* __restrict__ tilev, int ntiles, int trees, double* __restrict__ out) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= trees) return;
    const double* tv = tilev + (size_t)t * ntiles;
    double tot = tv[0];
    for (int i = 1; i < ntiles; ++i) tot = tot + tv[i];
    out[t] = tot;
}

// the launch carries the depth its chunk needs: depth * U * 2048 bytes of LDS per wave
template <int U, bool CODED>
inline void pt2_launch_as(const pt2_args& a, int trees, int depth, hipStream_t s) {
    hipLaunchKernelGGL((pt2_prune<U, CODED>), dim3((unsigned)trees * a.ntiles), dim3(64), (size_t)depth * U * PT2_SLOT_BYTES, s, a);
}
inline void pt2_launch(const pt2_args& a, int trees, int depth, bool coded, hipStream_t s) {
    const int U = pt2_unroll(depth);
    if (coded) {
        if (U == 4) pt2_launch_as<4, true>(a, trees, depth, s);
        else pt2_launch_as<2, true>(a, trees, depth, s);
    } else {
        if (U == 4) pt2_launch_as<4, false>(a, trees, depth, s);
        else pt2_launch_as<2, false>(a, trees, depth, s);
    }
}

#endif  // __HIPCC__
