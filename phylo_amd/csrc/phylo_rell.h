// phylo_rell.h -- phylo_rell: the RELL bootstrap over the per-site factors of a scored tree set.
// x = log(site factor); replicate b's counts cnt[b][s] by Philox stream 4 and integer histogramming; rl[t][b] the ONE fma chain
// over ascending s from +0.0, acc = fma(cnt[b][s], x[t][s], acc); best[b] the first greatest rl[.][b]; wins its histogram.
// The chain runs in v_mfma_f64_16x16x4: one instruction is, per element of a 16 x 16 tile, four correctly rounded fmas in
// ascending k with C first (tools/ubench/mfma_f64_probe.hip), so a wave that keeps a tile's accumulators across its walk over
// the sites computes the contract's bits by construction.  The host loop of phylo_debug_rell_host calls the same PM_HD functions.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "phylo_math.h"

#define PR_MAX_SITES 65535                        // counts are uint16: a replicate draws S sites, so a count is at most S
#define PR_MAX_REPS (1 << 20)
#define PR_CHUNK_BYTES ((size_t)256 << 20)        // counts and replicate scores of one chunk of replicates stay within this
#define PR_TT 64                                  // trees of a workgroup's tile (two waves of 32)
#define PR_TB 128                                 // replicates of a workgroup's tile (two waves of 64)
#define PR_KP 32                                  // sites of a staged panel
#define PR_XS (PR_TT + 16)                        // LDS strides in doubles, panels stored [site][tree] and [site][replicate]: a wave's
#define PR_CS (PR_TB + 16)                        // operand read (16 rows x 4 sites) then covers every bank once per half wave

// row stride of the counts: S rounded up to a multiple of 4 (a k step of the MFMA; rows start 8-byte aligned); the pad stays 0
PM_HD size_t pr_count_stride(int S) { return ((size_t)S + 3) & ~(size_t)3; }

// the site of draw j of replicate b (b: the GLOBAL replicate index): word j & 3 of the block at counter (b, 0, 4, j >> 2)
PM_HD uint32_t pr_site_of_word(uint32_t word, int S) { return (uint32_t)(((uint64_t)word * (uint64_t)(uint32_t)S) >> 32); }
PM_HD uint32_t pr_block_word(const pm_u32x4& r, int w) { return w == 0 ? r.x : w == 1 ? r.y : w == 2 ? r.z : r.w; }
PM_HD pm_u32x4 pr_draw_block(uint32_t b, uint32_t blk, uint64_t seed) { return pm_philox4x32(b, 0u, (uint32_t)PM_STREAM_BOOT, blk, seed); }

PM_HD bool pr_factor_ok(double v) { return pm_bits(v) - 1ull < 0x7fefffffffffffffull; }   // finite and > 0 (+0.0 wraps; sign set, inf, NaN are above)

// one step of the contract's chain
PM_HD double pr_chain_step(double cnt, double x, double acc) { return pm_fma(cnt, x, acc); }

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
// site factors -> logs, in place; *flag: an entry was not finite and > 0 (the host has refused such input already: a guard)
__global__ __launch_bounds__(256) void pr_log(double* __restrict__ x, size_t n, unsigned int* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = x[i];
    if (!pr_factor_ok(v)) *flag = 1u;
    x[i] = pm_log(v);
}

// counts of n replicates from global index b0 on: one thread per Philox block (four draws), counts as uint16 pairs in 32-bit
// words, added to with integer atomics (a count never exceeds S <= 65535, so no carry leaves its half).  cnt zeroed beforehand.
__global__ __launch_bounds__(256) void pr_counts(unsigned int* __restrict__ cnt, int S, size_t Sp, uint32_t b0, size_t n_threads, uint32_t nblk,
                                                 uint64_t seed) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_threads) return;
    const uint32_t row = (uint32_t)(i / nblk), blk = (uint32_t)(i - (size_t)row * nblk);
    const pm_u32x4 r = pr_draw_block(b0 + row, blk, seed);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if ((int)(4 * blk + w) < S) {
            const size_t e = (size_t)row * Sp + pr_site_of_word(pr_block_word(r, w), S);
            atomicAdd(cnt + (e >> 1), 1u << (16 * (unsigned)(e & 1)));
        }
    }
}

// a row of ones over the S sites: the observed score is the chain with every count 1, one more column of the first chunk
__global__ __launch_bounds__(256) void pr_ones(uint16_t* __restrict__ row, int S) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s < S) row[s] = 1;
}

typedef double pr_d4 __attribute__((ext_vector_type(4)));
typedef unsigned short pr_u16x4 __attribute__((ext_vector_type(4)));

struct pr_panel {                                 // what a thread carries of the NEXT panel while the waves multiply the current one
    double x[PR_TT * PR_KP / 256];
    pr_u16x4 c[PR_TB * PR_KP / 4 / 256];
};

__device__ __forceinline__ void pr_panel_load(pr_panel& p, const double* __restrict__ x, const uint16_t* __restrict__ cnt, int T, int S, size_t Sp,
                                              int ncols, int t0, int b0, int s0, int tid) {
#pragma unroll
    for (int i = 0; i < PR_TT * PR_KP / 256; ++i) {
        const int e = tid + 256 * i, k = e & (PR_KP - 1), row = e / PR_KP;
        const int t = t0 + row, s = s0 + k;
        p.x[i] = t < T && s < S ? x[(size_t)t * S + s] : 0.0;                  // the pad: x = 0.0 ...
    }
#pragma unroll
    for (int i = 0; i < PR_TB * PR_KP / 4 / 256; ++i) {
        const int q = tid + 256 * i, kq = q & (PR_KP / 4 - 1), rep = q / (PR_KP / 4);
        const int b = b0 + rep, s = s0 + 4 * kq;
        const pr_u16x4 z = {0, 0, 0, 0};
        p.c[i] = b < ncols && (size_t)s < Sp ? *(const pr_u16x4*)(cnt + (size_t)b * Sp + s) : z;   // ... and count 0
    }
}

__device__ __forceinline__ void pr_panel_store(const pr_panel& p, double* xs, double* cs, int tid) {
#pragma unroll
    for (int i = 0; i < PR_TT * PR_KP / 256; ++i) {
        const int e = tid + 256 * i, k = e & (PR_KP - 1), row = e / PR_KP;
        xs[k * PR_XS + row] = p.x[i];
    }
#pragma unroll
    for (int i = 0; i < PR_TB * PR_KP / 4 / 256; ++i) {
        const int q = tid + 256 * i, kq = q & (PR_KP / 4 - 1), rep = q / (PR_KP / 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) cs[(4 * kq + j) * PR_CS + rep] = (double)p.c[i][j];   // counts become doubles once, here
    }
}

// A workgroup's walk over ALL sites for its 64 trees x 128 columns (t0, b0), four waves of 32 x 64 = 2 x 4 MFMA tiles each, in
// steps of 4 sites with a wave's eight accumulators in registers: the body of pr_replicates and of prm_product (phylo_rell_ms.h),
// which differ in their epilogues alone.  xs, cs: the workgroup's panels.  Operand lanes (the probe's): A[row l & 15][k l >> 4],
// B[k l >> 4][col l & 15], D col l & 15, row (l >> 4) + 4 reg.  Trees, columns and sites past the end enter as 0.0 / count 0
// (fma(0, x, acc) == acc bit for bit: acc starts at +0.0, x is finite), so no MFMA sits under a divergent guard.
__device__ __forceinline__ void pr_walk(pr_d4 (&acc)[2][4], const double* __restrict__ x, const uint16_t* __restrict__ cnt, int T, int S, size_t Sp,
                                        int ncols, int t0, int b0, double* xs, double* cs) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wt = (wave & 1) * 32, wb = (wave >> 1) * 64;
    const int r = lane & 15, kk = lane >> 4;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = pr_d4{0.0, 0.0, 0.0, 0.0};
    pr_panel p;
    pr_panel_load(p, x, cnt, T, S, Sp, ncols, t0, b0, 0, tid);
#pragma unroll 1
    for (int s0 = 0; s0 < S; s0 += PR_KP) {
        __syncthreads();                                    // the waves are done with the previous panel
        pr_panel_store(p, xs, cs, tid);
        __syncthreads();
        if (s0 + PR_KP < S) pr_panel_load(p, x, cnt, T, S, Sp, ncols, t0, b0, s0 + PR_KP, tid);   // (workgroup-uniform)
#pragma unroll
        for (int ks = 0; ks < PR_KP / 4; ++ks) {
            const int k = 4 * ks + kk;
            double a[2], b[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) a[i] = xs[k * PR_XS + wt + 16 * i + r];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = cs[k * PR_CS + wb + 16 * j + r];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
        }
    }
}

// rl[t][b] for a chunk's columns: the walk, then every score stored
__global__ __launch_bounds__(256) void pr_replicates(const double* __restrict__ x, const uint16_t* __restrict__ cnt, int T, int S, size_t Sp, int ncols,
                                                     double* __restrict__ rl, size_t ldr) {
    __shared__ __attribute__((aligned(16))) double xs[PR_KP * PR_XS];
    __shared__ __attribute__((aligned(16))) double cs[PR_KP * PR_CS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t0 = blockIdx.x * PR_TT, b0 = blockIdx.y * PR_TB;
    const int wt = (wave & 1) * 32, wb = (wave >> 1) * 64;
    const int r = lane & 15, kk = lane >> 4;
    pr_d4 acc[2][4];
    pr_walk(acc, x, cnt, T, S, Sp, ncols, t0, b0, xs, cs);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = b0 + wb + 16 * j + r;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int t = t0 + wt + 16 * i + kk + 4 * g;
                if (t < T && b < ncols) rl[(size_t)t * ldr + b] = acc[i][j][g];
            }
        }
}

// best[b] = the first greatest rl[.][b] over the chunk's n replicate columns, wins[best[b]] += 1.  64 columns x 16 slices of
// trees per workgroup: a slice scans its contiguous range in ascending t, the slices are joined in ascending order, both with a
// strict >, so ties go to the lowest t.
__global__ __launch_bounds__(1024) void pr_best(const double* __restrict__ rl, size_t ldr, int T, int n, int32_t* __restrict__ best,
                                                unsigned long long* __restrict__ wins) {
    __shared__ double v_s[16][64];
    __shared__ int32_t t_s[16][64];
    const int col = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int b = blockIdx.x * 64 + col;
    const int per = (T + 15) / 16;
    const int ta = slice * per, tb = ta + per < T ? ta + per : T;
    double v = -pm_inf();
    int32_t at = -1;
    if (b < n)
        for (int t = ta; t < tb; ++t) {
            const double y = rl[(size_t)t * ldr + b];
            if (at < 0 || y > v) { v = y; at = t; }
        }
    v_s[slice][col] = v;
    t_s[slice][col] = at;
    __syncthreads();
    if (slice == 0 && b < n) {
        for (int q = 1; q < 16; ++q)
            if (t_s[q][col] >= 0 && (at < 0 || v_s[q][col] > v)) { v = v_s[q][col]; at = t_s[q][col]; }
        best[b] = at;
        atomicAdd(wins + at, 1ull);
    }
}

// column `col` of the scores as a dense vector (the observed scores)
__global__ __launch_bounds__(256) void pr_column(const double* __restrict__ rl, size_t ldr, size_t col, int T, double* __restrict__ out) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < T) out[t] = rl[(size_t)t * ldr + col];
}

#endif  // __HIPCC__

// ------------------------------------------------------------------------------------------------
// host: the checks of phylo_rell and the contract as a loop (phylo_debug_rell_host), over the functions above; a plain host
// compiler can build this part on its own (tests/rell_asan_main.cpp)
// ------------------------------------------------------------------------------------------------
// 0: fine; otherwise a message
inline int pr_check_shape(int T, int S, int B, char* msg, size_t nmsg) {
    if (T < 1) { snprintf(msg, nmsg, "need T >= 1 trees (T=%d)", T); return 1; }
    if (S < 1 || S > PR_MAX_SITES) { snprintf(msg, nmsg, "need 1 <= S <= %d sites (S=%d)", PR_MAX_SITES, S); return 1; }
    if (B < 1 || B > PR_MAX_REPS) { snprintf(msg, nmsg, "need 1 <= B <= %d replicates (B=%d)", PR_MAX_REPS, B); return 1; }
    return 0;
}

inline int pr_check_factors(int T, int S, const double* site_lik, char* msg, size_t nmsg) {
    for (int t = 0; t < T; ++t)
        for (int s = 0; s < S; ++s)
            if (!pr_factor_ok(site_lik[(size_t)t * S + s])) {
                snprintf(msg, nmsg, "tree %d, site %d: site factor %g is not a finite number > 0", t, s, site_lik[(size_t)t * S + s]);
                return 1;
            }
    return 0;
}

inline void pr_host_counts(int S, uint32_t b, uint64_t seed, int32_t* cnt /*[S], zeroed here*/) {
    for (int s = 0; s < S; ++s) cnt[s] = 0;
    for (int j = 0; j < S; j += 4) {
        const pm_u32x4 r = pr_draw_block(b, (uint32_t)(j >> 2), seed);
        for (int w = 0; w < 4 && j + w < S; ++w) ++cnt[pr_site_of_word(pr_block_word(r, w), S)];
    }
}

inline double pr_host_chain(int S, const int32_t* cnt, const double* x) {
    double acc = 0.0;
    for (int s = 0; s < S; ++s) acc = pr_chain_step((double)cnt[s], x[s], acc);
    return acc;
}

// replicates b0 .. b0 + nB - 1: counts [nB][S], x [T][S], rl [T][nB]; any output may be NULL, site_lik too if only counts are wanted
inline int pr_rell_host(int T, int S, const double* site_lik, int b0, int nB, uint64_t seed, int32_t* counts, double* x, double* rl, char* msg,
                        size_t nmsg) {
    if (!site_lik && (x || rl)) { snprintf(msg, nmsg, "site_lik is NULL"); return 1; }
    if (b0 < 0 || nB < 0 || (long long)b0 + nB > PR_MAX_REPS) { snprintf(msg, nmsg, "need 0 <= b0 and b0 + nB <= %d", PR_MAX_REPS); return 1; }
    if (pr_check_shape(T, S, nB > 0 ? nB : 1, msg, nmsg)) return 1;
    if (site_lik && pr_check_factors(T, S, site_lik, msg, nmsg)) return 1;
    std::vector<double> xs;
    if (site_lik && (x || rl)) {
        xs.resize((size_t)T * S);
        for (size_t i = 0; i < xs.size(); ++i) xs[i] = pm_log(site_lik[i]);
        if (x) memcpy(x, xs.data(), xs.size() * 8);
    }
    std::vector<int32_t> row((size_t)S);
    for (int b = 0; b < nB && (counts || rl); ++b) {
        pr_host_counts(S, (uint32_t)(b0 + b), seed, row.data());
        if (counts) memcpy(counts + (size_t)b * S, row.data(), (size_t)S * 4);
        if (rl)
            for (int t = 0; t < T; ++t) rl[(size_t)t * nB + b] = pr_host_chain(S, row.data(), xs.data() + (size_t)t * S);
    }
    return 0;
}
