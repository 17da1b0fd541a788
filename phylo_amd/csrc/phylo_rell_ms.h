// phylo_rell_ms.h -- phylo_rell_multiscale: the multiscale RELL bootstrap behind the AU test.
// K scales; replicate b of scale k draws draws[k] sites (not S): draw j is word j & 3 of the Philox block at counter
// (b, k, STREAM_BOOT, j >> 2), the site (word * S) >> 32.  rl[k][t][b] is section 12's ONE fma chain with these counts, best[k][b]
// the lexicographic maximum of (rl, -t) over t, wins[k][t] its histogram.  The product is pr_replicates' (pr_walk, phylo_rell.h:
// same tiles, panels and operand lanes); its epilogue keeps every column's maximum and writes one (double, int32) partial per
// tree tile and column instead of the matrix, and a join kernel reads those.
#pragma once
#include "phylo_rell.h"

#define PRM_MAX_SCALES 64
#define PRM_MAX_DRAWS 65535                       // a count is uint16 and may reach draws[k]
#define PRM_MAX_COLS PR_MAX_REPS                  // columns of a chunk: grid.y of the product stays below 65536

// column c of the call (linear over scales, c = k B + b) -> its scale and its replicate
PM_HD uint32_t prm_col_scale(uint32_t c, uint32_t B) { return c / B; }
PM_HD uint32_t prm_col_rep(uint32_t c, uint32_t B) { return c % B; }

// counter word 1, which is 0 in phylo_rell, carries the scale: scale 0 shares its stream with phylo_rell
PM_HD pm_u32x4 prm_draw_block(uint32_t b, uint32_t k, uint32_t blk, uint64_t seed) { return pm_philox4x32(b, k, (uint32_t)PM_STREAM_BOOT, blk, seed); }

// (v, t) beats (bv, bt) in the order of (value, -t); t < 0: no candidate (rows past T leave by index, never by value)
PM_HD bool prm_beats(double v, int t, double bv, int bt) { return t >= 0 && (bt < 0 || v > bv || (v == bv && t < bt)); }

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
// pr_counts over columns with their own scale and draw count: row i / nblk of the chunk is column col0 + row of the call; nblk
// covers the largest draw count of the chunk's scales, a thread whose block lies past its column's draws leaves.  cnt zeroed beforehand.
__global__ __launch_bounds__(256) void prm_counts(unsigned int* __restrict__ cnt, int S, size_t Sp, uint32_t col0, uint32_t B,
                                                  const int32_t* __restrict__ draws, size_t n_threads, uint32_t nblk, uint64_t seed) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_threads) return;
    const uint32_t row = (uint32_t)(i / nblk), blk = (uint32_t)(i - (size_t)row * nblk);
    const uint32_t k = prm_col_scale(col0 + row, B), b = prm_col_rep(col0 + row, B);
    const int nd = draws[k];
    if ((int)(4 * blk) >= nd) return;
    const pm_u32x4 r = prm_draw_block(b, k, blk, seed);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if ((int)(4 * blk + w) < nd) {
            const size_t e = (size_t)row * Sp + pr_site_of_word(pr_block_word(r, w), S);
            atomicAdd(cnt + (e >> 1), 1u << (16 * (unsigned)(e & 1)));
        }
    }
}

// pr_replicates' product (pr_walk) with the column maxima in its epilogue.  Columns 0 .. nrep - 1 are replicates; column nrep,
// where ncols > nrep, is the row of ones, whose scores are stored as the observed scores.  Per tree tile (blockIdx.x) and
// replicate column one partial: pval / pidx [tile][ldp].  STORE: the scores go to rl [T][ldr] as well.
template <bool STORE>
__global__ __launch_bounds__(256) void prm_product(const double* __restrict__ x, const uint16_t* __restrict__ cnt, int T, int S, size_t Sp, int ncols,
                                                   int nrep, double* __restrict__ pval, int32_t* __restrict__ pidx, size_t ldp,
                                                   double* __restrict__ obs, double* __restrict__ rl, size_t ldr) {
    __shared__ __attribute__((aligned(16))) double xs[PR_KP * PR_XS];
    __shared__ __attribute__((aligned(16))) double cs[PR_KP * PR_CS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t0 = blockIdx.x * PR_TT, b0 = blockIdx.y * PR_TB;
    const int wt = (wave & 1) * 32, wb = (wave >> 1) * 64;
    const int r = lane & 15, kk = lane >> 4;
    pr_d4 acc[2][4];
    pr_walk(acc, x, cnt, T, S, Sp, ncols, t0, b0, xs, cs);
    // 1. a lane's eight trees of each of its four columns, ascending t; rows past T carry +0.0 and leave by their index
    double bv[4];
    int bt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int b = b0 + wb + 16 * j + r;
        bv[j] = 0.0;
        bt[j] = -1;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int t = t0 + wt + 16 * i + kk + 4 * g;
                const double v = acc[i][j][g];
                if (t < T) {
                    if (STORE && b < nrep) rl[(size_t)t * ldr + b] = v;
                    if (b == nrep && b < ncols) obs[t] = v;
                    if (prm_beats(v, t, bv[j], bt[j])) { bv[j] = v; bt[j] = t; }
                }
            }
        // 2. the four lane groups (lane bits 4 and 5) hold the other rows of the same column
#pragma unroll
        for (int m = 16; m <= 32; m <<= 1) {
            const double ov = __shfl_xor(bv[j], m);
            const int ot = __shfl_xor(bt[j], m);
            if (prm_beats(ov, ot, bv[j], bt[j])) { bv[j] = ov; bt[j] = ot; }
        }
    }
    // 3. the workgroup's two tree halves, through the panels' LDS
    double* jv = xs;                                        // [2][PR_TB]
    int* jt = (int*)cs;                                     // [2][PR_TB]
    __syncthreads();                                        // the waves are done with the last panel
    if (kk == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            jv[(wave & 1) * PR_TB + wb + 16 * j + r] = bv[j];
            jt[(wave & 1) * PR_TB + wb + 16 * j + r] = bt[j];
        }
    }
    __syncthreads();
    if (tid < PR_TB) {
        const int b = b0 + tid;
        double v = jv[tid];
        int t = jt[tid];
        if (prm_beats(jv[PR_TB + tid], jt[PR_TB + tid], v, t)) { v = jv[PR_TB + tid]; t = jt[PR_TB + tid]; }
        if (b < nrep) {
            pval[(size_t)blockIdx.x * ldp + b] = v;
            pidx[(size_t)blockIdx.x * ldp + b] = t;
        }
    }
}

// one thread per replicate column: the tree tiles' partials in ascending tile order, best[c], wins[k][best] += 1
__global__ __launch_bounds__(256) void prm_join(const double* __restrict__ pval, const int32_t* __restrict__ pidx, size_t ldp, int ntiles, int n,
                                                uint32_t col0, uint32_t B, int T, int32_t* __restrict__ best, unsigned long long* __restrict__ wins) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n) return;
    double v = pval[c];
    int t = pidx[c];
    for (int q = 1; q < ntiles; ++q) {
        const double ov = pval[(size_t)q * ldp + c];
        const int ot = pidx[(size_t)q * ldp + c];
        if (prm_beats(ov, ot, v, t)) { v = ov; t = ot; }
    }
    best[c] = t;
    atomicAdd(wins + (size_t)prm_col_scale(col0 + (uint32_t)c, B) * T + t, 1ull);
}

#endif  // __HIPCC__

// ------------------------------------------------------------------------------------------------
// host: shape checks, the chunk plan and the contract as a loop (phylo_debug_rell_multiscale_host); a plain host compiler builds
// this part on its own (tests/rell_ms_asan_main.cpp)
// ------------------------------------------------------------------------------------------------
inline int prm_check_shape(int T, int S, int K, const int32_t* draws, int B, char* msg, size_t nmsg) {
    if (pr_check_shape(T, S, B, msg, nmsg)) return 1;
    if (K < 1 || K > PRM_MAX_SCALES) { snprintf(msg, nmsg, "need 1 <= K <= %d scales (K=%d)", PRM_MAX_SCALES, K); return 1; }
    if (!draws) { snprintf(msg, nmsg, "draws is NULL"); return 1; }
    for (int k = 0; k < K; ++k)
        if (draws[k] < 1 || draws[k] > PRM_MAX_DRAWS) {
            snprintf(msg, nmsg, "scale k=%d: need 1 <= draws[k] <= %d, the uint16 count bound (draws[%d]=%d)", k, PRM_MAX_DRAWS, k, (int)draws[k]);
            return 1;
        }
    return 0;
}

// bytes a column takes of a chunk: its counts, one partial per tree tile, its best, and its scores when they are asked for
inline size_t prm_col_bytes(int T, int S, bool scores) {
    return pr_count_stride(S) * 2 + (size_t)((T + PR_TT - 1) / PR_TT) * 12 + 4 + (scores ? (size_t)T * 8 : 0);
}

// columns per chunk: what PR_CHUNK_BYTES holds (at least one), at most PRM_MAX_COLS, `cap` if > 0 (PHYLO_RELL_CHUNK), K B
inline int prm_chunk_cols(int T, int S, int K, int B, bool scores, int cap) {
    size_t fit = PR_CHUNK_BYTES / prm_col_bytes(T, S, scores);
    if (fit < 1) fit = 1;
    if (fit > (size_t)PRM_MAX_COLS) fit = PRM_MAX_COLS;
    if (cap > 0 && (size_t)cap < fit) fit = (size_t)cap;
    const size_t all = (size_t)K * B;
    return (int)(all < fit ? all : fit);
}

// the largest draw count among the scales of columns c0 .. c0 + n - 1
inline int prm_max_draws(const int32_t* draws, int B, size_t c0, size_t n) {
    int m = 0;
    for (uint32_t k = prm_col_scale((uint32_t)c0, (uint32_t)B); k <= prm_col_scale((uint32_t)(c0 + n - 1), (uint32_t)B); ++k)
        if (draws[k] > m) m = draws[k];
    return m;
}

inline void prm_host_counts(int S, int nd, uint32_t b, uint32_t k, uint64_t seed, int32_t* cnt /*[S], zeroed here*/) {
    for (int s = 0; s < S; ++s) cnt[s] = 0;
    for (int j = 0; j < nd; j += 4) {
        const pm_u32x4 r = prm_draw_block(b, k, (uint32_t)(j >> 2), seed);
        for (int w = 0; w < 4 && j + w < nd; ++w) ++cnt[pr_site_of_word(pr_block_word(r, w), S)];
    }
}

// scale k0, replicates b0 .. b0 + nB - 1: counts [nB][S], rl [T][nB], best [nB]; any output may be NULL, site_lik too if only
// counts are wanted
inline int prm_rell_host(int T, int S, const double* site_lik, int K, const int32_t* draws, int k0, int b0, int nB, uint64_t seed, int32_t* counts,
                         double* rl, int32_t* best, char* msg, size_t nmsg) {
    if (!site_lik && (rl || best)) { snprintf(msg, nmsg, "site_lik is NULL"); return 1; }
    if (b0 < 0 || nB < 0 || (long long)b0 + nB > PR_MAX_REPS) { snprintf(msg, nmsg, "need 0 <= b0 and b0 + nB <= %d", PR_MAX_REPS); return 1; }
    if (prm_check_shape(T, S, K, draws, nB > 0 ? nB : 1, msg, nmsg)) return 1;
    if (k0 < 0 || k0 >= K) { snprintf(msg, nmsg, "need 0 <= k0 < K (k0=%d, K=%d)", k0, K); return 1; }
    if (site_lik && pr_check_factors(T, S, site_lik, msg, nmsg)) return 1;
    std::vector<double> xs, col;
    if (rl || best) {
        xs.resize((size_t)T * S);
        for (size_t i = 0; i < xs.size(); ++i) xs[i] = pm_log(site_lik[i]);
        col.resize((size_t)T);
    }
    std::vector<int32_t> row((size_t)S);
    for (int b = 0; b < nB && (counts || rl || best); ++b) {
        prm_host_counts(S, draws[k0], (uint32_t)(b0 + b), (uint32_t)k0, seed, row.data());
        if (counts) memcpy(counts + (size_t)b * S, row.data(), (size_t)S * 4);
        if (!rl && !best) continue;
        double bv = 0.0;
        int bt = -1;
        for (int t = 0; t < T; ++t) {
            col[t] = pr_host_chain(S, row.data(), xs.data() + (size_t)t * S);
            if (prm_beats(col[t], t, bv, bt)) { bv = col[t]; bt = t; }
            if (rl) rl[(size_t)t * nB + b] = col[t];
        }
        if (best) best[b] = bt;
    }
    return 0;
}
