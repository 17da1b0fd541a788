// Stand-alone host program for tests/test_rell_multiscale_cpu.py: the host half of phylo_amd/csrc/phylo_rell_ms.h -- the shape
// checks, the column -> (scale, replicate) map, the chunk plan and the loop that phylo_debug_rell_multiscale_host runs -- on
// exactly sized heap buffers (built with -fsanitize=address,undefined, a byte read or written outside a buffer ends the
// program), every output checked against its definition.  No GPU, nothing of the library.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "phylo_rell_ms.h"

static unsigned int g_x = 2463534242u;
static unsigned int rnd() { g_x = g_x * 1664525u + 1013904223u; return g_x >> 8; }

static long one_case(int T, int S, int K, const int32_t* draws, int k0, int b0, int nB, uint64_t seed) {
    long bad = 0;
    char msg[200];
    double* f = (double*)malloc((size_t)T * S * 8);
    double* rl = (double*)malloc((size_t)T * nB * 8);
    int32_t* cnt = (int32_t*)malloc((size_t)nB * S * 4);
    int32_t* cnt2 = (int32_t*)malloc((size_t)nB * S * 4);
    int32_t* best = (int32_t*)malloc((size_t)nB * 4);
    int32_t* best2 = (int32_t*)malloc((size_t)nB * 4);
    if (!f || !rl || !cnt || !cnt2 || !best || !best2) return 1000000;
    for (int i = 0; i < T * S; ++i) f[i] = exp(-1.0 - 29.0 * (rnd() % 100000) / 100000.0);
    f[0] = 5e-324;
    f[T * S - 1] = 1.0;
    f[(T * S) / 2] = 3.75;
    if (T > 2) memcpy(f + (size_t)(T - 1) * S, f + (size_t)1 * S, (size_t)S * 8);       // two identical rows: a tie goes to the lower one
    if (prm_rell_host(T, S, f, K, draws, k0, b0, nB, seed, cnt, rl, best, msg, sizeof msg)) return 1000000;
    for (int b = 0; b < nB; ++b) {
        long sum = 0;
        for (int s = 0; s < S; ++s) { sum += cnt[(size_t)b * S + s]; bad += cnt[(size_t)b * S + s] < 0; }
        bad += sum != draws[k0];
        int at = 0;
        for (int t = 0; t < T; ++t) {                                         // the chain once more, zero counts skipped: the same bits
            double acc = 0.0;
            for (int s = 0; s < S; ++s)
                if (cnt[(size_t)b * S + s]) acc = fma((double)cnt[(size_t)b * S + s], pm_log(f[(size_t)t * S + s]), acc);
            bad += pm_bits(acc) != pm_bits(rl[(size_t)t * nB + b]);
            if (rl[(size_t)t * nB + b] > rl[(size_t)at * nB + b]) at = t;     // first greatest
        }
        bad += best[b] != at;
        if (T > 2) bad += best[b] == T - 1;                                   // (the copy never wins)
    }
    // counts alone (no factors), best alone, and a window of one replicate: the same rows
    if (prm_rell_host(T, S, nullptr, K, draws, k0, b0, nB, seed, cnt2, nullptr, nullptr, msg, sizeof msg)) return 1000000;
    for (int i = 0; i < nB * S; ++i) bad += cnt2[i] != cnt[i];
    if (prm_rell_host(T, S, f, K, draws, k0, b0, nB, seed, nullptr, nullptr, best2, msg, sizeof msg)) return 1000000;
    for (int b = 0; b < nB; ++b) bad += best2[b] != best[b];
    if (prm_rell_host(T, S, f, K, draws, k0, b0 + nB - 1, 1, seed, cnt2, nullptr, best2, msg, sizeof msg)) return 1000000;
    for (int s = 0; s < S; ++s) bad += cnt2[s] != cnt[(size_t)(nB - 1) * S + s];
    bad += best2[0] != best[nB - 1];
    // refusals write nothing and say where
    f[T * S - 1] = 0.0;
    bad += !prm_rell_host(T, S, f, K, draws, k0, b0, nB, seed, cnt, rl, best, msg, sizeof msg);
    char want[64];
    snprintf(want, sizeof want, "tree %d, site %d", T - 1, S - 1);
    bad += !strstr(msg, want);
    bad += !prm_rell_host(T, S, f, K, draws, K, b0, nB, seed, cnt, rl, best, msg, sizeof msg);
    free(f); free(rl); free(cnt); free(cnt2); free(best); free(best2);
    return bad;
}

// the chunk plan walks every column once, in order, within its bounds
static long plan_case(int T, int S, int K, int B, bool scores, int cap, const int32_t* draws) {
    long bad = 0;
    const int chunk = prm_chunk_cols(T, S, K, B, scores, cap);
    const size_t all = (size_t)K * B;
    bad += chunk < 1 || (size_t)chunk > all || chunk > PRM_MAX_COLS || (cap > 0 && chunk > cap);
    bad += chunk > 1 && (size_t)chunk * prm_col_bytes(T, S, scores) > PR_CHUNK_BYTES;
    size_t seen = 0;
    for (size_t c0 = 0; c0 < all; c0 += (size_t)chunk) {
        const size_t n = all - c0 < (size_t)chunk ? all - c0 : (size_t)chunk;
        int m = 0;
        for (size_t c = c0; c < c0 + n; ++c) {
            const uint32_t k = prm_col_scale((uint32_t)c, (uint32_t)B), b = prm_col_rep((uint32_t)c, (uint32_t)B);
            bad += k >= (uint32_t)K || b >= (uint32_t)B || (size_t)k * B + b != c;
            if (draws[k] > m) m = draws[k];
            ++seen;
        }
        bad += prm_max_draws(draws, B, c0, n) != m;
    }
    bad += seen != all;
    return bad;
}

int main() {
    long bad = 0;
    const int32_t d1[] = {65535}, d5[] = {1, 3, 8}, d37[] = {18, 37, 52}, d1949[] = {975, 1949, 2729};
    bad += one_case(1, 1, 1, d1, 0, 0, 2, 7);
    for (int k = 0; k < 3; ++k) {
        bad += one_case(1, 5, 3, d5, k, 0, 1, 7);
        bad += one_case(3, 5, 3, d5, k, 69, 5, 0x9E3779B97F4A7C15ull);
        bad += one_case(5, 37, 3, d37, k, 3, 4, 1);
        bad += one_case(3, 1949, 3, d1949, k, PR_MAX_REPS - 2, 2, 1);
    }
    char msg[200];
    int32_t dbad[PRM_MAX_SCALES + 1];
    for (int k = 0; k <= PRM_MAX_SCALES; ++k) dbad[k] = 10;
    bad += prm_check_shape(1, 5, PRM_MAX_SCALES, dbad, 1, msg, sizeof msg) || !prm_check_shape(1, 5, PRM_MAX_SCALES + 1, dbad, 1, msg, sizeof msg) ||
           !prm_check_shape(1, 5, 0, dbad, 1, msg, sizeof msg) || !prm_check_shape(1, 5, 2, nullptr, 1, msg, sizeof msg) ||
           !prm_check_shape(0, 5, 2, dbad, 1, msg, sizeof msg) || !prm_check_shape(1, 5, 2, dbad, PR_MAX_REPS + 1, msg, sizeof msg);
    dbad[3] = 0;
    bad += !prm_check_shape(1, 5, 4, dbad, 1, msg, sizeof msg) || !strstr(msg, "k=3") || prm_check_shape(1, 5, 3, dbad, 1, msg, sizeof msg);
    dbad[3] = PRM_MAX_DRAWS + 1;
    bad += !prm_check_shape(1, 5, 4, dbad, 1, msg, sizeof msg) || !strstr(msg, "k=3");
    dbad[3] = PRM_MAX_DRAWS;
    bad += prm_check_shape(1, 5, 4, dbad, 1, msg, sizeof msg);
    bad += plan_case(5, 37, 3, 150, true, 0, d37) + plan_case(5, 37, 3, 150, false, 100, d37) + plan_case(130, 37, 3, 150, true, 7, d37);
    bad += plan_case(4096, 1949, 3, 40000, false, 0, d1949) + plan_case(4096, 1949, 3, 40000, true, 0, d1949);
    bad += plan_case(1 << 20, 65535, 1, 40, true, 0, d1) + plan_case(3, 5, 3, 4, false, 1, d5);   // few columns fit; one at a time
    bad += prm_col_bytes(64, 4, false) != 8 + 12 + 4 || prm_col_bytes(65, 5, true) != 16 + 24 + 4 + 65 * 8;
    bad += !prm_beats(1.0, 3, 1.0, 5) || prm_beats(1.0, 5, 1.0, 3) || !prm_beats(-2.0, 0, 0.0, -1) || prm_beats(0.0, -1, -2.0, 0) ||
           !prm_beats(2.0, 9, 1.0, 0) || prm_beats(1.0, 0, 2.0, 9);
    printf("rell multiscale host: %ld values differ\n", bad);
    return bad ? 1 : 0;
}
