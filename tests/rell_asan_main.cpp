// Stand-alone host program for tests/test_rell_cpu.py: the host half of phylo_amd/csrc/phylo_rell.h -- the checks and the loop
// that phylo_debug_rell_host runs -- on exactly sized heap buffers (built with -fsanitize=address,undefined, a byte read or written
// outside a buffer ends the program), every output checked against its definition.  No GPU, nothing of the library.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "phylo_rell.h"

static unsigned int g_x = 2463534242u;
static unsigned int rnd() { g_x = g_x * 1664525u + 1013904223u; return g_x >> 8; }

static long one_case(int T, int S, int b0, int nB, uint64_t seed) {
    long bad = 0;
    char msg[200];
    double* f = (double*)malloc((size_t)T * S * 8);
    double* x = (double*)malloc((size_t)T * S * 8);
    double* rl = (double*)malloc((size_t)T * nB * 8);
    int32_t* cnt = (int32_t*)malloc((size_t)nB * S * 4);
    int32_t* cnt2 = (int32_t*)malloc((size_t)nB * S * 4);
    if (!f || !x || !rl || !cnt || !cnt2) return 1000000;
    for (int i = 0; i < T * S; ++i) f[i] = exp(-1.0 - 29.0 * (rnd() % 100000) / 100000.0);
    f[0] = 5e-324;
    f[T * S - 1] = 1.0;
    f[(T * S) / 2] = 3.75;
    if (pr_rell_host(T, S, f, b0, nB, seed, cnt, x, rl, msg, sizeof msg)) return 1000000;
    for (int i = 0; i < T * S; ++i) bad += !(fabs(x[i] - log(f[i])) <= 1e-15 * fabs(log(f[i])));
    for (int b = 0; b < nB; ++b) {
        long sum = 0;
        for (int s = 0; s < S; ++s) { sum += cnt[(size_t)b * S + s]; bad += cnt[(size_t)b * S + s] < 0; }
        bad += sum != S;
        for (int t = 0; t < T; ++t) {                                         // the chain once more, zero counts skipped: the same bits
            double acc = 0.0;
            for (int s = 0; s < S; ++s)
                if (cnt[(size_t)b * S + s]) acc = fma((double)cnt[(size_t)b * S + s], x[(size_t)t * S + s], acc);
            bad += pm_bits(acc) != pm_bits(rl[(size_t)t * nB + b]);
        }
    }
    // counts alone (no factors), and a window of one replicate: the same rows
    if (pr_rell_host(T, S, nullptr, b0, nB, seed, cnt2, nullptr, nullptr, msg, sizeof msg)) return 1000000;
    for (int i = 0; i < nB * S; ++i) bad += cnt2[i] != cnt[i];
    if (pr_rell_host(T, S, f, b0 + nB - 1, 1, seed, cnt2, nullptr, nullptr, msg, sizeof msg)) return 1000000;
    for (int s = 0; s < S; ++s) bad += cnt2[s] != cnt[(size_t)(nB - 1) * S + s];
    // refusals write nothing and say where
    f[T * S - 1] = 0.0;
    bad += !pr_rell_host(T, S, f, b0, nB, seed, cnt, x, rl, msg, sizeof msg);
    char want[64];
    snprintf(want, sizeof want, "tree %d, site %d", T - 1, S - 1);
    bad += !strstr(msg, want);
    free(f); free(x); free(rl); free(cnt); free(cnt2);
    return bad;
}

int main() {
    long bad = 0;
    const int sizes[] = {1, 3, 4, 5, 63, 64, 65, 257, 1949};
    for (int S : sizes) {
        bad += one_case(1, S, 0, 1, 7);
        bad += one_case(3, S, 69, 5, 0x9E3779B97F4A7C15ull);
    }
    bad += one_case(2, PR_MAX_SITES, PR_MAX_REPS - 2, 2, 1);
    char msg[200];
    bad += !pr_check_shape(1, PR_MAX_SITES + 1, 1, msg, sizeof msg) || !pr_check_shape(0, 1, 1, msg, sizeof msg) ||
           !pr_check_shape(1, 1, 0, msg, sizeof msg) || !pr_check_shape(1, 1, PR_MAX_REPS + 1, msg, sizeof msg) ||
           pr_check_shape(1, PR_MAX_SITES, PR_MAX_REPS, msg, sizeof msg);
    bad += pr_count_stride(1) != 4 || pr_count_stride(4) != 4 || pr_count_stride(65) != 68 || pr_count_stride(PR_MAX_SITES) != 65536;
    const double nan = pm_nan();
    bad += pr_factor_ok(0.0) || pr_factor_ok(-0.0) || pr_factor_ok(-1.0) || pr_factor_ok(pm_inf()) || pr_factor_ok(nan) || !pr_factor_ok(5e-324) ||
           !pr_factor_ok(1.7976931348623157e308);
    printf("rell host: %ld values differ\n", bad);
    return bad ? 1 : 0;
}
