// The host half of phylo_treegrad_rates.h as a program of its own, for the host compiler's sanitizers (test_treegrad_rates_cpu.py):
// plans over a sweep of shapes (offsets ascending and aligned, the chunk and the grid cap within their bounds, the slab a plan
// describes large enough for what the host copies into it), the mixture checks and the coefficient block.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "phylo_treegrad_rates.h"

static int failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            ++failed;                                                  \
            printf("line %d: %s\n", __LINE__, #cond);                 \
        }                                                              \
    } while (0)

int main() {
    const int Ns[] = {2, 3, 5, 12, 65, 512}, tiles[] = {1, 3, 17}, Ts[] = {1, 7, 4096}, Cs[] = {1, 2, 5, 16}, envs[] = {0, 1, 5};
    long plans = 0;
    for (int N : Ns)
        for (int nt : tiles)
            for (int T : Ts)
                for (int C : Cs)
                    for (int env : envs)
                        for (int form = 0; form < 8; ++form) {
                            const bool coded = form & 1, curv = form & 2, params = form & 4;
                            ptgr_plan p;
                            EXPECT(ptgr_make_plan(N, nt, T, C, coded, curv, params, 256, env, &p) == 0);
                            ++plans;
                            const size_t R = (size_t)N - 1;
                            EXPECT(p.wg_store == (size_t)C * R * PTG_U * PTG_SLOT_BYTES);
                            EXPECT(p.nq == (curv ? 2 : 1) && p.np == (params ? 2 : 0) && p.ncoef == 3 * C);
                            // chunk and grid within their bounds, offsets ascending and aligned, regions apart and inside the slab
                            pts_region r[PTS_MAX_REGIONS];
                            const int nr = ptgr_regions(N, nt, C, coded, p, r);
                            const pts_plan_facts f = ptg_plan_facts(p, nt, T, 256, env, 0);
                            EXPECT(pts_check_plan(r, nr, f) == 0);
                            // a buffer of the plan's size takes every region end to end
                            if (p.total < ((size_t)8 << 20)) {
                                std::vector<unsigned char> slab(p.total);
                                EXPECT(pts_fill_plan(r, nr, f, slab.data()) == 0);
                            }
                        }
    {   // shapes without a plan
        ptgr_plan p;
        EXPECT(ptgr_make_plan(1, 1, 1, 4, true, true, true, 256, 0, &p) == 1);
        EXPECT(ptgr_make_plan(5, 0, 1, 4, true, true, true, 256, 0, &p) == 1);
        EXPECT(ptgr_make_plan(5, 1, 0, 4, true, true, true, 256, 0, &p) == 1);
        EXPECT(ptgr_make_plan(5, 1, 1, 0, true, true, true, 256, 0, &p) == 1);
        EXPECT(ptgr_make_plan(5, 1, 1, 17, true, true, true, 256, 0, &p) == 1);
        EXPECT(ptgr_make_plan(5, 1, 1, 4, true, true, true, 0, 0, &p) == 1);
        // the shapes DESIGN.md names: DS1 (27 taxa) under 4 categories, and 512 taxa under 16
        EXPECT(ptgr_make_plan(27, 4, 4096, 4, true, true, true, 256, 0, &p) == 0 && p.wg_store == (size_t)416 << 10);
        EXPECT(ptgr_make_plan(512, 2, 11, 16, true, true, true, 256, 0, &p) == 0 && p.grid == 8);
        EXPECT(ptgr_lds_bytes(512, 9, 16, true, true) <= PTGR_MAX_LDS);
        EXPECT(ptgr_lds_bytes(512, 9, 16, true, true) == (size_t)9 * 4096 + 2 * 2 * 511 * 8 + 16 * 65 * 8);
    }
    {   // the mixture of a tree
        const int N = 4, C = 3;
        double blen[6] = {0.1, 0.0, 0.3, 2.0, 0.5, 0.7}, rate[3] = {0.0, 0.5, 2.0}, weight[3] = {0.2, 0.0, 0.8};
        char msg[200];
        EXPECT(ptgr_check_mixture(N, blen, C, rate, weight, msg, sizeof msg) == 0);
        const double bad[] = {-1e-9, std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity()};
        for (double v : bad) {
            rate[2] = v;
            EXPECT(ptgr_check_mixture(N, blen, C, rate, weight, msg, sizeof msg) == 1 && strstr(msg, "rate") && strstr(msg, "category 2"));
            rate[2] = 2.0;
            weight[1] = v;
            EXPECT(ptgr_check_mixture(N, blen, C, rate, weight, msg, sizeof msg) == 1 && strstr(msg, "weight") && strstr(msg, "category 1"));
            weight[1] = 0.0;
        }
        blen[3] = 1e308;
        EXPECT(ptgr_check_mixture(N, blen, C, rate, weight, msg, sizeof msg) == 1 && strstr(msg, "row 1, category 2"));
        char tiny[8];                                       // a short message buffer is not overrun
        EXPECT(ptgr_check_mixture(N, blen, C, rate, weight, tiny, sizeof tiny) == 1 && strlen(tiny) < sizeof tiny);
        double coef[9];
        ptgr_coefficients(C, rate, weight, coef);
        for (int k = 0; k < C; ++k) {
            EXPECT(coef[k] == weight[k] && coef[C + k] == weight[k] * rate[k] && coef[2 * C + k] == (weight[k] * rate[k]) * rate[k]);
        }
    }
    printf("%ld plans; %d checks failed\n", plans, failed);
    return failed ? 1 : 0;
}
