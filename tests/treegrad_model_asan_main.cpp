// The host half of phylo_treegrad_model.h as a program of its own, for the host compiler's sanitizers (test_treegrad_model_cpu.py):
// plans over a sweep of shapes (offsets ascending and aligned, the chunk and the grid cap within their bounds, the slab a plan
// describes large enough for what the host copies into it and the kernels write), the LDS of a launch at its edges, and the shapes
// that must be refused.
#include <cstdio>
#include <vector>

#include "phylo_treegrad_model.h"

static int failed = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            ++failed;                                                  \
            printf("line %d: %s\n", __LINE__, #cond);                 \
        }                                                              \
    } while (0)

int main() {
    const int Ns[] = {2, 3, 5, 12, 65, 512}, tiles[] = {1, 3, 17}, Ts[] = {1, 7, 4096}, Ps[] = {1, 2, 12, 16}, envs[] = {0, 1, 5};
    long plans = 0;
    for (int N : Ns)
        for (int nt : tiles)
            for (int T : Ts)
                for (int P : Ps)
                    for (int env : envs)
                        for (int form = 0; form < 4; ++form) {
                            const bool coded = form & 1, grad = form & 2;
                            ptm_plan p;
                            EXPECT(ptm_make_plan(N, nt, T, P, coded, grad, 256, env, &p) == 0);
                            ++plans;
                            const size_t R = (size_t)N - 1;
                            EXPECT(p.chunk >= 1 && p.chunk <= T && (env == 0 || p.chunk <= env));
                            EXPECT(p.chunk == 1 || (size_t)p.chunk * p.per_tree <= PTG_CHUNK_BYTES);
                            EXPECT(p.grid >= 1 && (size_t)p.grid <= (size_t)p.chunk * nt && p.grid <= 256 * PTG_WG_PER_CU);
                            EXPECT(p.grid == 1 || (size_t)p.grid * p.wg_store <= PTG_STORE_BYTES);
                            EXPECT(p.wg_store == R * PTG_U * PTG_SLOT_BYTES);
                            EXPECT(p.nm == P + 4);
                            const size_t offs[] = {p.o_prior, p.o_dirs, p.o_ops, p.o_dops, p.o_P, p.o_D, p.o_t, p.o_gap, p.o_tilev, p.o_out,
                                                   p.o_dtile, p.o_dout, p.o_mtile, p.o_mout, p.o_store, p.total};
                            const size_t n = (size_t)p.chunk;
                            // (with grad, ptg_dmats writes M' behind M and its second output, 2 R matrices, where D is built next)
                            const size_t need[] = {32, (size_t)P * 128, n * R * 16, n * R * 16, n * (grad ? 2 : 1) * R * 256, n * 2 * R * P * 128,
                                                   n * R * 16, coded ? n * R * 64 : 0, n * nt * 8, n * 8, grad ? n * nt * 2 * R * 8 : 0,
                                                   grad ? n * 2 * R * 8 : 0, n * nt * (P + 4) * 8, n * (P + 4) * 8, (size_t)p.grid * p.wg_store};
                            EXPECT(n * 2 * R * 128 <= need[5]);
                            for (int k = 0; k < 15; ++k) {
                                EXPECT(offs[k] % 256 == 0);
                                EXPECT(offs[k + 1] >= offs[k] + need[k]);
                            }
                            // a buffer of the plan's size takes every region's first and last byte
                            if (p.total < ((size_t)8 << 20)) {
                                std::vector<unsigned char> slab(p.total);
                                for (int k = 0; k < 15; ++k)
                                    if (need[k]) slab[offs[k]] = 1, slab[offs[k] + need[k] - 1] = 1;
                            }
                        }
    {   // the edges the issue names: N = 2 and 512, P = 1 and 16, T = 1, a chunk cap of 1
        ptm_plan p;
        EXPECT(ptm_make_plan(2, 1, 1, 1, true, true, 256, 0, &p) == 0 && p.chunk == 1 && p.grid == 1 && p.wg_store == 4096);
        EXPECT(ptm_make_plan(512, 2, 11, 16, true, true, 256, 1, &p) == 0 && p.chunk == 1 && p.grid == 2);
        EXPECT(ptm_make_plan(512, 2, 11, 16, true, true, 256, 0, &p) == 0 && p.chunk == 11 && p.grid == 22);
        EXPECT(ptm_make_plan(512, 1, 4096, 16, false, false, 256, 0, &p) == 0 && (size_t)p.chunk * p.per_tree <= PTG_CHUNK_BYTES &&
               (size_t)(p.chunk + 1) * p.per_tree > PTG_CHUNK_BYTES && p.grid == p.chunk);
        // the LDS of a launch: the issue's 52 KiB at N = 512, P = 16 with nine slots, and the deepest schedule still inside 64 KiB
        EXPECT(ptm_lds_bytes(512, 9, 16, true) == (size_t)9 * 4096 + 2 * 511 * 8 + 16 * 64 * 8);
        EXPECT(ptm_lds_bytes(512, 9, 16, true) <= (size_t)52 << 10);
        EXPECT(ptm_lds_bytes(512, 10, 16, true) <= PTM_MAX_LDS);
        EXPECT(ptm_lds_bytes(2, 1, 1, false) == 4096 + 512);
        EXPECT(ptm_lds_bytes(512, 10, 16, false) + 2 * 511 * 8 == ptm_lds_bytes(512, 10, 16, true));
        EXPECT(ptm_lds_bytes(512, 14, 16, true) > PTM_MAX_LDS);          // what a call would be refused for
        // shapes without a plan
        EXPECT(ptm_make_plan(1, 1, 1, 4, true, true, 256, 0, &p) == 1);
        EXPECT(ptm_make_plan(5, 0, 1, 4, true, true, 256, 0, &p) == 1);
        EXPECT(ptm_make_plan(5, 1, 0, 4, true, true, 256, 0, &p) == 1);
        EXPECT(ptm_make_plan(5, 1, 1, 0, true, true, 256, 0, &p) == 1);
        EXPECT(ptm_make_plan(5, 1, 1, 17, true, true, 256, 0, &p) == 1);
        EXPECT(ptm_make_plan(5, 1, 1, -3, true, true, 256, 0, &p) == 1);
        EXPECT(ptm_make_plan(5, 1, 1, 4, true, true, 0, 0, &p) == 1);
    }
    printf("%ld plans; %d checks failed\n", plans, failed);
    return failed ? 1 : 0;
}
