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
                            EXPECT(p.wg_store == R * PTG_U * PTG_SLOT_BYTES);
                            EXPECT(p.nm == P + 4);
                            // chunk and grid within their bounds, offsets ascending and aligned, regions apart and inside the slab
                            pts_region r[PTS_MAX_REGIONS];
                            const int nr = ptm_regions(N, nt, P, coded, grad, p, r);
                            const pts_plan_facts f = ptg_plan_facts(p, nt, T, 256, env, 0);
                            EXPECT(pts_check_plan(r, nr, f) == 0);
                            // (with grad, ptg_dmats writes M' behind M and its second output, 2 R matrices, where D is built next)
                            EXPECT(r[5].off == &p.o_D && (size_t)p.chunk * 2 * R * 128 <= (size_t)p.chunk * r[5].bytes);
                            // a buffer of the plan's size takes every region end to end
                            if (p.total < ((size_t)8 << 20)) {
                                std::vector<unsigned char> slab(p.total);
                                EXPECT(pts_fill_plan(r, nr, f, slab.data()) == 0);
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
