// Stand-alone host program for tests/test_treegrad_cpu.py: the host half of phylo_amd/csrc/phylo_treegrad.h -- the plan of a call
// (chunk of trees, slab layout, capped grid) and the downward operations of a scheduled tree -- on exactly sized heap buffers
// (built with -fsanitize=address,undefined, a byte read or written outside a buffer ends the program), every output checked
// against its definition.  No GPU, nothing of the library.
#include <stdio.h>
#include <stdlib.h>

#include "phylo_treegrad.h"

static unsigned int g_x = 2463534242u;
static unsigned int rnd() { g_x = g_x * 1664525u + 1013904223u; return g_x >> 8; }

static long check_plan(int N, int ntiles, int T, bool coded, bool curv, int n_cus, int env_chunk) {
    long bad = 0;
    ptg_plan p;
    if (ptg_make_plan(N, ntiles, T, coded, curv, n_cus, env_chunk, &p)) return 1000000;
    bad += p.nq != (curv ? 2 : 1);
    bad += p.wg_store != ((size_t)N - 1) * PTG_U * PTG_SLOT_BYTES;
    // the chunk and the grid within their bounds; every region holds what the host carves from it, in order, 256-byte aligned,
    // inside the slab; the bytes of a tree are the sum of the list (pts_check_plan, over the plan's own regions)
    pts_region r[PTS_MAX_REGIONS];
    bad += pts_check_plan(r, ptg_regions(N, ntiles, coded, p, r), ptg_plan_facts(p, ntiles, T, n_cus, env_chunk, 0));
    return bad;
}

// a random tree in rows (children-first) and a schedule in row order: what ptg_down_ops needs of pt2_schedule is the row and which
// sources are leaves
static long check_down_ops(int N) {
    long bad = 0;
    const int R = N - 1;
    int32_t* child = (int32_t*)malloc((size_t)R * 2 * 4);
    int32_t* ops = (int32_t*)malloc((size_t)R * 4 * 4);
    int32_t* dops = (int32_t*)malloc((size_t)R * 4 * 4);
    int* roots = (int*)malloc((size_t)N * sizeof(int));
    if (!child || !ops || !dops || !roots) return 1000000;
    int n_roots = N;
    for (int i = 0; i < N; ++i) roots[i] = i;
    for (int i = 0; i < R; ++i) {
        for (int sd = 0; sd < 2; ++sd) {
            const int j = (int)(rnd() % (unsigned)n_roots);
            child[2 * i + sd] = roots[j];
            roots[j] = roots[--n_roots];
        }
        roots[n_roots++] = N + i;
        ops[4 * i] = 0;
        ops[4 * i + 1] = child[2 * i] < N ? child[2 * i] : ~0;
        ops[4 * i + 2] = child[2 * i + 1] < N ? child[2 * i + 1] : ~1;
        ops[4 * i + 3] = i;
    }
    bad += ptg_down_ops(N, child, ops, dops) != 0;
    for (int i = 0; i < R; ++i) {
        bad += dops[4 * i + 2] != i || dops[4 * i + 3] != 0;
        for (int sd = 0; sd < 2; ++sd) {
            const int ch = child[2 * i + sd], d = dops[4 * i + sd];
            bad += ch < N ? d != ch : (d >= 0 || ~d != ch - N || ~d >= i);
        }
    }
    // refusals: a row out of range, the root not last, a child from a later row, a leaf where the schedule has a slot
    const int32_t keep = ops[3];
    ops[3] = R;
    bad += !ptg_down_ops(N, child, ops, dops);
    ops[3] = -1;
    bad += !ptg_down_ops(N, child, ops, dops);
    ops[3] = keep;
    if (R > 1) {
        ops[4 * (R - 1) + 3] = 0;
        bad += !ptg_down_ops(N, child, ops, dops);
        ops[4 * (R - 1) + 3] = R - 1;
        const int32_t c0 = child[0];
        child[0] = N + R - 1;
        bad += !ptg_down_ops(N, child, ops, dops);
        child[0] = c0;
    }
    ops[1] = ~ops[1];
    bad += !ptg_down_ops(N, child, ops, dops);
    free(child); free(ops); free(dops); free(roots);
    return bad;
}

int main() {
    long bad = 0;
    const int Ns[] = {2, 3, 5, 12, 33, 70, 128, 512};
    const int tiles[] = {1, 3, 64};
    const int Ts[] = {1, 5, 37, 4096, 1 << 20};
    const int cus[] = {1, 64, 256, 304};
    for (int N : Ns)
        for (int nt : tiles)
            for (int T : Ts)
                for (int cu : cus)
                    for (int flags = 0; flags < 4; ++flags) {
                        bad += check_plan(N, nt, T, flags & 1, flags & 2, cu, 0);
                        bad += check_plan(N, nt, T, flags & 1, flags & 2, cu, 5);
                    }
    bad += check_plan(512, 0x7fffffff / 2, 1 << 20, true, true, 256, 0);           // items of a chunk stay within an int
    ptg_plan p;
    bad += !ptg_make_plan(1, 1, 1, false, false, 1, 0, &p) || !ptg_make_plan(5, 0, 1, false, false, 1, 0, &p) ||
           !ptg_make_plan(5, 1, 0, false, false, 1, 0, &p) || !ptg_make_plan(5, 1, 1, false, false, 0, 0, &p);
    for (int N : Ns)
        for (int rep = 0; rep < 3; ++rep) bad += check_down_ops(N);
    printf("treegrad host: %ld values differ\n", bad);
    return bad ? 1 : 0;
}
