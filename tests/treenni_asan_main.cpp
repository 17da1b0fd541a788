// Stand-alone host program for tests/test_treenni_cpu.py: the host half of phylo_amd/csrc/phylo_treenni.h -- the plan of a call
// (chunk of trees, slab layout, capped grid) and the operations of an operation's children -- on exactly sized heap buffers (built
// with -fsanitize=address,undefined, a byte read or written outside a buffer ends the program), every output checked against its
// definition.  No GPU, nothing of the library.
#include <stdio.h>
#include <stdlib.h>

#include "phylo_treenni.h"

static unsigned int g_x = 2463534242u;
static unsigned int rnd() { g_x = g_x * 1664525u + 1013904223u; return g_x >> 8; }

static long check_plan(int N, int ntiles, int T, bool coded, int n_cus, int env_chunk) {
    long bad = 0;
    ptn_plan p;
    if (ptn_make_plan(N, ntiles, T, coded, n_cus, env_chunk, &p)) return 1000000;
    bad += p.wg_store != ((size_t)N - 1) * PTG_U * PTG_SLOT_BYTES;
    // the chunk and the grid within their bounds; every region holds what the host carves from it, in order, 256-byte aligned,
    // inside the slab; per-tree bytes are what the regions of a chunk hold (pts_check_plan, over the plan's own regions)
    pts_region r[PTS_MAX_REGIONS];
    bad += pts_check_plan(r, ptn_regions(N, ntiles, coded, p, r), ptg_plan_facts(p, ntiles, T, n_cus, env_chunk, 0));
    return bad;
}

// a random tree in rows (children-first) under two schedules: the rows in their order, and the rows children-first from the root
// with the right child first; what ptn_nni_ops needs of pt2_schedule is the row of every operation
static long check_nni_ops(int N, int order) {
    long bad = 0;
    const int R = N - 1;
    int32_t* child = (int32_t*)malloc((size_t)R * 2 * 4);
    int32_t* ops = (int32_t*)malloc((size_t)R * 4 * 4);
    int32_t* dops = (int32_t*)malloc((size_t)R * 4 * 4);
    int32_t* nops = (int32_t*)malloc((size_t)R * 4 * 4);
    int* roots = (int*)malloc((size_t)N * sizeof(int));
    int* seq = (int*)malloc((size_t)R * sizeof(int));
    int* stack = (int*)malloc((size_t)2 * N * sizeof(int));
    if (!child || !ops || !dops || !nops || !roots || !seq || !stack) return 1000000;
    int n_roots = N;
    for (int i = 0; i < N; ++i) roots[i] = i;
    for (int i = 0; i < R; ++i) {
        for (int sd = 0; sd < 2; ++sd) {
            const int j = (int)(rnd() % (unsigned)n_roots);
            child[2 * i + sd] = roots[j];
            roots[j] = roots[--n_roots];
        }
        roots[n_roots++] = N + i;
    }
    if (order == 0) {
        for (int i = 0; i < R; ++i) seq[i] = i;
    } else {                                                // the root first, then the left child's rows ...: read backwards
        int n_seq = 0, top = 0;
        stack[top++] = R - 1;
        while (top) {
            const int r = stack[--top];
            seq[R - 1 - n_seq++] = r;
            for (int sd = 0; sd < 2; ++sd)
                if (child[2 * r + sd] >= N) stack[top++] = child[2 * r + sd] - N;
        }
        bad += n_seq != R;
    }
    for (int i = 0; i < R; ++i) {
        const int r = seq[i];
        ops[4 * i] = 0;
        ops[4 * i + 1] = child[2 * r] < N ? child[2 * r] : ~0;
        ops[4 * i + 2] = child[2 * r + 1] < N ? child[2 * r + 1] : ~1;
        ops[4 * i + 3] = r;
    }
    bad += ptg_down_ops(N, child, ops, dops) != 0;
    bad += ptn_nni_ops(N, ops, dops, nops) != 0;
    for (int i = 0; i < R; ++i) {
        bad += nops[4 * i + 2] != 0 || nops[4 * i + 3] != 0;
        for (int sd = 0; sd < 2; ++sd) {
            const int ch = child[2 * seq[i] + sd], j = nops[4 * i + sd];
            bad += ch < N ? j != -1 : (j < 0 || j >= i || seq[j] != ch - N);
        }
    }
    // refusals: a row out of range, a row with two operations, a parent's operation before its child's
    const int32_t keep = ops[3];
    ops[3] = R;
    bad += !ptn_nni_ops(N, ops, dops, nops);
    ops[3] = -1;
    bad += !ptn_nni_ops(N, ops, dops, nops);
    ops[3] = keep;
    if (R > 1) {
        ops[7] = ops[3];
        bad += !ptn_nni_ops(N, ops, dops, nops);
        ops[7] = seq[1];
        int32_t t4[4], d4[4];                               // the root's operation first: its internal child has none yet
        for (int k = 0; k < 4; ++k) { t4[k] = ops[k]; d4[k] = dops[k]; ops[k] = ops[4 * (R - 1) + k]; dops[k] = dops[4 * (R - 1) + k]; }
        for (int k = 0; k < 4; ++k) { ops[4 * (R - 1) + k] = t4[k]; dops[4 * (R - 1) + k] = d4[k]; }
        if (N > 2) bad += !ptn_nni_ops(N, ops, dops, nops);
    }
    free(child); free(ops); free(dops); free(nops); free(roots); free(seq); free(stack);
    return bad;
}

int main() {
    long bad = 0;
    const int Ns[] = {2, 3, 4, 5, 12, 33, 70, 128, 511, 512};
    const int tiles[] = {1, 2, 3, 64};
    const int Ts[] = {1, 5, 37, 4096, 1 << 20};
    const int cus[] = {1, 64, 256, 304};
    for (int N : Ns)
        for (int nt : tiles)
            for (int T : Ts)
                for (int cu : cus)
                    for (int coded = 0; coded < 2; ++coded) {
                        bad += check_plan(N, nt, T, coded, cu, 0);
                        bad += check_plan(N, nt, T, coded, cu, 1);
                        bad += check_plan(N, nt, T, coded, cu, 5);
                    }
    bad += check_plan(512, 0x7fffffff / 2, 1 << 20, true, 256, 0);                 // items of a chunk stay within an int
    ptn_plan p;
    bad += !ptn_make_plan(1, 1, 1, false, 1, 0, &p) || !ptn_make_plan(5, 0, 1, false, 1, 0, &p) || !ptn_make_plan(5, 1, 0, false, 1, 0, &p) ||
           !ptn_make_plan(5, 1, 1, false, 0, 0, &p);
    for (int N = 2; N <= 512; N += (N < 40 ? 1 : 59))
        for (int order = 0; order < 2; ++order) bad += check_nni_ops(N, order);
    for (int order = 0; order < 2; ++order) bad += check_nni_ops(512, order);
    printf("treenni host: %ld values differ\n", bad);
    return bad ? 1 : 0;
}
