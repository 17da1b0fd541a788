// Stand-alone host program for tests/test_treenni_rates_cpu.py: the host half of phylo_amd/csrc/phylo_treenni_rates.h -- the plan of
// a call (chunk of trees, slab layout, capped grid) and the LDS of a launch with its refusal -- every output checked against its
// definition (built with -fsanitize=address,undefined).  No GPU, nothing of the library.  With six arguments (N, site tiles, T, C,
// coded, compute units) it prints that call's chunk and grid instead.
#include <stdio.h>
#include <stdlib.h>

#include "phylo_treenni_rates.h"

static long check_plan(int N, int ntiles, int T, int C, bool coded, int n_cus, int env_chunk) {
    long bad = 0;
    ptnr_plan p;
    if (ptnr_make_plan(N, ntiles, T, C, coded, n_cus, env_chunk, &p)) return 1000000;
    const size_t R = (size_t)N - 1, n = (size_t)p.chunk, nc = (size_t)C;
    bad += p.chunk < T && (env_chunk <= 0 || p.chunk < env_chunk) && ((size_t)p.chunk + 1) * p.per_tree <= PTG_CHUNK_BYTES &&
           ((size_t)p.chunk + 1) * ntiles <= 0x7fffffffu;                          // ... and no tree more would fit
    // the grid: min(items, 8 per compute unit, 256 MiB of node stores), at least 1
    size_t want = PTG_STORE_BYTES / p.wg_store;
    if (want > (size_t)n_cus * PTG_WG_PER_CU) want = (size_t)n_cus * PTG_WG_PER_CU;
    if (want < 1) want = 1;
    if (want > n * ntiles) want = n * ntiles;
    bad += (size_t)p.grid != want;
    bad += p.wg_store != nc * R * PTG_U * PTG_SLOT_BYTES;
    // the chunk within its bounds (within the budget when it holds more than one tree), items within an int, the grid within its
    // caps; every region holds what the host carves from it, in order, 256-byte aligned, inside the slab, none overlapping the
    // next; per-tree bytes are what the regions of a chunk hold (pts_check_plan, over the plan's own regions)
    pts_region r[PTS_MAX_REGIONS];
    bad += pts_check_plan(r, ptnr_regions(N, ntiles, C, coded, p, r), ptg_plan_facts(p, ntiles, T, n_cus, env_chunk, 0));
    return bad;
}

int main(int argc, char** argv) {
    if (argc == 7) {               // N ntiles T C coded cus: the plan's chunk and grid, for tests/test_treenni_rates_edges_cpu.py
        ptnr_plan q;
        if (ptnr_make_plan(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]) != 0, atoi(argv[6]), 0, &q)) return 2;
        printf("chunk %d grid %d per_tree %zu wg_store %zu\n", q.chunk, q.grid, q.per_tree, q.wg_store);
        return 0;
    }
    long bad = 0;
    const int Ns[] = {2, 3, 4, 5, 12, 33, 70, 128, 511, 512};
    const int tiles[] = {1, 2, 3, 64};
    const int Ts[] = {1, 5, 37, 4096, 1 << 20};
    const int cus[] = {1, 64, 256, 304};
    const int Cs[] = {1, 2, 5, 16};
    for (int N : Ns)
        for (int nt : tiles)
            for (int T : Ts)
                for (int cu : cus)
                    for (int C : Cs)
                        for (int coded = 0; coded < 2; ++coded) {
                            bad += check_plan(N, nt, T, C, coded, cu, 0);
                            bad += check_plan(N, nt, T, C, coded, cu, 1);
                            bad += check_plan(N, nt, T, C, coded, cu, 5);
                        }
    bad += check_plan(512, 0x7fffffff / 2, 1 << 20, 16, true, 256, 0);             // items of a chunk stay within an int
    ptnr_plan p;
    bad += !ptnr_make_plan(1, 1, 1, 1, false, 1, 0, &p) || !ptnr_make_plan(5, 0, 1, 1, false, 1, 0, &p) || !ptnr_make_plan(5, 1, 0, 1, false, 1, 0, &p) ||
           !ptnr_make_plan(5, 1, 1, 1, false, 0, 0, &p) || !ptnr_make_plan(5, 1, 1, 0, false, 1, 0, &p) ||
           !ptnr_make_plan(5, 1, 1, PTGR_MAX_CATS + 1, false, 1, 0, &p);
    // the large corner: N = 512 under 16 categories is a 32 MiB store per workgroup, 8 workgroups, 9 slots + acc = 44 KiB of LDS
    bad += ptnr_make_plan(512, 2, 3, 16, true, 256, 0, &p) != 0 || p.grid != 6 || p.wg_store != ((size_t)16 * 511 * 4096);
    bad += ptnr_make_plan(512, 2, 64, 16, true, 256, 0, &p) != 0 || p.grid != 8;
    bad += ptnr_lds_bytes(512, 9) != (size_t)9 * 4096 + 2 * 511 * 8 || ptnr_lds_bytes(512, 9) > PTGR_MAX_LDS;
    // the refusal: the deepest schedule there is (10 slots, floor(log2 512) + 1) stays inside at every N up to 512 ...
    for (int N = 2; N <= 512; ++N) bad += ptnr_lds_bytes(N, 10) > PTGR_MAX_LDS;
    // ... and a launch that would not is refused by the same comparison the entry point makes
    bad += !(ptnr_lds_bytes(512, 15) > PTGR_MAX_LDS) || !(ptnr_lds_bytes(4097, 8) > PTGR_MAX_LDS) || ptnr_lds_bytes(2, 1) != 4096 + 16;
    printf("treenni_rates host: %ld values differ\n", bad);
    return bad ? 1 : 0;
}
