// Stand-alone host program for tests/test_treeanc_cpu.py: the host half of phylo_amd/csrc/phylo_treeanc.h -- the plan of a call of
// phylo_trees_ancestral (chunk of trees bounded by the slab, by the staging of the requested outputs and by the caller; slab
// layout; capped grid) -- built with -fsanitize=address,undefined, every output checked against its definition, and a plan's
// regions written end to end into a heap buffer of exactly the slab's size where that is small.  No GPU, nothing of the library.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "phylo_treeanc.h"

static size_t cell_bytes(unsigned outs) { return (outs & PTA_POST ? 32 : 0) + (outs & PTA_STATE ? 1 : 0) + (outs & PTA_PMAX ? 8 : 0); }

static long check_plan(int N, int S, int ntiles, int T, bool coded, unsigned outs, int n_cus, int env_chunk) {
    long bad = 0;
    pta_plan p;
    const size_t R = (size_t)N - 1, tree_out = R * (size_t)S * cell_bytes(outs);
    const int rc = pta_make_plan(N, S, ntiles, T, coded, outs, n_cus, env_chunk, &p);
    if (tree_out > PTA_OUT_MAX) return (rc != 2) + (p.out_tree != tree_out);          // refused, naming the size
    if (rc) return 1000000;
    const size_t n = (size_t)p.chunk;
    bad += p.out_tree != tree_out;
    bad += p.out_region != (tree_out > PTA_OUT_BYTES ? tree_out : PTA_OUT_BYTES);     // grows to one tree's need, never further
    // the chunk within the slab's budget (more than one tree), the caller's cap and T, its outputs within the staging region, its
    // items within an int; the grid within its caps; every region aligned, in order, apart and inside the slab
    pts_region r[PTS_MAX_REGIONS];
    const int nr = pta_regions(N, S, ntiles, coded, outs, p, r);
    const pts_plan_facts f = ptg_plan_facts(p, ntiles, T, n_cus, env_chunk, p.out_region);
    bad += pts_check_plan(r, nr, f);
    // the chunk is the SMALLEST of the three bounds: one more tree would break one of them (or there is none left)
    if (p.chunk < T && !(env_chunk > 0 && p.chunk == env_chunk))
        bad += (n + 1) * p.per_tree <= PTG_CHUNK_BYTES && (n + 1) * tree_out <= p.out_region && (n + 1) * (size_t)ntiles <= 0x7fffffffu;
    bad += p.wg_store != R * PTG_U * PTG_SLOT_BYTES;
    // the grid cap is ptg_make_plan's
    ptg_plan gp;
    if (!ptg_make_plan(N, ntiles, p.chunk, coded, false, n_cus, p.chunk, &gp)) bad += gp.chunk == p.chunk && gp.grid != p.grid;
    if (p.total <= ((size_t)8 << 20)) {                     // every region written end to end inside an exactly sized buffer
        unsigned char* slab = (unsigned char*)malloc(p.total);
        if (!slab) return 1000000;
        bad += pts_fill_plan(r, nr, f, slab);               // no region overwrote another
        free(slab);
    }
    return bad;
}

int main() {
    long bad = 0;
    const int Ns[] = {2, 3, 5, 12, 33, 128, 512};
    const int Ss[] = {1, 70, 4100};
    const int Ts[] = {1, 5, 37, 4096, 1 << 20};
    const int cus[] = {1, 64, 256};
    for (int N : Ns)
        for (int S : Ss)
            for (int T : Ts)
                for (int cu : cus)
                    for (unsigned outs = 1; outs < 8; ++outs)
                        for (int coded = 0; coded < 2; ++coded) {
                            const int nt = (S + 2047) / 2048;
                            bad += check_plan(N, S, nt, T, coded, outs, cu, 0);
                            bad += check_plan(N, S, nt, T, coded, outs, cu, 5);
                        }
    pta_plan p;
    // output-bound chunks: N = 128, S = 4100 with post takes 127 * 4100 * 32 B = 16.7 MB a tree -- 16 trees fill 256 MiB where the
    // slab alone would hold more than a thousand
    bad += pta_make_plan(128, 4100, 3, 4096, true, PTA_POST, 256, 0, &p) != 0;
    bad += p.chunk != (int)(PTA_OUT_BYTES / ((size_t)127 * 4100 * 32)) || p.chunk != 16;
    bad += pta_make_plan(128, 4100, 3, 4096, true, PTA_STATE, 256, 0, &p) != 0;       // states alone: 0.52 MB a tree, 515 of them
    bad += p.chunk != (int)(PTA_OUT_BYTES / ((size_t)127 * 4100));
    // one tree over 256 MiB: N = 512, S = 20000 with all three is 511 * 20000 * 41 B = 419 MB -- the region grows to it, one tree a chunk
    bad += check_plan(512, 20000, 10, 7, true, 7u, 256, 0);
    bad += pta_make_plan(512, 20000, 10, 7, true, 7u, 256, 0, &p) != 0;
    bad += p.chunk != 1 || p.out_region != (size_t)511 * 20000 * 41 || p.out_region <= PTA_OUT_BYTES;
    // the refusal: N = 512, S = 70000 with post is 511 * 70000 * 32 B = 1.14 GB; states alone (36 MB) are fine
    bad += pta_make_plan(512, 70000, 35, 3, true, PTA_POST, 256, 0, &p) != 2 || p.out_tree != (size_t)511 * 70000 * 32;
    bad += check_plan(512, 70000, 35, 3, true, PTA_POST | PTA_PMAX, 256, 0);
    bad += check_plan(512, 70000, 35, 3, true, PTA_STATE, 256, 0);
    // exactly 1 GiB is allowed, one byte more is not
    bad += pta_make_plan(2, 1 << 25, 1, 1, false, PTA_POST, 1, 0, &p) != 0 || p.out_tree != PTA_OUT_MAX;
    bad += pta_make_plan(2, (1 << 25) + 1, 1, 1, false, PTA_POST, 1, 0, &p) != 2;
    // items of a chunk stay within an int
    bad += check_plan(512, 70, 0x7fffffff / 2, 1 << 20, true, PTA_STATE, 256, 0);
    // no plan
    bad += pta_make_plan(1, 1, 1, 1, false, 1u, 1, 0, &p) != 1 || pta_make_plan(5, 0, 1, 1, false, 1u, 1, 0, &p) != 1 ||
           pta_make_plan(5, 1, 0, 1, false, 1u, 1, 0, &p) != 1 || pta_make_plan(5, 1, 1, 0, false, 1u, 1, 0, &p) != 1 ||
           pta_make_plan(5, 1, 1, 1, false, 1u, 0, 0, &p) != 1 || pta_make_plan(5, 1, 1, 1, false, 0u, 1, 0, &p) != 1 ||
           pta_make_plan(5, 1, 1, 1, false, 8u, 1, 0, &p) != 1;
    printf("treeanc host: %ld values differ\n", bad);
    return bad ? 1 : 0;
}
