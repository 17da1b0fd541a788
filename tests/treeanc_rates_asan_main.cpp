// Stand-alone host program for tests/test_treeanc_rates_cpu.py: the host half of phylo_amd/csrc/phylo_treeanc_rates.h -- the plan
// of a call of phylo_trees_ancestral_rates (chunk of trees bounded by the slab, by the staging of the requested outputs and by
// the caller; slab layout; capped grid), the coefficient block and the mixture checks it shares with phylo_trees_grad_rates --
// built with -fsanitize=address,undefined, every output checked against its definition, and a plan's regions written end to end
// into a heap buffer of exactly the slab's size where that is small.  No GPU, nothing of the library.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "phylo_treeanc_rates.h"

static size_t tree_bytes(int N, int S, int C, unsigned outs) {
    const size_t cell = (outs & PTAR_POST ? 32 : 0) + (outs & PTAR_STATE ? 1 : 0) + (outs & PTAR_PMAX ? 8 : 0);
    return ((size_t)N - 1) * (size_t)S * cell + (size_t)S * ((outs & PTAR_CATPOST ? 8 * (size_t)C : 0) + (outs & PTAR_SITERATE ? 8 : 0));
}

static long check_plan(int N, int S, int ntiles, int T, int C, bool coded, unsigned outs, int n_cus, int env_chunk) {
    long bad = 0;
    ptar_plan p;
    const size_t R = (size_t)N - 1, nc = (size_t)C, tree_out = tree_bytes(N, S, C, outs);
    const int rc = ptar_make_plan(N, S, ntiles, T, C, coded, outs, n_cus, env_chunk, &p);
    if (tree_out > PTA_OUT_MAX) return (rc != 2) + (p.out_tree != tree_out);          // refused, naming the size
    if (rc) return 1000000;
    const size_t n = (size_t)p.chunk;
    bad += p.out_tree != tree_out;
    bad += p.out_region != (tree_out > PTA_OUT_BYTES ? tree_out : PTA_OUT_BYTES);     // grows to one tree's need, never further
    // the chunk within the slab's budget (more than one tree), the caller's cap and T, its outputs within the staging region, its
    // items within an int; the grid within its caps; every region aligned, in order, apart and inside the slab
    pts_region r[PTS_MAX_REGIONS];
    const int nr = ptar_regions(N, S, ntiles, C, coded, outs, p, r);
    const pts_plan_facts f = ptg_plan_facts(p, ntiles, T, n_cus, env_chunk, p.out_region);
    bad += pts_check_plan(r, nr, f);
    bad += p.ncoef != 2 * C;
    // the slab is accounted as ptgr_make_plan's without M', M'', the given lengths, the derivative tiles and sums, and with w | r
    // in the place of w | u | v
    ptgr_plan gp;
    if (ptgr_make_plan(N, ntiles, T, C, coded, false, false, n_cus, env_chunk, &gp)) return 1000000;
    bad += p.per_tree + nc * R * 512 + R * 16 + nc * 8 + (size_t)ntiles * 2 * R * 8 + 2 * R * 8 != gp.per_tree;
    // the chunk is the SMALLEST of the three bounds: one more tree would break one of them (or there is none left)
    if (p.chunk < T && !(env_chunk > 0 && p.chunk == env_chunk))
        bad += (n + 1) * p.per_tree <= PTG_CHUNK_BYTES && (n + 1) * tree_out <= p.out_region && (n + 1) * (size_t)ntiles <= 0x7fffffffu;
    bad += p.wg_store != nc * R * PTG_U * PTG_SLOT_BYTES;
    // the grid cap is ptgr_make_plan's
    if (!ptgr_make_plan(N, ntiles, p.chunk, C, coded, false, false, n_cus, p.chunk, &gp)) bad += gp.chunk == p.chunk && gp.grid != p.grid;
    if (p.total <= ((size_t)8 << 20)) {                     // every region written end to end inside an exactly sized buffer
        unsigned char* slab = (unsigned char*)malloc(p.total);
        if (!slab) return 1000000;
        bad += pts_fill_plan(r, nr, f, slab);               // no region overwrote another
        free(slab);
    }
    return bad;
}

static long check_mixtures() {
    long bad = 0;
    char msg[200];
    const int N = 5;
    double blen[8] = {0.1, 0.2, 0.0, 0.4, 0.5, 0.6, 0.7, 0.8};
    for (int C : {1, 5, 16}) {
        std::vector<double> rate((size_t)C), weight((size_t)C), coef((size_t)2 * C);      // exactly sized: a read past C is caught
        for (int k = 0; k < C; ++k) {
            rate[k] = 0.25 * k;                             // a rate-0 category is ordinary
            weight[k] = k == 1 ? 0.0 : 1.0 / C;             // and so is a zero weight
        }
        bad += ptgr_check_mixture(N, blen, C, rate.data(), weight.data(), msg, sizeof msg) != 0;
        ptar_coefficients(C, rate.data(), weight.data(), coef.data());
        for (int k = 0; k < C; ++k) bad += coef[k] != weight[k] || coef[C + k] != rate[k];
        const int last = C - 1;
        const double keep_r = rate[last], keep_w = weight[last];
        for (double v : {-1e-9, (double)NAN, (double)INFINITY}) {
            rate[last] = v;
            bad += ptgr_check_mixture(N, blen, C, rate.data(), weight.data(), msg, sizeof msg) != 1;
            snprintf(msg + 150, 40, "category %d", last);
            bad += strstr(msg, msg + 150) == nullptr;       // the message names the category
            rate[last] = keep_r;
            weight[last] = v;
            bad += ptgr_check_mixture(N, blen, C, rate.data(), weight.data(), msg, sizeof msg) != 1;
            weight[last] = keep_w;
        }
        rate[last] = 1e308;                                 // a scaled length that is not finite: row 3, the last category
        blen[7] = 1e10;
        bad += ptgr_check_mixture(N, blen, C, rate.data(), weight.data(), msg, sizeof msg) != 1;
        bad += strstr(msg, "row 3") == nullptr;
        blen[7] = 0.8;
    }
    return bad;
}

int main() {
    long bad = 0;
    const int Ns[] = {2, 3, 5, 12, 128, 512};
    const int Ss[] = {1, 70, 4100};
    const int Ts[] = {1, 37, 4096, 1 << 20};
    const int cus[] = {1, 256};
    const int Cs[] = {1, 5, 16};
    for (int N : Ns)
        for (int S : Ss)
            for (int T : Ts)
                for (int cu : cus)
                    for (int C : Cs)
                        for (unsigned outs = 1; outs < 32; ++outs)
                            for (int coded = 0; coded < 2; ++coded) {
                                const int nt = (S + 2047) / 2048;
                                bad += check_plan(N, S, nt, T, C, coded, outs, cu, 0);
                                bad += check_plan(N, S, nt, T, C, coded, outs, cu, 5);      // env-bound chunks
                            }
    ptar_plan p;
    // slab-bound chunks: N = 128, S = 70, C = 16, states alone -- 127 * 16 * 336 + ... = 687 KB of slab a tree, 97 trees in 64 MiB,
    // where the staging (8.9 KB a tree) would hold thirty thousand
    bad += ptar_make_plan(128, 70, 1, 4096, 16, true, PTAR_STATE, 256, 0, &p) != 0;
    bad += p.chunk != (int)(PTG_CHUNK_BYTES / p.per_tree) || p.per_tree != (size_t)127 * 32 + (size_t)16 * 127 * 336 + 32 * 8 + 8 + 8 ||
           p.chunk != 97;
    // output-bound chunks: N = 128, S = 4100, C = 1 with post takes 127 * 4100 * 32 B = 16.7 MB a tree -- 16 trees fill 256 MiB
    bad += ptar_make_plan(128, 4100, 3, 4096, 1, true, PTAR_POST, 256, 0, &p) != 0;
    bad += p.chunk != (int)(PTA_OUT_BYTES / ((size_t)127 * 4100 * 32)) || p.chunk != 16;
    // ... and catpost and siterate alone at C = 16: 4100 * (128 + 8) B = 558 KB a tree, 481 trees of staging, 1122 of slab
    bad += ptar_make_plan(12, 4100, 3, 4096, 16, true, PTAR_CATPOST | PTAR_SITERATE, 256, 0, &p) != 0;
    bad += p.out_tree != (size_t)4100 * 136 || p.chunk != (int)(PTA_OUT_BYTES / p.out_tree);
    // env-bound chunks
    bad += ptar_make_plan(12, 70, 1, 4096, 5, true, PTAR_ALL, 256, 3, &p) != 0 || p.chunk != 3;
    bad += ptar_make_plan(12, 70, 1, 2, 5, true, PTAR_ALL, 256, 3, &p) != 0 || p.chunk != 2;
    // C = 1 and C = 16 at one shape: the node store of a workgroup and the coefficient block scale with C
    bad += ptar_make_plan(12, 130, 3, 37, 1, true, PTAR_ALL, 256, 0, &p) != 0 || p.wg_store != (size_t)11 * 4096 || p.ncoef != 2;
    bad += ptar_make_plan(12, 130, 3, 37, 16, true, PTAR_ALL, 256, 0, &p) != 0 || p.wg_store != (size_t)16 * 11 * 4096 || p.ncoef != 32;
    // one tree over 256 MiB: N = 512, S = 20000, C = 16 with all five is 511 * 20000 * 41 + 20000 * 136 B = 422 MB -- the region
    // grows to it, one tree a chunk
    bad += check_plan(512, 20000, 10, 7, 16, true, PTAR_ALL, 256, 0);
    bad += ptar_make_plan(512, 20000, 10, 7, 16, true, PTAR_ALL, 256, 0, &p) != 0;
    bad += p.chunk != 1 || p.out_region != (size_t)511 * 20000 * 41 + (size_t)20000 * 136 || p.out_region <= PTA_OUT_BYTES;
    // the refusal: N = 512, S = 70000 with post is 511 * 70000 * 32 B = 1.14 GB; states and the site rates (36 MB) are fine
    bad += ptar_make_plan(512, 70000, 35, 3, 5, true, PTAR_POST, 256, 0, &p) != 2 || p.out_tree != (size_t)511 * 70000 * 32;
    bad += check_plan(512, 70000, 35, 3, 5, true, PTAR_POST | PTAR_CATPOST, 256, 0);
    bad += check_plan(512, 70000, 35, 3, 5, true, PTAR_STATE | PTAR_CATPOST | PTAR_SITERATE, 256, 0);
    // exactly 1 GiB is allowed, one byte more is not
    bad += ptar_make_plan(2, 1 << 25, 1, 1, 1, false, PTAR_POST, 1, 0, &p) != 0 || p.out_tree != PTA_OUT_MAX;
    bad += ptar_make_plan(2, 1 << 25, 1, 1, 1, false, PTAR_POST | PTAR_STATE, 1, 0, &p) != 2;
    // the grid cap at N = 512, C = 16: 16 * 511 * 2 * 2 KiB = 32 MiB of node store per workgroup, 8 of them in 256 MiB
    bad += ptar_make_plan(512, 65, 2, 131, 16, true, PTAR_ALL, 256, 0, &p) != 0 || p.grid != 8;
    bad += ptar_make_plan(512, 65, 2, 3, 16, true, PTAR_ALL, 256, 0, &p) != 0 || p.grid != 6;          // fewer items than the cap
    bad += ptar_make_plan(5, 130, 3, 4096, 5, true, PTAR_ALL, 256, 0, &p) != 0 || p.grid != 8 * 256;   // small trees: 8 per compute unit
    // items of a chunk stay within an int
    bad += check_plan(512, 70, 0x7fffffff / 2, 1 << 20, 5, true, PTAR_STATE, 256, 0);
    // no plan
    bad += ptar_make_plan(1, 1, 1, 1, 1, false, 1u, 1, 0, &p) != 1 || ptar_make_plan(5, 0, 1, 1, 1, false, 1u, 1, 0, &p) != 1 ||
           ptar_make_plan(5, 1, 0, 1, 1, false, 1u, 1, 0, &p) != 1 || ptar_make_plan(5, 1, 1, 0, 1, false, 1u, 1, 0, &p) != 1 ||
           ptar_make_plan(5, 1, 1, 1, 1, false, 1u, 0, 0, &p) != 1 || ptar_make_plan(5, 1, 1, 1, 1, false, 0u, 1, 0, &p) != 1 ||
           ptar_make_plan(5, 1, 1, 1, 1, false, 32u, 1, 0, &p) != 1 || ptar_make_plan(5, 1, 1, 1, 0, false, 1u, 1, 0, &p) != 1 ||
           ptar_make_plan(5, 1, 1, 1, 17, false, 1u, 1, 0, &p) != 1;
    bad += check_mixtures();
    printf("treeanc_rates host: %ld values differ\n", bad);
    return bad ? 1 : 0;
}
