// Stand-alone host program for tests/test_treeset_plan_cpu.py: pt2_make_plan of phylo_amd/csrc/phylo_treeset.h -- the plan of
// phylo_trees_loglik and phylo_trees_loglik_rates (chunk of trees, whether the row of site values is carried, slab layout) -- built
// with -fsanitize=address,undefined, every plan checked by pts_check_plan over its own regions and, where it is small, written end
// to end into a heap buffer of exactly the slab's size.  No GPU, nothing of the library.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "phylo_treeset.h"

// depths of T trees: 0 all deep, 1 all shallow enough for the four-step kernel, 2 the last tree alone shallow
static std::vector<int> depths(int T, int pattern) {
    std::vector<int> d((size_t)T);                          // exactly sized: a read past T is caught
    for (int t = 0; t < T; ++t) d[t] = pattern == 0 ? 7 : pattern == 1 ? 2 : (t == T - 1 ? 1 : 5);
    return d;
}

static long check_plan(int N, int S, int ntiles, int T, int nc, bool mix, bool coded, bool want_sites, bool want_cat, int env_chunk, int pattern) {
    long bad = 0;
    pt2_plan p;
    const std::vector<int> d = depths(mix ? T : 0, pattern);
    if (pt2_make_plan(N, S, ntiles, T, nc, mix, coded, want_sites, want_cat, env_chunk, mix ? d.data() : nullptr, &p)) return 1000000;
    const size_t R = (size_t)N - 1, n = (size_t)p.chunk;
    // the row is carried when asked for, and in a rates call exactly when one of ITS chunks is at most two slots deep
    bool shallow = false;
    for (int t0 = 0; mix && t0 < T; t0 += p.chunk) shallow |= pt2_unroll(*std::max_element(d.begin() + t0, d.begin() + std::min(T, t0 + p.chunk))) == 4;
    bad += want_sites && !p.sites;
    bad += !mix && p.sites != want_sites;
    bad += mix && !want_sites && p.sites != shallow;
    bad += p.per_tree != R * 16 + (size_t)nc * R * (16 + 256 + (coded ? 64 : 0)) + (size_t)ntiles * 8 + 8 + (p.sites ? (size_t)S * 8 : 0) +
                             (want_cat ? (size_t)nc * S * 8 : 0);
    // the chunk takes no tree more than fits
    bad += p.chunk < T && (env_chunk <= 0 || p.chunk < env_chunk) && (n + 1) * p.per_tree <= PT2_SCRATCH_BYTES && (n + 1) * (size_t)ntiles <= 0x7fffffffu;
    pts_region r[PTS_MAX_REGIONS];
    const int nr = pt2_regions(N, S, ntiles, nc, coded, p.sites, want_cat, p, r);
    const pts_plan_facts f = {p.chunk, 0, p.per_tree, 0, p.total, p.total, ntiles, T, 1, env_chunk, PT2_SCRATCH_BYTES, 0, 0, 0};
    bad += pts_check_plan(r, nr, f);
    // 256-byte alignment costs at most 255 bytes a region over the packed sum
    bad += p.total < n * p.per_tree + 256 || p.total > n * p.per_tree + 256 + 255 * (size_t)(nr - 1);
    if (p.total <= ((size_t)1 << 20)) {
        unsigned char* slab = (unsigned char*)malloc(p.total);
        if (!slab) return 1000000;
        bad += pts_fill_plan(r, nr, f, slab);
        free(slab);
    }
    return bad;
}

int main() {
    long bad = 0;
    const int Ns[] = {2, 3, 4, 5, 12, 33, 70, 128, 511, 512};
    const int tiles[] = {1, 2, 3, 64};
    const int Ts[] = {1, 5, 37, 4096};
    const int Ss[] = {1, 130, 50000};
    const int Cs[] = {1, 4, 16};
    int i = 0;
    for (int N : Ns)
        for (int nt : tiles)
            for (int T : Ts)
                for (int S : Ss)
                    for (int env : {0, 1, 5})
                        for (int form = 0; form < 4; ++form) {
                            bad += check_plan(N, S, nt, T, 1, false, form & 1, form & 2, false, env, 0);
                            const int C = Cs[(i / 3) % 3], pattern = i % 3, cat = (i / 2) % 2;      // cycling: every value meets every form
                            bad += check_plan(N, S, nt, T, C, true, form & 1, form & 2, cat, env, pattern);
                            ++i;
                        }
    bad += check_plan(12, 130, 3, 1 << 20, 4, true, true, false, true, 0, 2);
    bad += check_plan(512, 70, 0x7fffffff / 2, 1 << 20, 1, false, true, false, false, 0, 0);      // items of a chunk stay within an int
    pt2_plan p;
    // the row shrinks the chunk, and the smaller chunks are looked at again: 12 taxa, 50000 sites, 16 categories; without the row
    // 59520 bytes a tree, 1127 trees a chunk, so the 1128th tree is a chunk of its own, and it alone is shallow
    {
        const std::vector<int> deep = depths(4096, 0);
        bad += pt2_make_plan(12, 50000, 25, 4096, 16, true, true, false, false, 0, deep.data(), &p) != 0 || p.sites || p.chunk != 1127;
        bad += p.per_tree != (size_t)11 * 16 + (size_t)16 * 11 * 336 + 25 * 8 + 8;
        const std::vector<int> d = depths(1128, 2);
        bad += pt2_make_plan(12, 50000, 25, 1128, 16, true, true, false, false, 0, d.data(), &p) != 0 || !p.sites;
        bad += p.per_tree != (size_t)11 * 16 + (size_t)16 * 11 * 336 + 25 * 8 + 8 + 50000 * 8 || p.chunk != (int)(PT2_SCRATCH_BYTES / p.per_tree);
        bad += pt2_make_plan(12, 50000, 25, 1127, 16, true, true, false, false, 0, d.data(), &p) != 0 || p.sites || p.chunk != 1127;
    }
    // no plan
    const int one = 1;
    bad += pt2_make_plan(1, 1, 1, 1, 1, false, false, false, false, 0, nullptr, &p) != 1 ||
           pt2_make_plan(5, 0, 1, 1, 1, false, false, false, false, 0, nullptr, &p) != 1 ||
           pt2_make_plan(5, 1, 0, 1, 1, false, false, false, false, 0, nullptr, &p) != 1 ||
           pt2_make_plan(5, 1, 1, 0, 1, false, false, false, false, 0, nullptr, &p) != 1 ||
           pt2_make_plan(5, 1, 1, 1, 0, true, false, false, false, 0, &one, &p) != 1 ||
           pt2_make_plan(5, 1, 1, 1, PT2_MAX_CATS + 1, true, false, false, false, 0, &one, &p) != 1 ||
           pt2_make_plan(5, 1, 1, 1, 4, true, false, false, false, 0, nullptr, &p) != 1 ||
           pt2_make_plan(5, 1, 1, 1, 4, true, false, true, false, 0, nullptr, &p) != 0;
    printf("treeset host: %ld values differ\n", bad);
    return bad ? 1 : 0;
}
