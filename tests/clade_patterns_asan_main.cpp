// Stand-alone host program for tests/test_clade_patterns_cpu.py: the clade-table builder and its rule of
// phylo_amd/csrc/phylo_site_patterns.h on exactly sized heap buffers (built with -fsanitize=address,undefined, a byte read or written
// outside a buffer ends the program), every block checked against its definition.  No GPU, nothing of the library.
// With arguments `N S file` (N * S raw byte codes, leaf by leaf) it builds that alignment's tables twenty times and prints the
// fastest build's time beside pk_pat_build's: what phylo_set_leaves pays on the host (build it without sanitizers for that).
#include <stdio.h>
#include <stdlib.h>

#include <chrono>

#include "phylo_site_patterns.h"

static unsigned int g_x = 2463534242u;
static unsigned int rnd() { g_x = g_x * 1664525u + 1013904223u; return g_x >> 8; }

static long one_case(int N, int S, int ncodes) {
    long bad = 0;
    uint8_t* codes = (uint8_t*)malloc((size_t)N * S);
    int32_t* pat = (int32_t*)malloc((size_t)S * sizeof(int32_t));
    int32_t* rep = (int32_t*)malloc((size_t)S * sizeof(int32_t));
    if (!codes || !pat || !rep) return 1000000;
    for (int i = 0; i < N * S; ++i) codes[i] = (uint8_t)(rnd() % (unsigned)ncodes);
    const int U = pk_pat_columns(codes, N, S, pat, rep);
    if (U > PK_PAT_MAX_U) { free(codes); free(pat); free(rep); return 0; }     // (no tables: phylo_set_leaves builds none)
    const pk_clade_layout L = pk_clade_layout_of(N, S, U);
    const size_t nZ = (size_t)1 << N;
    bad += L.stride != PK_CLADE_HDR_BYTES + L.rep_bytes + L.image_bytes || L.total != L.codes_bytes + nZ * L.stride;
    bad += L.codes_bytes != pk_packed_bytes(N, S) || L.image_bytes != pk_pat_image_bytes(S) || L.rep_bytes != (size_t)((U + 63) / 64 + 2) * 256;
    uint8_t* out = (uint8_t*)malloc(L.total);
    uint16_t* cls = (uint16_t*)malloc(nZ * (size_t)U * 2);
    uint16_t* first = (uint16_t*)malloc((size_t)S * 2);      // class -> its first site, per bitset
    if (!out || !cls || !first) return 1000000;
    memset(out, 0xee, L.total);
    pk_clade_build(codes, N, S, pat, rep, U, out, cls);
    const size_t leaf_bytes = pk_packed_leaf_bytes(S);
    for (int l = 0; l < N; ++l)
        for (size_t i = 0; i < leaf_bytes; ++i) bad += out[(size_t)l * leaf_bytes + i] != (i < (size_t)S ? codes[(size_t)l * S + i] : 0);
    for (size_t Z = 0; Z < nZ; ++Z) {
        int leaves = 0;
        for (int b = 0; b < N; ++b) leaves += (int)(Z >> b & 1);
        const uint8_t* blk = out + L.codes_bytes + Z * L.stride;
        if (leaves < 3) {                                                        // not written
            for (size_t i = 0; i < L.stride; ++i) bad += blk[i] != 0xee;
            continue;
        }
        const uint32_t UZ = *(const uint32_t*)blk;
        const uint32_t* ro = (const uint32_t*)(blk + PK_CLADE_HDR_BYTES);
        const uint16_t* img = (const uint16_t*)(blk + PK_CLADE_HDR_BYTES + L.rep_bytes);
        if (UZ < 1 || UZ > (uint32_t)U) { ++bad; continue; }
        for (size_t i = 4; i < PK_CLADE_HDR_BYTES; ++i) bad += blk[i] != 0;
        for (size_t w = 0; w < L.rep_bytes / 4; ++w) {
            if (w >= UZ) { bad += ro[w] != 0; continue; }
            bad += ro[w] % 32 != 0 || ro[w] / 32 >= (uint32_t)S || (w && ro[w] <= ro[w - 1]);
        }
        // every site: its class from the image, the class of its global pattern, agreement with the class's first site on Z's leaves
        uint32_t seen = 0;
        const size_t n = L.image_bytes / 2;
        for (size_t i = 0; i < n; ++i) {
            const size_t Jc = i / 1024, h = i / 512 % 2, c = i / 8 % 64, j = i % 8, s = 64 * (16 * Jc + 8 * h + j) + c;
            if (s >= (size_t)S) { bad += img[i] != (uint16_t)(8 * UZ); continue; }
            if (img[i] % 8 != 0 || img[i] / 8 >= UZ) { ++bad; continue; }
            first[s] = (uint16_t)(img[i] / 8);
        }
        for (int s = 0; s < S; ++s) {
            const uint32_t k = first[s];
            bad += cls[Z * U + pat[s]] != k;
            if (k > seen) { ++bad; continue; }                                   // numbered by first occurrence
            if (k == seen) { bad += ro[k] != 32u * (uint32_t)s; ++seen; }
            const int r = (int)(ro[k] / 32);
            for (int l = 0; l < N; ++l)
                if (Z >> l & 1) bad += codes[(size_t)l * S + r] != codes[(size_t)l * S + s];
        }
        bad += seen != UZ;
        // distinct: two representatives differ on some leaf of Z
        for (uint32_t a = 0; a < UZ && UZ <= 130; ++a)
            for (uint32_t b = a + 1; b < UZ; ++b) {
                bool eq = true;
                for (int l = 0; l < N && eq; ++l)
                    if (Z >> l & 1) eq = codes[(size_t)l * S + ro[a] / 32] == codes[(size_t)l * S + ro[b] / 32];
                bad += eq;
            }
    }
    free(out); free(cls); free(first); free(codes); free(pat); free(rep);
    return bad;
}

static int time_file(int N, int S, const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) return 2;
    std::vector<uint8_t> codes((size_t)N * S);
    const size_t got = fread(codes.data(), 1, codes.size(), f);
    fclose(f);
    if (got != codes.size()) return 2;
    std::vector<uint8_t> tables(pk_leaf_image_bytes(N, S) - pk_pat_offset(N, S));
    std::vector<int32_t> pat, rep;
    double best_pat = 1e30, best_clade = 1e30;
    int U = 0;
    std::vector<uint8_t> out;
    for (int it = 0; it < 20; ++it) {
        const auto t0 = std::chrono::steady_clock::now();
        U = pk_pat_build(codes.data(), N, S, tables.data(), pat, rep);
        const auto t1 = std::chrono::steady_clock::now();
        if (U > PK_PAT_MAX_U || N > PK_CLADE_MAX_N) return 3;
        out.resize(pk_clade_layout_of(N, S, U).total);
        const auto t2 = std::chrono::steady_clock::now();
        pk_clade_build(codes.data(), N, S, pat.data(), rep.data(), U, out.data(), nullptr);
        const auto t3 = std::chrono::steady_clock::now();
        const double a = std::chrono::duration<double, std::milli>(t1 - t0).count(), b = std::chrono::duration<double, std::milli>(t3 - t2).count();
        best_pat = a < best_pat ? a : best_pat;
        best_clade = b < best_clade ? b : best_clade;
    }
    printf("N = %d, S = %d, U = %d: pattern tables %.3f ms, clade tables %.3f ms (%zu bytes)\n", N, S, U, best_pat, best_clade, out.size());
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 4) return time_file(atoi(argv[1]), atoi(argv[2]), argv[3]);
    long bad = 0;
    const int sizes[] = {1, 2, 63, 64, 65, 130, 898, 1025};
    for (int S : sizes) {
        bad += one_case(3, S, 5);
        bad += one_case(4, S, 4);
        bad += one_case(6, S, 2);                          // at most 64 distinct columns
        bad += one_case(7, S, 3);
    }
    bad += one_case(10, 300, 2);
    // the rule on both sides of its caps
    bad += !pk_clade_take(true, 12, 898, 413, PK_CLADE_AUTO) || !pk_clade_take(true, 12, 898, 413, PK_CLADE_FORCE);
    bad += pk_clade_take(true, 12, 898, 413, PK_CLADE_OFF) || pk_clade_take(false, 12, 898, 413, PK_CLADE_FORCE);
    bad += pk_clade_take(true, 13, 898, 413, PK_CLADE_FORCE) || pk_clade_take(true, 2, 898, 20, PK_CLADE_FORCE) || !pk_clade_take(true, 3, 898, 20, PK_CLADE_AUTO);
    bad += !pk_clade_take(true, 12, 2048, 512, PK_CLADE_AUTO) || pk_clade_take(true, 12, 3072, 512, PK_CLADE_FORCE);
    bad += pk_clade_layout_of(12, 898, 413).total != 18886656 || pk_clade_layout_of(12, 898, 413).total > PK_CLADE_MAX_BYTES;
    printf("clade patterns: %ld values differ\n", bad);
    return bad ? 1 : 0;
}
