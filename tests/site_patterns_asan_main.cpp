// Stand-alone host program for tests/test_site_patterns_cpu.py: the builder and the rule of phylo_amd/csrc/phylo_site_patterns.h on
// exactly sized heap buffers (built with -fsanitize=address,undefined, a byte read or written outside a buffer ends the program),
// every table checked against its definition.  No GPU, nothing of the library.
#include <stdio.h>
#include <stdlib.h>

#include "phylo_site_patterns.h"

static unsigned int g_x = 2463534242u;
static unsigned int rnd() { g_x = g_x * 1664525u + 1013904223u; return g_x >> 8; }

// codes [N][S] with columns drawn from `pool` columns made at random (pool 0: every site a column of its own choice)
static long one_case(int N, int S, int pool, int want_U) {
    long bad = 0;
    uint8_t* codes = (uint8_t*)malloc((size_t)N * S);
    uint8_t* cols = (uint8_t*)malloc((size_t)N * (pool > 0 ? pool : 1));
    int32_t* pat = (int32_t*)malloc((size_t)S * sizeof(int32_t));
    int32_t* rep = (int32_t*)malloc((size_t)S * sizeof(int32_t));
    if (!codes || !cols || !pat || !rep) return 1000000;
    for (int i = 0; i < N * (pool > 0 ? pool : 1); ++i) cols[i] = (uint8_t)(rnd() % 5);
    for (int s = 0; s < S; ++s) {
        const int p = pool > 0 ? (int)(rnd() % (unsigned)pool) : -1;
        for (int l = 0; l < N; ++l) codes[(size_t)l * S + s] = p >= 0 ? cols[(size_t)l * pool + p] : (uint8_t)(rnd() % 5);
    }
    const int U = pk_pat_columns(codes, N, S, pat, rep);
    if (want_U >= 0 && U != want_U) ++bad;
    if (U < 1 || U > S) ++bad;
    for (int u = 0; u < U; ++u) {
        if (u && rep[u] <= rep[u - 1]) ++bad;                                 // numbered by first occurrence
        if (pat[rep[u]] != u) ++bad;
    }
    for (int s = 0; s < S; ++s) {
        if (pat[s] < 0 || pat[s] >= U || rep[pat[s]] > s) { ++bad; continue; }
        for (int l = 0; l < N; ++l) bad += codes[(size_t)l * S + rep[pat[s]]] != codes[(size_t)l * S + s];
    }
    for (int a = 0; a < U; ++a)                                               // distinct
        for (int b = a + 1; b < U && U <= 600; ++b) {
            bool eq = true;
            for (int l = 0; l < N && eq; ++l) eq = codes[(size_t)l * S + rep[a]] == codes[(size_t)l * S + rep[b]];
            bad += eq;
        }
    if (U <= PK_PAT_IMAGE_MAX_U) {
        const size_t n = pk_pat_image_bytes(S) / 2;
        uint16_t* image = (uint16_t*)malloc(n * 2);
        if (!image) return 1000000;
        pk_pat_pack_image(pat, S, U, image);
        if (n != (size_t)pk_packed_chunks(S) * 1024) ++bad;
        for (size_t i = 0; i < n; ++i) {
            const size_t Jc = i / 1024, h = i / 512 % 2, c = i / 8 % 64, j = i % 8, s = 64 * (16 * Jc + 8 * h + j) + c;
            bad += image[i] != (uint16_t)(8 * (s < (size_t)S ? pat[s] : U));
        }
        free(image);
    }
    // everything at once, into a buffer of exactly the tables' size
    {
        const size_t bytes = pk_leaf_image_bytes(N, S) - pk_pat_offset(N, S);
        uint8_t* tables = (uint8_t*)malloc(bytes);
        if (!tables) return 1000000;
        memset(tables, 0xee, bytes);
        if (pk_pat_build(codes, N, S, tables) != U) ++bad;
        if (U <= PK_PAT_MAX_U) {
            const uint32_t* off = (const uint32_t*)(tables + pk_pat_image_bytes(S));
            for (int u = 0; u < PK_PAT_REP_WORDS; ++u) bad += off[u] != (u < U ? 32u * (uint32_t)rep[u] : 0u);
            const uint8_t* rl = tables + pk_pat_image_bytes(S) + pk_pat_rep_bytes();
            const size_t leaf = pk_packed_leaf_bytes(U), stride = pk_packed_leaf_bytes(S);     // a leaf's image, at the S-site image's stride
            for (int l = 0; l < N; ++l)
                for (size_t i = 0; i < stride; ++i) {
                    const size_t u = 64 * (16 * (i / 1024) + i % 16) + (i % 1024) / 16;
                    const uint8_t want = i >= leaf ? (uint8_t)0xee : u < (size_t)U ? codes[(size_t)l * S + rep[u]] : (uint8_t)PK_PAD_CODE;
                    bad += rl[(size_t)l * stride + i] != want;
                }
            if (pk_pat_lds_bytes(U) < 8 * ((size_t)U + 1) || pk_pat_lds_bytes(U) > 8 * (PK_PAT_MAX_U + 1)) ++bad;
        } else {
            for (size_t i = 0; i < bytes; ++i) bad += tables[i] != 0xee;      // not written
        }
        free(tables);
    }
    free(codes); free(cols); free(pat); free(rep);
    return bad;
}

int main() {
    long bad = 0;
    const int sizes[] = {1, 2, 63, 64, 65, 898, 1023, 1024, 1025, 2049};
    for (int S : sizes) {
        bad += one_case(5, S, 1, 1);                       // all columns equal
        bad += one_case(2, S, 0, -1);                      // at most 25 distinct
        bad += one_case(7, S, 0, -1);                      // nearly all distinct
        bad += one_case(5, S, S / 2 + 1, -1);
    }
    bad += one_case(12, 9000, 0, -1);                      // U beyond the image's 16 bits
    // the rule on both sides of its thresholds
    bad += !pk_pat_take(898, 413, true, 1, PK_PAT_AUTO);
    bad += pk_pat_take(898, 413, true, 1, PK_PAT_OFF) || pk_pat_take(898, 413, false, 1, PK_PAT_AUTO) || pk_pat_take(898, 413, true, 2, PK_PAT_FORCE);
    bad += !pk_pat_take(4096, PK_PAT_MAX_U, true, 1, PK_PAT_AUTO) || pk_pat_take(4096, PK_PAT_MAX_U + 1, true, 1, PK_PAT_FORCE);
    bad += pk_pat_take(64, 64, true, 1, PK_PAT_AUTO) || !pk_pat_take(64, 64, true, 1, PK_PAT_FORCE);
    printf("site patterns: %ld values differ\n", bad);
    return bad ? 1 : 0;
}
