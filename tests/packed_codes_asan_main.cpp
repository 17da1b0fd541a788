// Stand-alone host program for tests/test_packed_codes_cpu.py: the packer of phylo_amd/csrc/phylo_packed_codes.h on exactly
// sized heap buffers (built with -fsanitize=address,undefined, a byte read or written outside either buffer ends the program),
// every byte of the image checked against the layout.  No GPU, nothing of the library.
#include <stdio.h>
#include <stdlib.h>

#include "phylo_packed_codes.h"

int main() {
    const int sizes[] = {1, 2, 63, 64, 65, 898, 1023, 1024, 1025, 2049};
    const int taxa[] = {2, 5};
    long bad = 0;
    unsigned int x = 12345u;
    for (int S : sizes)
        for (int N : taxa) {
            uint8_t* codes = (uint8_t*)malloc((size_t)N * S);
            uint8_t* packed = (uint8_t*)malloc(pk_packed_bytes(N, S));
            if (!codes || !packed) return 2;
            for (size_t i = 0; i < (size_t)N * S; ++i) { x = x * 1664525u + 1013904223u; codes[i] = (uint8_t)((x >> 24) % 5); }
            pk_pack_leaf_codes(codes, N, S, packed);
            const size_t leaf = pk_packed_leaf_bytes(S);
            if (leaf != (size_t)pk_packed_chunks(S) * 1024 || pk_packed_chunks(S) != ((S + 63) / 64 + 15) / 16) ++bad;
            for (int l = 0; l < N; ++l)
                for (size_t i = 0; i < leaf; ++i) {
                    const size_t s = 64 * (16 * (i / 1024) + i % 16) + (i % 1024) / 16;
                    const uint8_t want = s < (size_t)S ? codes[(size_t)l * S + s] : (uint8_t)PK_PAD_CODE;
                    if (packed[(size_t)l * leaf + i] != want) ++bad;
                }
            free(codes);
            free(packed);
        }
    printf("packed codes: %ld bytes differ\n", bad);
    return bad ? 1 : 0;
}
