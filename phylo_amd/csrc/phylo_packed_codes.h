// Packed image of the leaf codes (host only; no HIP in this header, so a stand-alone program can include it).
//
// The byte codes [N][S] serve a wave one byte per lane and 64-site step.  The packed image serves the 16 codes a lane needs for 16
// consecutive steps as 16 contiguous bytes, chunk-major, so a wave's load of one chunk is 1 KiB contiguous whatever S is:
//     packed[((leaf * nC + Jc) * 64 + c) * 16 + j] = code of site 64 * (16 * Jc + j) + c,      nC = ceil(ceil(S / 64) / 16)
// A site tile starts at a multiple of 64, so a site's column is s mod 64 and its step s / 64 for every tile.  Sites >= S hold
// PK_PAD_CODE, a sixth code whose site likelihood is exactly 1.0 (pk_rank_merge_nostore: lik25's entry 30).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define PK_PAD_CODE 5
#define PK_CHUNK_STEPS 16                // steps of 64 sites per chunk: one 16-byte load per lane
#define PK_CHUNK_BYTES 1024              // 64 lanes x 16 bytes

static inline int pk_packed_chunks(int S) { return (S + 64 * PK_CHUNK_STEPS - 1) / (64 * PK_CHUNK_STEPS); }
static inline size_t pk_packed_leaf_bytes(int S) { return (size_t)pk_packed_chunks(S) * PK_CHUNK_BYTES; }
static inline size_t pk_packed_bytes(int N, int S) { return (size_t)N * pk_packed_leaf_bytes(S); }
// the byte codes [N][S] and, 16-byte aligned behind them, their packed image: one buffer on the device, one upload
static inline size_t pk_packed_offset(int N, int S) { return ((size_t)N * S + 15) & ~(size_t)15; }
static inline size_t pk_codes_image_bytes(int N, int S) { return pk_packed_offset(N, S) + pk_packed_bytes(N, S); }

// codes: [N][S] byte codes; packed: pk_packed_bytes(N, S) bytes.  One pass over the codes: a step's 64 codes go to stride-16 bytes
// of one chunk (the chunk, 1 KiB, stays in the first-level cache while its 16 steps are written).
static inline void pk_pack_leaf_codes(const uint8_t* codes, int N, int S, uint8_t* packed) {
    const size_t leaf_bytes = pk_packed_leaf_bytes(S);
    memset(packed, PK_PAD_CODE, (size_t)N * leaf_bytes);
    const int nsteps = (S + 63) / 64;
    for (int leaf = 0; leaf < N; ++leaf) {
        const uint8_t* src = codes + (size_t)leaf * S;
        uint8_t* dst = packed + (size_t)leaf * leaf_bytes;
        for (int q = 0; q < nsteps; ++q) {
            const int n = S - 64 * q < 64 ? S - 64 * q : 64;
            uint8_t* d = dst + (size_t)(q / PK_CHUNK_STEPS) * PK_CHUNK_BYTES + (q % PK_CHUNK_STEPS);
            const uint8_t* s = src + (size_t)64 * q;
            for (int c = 0; c < n; ++c) d[c * 16] = s[c];
        }
    }
}
