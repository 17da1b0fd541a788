// Site patterns of a coded alignment (host only; no HIP in this header, so a stand-alone program can include it).
//
// A node's row at a site is computed from its children's rows at that site alone, by the same operations at every site, so two sites
// with the same COLUMN of leaf codes carry bit-identical rows in every node and bit-identical site likelihoods in every merge.
// pk_rank_merge_nostore therefore computes a merge's site likelihood once per DISTINCT column (phase 1: a table in LDS) and takes the
// product over ALL S sites, in the unchanged lane, step and pair order, by looking the factors up (phase 2).  What it needs per
// alignment is built here, once, by phylo_set_leaves, and goes up behind the codes and their packed image in the same copy:
//
//   distinct columns   U of them, numbered by first occurrence: pat[s] = the number of site s's column, rep[u] = the first site that
//                      shows column u (rep ascends, rep[pat[s]] <= s).
//   pattern image      for every site the BYTE offset 8 pat[s] of its column's table entry, 16 bits, laid out like the leaf image:
//                      chunk-major, a chunk = 16 steps of 64 sites = two 1 KiB halves of 8 steps each, a lane's 8 steps of a half 16
//                      contiguous bytes, so a wave's load of a half is 1 KiB contiguous and the walk extracts with constant shifts:
//                          image[((Jc * 2 + h) * 64 + c) * 8 + j] = 8 * pat[64 * (16 * Jc + 8 * h + j) + c]
//                      Sites >= S hold 8 U, the pad entry, whose value is exactly 1.0.
//   representatives    off[u] = 32 rep[u], the byte offset of the representative site's row in a node, for u < U; 0 behind them up to
//                      PK_PAT_REP_WORDS (a lane reads off[lane + 64 j] one and two steps ahead of the step it computes: always a site
//                      of the row, never a clamp).
//   representative     the code matrix [N][U] of the representative sites through pk_pack_leaf_codes, leaf by leaf at the stride of the
//   leaf image         S-site image (U <= S: it fits), so a leaf's two images lie a fixed distance apart and the merge record, which
//                      holds the first, needs no slot for the second: the coded side of phase 1 walks it as the mixed loops walk
//                      the S-site image.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "phylo_packed_codes.h"

#define PK_PAT_MAX_U 512                 // the table, 8 (U + 1) bytes, beside the kernel's other LDS: 32 workgroups per CU in 160 KiB
#define PK_PAT_REP_WORDS 1024            // 64 (PK_PAT_MAX_U / 64 + 2) rounded up: one 4 KiB block
#define PK_PAT_HALF_BYTES 1024           // 64 lanes x 8 steps x 2 bytes
#define PK_PAT_IMAGE_MAX_U 8191          // 8 U must fit the image's 16 bits

enum { PK_PAT_OFF = 0, PK_PAT_AUTO = 1, PK_PAT_FORCE = 2 };   // PHYLO_SITE_PATTERNS = 0, unset, force

static inline size_t pk_pat_image_bytes(int S) { return (size_t)pk_packed_chunks(S) * 2 * PK_PAT_HALF_BYTES; }
static inline size_t pk_pat_rep_bytes() { return (size_t)PK_PAT_REP_WORDS * 4; }
// the tables behind the codes' image, each 16-byte aligned: pattern image, representatives, representative leaf image (U at its cap)
static inline size_t pk_pat_offset(int N, int S) { return (pk_codes_image_bytes(N, S) + 15) & ~(size_t)15; }
static inline size_t pk_pat_rep_offset(int N, int S) { return pk_pat_offset(N, S) + pk_pat_image_bytes(S); }
static inline size_t pk_pat_leaf_offset(int N, int S) { return pk_pat_rep_offset(N, S) + pk_pat_rep_bytes(); }
static inline size_t pk_leaf_image_bytes(int N, int S) { return pk_pat_leaf_offset(N, S) + pk_packed_bytes(N, S); }
// the table in LDS: one entry per lane of every phase-1 step, and the pad entry
static inline size_t pk_pat_lds_bytes(int U) { return ((size_t)((U + 63) / 64) * 64 + 1) * 8; }

// The distinct columns of byte codes [N][S]: pat[S], rep[S] (its first U entries are written); returns U.  One pass over the codes
// for a 64-bit hash per column (row by row, the way they lie in memory), then one pass over the sites through an open-addressed
// table of first occurrences; sites with the same hash are compared code by code, so a collision costs time, never a wrong number.
static inline int pk_pat_columns(const uint8_t* codes, int N, int S, int32_t* pat, int32_t* rep) {
    std::vector<uint64_t> h((size_t)S, 0xcbf29ce484222325ull);
    for (int leaf = 0; leaf < N; ++leaf) {
        const uint8_t* row = codes + (size_t)leaf * S;
        for (int s = 0; s < S; ++s) h[s] = (h[s] ^ row[s]) * 0x100000001b3ull;
    }
    size_t cap = 16;
    while (cap < (size_t)S * 2) cap <<= 1;
    std::vector<int32_t> slot(cap, -1);                    // the number of the column first seen with this hash, or -1
    int U = 0;
    for (int s = 0; s < S; ++s) {
        uint64_t x = h[s];
        x ^= x >> 29;
        size_t i = (size_t)(x * 0x9e3779b97f4a7c15ull >> 20) & (cap - 1);
        int u = -1;
        for (;; i = (i + 1) & (cap - 1)) {
            const int32_t cand = slot[i];
            if (cand < 0) break;
            const int r = rep[cand];
            if (h[r] != h[s]) continue;
            bool eq = true;
            for (int leaf = 0; leaf < N && eq; ++leaf) eq = codes[(size_t)leaf * S + r] == codes[(size_t)leaf * S + s];
            if (eq) { u = cand; break; }
        }
        if (u < 0) {
            u = U++;
            rep[u] = s;
            slot[i] = u;
        }
        pat[s] = u;
    }
    return U;
}
// the pattern image (pk_pat_image_bytes(S) bytes) of pat[S] with U <= PK_PAT_IMAGE_MAX_U distinct columns
static inline void pk_pat_pack_image(const int32_t* pat, int S, int U, uint16_t* image) {
    const size_t n = pk_pat_image_bytes(S) / 2;
    const uint16_t pad = (uint16_t)(8 * U);
    for (size_t i = 0; i < n; ++i) image[i] = pad;
    const int nsteps = (S + 63) / 64;
    for (int q = 0; q < nsteps; ++q) {
        const int cnt = S - 64 * q < 64 ? S - 64 * q : 64;
        uint16_t* d = image + ((size_t)(q / PK_CHUNK_STEPS) * 2 + (q % PK_CHUNK_STEPS) / 8) * (PK_PAT_HALF_BYTES / 2) + q % 8;
        const int32_t* p = pat + (size_t)64 * q;
        for (int c = 0; c < cnt; ++c) d[c * 8] = (uint16_t)(8 * p[c]);
    }
}
// the representatives' row offsets (PK_PAT_REP_WORDS words) for U <= PK_PAT_MAX_U
static inline void pk_pat_rep_offsets(const int32_t* rep, int U, uint32_t* off) {
    for (int u = 0; u < PK_PAT_REP_WORDS; ++u) off[u] = u < U ? 32u * (uint32_t)rep[u] : 0u;
}
// the representative leaf image: leaf l's pk_packed_leaf_bytes(U) bytes at packed + l * stride (stride >= that; the bytes between
// two leaves' images are not written)
static inline void pk_pat_rep_leaf_image(const uint8_t* codes, int N, int S, const int32_t* rep, int U, uint8_t* packed, size_t stride) {
    std::vector<uint8_t> cu((size_t)U);
    for (int leaf = 0; leaf < N; ++leaf) {
        for (int u = 0; u < U; ++u) cu[u] = codes[(size_t)leaf * S + rep[u]];
        pk_pack_leaf_codes(cu.data(), 1, U, packed + (size_t)leaf * stride);
    }
}
// Everything at once, as phylo_set_leaves calls it: `tables` is the image buffer from pk_pat_offset(N, S) on.  Returns U; the tables
// are written only when U <= PK_PAT_MAX_U (no launch reads them otherwise).
// (pat, rep: the columns as pk_pat_columns leaves them, for what is built from them next)
static inline int pk_pat_build(const uint8_t* codes, int N, int S, uint8_t* tables, std::vector<int32_t>& pat, std::vector<int32_t>& rep) {
    pat.resize((size_t)S); rep.resize((size_t)S);
    const int U = pk_pat_columns(codes, N, S, pat.data(), rep.data());
    if (U <= PK_PAT_MAX_U) {
        pk_pat_pack_image(pat.data(), S, U, (uint16_t*)tables);
        pk_pat_rep_offsets(rep.data(), U, (uint32_t*)(tables + pk_pat_image_bytes(S)));
        pk_pat_rep_leaf_image(codes, N, S, rep.data(), U, tables + pk_pat_image_bytes(S) + pk_pat_rep_bytes(), pk_packed_leaf_bytes(S));
    }
    return U;
}
static inline int pk_pat_build(const uint8_t* codes, int N, int S, uint8_t* tables) {
    std::vector<int32_t> pat, rep;
    return pk_pat_build(codes, N, S, tables, pat, rep);
}

// ---- The rule: does pk_rank_merge_nostore take the pattern form for these leaves?
// Valid: coded leaves, the row ONE site tile (it then starts at site 0, a chunk boundary), U <= PK_PAT_MAX_U.
// Worth it: with nS = ceil(S / 64) and nU = ceil(U / 64) steps, a wave with ONE uncoded child (13 of every 14 waves the form
// changes on the flagship) executes, in vector instructions,
//     today      nS * PK_PAT_C_STEP                                      (pk_rows_fast_mixed: per 64-site step)
//     this form  nU * PK_PAT_C_PHASE1 + nS * PK_PAT_C_WALK + PK_PAT_C_FIXED
// and a leaf x leaf wave nothing more.  The counts are read off the compiled loops of pk_rank_merge_nostore (gfx950, -O3,
// -ffp-contract=off; the vector instructions between a loop's label and its back branch in the code object's assembly):
//     PK_PAT_C_STEP    38   pk_rows_fast_mixed's pair of steps: 76 (50 fp64; 26 for the code bytes, the leaf table's address, two
//                           clamps, two selects, three keys and minima, the product's exponent and mantissa)
//     PK_PAT_C_PHASE1  33   phase 1's pair: 66 (48 fp64; no product, one key and one select per step, the table's address)
//     PK_PAT_C_WALK     7   phase 2's chunk of sixteen steps: 109 (16 fp64 multiplies, 16 extracts, 8 keys and minima, the products'
//                           exponents and mantissas)
//     PK_PAT_C_FIXED   30   outside the loops: the pad entry, the requests' addresses, the eight image words, the flags' test
// (two internal children: 162 today, 47 in phase 1 -- the form gains more there, so the rule follows the mixed wave).
// Instructions are not all of a wave's time: the walk's reads depend on phase 1's writes through LDS, and a phase-1 row is
// gathered through an offset the lane has to load first.  Measured (profiles/r08_summary.md, 40 960-particle launches): primate.p,
// 36 % fewer instructions in a mixed wave by these counts, launch -16 %; hohna_DS5 (6 -> 4 steps), 10.5 % fewer, launch +1.7 % --
// a tenth does not pay for the second phase.  So the form is taken only where it saves at least a FIFTH of today's count:
//     10 * (nU * C_PHASE1 + nS * C_WALK + C_FIXED) <= 8 * nS * C_STEP
// primate.p (15 -> 7 steps): 3660 <= 4560, taken.  hohna_DS5 (6 -> 4): 2040 > 1824, not taken.  hohna_DS6 (18 -> 8): 4200 <= 5472.
// hohna_DS8 (16 -> 7): 3730 <= 4864.  primates_small (12 -> 5): 2790 <= 3648.  S = U = 64 (1 -> 1): 700 > 304, never.
#define PK_PAT_C_STEP 38
#define PK_PAT_C_PHASE1 33
#define PK_PAT_C_WALK 7
#define PK_PAT_C_FIXED 30
static inline bool pk_pat_valid(int S, int U, bool coded, int ntiles) {
    return coded && ntiles == 1 && S >= 1 && U >= 1 && U <= PK_PAT_MAX_U;
}
static inline bool pk_pat_take(int S, int U, bool coded, int ntiles, int sw) {
    if (sw == PK_PAT_OFF || !pk_pat_valid(S, U, coded, ntiles)) return false;
    if (sw == PK_PAT_FORCE) return true;
    const long nS = (S + 63) / 64, nU = (U + 63) / 64;
    return 10 * (nU * PK_PAT_C_PHASE1 + nS * PK_PAT_C_WALK + PK_PAT_C_FIXED) <= 8 * nS * PK_PAT_C_STEP;
}

// ---- Clade patterns: one site likelihood per distinct column of the MERGED CLADE.
// The factor of a merge at a site depends only on the column restricted to the leaves below the new node: the induction above holds
// clade by clade (two sites whose columns agree on the leaves of Z = L u R carry bit-identical rows in L and in R).  Most merges
// build small clades, whose restricted columns are few, so phase 1 of the pattern form runs ceil(U_Z / 64) steps and not
// ceil(U / 64).  What a wave needs is one BLOCK per clade, found from the clade's leaf bitset alone (the bookkeeping hands the
// bitset to the merge in the high bits of the record's flag word): blocks are indexed directly by the bitset, all 2^N of them at one
// stride -- no directory, no dependent load in the wave's start-up.  The buffer (pk_clade_layout):
//
//   byte codes          [N][pk_packed_leaf_bytes(S)]: the one-byte codes again, leaf by leaf at the stride of the packed image, so a
//                       coded child's codes lie a fixed distance from its packed image (which the record holds) and a lane gathers
//                       the code of its representative site at (row offset >> 5).  Bytes past S are 0 and never read.
//   block Z             for every bitset Z < 2^N with at least three leaves (the others are never merged into by an uncoded child):
//       header          256 bytes, word 0 = U_Z, the distinct columns of the alignment restricted to Z's leaves
//       representatives off[c] = 32 * (first site of class c), c < U_Z, 0 behind them: 64 (ceil(U / 64) + 2) words (phase 1 reads
//                       one and two steps ahead).  Classes are numbered by first occurrence, so the representatives ascend.
//       site image      pk_pat_pack_image's layout exactly, 8 * class of every site, pad entry 8 U_Z.
//
// Built incrementally: the classes of Z are the classes of Z minus its highest leaf, refined by that leaf's code -- over the U
// global patterns, not the S sites (global patterns are numbered by first occurrence, so first occurrence among patterns IS first
// occurrence among sites).
#define PK_CLADE_MAX_N 12                // 2^N blocks, and the bitset's 12 bits in the flag word
#define PK_CLADE_MAX_BYTES ((size_t)32 << 20)   // the buffer's cap; primate.p (12 x 898, U = 413): 18 886 656 bytes
#define PK_CLADE_HDR_BYTES 256
#define PK_CLADE_DEFAULT 1               // PHYLO_CLADE_PATTERNS unset: the form is taken where it is eligible

enum { PK_CLADE_OFF = 0, PK_CLADE_AUTO = 1, PK_CLADE_FORCE = 2 };   // PHYLO_CLADE_PATTERNS = 0, unset, force

struct pk_clade_layout { size_t codes_bytes, rep_bytes, image_bytes, stride, total; };
static inline pk_clade_layout pk_clade_layout_of(int N, int S, int U) {
    pk_clade_layout L;
    L.codes_bytes = pk_packed_bytes(N, S);
    L.rep_bytes = (size_t)((U + 63) / 64 + 2) * 256;
    L.image_bytes = pk_pat_image_bytes(S);
    L.stride = PK_CLADE_HDR_BYTES + L.rep_bytes + L.image_bytes;
    L.total = L.codes_bytes + (N <= 30 ? ((size_t)1 << N) : ((size_t)1 << 30)) * L.stride;
    return L;
}
// The rule: the pattern form is taken (pk_pat_take), at least three and at most PK_CLADE_MAX_N taxa, the buffer within its cap.
static inline bool pk_clade_take(bool pat_taken, int N, int S, int U, int sw) {
    if (sw == PK_CLADE_OFF || (sw == PK_CLADE_AUTO && !PK_CLADE_DEFAULT)) return false;
    if (!pat_taken || N < 3 || N > PK_CLADE_MAX_N) return false;
    return pk_clade_layout_of(N, S, U).total <= PK_CLADE_MAX_BYTES;
}
// The buffer (pk_clade_layout_of(N, S, U).total bytes) of byte codes [N][S] with their global patterns pat[S], rep[U] (pk_pat_columns).
// Blocks of fewer than three leaves are not written.  cls_out, if given: [2^N][U], the class of every global pattern in every
// bitset (bitset 0: one class).
static inline void pk_clade_build(const uint8_t* codes, int N, int S, const int32_t* pat, const int32_t* rep, int U, uint8_t* out,
                                  uint16_t* cls_out) {
    const pk_clade_layout L = pk_clade_layout_of(N, S, U);
    const size_t leaf_bytes = pk_packed_leaf_bytes(S);
    memset(out, 0, L.codes_bytes);
    for (int leaf = 0; leaf < N; ++leaf) memcpy(out + (size_t)leaf * leaf_bytes, codes + (size_t)leaf * S, (size_t)S);
    std::vector<uint8_t> cu((size_t)N * U);                // the representatives' codes
    for (int leaf = 0; leaf < N; ++leaf)
        for (int u = 0; u < U; ++u) cu[(size_t)leaf * U + u] = codes[(size_t)leaf * S + rep[u]];
    // the global pattern of every entry of a site image, U for the pad
    const size_t nimg = L.image_bytes / 2;
    std::vector<uint16_t> pidx(nimg, (uint16_t)U);
    std::vector<uint16_t> off8((size_t)U + 1);             // 8 * class of every global pattern in the current bitset, then the pad
    for (int s = 0; s < S; ++s) {
        const int q = s / 64, c = s % 64;
        pidx[((size_t)(q / PK_CHUNK_STEPS) * 2 + (q % PK_CHUNK_STEPS) / 8) * (PK_PAT_HALF_BYTES / 2) + (size_t)c * 8 + q % 8] = (uint16_t)pat[s];
    }
    const size_t nZ = (size_t)1 << N;
    std::vector<uint16_t> cls_own;
    uint16_t* cls = cls_out;
    if (!cls) { cls_own.resize(nZ * U); cls = cls_own.data(); }
    for (int u = 0; u < U; ++u) cls[u] = 0;
    std::vector<int32_t> stamp((size_t)U * 6, 0);          // the bitset that last saw (class of Z minus its highest leaf, code)
    std::vector<uint16_t> id((size_t)U * 6);
    std::vector<uint32_t> first((size_t)U + 1);            // the representatives' row offsets of the current bitset
    const size_t rep_words = L.rep_bytes / 4;
    for (size_t Z = 1; Z < nZ; ++Z) {
        int h = 0, leaves = 0;
        for (int b = 0; b < N; ++b)
            if (Z >> b & 1) { h = b; ++leaves; }
        const uint16_t* cp = cls + (Z ^ ((size_t)1 << h)) * U;
        uint16_t* cz = cls + Z * U;
        const uint8_t* ch = cu.data() + (size_t)h * U;
        // (no branch on "a new class": it is unpredictable and would cost more than everything else here -- the class number and
        // the representative are written every time and kept only where the count moves on)
        int n = 0;
        for (int u = 0; u < U; ++u) {
            const size_t key = (size_t)cp[u] * 6 + ch[u];
            const unsigned int fresh = stamp[key] != (int32_t)Z, keep = fresh - 1u;   // (keep: all ones where the class is known)
            stamp[key] = (int32_t)Z;
            const uint16_t k = (uint16_t)(((unsigned int)n & ~keep) | (id[key] & keep));
            id[key] = k;
            first[n] = 32u * (uint32_t)rep[u];
            n += fresh;
            cz[u] = k;
        }
        if (leaves < 3) continue;
        uint8_t* blk = out + L.codes_bytes + Z * L.stride;
        uint32_t* ro = (uint32_t*)(blk + PK_CLADE_HDR_BYTES);
        memcpy(ro, first.data(), (size_t)n * 4);
        for (size_t w = (size_t)n; w < rep_words; ++w) ro[w] = 0u;
        memset(blk, 0, PK_CLADE_HDR_BYTES);
        *(uint32_t*)blk = (uint32_t)n;
        uint16_t* img = (uint16_t*)(blk + PK_CLADE_HDR_BYTES + L.rep_bytes);
        for (int u = 0; u < U; ++u) off8[u] = (uint16_t)(8 * cz[u]);
        off8[U] = (uint16_t)(8 * n);
        for (size_t i = 0; i < nimg; ++i) img[i] = off8[pidx[i]];
    }
}
