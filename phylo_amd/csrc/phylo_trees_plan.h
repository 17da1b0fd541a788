// phylo_trees_plan.h -- the form of the tree posterior's two device passes (phylo_hip.hip: tree_summary_impl and tree_branches_impl
// with their ts_* / tb_* stages; kernels in phylo_trees.h).  Plain C++, no HIP, like phylo_sweep_plan.h: the
// same functions run in the driver and behind phylo_debug_tree_plan (tests/test_treeplan_cpu.py restates the rules).
//
// What is decided HERE and nowhere else, once per call: the refusals, the sizes, the radix bits of every sort, the 64-bit (wide)
// keys and the gather of the branch pass, the layout of the two scratch slabs, and what stats.n_launches counts.  The stages of
// the driver only read the plan.  rocPRIM's temporary-storage size is a fact passed in (the driver queries it).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

inline unsigned pt_bit_length(size_t v) { unsigned b = 0; while (v) { ++b; v >>= 1; } return b ? b : 1; }

// ---- slabs: every buffer of a pass, carved from one scratch slot ---------------------------------------------------------------
// One list per slab, X(name, element type, elements), in slab order (the order is part of the contract: the total is what
// scratch_get is asked for).  It makes the names (pt_slab::name), the layout (pt_plan_slab / pb_plan_slab) and, in the driver, the
// pointers of pt_bufs / pb_bufs (slab_carve).  The counts are expressions over the locals of the layout function.
#define PT_SLAB_BUFS(X)                                                                                                          \
    X(u, unsigned long long, Ks) X(U, unsigned long long, G) X(bits, unsigned long long, (size_t)(R - 1) * W * Ks)                \
    X(kA, unsigned long long, Em) X(kB, unsigned long long, Em) X(val, unsigned long long, Em) X(scan, unsigned long long, Em)    \
    X(weight, unsigned long long, Em) X(srt, unsigned long long, Es) X(hp, unsigned long long, Ks)                                \
    X(o_cbits, unsigned long long, Es * W) X(o_cw, unsigned long long, Es) X(o_tw, unsigned long long, Ks)                        \
    X(child, int32_t, p.world > 1 ? (size_t)R * Ks * 2 : 0) X(slot, int32_t, (size_t)R * Ks)                                      \
    X(o_cg, int32_t, Es) X(o_tn, int32_t, Ks) X(o_trep, int32_t, Ks) X(o_tg, int32_t, Ks) X(o_ptopo, int32_t, Ks)                 \
    X(vA, uint32_t, Em) X(vB, uint32_t, Em) X(flag, uint32_t, Em) X(sid, uint32_t, Em) X(cid, uint32_t, Es)                       \
    X(seg_start, uint32_t, Em) X(count, uint32_t, Em) X(group, uint32_t, Em) X(first, uint32_t, Em) X(tid, uint32_t, Ks)          \
    X(pos, uint32_t, Ks) X(err, uint32_t, 4) X(vC, uint32_t, Em) X(vD, uint32_t, Em) X(temp, unsigned char, p.temp_bytes)

#define PB_SLAB_BUFS(X)                                                                                                          \
    X(ebr, double, (size_t)(R - 1) * Ks) X(lbr, double, (size_t)N * Ks)                                                           \
    X(gbl, double, p.gather ? (size_t)R * Ks : 0) X(gbr, double, p.gather ? (size_t)R * Ks : 0)                                   \
    X(o_cs, double, (size_t)p.nc * 4) X(o_ls, double, (size_t)G * N * 4) X(o_ts, double, (size_t)p.nt * nb * 4)                   \
    X(wA, unsigned long long, p.wide ? Es : 0) X(wB, unsigned long long, p.wide ? Es : 0)                                         \
    X(cpos, uint32_t, Es) X(kA, uint32_t, Es) X(kB, uint32_t, Es) X(vA, uint32_t, Es) X(vB, uint32_t, Es)                         \
    X(cstart, uint32_t, (size_t)p.nc + 1) X(toff, uint32_t, (size_t)p.nt) X(o_tc, int32_t, (size_t)p.nt * L)                      \
    X(temp, unsigned char, p.temp_bytes)

#define PT_SLAB_NAME(name, T, n) name,
struct pt_slab { enum { PT_SLAB_BUFS(PT_SLAB_NAME) NBUF }; size_t off[NBUF], bytes[NBUF], total; };
struct pb_slab { enum { PB_SLAB_BUFS(PT_SLAB_NAME) NBUF }; size_t off[NBUF], bytes[NBUF], total; };
#undef PT_SLAB_NAME

// buffer `id` of `bytes` bytes starts where the slab ends; every buffer starts on a multiple of 256 bytes
template <typename SLAB>
inline void slab_add(SLAB& s, int id, size_t bytes) {
    s.off[id] = s.total;
    s.bytes[id] = bytes;
    s.total += (bytes + 255) / 256 * 256;
}
#define PT_SLAB_ADD(name, T, n) slab_add(p.slab, p.slab.name, (size_t)(n) * sizeof(T));

// ---- the summary (phylo_tree_summary) ------------------------------------------------------------------------------------------
struct pt_facts {
    int N, K, G, world;                // (K: all ranks' particles; G: the groups of the summarised sweep, K % G == 0)
};

enum { PT_MAX_WORDS = 8 };             // bitset words of a clade: ceil(PK_MAX_TAXA / 64)

struct pt_plan {
    int N, K, G, world;
    int R, L, W, Kg;                   // rank events; clades per tree; words per bitset; particles per group
    long long E, Emax;                 // clade entries L K; the longest array any sort or scan sees: max(E, K)
    bool groups;                       // G > 1: every sort by content is followed by a stable pass on the group
    // radix bits of the sort passes (all stable, on bits [0, bits))
    unsigned word_bits[PT_MAX_WORDS];  // clades by bitset word w, least significant word first
    unsigned group_bits;               // ... then by group; the topologies by group behind their hash alike
    unsigned weight_bits;              // segments by weight (descending); the topology hash uses all 64 too
    unsigned order_group_bits;         // the output order's last pass: the group (G itself marks the elements that head no segment)
    unsigned cid_bits;                 // (particle, clade id) pairs: every particle's clade ids ascending
    unsigned rep_bits;                 // topologies by representative particle
    size_t temp_bytes;
    pt_slab slab;
};

// The argument refusals of a summary, in the order phylo_tree_summary checks them behind its state checks (PHYLO_EINVAL)
inline bool pt_refuses(const pt_facts& f, char* msg, size_t n) {
    if (f.N < 3) return snprintf(msg, n, "phylo_tree_summary needs N >= 3 taxa (got %d)", f.N), true;
    const long long E = (long long)(f.N - 2) * f.K, Emax = E > f.K ? E : f.K;
    if (Emax >= 0xffffffffll)
        return snprintf(msg, n, "phylo_tree_summary: (N - 2) K = %lld clade entries exceed 2^32 - 1", E), true;
    return false;
}

inline pt_plan pt_plan_form(const pt_facts& f) {
    pt_plan p{};
    p.N = f.N; p.K = f.K; p.G = f.G; p.world = f.world;
    p.R = f.N - 1; p.L = f.N - 2; p.W = (f.N + 63) / 64; p.Kg = f.K / f.G;
    p.E = (long long)p.L * f.K; p.Emax = p.E > f.K ? p.E : f.K;
    p.groups = f.G > 1;
    for (int w = 0; w < p.W; ++w) p.word_bits[w] = (unsigned)(f.N - 64 * w < 64 ? f.N - 64 * w : 64);
    p.group_bits = pt_bit_length((size_t)f.G - 1);
    p.weight_bits = 64;
    p.order_group_bits = pt_bit_length((size_t)f.G);
    p.cid_bits = 32 + pt_bit_length((size_t)f.K - 1);
    p.rep_bits = pt_bit_length((size_t)f.K);
    return p;
}

// the layout of scratch slot 12, once rocPRIM's temporary storage for arrays of Emax elements is known
inline void pt_plan_slab(pt_plan& p, size_t temp_bytes) {
    const int R = p.R, W = p.W, G = p.G;
    const size_t Ks = p.K, Es = p.E, Em = p.Emax;
    p.temp_bytes = temp_bytes;
    p.slab.total = 0;
    PT_SLAB_BUFS(PT_SLAB_ADD)
}

// The sort passes in issue order: their radix bits into bits[], their number returned (at most PT_MAX_WORDS + 9)
inline int pt_plan_sorts(const pt_plan& p, unsigned* bits) {
    int n = 0;
    for (int w = 0; w < p.W; ++w) bits[n++] = p.word_bits[w];         // clades: the bitset words
    if (p.groups) bits[n++] = p.group_bits;
    bits[n++] = p.weight_bits;                                         // clade order
    if (p.groups) bits[n++] = p.order_group_bits;
    bits[n++] = p.cid_bits;                                            // every particle's clade ids
    bits[n++] = p.weight_bits;                                         // topologies: the hash
    if (p.groups) bits[n++] = p.group_bits;
    bits[n++] = p.rep_bits;                                            // topology order
    bits[n++] = p.weight_bits;
    if (p.groups) bits[n++] = p.order_group_bits;
    return n;
}

// What phylo_tree_summary counts into stats.n_launches: every kernel, sort and scan of the stages (a sort or scan counts 1
// whatever rocPRIM launches for it; the memset, the copies and the events are not counted).  Weights and walk 2; per bitset word
// keys + sort; clade groups 5, order 2, output 1; in-particle sort and hash 2 + 2; topology groups 5, order 4, output 3; and
// keys + sort for each of the four group passes of a batch.
inline int pt_plan_launches(const pt_plan& p) { return 26 + 2 * p.W + (p.groups ? 8 : 0); }

// ---- the branch pass (phylo_tree_branches) ---------------------------------------------------------------------------------------
struct pb_facts {
    int N, K, G, world;                // (G: the summary's)
    long long nc, nt;                  // the summary's rows: clades and topologies, over all groups
    bool kept_whole;                   // the sweep kept its graph and left whole-K branch lengths (graph_gather)
    bool force_wide;                   // PHYLO_TREE_WIDE_KEYS (tests): the 64-bit keys at any size
};

struct pb_plan {
    int N, K, G, world;
    int R, L, Kg;
    long long E, nc, nt, nb;           // nb: the 2N - 2 branches of a topology row
    unsigned cbits, tbits;             // bits of a clade row, of a topology row
    bool wide;                         // (topology, clade) keys need more than 32 bits: the 64-bit sort
    bool gather;                       // sharded and no whole-K branch lengths kept: two host collectives
    size_t temp_bytes;
    pb_slab slab;
};

// The refusal behind the state checks of phylo_tree_branches (PHYLO_ESTATE)
inline bool pb_refuses(const pb_facts& f, char* msg, size_t n) {
    const long long E = (long long)(f.N - 2) * f.K;
    if (f.nc < 1 || f.nt < 1 || f.nc > E || f.nt > f.K) return snprintf(msg, n, "phylo_tree_branches: the summary holds no rows"), true;
    return false;
}

inline pb_plan pb_plan_form(const pb_facts& f) {
    pb_plan p{};
    p.N = f.N; p.K = f.K; p.G = f.G; p.world = f.world;
    p.R = f.N - 1; p.L = f.N - 2; p.Kg = f.K / f.G;
    p.E = (long long)p.L * f.K; p.nc = f.nc; p.nt = f.nt; p.nb = 2LL * f.N - 2;
    p.cbits = pt_bit_length((size_t)f.nc - 1);
    p.tbits = pt_bit_length((size_t)f.nt - 1);
    p.wide = f.force_wide || p.cbits + p.tbits > 32;       // 32 bits hold the keys on all but huge tables
    p.gather = f.world > 1 && !f.kept_whole;
    return p;
}

// the layout of scratch slot 13 (temporary storage: the 32-bit sort of E pairs, the 64-bit one when wide, the scan of nt counts)
inline void pb_plan_slab(pb_plan& p, size_t temp_bytes) {
    const int N = p.N, R = p.R, L = p.L, G = p.G;
    const size_t Ks = p.K, Es = p.E, nb = p.nb;
    p.temp_bytes = temp_bytes;
    p.slab.total = 0;
    PB_SLAB_BUFS(PT_SLAB_ADD)
}

// What phylo_tree_branches counts: walk 1; clade rows 5 (invert, keys, sort, starts, sums); leaf rows 1; topology rows 4 (scan,
// keys, sort, sums), the same for both key widths.
inline int pb_plan_launches(const pb_plan&) { return 11; }
