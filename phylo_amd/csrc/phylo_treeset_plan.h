// phylo_treeset_plan.h -- the one slab builder and the one chunk / grid rule behind the plan of every scored-tree-set call
// (DESIGN.md section 15c).  A call's slab is a list of regions in slab order, then the node store of its resident workgroups.  A
// plan function states its regions once; the bytes of a tree, the chunk, the grid, the offsets and the total all follow from that
// list here, and pts_check_plan checks any plan against its list (the tests/*_asan_main.cpp programs).  Plain C++, no HIP.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

enum pts_kind {
    PTS_FIXED,                     // `bytes` once, whatever the chunk
    PTS_TREE,                      // `bytes` per tree of the chunk, counted in per_tree: the chunk budget bounds their sum
    PTS_STAGED                     // `bytes` per tree of the chunk, staging of requested outputs: bounded by the staging cap instead
};

struct pts_region {
    pts_kind kind;
    size_t bytes;
    bool present;                  // an absent region takes no bytes; its offset is that of the next region
    size_t* off;                   // where its offset goes: a field of the call's plan
};

#define PTS_MAX_REGIONS 16                        // regions of the longest list (the callers' arrays)

inline size_t pts_up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the bytes one tree adds to a chunk: the sum of the present regions of one kind
inline size_t pts_sum(const pts_region* r, int nr, pts_kind kind) {
    size_t s = 0;
    for (int i = 0; i < nr; ++i)
        if (r[i].present && r[i].kind == kind) s += r[i].bytes;
    return s;
}

// Trees per chunk: what the budget holds, at least 1; at most 0x7fffffff / ntiles (items of a chunk are counted in an int); at most
// out_region / out_tree where the call stages outputs (out_tree > 0); at most env_chunk when > 0 (PHYLO_TREES_CHUNK); at most T.
inline int pts_chunk(size_t per_tree, int ntiles, int T, int env_chunk, size_t budget, size_t out_region, size_t out_tree) {
    size_t fit = budget / per_tree;
    if (fit < 1) fit = 1;
    if (fit > (size_t)(0x7fffffff / ntiles)) fit = (size_t)(0x7fffffff / ntiles);
    if (out_tree > 0 && out_region / out_tree < fit) fit = out_region / out_tree;      // >= 1: the region grows to one tree's need
    if (env_chunk > 0 && (size_t)env_chunk < fit) fit = (size_t)env_chunk;
    if (fit > (size_t)T) fit = (size_t)T;
    return (int)fit;
}

// Workgroups of a full chunk: min(items, max(1, min(store_bytes / wg_store, n_cus * wg_per_cu)))
inline int pts_grid(size_t items, size_t wg_store, int n_cus, size_t store_bytes, int wg_per_cu) {
    size_t cap = store_bytes / wg_store;
    if (cap > (size_t)n_cus * wg_per_cu) cap = (size_t)n_cus * wg_per_cu;
    if (cap < 1) cap = 1;
    return (int)(items < cap ? items : cap);
}

// Offsets of the regions for a chunk of n trees, each a multiple of 256, then the node store (store_bytes, at *o_store when given).
// Returns the total.
inline size_t pts_lay_out(const pts_region* r, int nr, size_t n, size_t store_bytes, size_t* o_store) {
    size_t o = 0;
    for (int i = 0; i < nr; ++i) {
        *r[i].off = o;
        if (r[i].present) o += pts_up256(r[i].kind == PTS_FIXED ? r[i].bytes : n * r[i].bytes);
    }
    if (o_store) *o_store = o;
    return o + store_bytes;
}

// What a plan function passes to pts_check_plan beside its regions (r's offsets are the checked plan's own fields)
struct pts_plan_facts {
    int chunk, grid;               // grid 0 and wg_store 0: a call without a node store
    size_t per_tree, wg_store, o_store, total;
    int ntiles, T, n_cus, env_chunk;
    size_t chunk_budget, store_budget;
    int wg_per_cu;
    size_t out_region;             // 0: no staging
};

// The number of violated properties of a plan: offsets aligned and ordered, regions apart and inside total, per_tree the sum of the
// list, the chunk within every bound, items in an int, the grid within its caps.
inline long pts_check_plan(const pts_region* r, int nr, const pts_plan_facts& f) {
    long bad = 0;
    const size_t n = (size_t)f.chunk, store = (size_t)f.grid * f.wg_store;
    size_t end = 0, tree_sum = 0;                           // end of the regions so far; bytes of the PTS_TREE regions of the chunk
    for (int i = 0; i < nr; ++i) {
        const size_t o = *r[i].off, need = !r[i].present ? 0 : r[i].kind == PTS_FIXED ? r[i].bytes : n * r[i].bytes;
        bad += o % 256 != 0;
        bad += o < end;                                     // ordered, and apart from the one before
        end = o + need;
        if (r[i].present && r[i].kind == PTS_TREE) tree_sum += need;
    }
    bad += f.o_store % 256 != 0 || f.o_store < end;
    bad += f.o_store + store > f.total;                     // every region lies inside total (they are ordered)
    bad += f.per_tree * n != tree_sum || f.per_tree != pts_sum(r, nr, PTS_TREE);
    bad += f.chunk < 1 || f.chunk > f.T || (f.env_chunk > 0 && f.chunk > f.env_chunk);
    bad += f.chunk > 1 && n * f.per_tree > f.chunk_budget;
    bad += n * pts_sum(r, nr, PTS_STAGED) > f.out_region;
    bad += n * (size_t)f.ntiles > 0x7fffffffu;
    if (f.wg_store) {
        bad += f.grid < 1 || (size_t)f.grid > n * (size_t)f.ntiles || f.grid > f.n_cus * f.wg_per_cu;
        bad += f.grid > 1 && store > f.store_budget;
    } else
        bad += f.grid != 0;
    return bad;
}

// every region written end to end into a heap buffer of exactly `total` bytes (under the address sanitizer: nothing past the end),
// then read back: no region overwrote another.  buf: total bytes.
inline long pts_fill_plan(const pts_region* r, int nr, const pts_plan_facts& f, unsigned char* buf) {
    long bad = 0;
    const size_t n = (size_t)f.chunk, store = (size_t)f.grid * f.wg_store;
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = 0; i <= nr; ++i) {
            const size_t o = i < nr ? *r[i].off : f.o_store;
            const size_t need = i == nr ? store : !r[i].present ? 0 : r[i].kind == PTS_FIXED ? r[i].bytes : n * r[i].bytes;
            if (!need) continue;
            if (pass == 0)
                memset(buf + o, i, need);
            else
                bad += buf[o] != (unsigned char)i || buf[o + need - 1] != (unsigned char)i;
        }
    }
    return bad;
}
