// phylo_launch_map.h -- which wave of a launch takes which item (pk_rank_merge_nostore; the particle part of pk_rank_book_chain).
// Plain C++ for host and device, stated here once: the driver sizes the grid with pk_launch_grid, the kernels ask pk_launch_item,
// and phylo_debug_launch_map runs the same two functions for tests/test_launch_map_cpu.py.
//
// A launch of n items at W waves per workgroup.  Workgroups are dealt round-robin to the 8 XCDs (observed, not promised: the result
// never depends on it).  With `xcd` set, each XCD gets a CONTIGUOUS range of slots, i.e. of particles, so that the particles of one
// sweep, which read the same few ancestors' rows and clade blocks, share one L2:
//   the grid is ceil(n / W) rounded up to a multiple of 8;
//   workgroup b takes slot (b & 7) * (grid >> 3) + (b >> 3);
//   wave w of that workgroup takes item slot * W + w; an item >= n has no work and its wave returns at once.
// Without it: slot = b, the grid is ceil(n / W).
#pragma once

#if defined(__HIPCC__)
#define PK_LM_HD __host__ __device__ __forceinline__
#else
#define PK_LM_HD inline
#endif

// (int throughout: a launch has fewer than 2^31 items, and the kernels compute this on the scalar pipe)
PK_LM_HD int pk_launch_grid(int n, int W, bool xcd) {
    const int g = (n + W - 1) / W;
    return xcd ? (g + 7) & ~7 : g;
}
PK_LM_HD int pk_launch_slot(int b, int grid, bool xcd) { return xcd ? (b & 7) * (grid >> 3) + (b >> 3) : b; }
PK_LM_HD int pk_launch_item(int b, int grid, int W, int w, bool xcd) { return pk_launch_slot(b, grid, xcd) * W + w; }
