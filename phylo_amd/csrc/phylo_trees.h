// phylo_trees.h -- summary of the tree posterior of the last sweep (phylo_tree_summary): integer weights of
// the final particles, the non-trivial clades of every particle's tree with their exact u64 weights, and the topologies (clade
// sets) with their weights, particle counts and representatives.  Runs on the context's stream after the sweep, never inside it;
// reads the sweep's children records and last log-weight row and writes nothing the sweep owns.
//
// Layouts (R = N - 1 rank events, L = N - 2 clades per tree, E = L K clade entries, entry e = r K + k: the clade below the node of
// rank event r < R - 1 in particle k's tree; W = ceil(N / 64) words per bitset, taxon i = bit i % 64 of word i / 64):
//   slot  [R][K]       int32   node id of rank event r in particle k's tree (every tree has exactly one node per rank event)
//   bits  [R-1][W][K]  uint64  clade bitsets of the entries, word-major so that the walk's stores coalesce
// Sorts and segment sums use rocPRIM's (stable, LSD) radix sort and scans: no atomics on the sums, so a degenerate genealogy
// (one clade held by every particle) costs what any other does.  The only float operation is the exp of the weights.
#pragma once

#include <rocprim/device/device_scan.hpp>

#include "phylo_math.h"

#define PT_NT 256
enum { PT_ERR_TREE = 1, PT_ERR_COLLISION = 2 };

// device buffers of one summary, carved from one slab (layout: phylo_trees_plan.h); the o_* tables are what the fetch reads
struct pt_bufs {
    unsigned long long *u = nullptr, *U = nullptr, *bits = nullptr, *kA = nullptr, *kB = nullptr, *val = nullptr, *scan = nullptr;
    unsigned long long *weight = nullptr, *srt = nullptr, *hp = nullptr, *o_cbits = nullptr, *o_cw = nullptr, *o_tw = nullptr;
    int32_t *child = nullptr, *slot = nullptr, *o_cg = nullptr, *o_tn = nullptr, *o_trep = nullptr, *o_tg = nullptr, *o_ptopo = nullptr;
    uint32_t *vA = nullptr, *vB = nullptr, *flag = nullptr, *sid = nullptr, *cid = nullptr, *seg_start = nullptr, *count = nullptr;
    uint32_t *group = nullptr, *first = nullptr, *tid = nullptr, *pos = nullptr;
    uint32_t *vC = nullptr, *vD = nullptr;   // the topology stage's values: the clade order (cord, in vA or vB) outlives the summary
    const uint32_t* cord = nullptr;          // clade segment of every output row (phylo_tree_branches inverts it)
    uint32_t* err = nullptr;                 // [0] PT_ERR_* bits, [1] clade count, [2] topology count
    unsigned char* temp = nullptr;           // rocPRIM's temporary storage
};

// u_k = floor(exp(logw[R-1][k] - max_g) 2^44) per group g of Kg columns (the resampling contract's integer weights, same NaN /
// all-bad rules as the scan), and U_g = sum of the group's u_k (u64, tree reduction in LDS).  One workgroup per group.
__global__ void __launch_bounds__(PT_NT) pt_weights(const double* __restrict__ logw_last, int Kg, unsigned long long* __restrict__ u,
                                                    unsigned long long* __restrict__ U) {
    __shared__ double smax[PT_NT];
    __shared__ unsigned long long ssum[PT_NT];
    const int g = blockIdx.x, t = threadIdx.x;
    const double* w = logw_last + (size_t)g * Kg;
    double m = -pm_inf();
    for (int j = t; j < Kg; j += PT_NT) {
        const double v = w[j];
        if (!pm_isnan(v) && v > m) m = v;
    }
    smax[t] = m;
    __syncthreads();
    for (int s = PT_NT / 2; s > 0; s >>= 1) {
        if (t < s && smax[t + s] > smax[t]) smax[t] = smax[t + s];
        __syncthreads();
    }
    m = smax[0];
    const bool all_bad = !(m > -pm_inf()) || m == pm_inf();
    unsigned long long part = 0;
    for (int j = t; j < Kg; j += PT_NT) {
        const unsigned long long x = pm_weight_int(w[j], m, all_bad);
        u[(size_t)g * Kg + j] = x;
        part += x;
    }
    ssum[t] = part;
    __syncthreads();
    for (int s = PT_NT / 2; s > 0; s >>= 1) {
        if (t < s) ssum[t] += ssum[t + s];
        __syncthreads();
    }
    if (t == 0) U[g] = ssum[0];
}

// One thread per final particle k: the nodes of its tree top-down (slot), then the clade bitsets bottom-up, one word at a time
// (no per-thread arrays: nothing leaves registers).  A malformed record (child id out of range, a rank event met twice or
// never) raises PT_ERR_TREE and the particle writes no clades.
__global__ void __launch_bounds__(PT_NT) pt_walk(const int32_t* __restrict__ child, int N, int K, int W, int32_t* __restrict__ slot,
                                                 unsigned long long* __restrict__ bits, unsigned int* __restrict__ err) {
    const int k = blockIdx.x * PT_NT + threadIdx.x;
    if (k >= K) return;
    const int R = N - 1;
    const long long n_nodes = (long long)N + (long long)R * K;
    for (int r = 0; r < R - 1; ++r) slot[(size_t)r * K + k] = -1;
    slot[(size_t)(R - 1) * K + k] = N + (R - 1) * K + k;
    bool bad = false;
    for (int r = R - 1; r >= 0 && !bad; --r) {
        const int nd = slot[(size_t)r * K + k];
        const int kk = nd - N - r * K;
        if (nd < 0 || kk < 0 || kk >= K) { bad = true; break; }
        for (int s = 0; s < 2; ++s) {
            const int c = child[((size_t)r * K + kk) * 2 + s];
            if (c < 0 || c >= n_nodes) { bad = true; break; }
            if (c < N) continue;
            const int rc = (c - N) / K;
            if (rc >= r || slot[(size_t)rc * K + k] != -1) { bad = true; break; }
            slot[(size_t)rc * K + k] = c;
        }
    }
    if (bad) {
        atomicOr(err, (unsigned int)PT_ERR_TREE);
        return;
    }
    for (int w = 0; w < W; ++w) {
        for (int r = 0; r < R - 1; ++r) {
            const int nd = slot[(size_t)r * K + k];
            const int kk = nd - N - r * K;
            unsigned long long b = 0;
            for (int s = 0; s < 2; ++s) {
                const int c = child[((size_t)r * K + kk) * 2 + s];
                if (c < N) b |= (c >> 6) == w ? 1ull << (c & 63) : 0ull;
                else b |= bits[((size_t)((c - N) / K) * W + w) * K + k];
            }
            bits[((size_t)r * W + w) * K + k] = b;
        }
    }
}

// keys of one LSD pass over the entries in their current order perm: word w of the clade bitset, or (w < 0) the group.  perm ==
// nullptr: the identity (first pass; vout receives it).  Also the group keys of particles (E = K: entry k is particle k).
__global__ void pt_clade_keys(const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ perm, long long E, int K, int W,
                              int w, int Kg, unsigned long long* __restrict__ key, uint32_t* __restrict__ vout) {
    const long long i = (long long)blockIdx.x * PT_NT + threadIdx.x;
    if (i >= E) return;
    const uint32_t e = perm ? perm[i] : (uint32_t)i;
    if (!perm) vout[i] = e;
    const uint32_t r = e / (uint32_t)K, k = e % (uint32_t)K;
    key[i] = w >= 0 ? bits[((size_t)r * W + w) * K + k] : (unsigned long long)(k / (uint32_t)Kg);
}

// clade segment heads of the sorted entries (equal bitset and group) and the values their sums scan: val[i] = u of the particle
__global__ void pt_clade_heads(const unsigned long long* __restrict__ bits, const uint32_t* __restrict__ perm, long long E, int K, int W,
                               int Kg, const unsigned long long* __restrict__ u, uint32_t* __restrict__ flag,
                               unsigned long long* __restrict__ val) {
    const long long i = (long long)blockIdx.x * PT_NT + threadIdx.x;
    if (i >= E) return;
    const uint32_t e = perm[i], r = e / (uint32_t)K, k = e % (uint32_t)K;
    bool head = i == 0;
    if (!head) {
        const uint32_t ep = perm[i - 1], rp = ep / (uint32_t)K, kp = ep % (uint32_t)K;
        head = k / (uint32_t)Kg != kp / (uint32_t)Kg;
        for (int w = 0; w < W && !head; ++w)
            head = bits[((size_t)r * W + w) * K + k] != bits[((size_t)rp * W + w) * K + kp];
    }
    flag[i] = head ? 1u : 0u;
    val[i] = u[k];
}

// After the scans (sid = inclusive sum of the heads: 1-based segment ids): every element's segment id, stored at the element's
// identity (id_of[perm[i]]: the clade id of entry e, or the topology of particle k), and every segment's start.
__global__ void pt_seg_ids(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ sid,
                           long long E, uint32_t* __restrict__ id_of, uint32_t* __restrict__ seg_start) {
    const long long i = (long long)blockIdx.x * PT_NT + threadIdx.x;
    if (i >= E) return;
    const uint32_t s = sid[i] - 1;
    id_of[perm[i]] = s;
    if (flag[i]) seg_start[s] = (uint32_t)i;
}

// One thread per slot s < E of the segment tables (slots past the segment count n = sid[E-1] are padding, ordered last):
// weight = difference of the inclusive u64 scan across the segment (exact modulo 2^64, and every weight is below 2^64), element
// count, group, first element in sorted order (of a topology: its smallest particle, the sorts being stable over particles in
// ascending order).  perm holds entries e = r K + k or particles k: e % K is the particle.
__global__ void pt_seg_sums(const uint32_t* __restrict__ perm, const uint32_t* __restrict__ sid, const uint32_t* __restrict__ seg_start,
                            const unsigned long long* __restrict__ scan, long long E, int K, int Kg, int G,
                            unsigned long long* __restrict__ weight, uint32_t* __restrict__ count, uint32_t* __restrict__ group,
                            uint32_t* __restrict__ first) {
    const long long s = (long long)blockIdx.x * PT_NT + threadIdx.x;
    if (s >= E) return;
    const long long n = sid[E - 1];
    if (s >= n) {
        weight[s] = 0;
        count[s] = 0;
        group[s] = (uint32_t)G;
        first[s] = 0xffffffffu;
        return;
    }
    const long long b = seg_start[s], e = s + 1 < n ? (long long)seg_start[s + 1] : E;
    weight[s] = scan[e - 1] - (b ? scan[b - 1] : 0ull);
    count[s] = (uint32_t)(e - b);
    const uint32_t m = perm[b];
    group[s] = (m % (uint32_t)K) / (uint32_t)Kg;
    first[s] = m;
}

// keys of the ordering passes over the segment slots: 0 ~weight (descending), 1 group, 2 the first element's particle (ascending
// representative; padding K).  order == nullptr: the identity (first pass; vout receives it).
__global__ void pt_order_keys(const uint32_t* __restrict__ order, long long n, int what, int K, const unsigned long long* __restrict__ weight,
                              const uint32_t* __restrict__ group, const uint32_t* __restrict__ first, unsigned long long* __restrict__ key,
                              uint32_t* __restrict__ vout) {
    const long long i = (long long)blockIdx.x * PT_NT + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = order ? order[i] : (uint32_t)i;
    if (!order) vout[i] = s;
    unsigned long long x;
    if (what == 0) x = ~weight[s];
    else if (what == 1) x = group[s];
    else x = first[s] == 0xffffffffu ? (unsigned long long)K : (unsigned long long)(first[s] % (uint32_t)K);
    key[i] = x;
}

// (particle, clade id) keys of the per-particle sort: once sorted, particle k's ids are the low words of
// sorted[k L .. (k+1) L), ascending
__global__ void pt_topo_pairs(const uint32_t* __restrict__ cid, long long E, int K, unsigned long long* __restrict__ key,
                              uint32_t* __restrict__ vout) {
    const long long i = (long long)blockIdx.x * PT_NT + threadIdx.x;
    if (i >= E) return;
    key[i] = ((unsigned long long)(i % K) << 32) | cid[i];
    vout[i] = 0;
}

__device__ __forceinline__ unsigned long long pt_mix(unsigned long long x) {   // splitmix64's finaliser
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// routing key of particle k's topology: a hash of its sorted clade-id vector (equality is then checked element by element);
// hp[k] keeps it by particle
__global__ void pt_topo_hash(const unsigned long long* __restrict__ sorted, int K, int L, unsigned long long* __restrict__ key,
                             uint32_t* __restrict__ vout, unsigned long long* __restrict__ hp) {
    const int k = blockIdx.x * PT_NT + threadIdx.x;
    if (k >= K) return;
    unsigned long long h = 0x9e3779b97f4a7c15ull;
    for (int j = 0; j < L; ++j) h = pt_mix(h ^ (sorted[(size_t)k * L + j] & 0xffffffffull));
    key[k] = h;
    hp[k] = h;
    vout[k] = (uint32_t)k;
}

// topology segment heads over the particles sorted by (group, hash): a new group or hash opens a segment; equal routing keys must
// hold equal clade-id vectors, checked against the predecessor (equality is transitive: against the head) -- a mismatch is a hash
// collision, reported (PT_ERR_COLLISION) and never merged.  val[i] = u of the particle.
__global__ void pt_topo_heads(const unsigned long long* __restrict__ hp, const uint32_t* __restrict__ perm,
                              const unsigned long long* __restrict__ sorted, int K, int L, int Kg, const unsigned long long* __restrict__ u,
                              uint32_t* __restrict__ flag, unsigned long long* __restrict__ val, unsigned int* __restrict__ err) {
    const int i = blockIdx.x * PT_NT + threadIdx.x;
    if (i >= K) return;
    const uint32_t k = perm[i];
    bool head = i == 0;
    if (!head) {
        const uint32_t kp = perm[i - 1];
        head = hp[k] != hp[kp] || k / (uint32_t)Kg != kp / (uint32_t)Kg;
        if (!head) {
            bool same = true;
            for (int j = 0; j < L && same; ++j)
                same = (uint32_t)sorted[(size_t)k * L + j] == (uint32_t)sorted[(size_t)kp * L + j];
            if (!same) atomicOr(err, (unsigned int)PT_ERR_COLLISION);
        }
    }
    flag[i] = head ? 1u : 0u;
    val[i] = u[k];
}

// position of every segment slot in the output order (pos[order[j]] = j)
__global__ void pt_invert(const uint32_t* __restrict__ order, long long n, uint32_t* __restrict__ pos) {
    const long long j = (long long)blockIdx.x * PT_NT + threadIdx.x;
    if (j >= n) return;
    pos[order[j]] = (uint32_t)j;
}

// the output tables in order, rows j < n = sid[E-1]: clade j = segment order[j] (its bitset read at its first entry)
__global__ void pt_clade_out(const uint32_t* __restrict__ order, const uint32_t* __restrict__ sid, long long E, int K, int W,
                             const unsigned long long* __restrict__ bits, const unsigned long long* __restrict__ weight,
                             const uint32_t* __restrict__ group, const uint32_t* __restrict__ first, unsigned long long* __restrict__ o_bits,
                             unsigned long long* __restrict__ o_weight, int32_t* __restrict__ o_group) {
    const long long j = (long long)blockIdx.x * PT_NT + threadIdx.x;
    if (j >= E || j >= (long long)sid[E - 1]) return;
    const uint32_t s = order[j], e = first[s], r = e / (uint32_t)K, k = e % (uint32_t)K;
    for (int w = 0; w < W; ++w) o_bits[(size_t)j * W + w] = bits[((size_t)r * W + w) * K + k];
    o_weight[j] = weight[s];
    o_group[j] = (int32_t)group[s];
}

// ... topology j: weight, particle count, group, representative (inside its group)
__global__ void pt_topo_out(const uint32_t* __restrict__ order, const uint32_t* __restrict__ sid, int K, int Kg,
                            const unsigned long long* __restrict__ weight, const uint32_t* __restrict__ count,
                            const uint32_t* __restrict__ group, const uint32_t* __restrict__ first, unsigned long long* __restrict__ o_weight,
                            int32_t* __restrict__ o_count, int32_t* __restrict__ o_rep, int32_t* __restrict__ o_group) {
    const int j = blockIdx.x * PT_NT + threadIdx.x;
    if (j >= K || j >= (int)sid[K - 1]) return;
    const uint32_t s = order[j];
    o_weight[j] = weight[s];
    o_count[j] = (int32_t)count[s];
    o_group[j] = (int32_t)group[s];
    o_rep[j] = (int32_t)(first[s] % (uint32_t)Kg);
}

// particle k's topology: its segment's row in the output (over all groups; the fetch subtracts the group's first row)
__global__ void pt_particle_topo(const uint32_t* __restrict__ tid, const uint32_t* __restrict__ pos, int K, int32_t* __restrict__ out) {
    const int k = blockIdx.x * PT_NT + threadIdx.x;
    if (k >= K) return;
    out[k] = (int32_t)pos[tid[k]];
}

// ---- branch lengths of the tree posterior (phylo_tree_branches) ------------------------------------------
// For the last summary: the length of the branch above every clade entry and every leaf of every final particle's tree (pb_walk),
// then S1 = sum of u_k b, S2 = sum of (u_k b) b, min and max of b over three families of segments by ONE kernel (pb_seg_sums):
// the clade rows, the leaves of every group, and the 2N - 2 branches of every topology row.  Canonical segment sum: element j of a
// segment goes to column j mod 64, a column adds its elements in increasing j from +0.0, the 64 columns are added by the
// adjacent-pair tree (pk_wave_tree_sum, phylo_kernels.h, included before this file).  One wavefront owns a segment, lane = column:
// no atomics, and the result does not depend on how segments are spread over workgroups.
struct pb_bufs {
    double *ebr = nullptr, *lbr = nullptr;   // [R-1][K] branch above entry (r, k); [N][K] branch above leaf i of particle k
    double *gbl = nullptr, *gbr = nullptr;   // sharded without a kept graph: the whole-K branch lengths [R][K]
    uint32_t *cpos = nullptr, *kA = nullptr, *kB = nullptr, *vA = nullptr, *vB = nullptr, *cstart = nullptr, *toff = nullptr;
    unsigned long long *wA = nullptr, *wB = nullptr;      // 64-bit (topology, clade) keys, only when 32 bits do not hold them
    const uint32_t *cperm = nullptr, *tperm = nullptr;    // entries sorted by clade row / by (topology row, clade row)
    double *o_cs = nullptr, *o_ls = nullptr, *o_ts = nullptr;   // [n_clades][4], [G][N][4], [n_topologies][2N-2][4]
    int32_t* o_tc = nullptr;                 // [n_topologies][N-2] clade rows (over all groups; the fetch subtracts the group's first)
    unsigned char* temp = nullptr;
};

// One thread per final particle k: the branch above each child of the node of every rank event of its tree.  slot was validated
// by pt_walk; a record that does not fit is still refused here (PT_ERR_TREE in the word given) before anything is indexed by it.
__global__ void __launch_bounds__(PT_NT) pb_walk(const int32_t* __restrict__ child, const int32_t* __restrict__ slot,
                                                 const double* __restrict__ bl, const double* __restrict__ br, int N, int K,
                                                 double* __restrict__ ebr, double* __restrict__ lbr, unsigned int* __restrict__ err) {
    const int k = blockIdx.x * PT_NT + threadIdx.x;
    if (k >= K) return;
    const int R = N - 1;
    const long long n_nodes = (long long)N + (long long)R * K;
    for (int r = R - 1; r >= 0; --r) {
        const int nd = slot[(size_t)r * K + k];
        const int kk = nd - N - r * K;
        if (nd < 0 || kk < 0 || kk >= K) { atomicOr(err, (unsigned int)PT_ERR_TREE); return; }
        const size_t rec = (size_t)r * K + kk;
        for (int s = 0; s < 2; ++s) {
            const int c = child[rec * 2 + s];
            const double b = s ? br[rec] : bl[rec];
            if (c < 0 || c >= n_nodes) { atomicOr(err, (unsigned int)PT_ERR_TREE); return; }
            if (c < N) lbr[(size_t)c * K + k] = b;
            else {
                const int rc = (c - N) / K;
                if (rc >= r) { atomicOr(err, (unsigned int)PT_ERR_TREE); return; }
                ebr[(size_t)rc * K + k] = b;
            }
        }
    }
}

// keys of the two entry sorts, values = the entry.  topo == nullptr: element i is entry i, key = its clade's output row (stable
// over ascending entries: the contract's order inside a clade segment).  Otherwise element i = k L + r is entry r K + k, key =
// (topology row of k) << cbits | clade row: stable over ascending particles, and topology t's rows come out as N - 2 runs of
// n(t) entries each.  KEY is uint32_t whenever the key fits.
template <typename KEY>
__global__ void pb_entry_keys(const uint32_t* __restrict__ cid, const uint32_t* __restrict__ cpos, const int32_t* __restrict__ topo,
                              long long E, int K, int L, int cbits, KEY* __restrict__ key, uint32_t* __restrict__ val) {
    const long long i = (long long)blockIdx.x * PT_NT + threadIdx.x;
    if (i >= E) return;
    uint32_t e = (uint32_t)i;
    KEY x = 0;
    if (topo) {
        const uint32_t k = (uint32_t)(i / L), r = (uint32_t)(i % L);
        e = r * (uint32_t)K + k;
        x = (KEY)((KEY)(uint32_t)topo[k] << cbits);
    }
    key[i] = x | (KEY)cpos[cid[e]];
    val[i] = e;
}

// first element of every clade row in the entries sorted by row (every row holds at least one entry); cstart[n_rows] = E
__global__ void pb_clade_starts(const uint32_t* __restrict__ key, long long E, uint32_t n_rows, uint32_t* __restrict__ cstart) {
    const long long i = (long long)blockIdx.x * PT_NT + threadIdx.x;
    if (i >= E) return;
    const uint32_t row = key[i];
    if (row < n_rows && (i == 0 || key[i - 1] != row)) cstart[row] = (uint32_t)i;
    if (i == 0) cstart[n_rows] = (uint32_t)E;
}

struct pb_seg_args {
    const unsigned long long* u;      // [K]
    const double *ebr, *lbr;
    const uint32_t *cperm, *cstart;   // clade rows
    const uint32_t *tperm, *toff;     // topology rows: toff[t] = particles in the rows before t
    const int32_t* tn;                // [n_topologies] particle counts
    double* out;                      // [n_seg][4]
    int32_t* o_tc;
    long long n_seg;
    int N, K, Kg, cmask_bits;
};

enum { PB_CLADES = 0, PB_LEAVES = 1, PB_TOPOS = 2 };

template <typename KEY>
__device__ __forceinline__ uint32_t pb_low(const KEY* key, size_t i, int bits) {
    return (uint32_t)(key[i] & (((KEY)1 << bits) - 1));
}

// One wavefront per segment, PT_NT / 64 segments per workgroup (the segments of a family are numbered densely, so short ones
// pack four to a workgroup and a long one keeps one wave busy while the others retire).  S1, S2, min, max in one pass.
template <int FAMILY, typename KEY>
__global__ void __launch_bounds__(PT_NT) pb_seg_sums(pb_seg_args a, const KEY* __restrict__ tkey) {
    const long long seg = (long long)blockIdx.x * (PT_NT / 64) + (threadIdx.x >> 6);   // wave-uniform
    if (seg >= a.n_seg) return;
    const uint32_t lane = threadIdx.x & 63;
    const int N = a.N, K = a.K, L = N - 2;
    const uint32_t* list = nullptr;        // the segment's elements: entries (e % K = particle), or nullptr: particles base + j
    const double* leaf = nullptr;          // the leaf's row of lbr, or nullptr: the branch above the entry
    uint32_t len, base = 0;
    if (FAMILY == PB_CLADES) {
        const uint32_t b = a.cstart[seg];
        len = a.cstart[seg + 1] - b;
        list = a.cperm + b;
    } else if (FAMILY == PB_LEAVES) {
        const int g = (int)(seg / N), i = (int)(seg % N);
        len = (uint32_t)a.Kg;
        base = (uint32_t)g * (uint32_t)a.Kg;
        leaf = a.lbr + (size_t)i * K;
    } else {
        const int nb = 2 * N - 2, t = (int)(seg / nb), q = (int)(seg % nb);
        len = (uint32_t)a.tn[t];
        const size_t first = (size_t)L * a.toff[t];            // topology t's N - 2 runs of len entries start here
        if (q < N) {
            list = a.tperm + first;                            // (the first run names t's particles in ascending order)
            leaf = a.lbr + (size_t)q * K;
        } else {
            const size_t run = first + (size_t)(q - N) * len;
            list = a.tperm + run;
            if (lane == 0) a.o_tc[(size_t)t * L + (q - N)] = (int32_t)pb_low(tkey, run, a.cmask_bits);
        }
    }
    double s1 = 0.0, s2 = 0.0, mn = pm_inf(), mx = -pm_inf();
#pragma unroll 4
    for (uint32_t j = lane; j < len; j += 64) {
        uint32_t k = base + j;
        double b;
        if (list) {
            const uint32_t e = list[j];
            k = e % (uint32_t)K;
            b = leaf ? leaf[k] : a.ebr[e];
        } else b = leaf[k];
        const double x = (double)a.u[k] * b;
        const double y = x * b;
        s1 = s1 + x;
        s2 = s2 + y;
        mn = b < mn ? b : mn;
        mx = b > mx ? b : mx;
    }
    s1 = pk_wave_tree_sum(s1);
    s2 = pk_wave_tree_sum(s2);
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double on = __shfl_xor(mn, off, 64), ox = __shfl_xor(mx, off, 64);
        mn = on < mn ? on : mn;
        mx = ox > mx ? ox : mx;
    }
    if (lane == 0) {
        double* o = a.out + (size_t)seg * 4;
        o[0] = s1; o[1] = s2; o[2] = mn; o[3] = mx;
    }
}
