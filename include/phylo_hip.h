/* phylo_hip.h -- C ABI of libphylo_hip.so: the MI355X-native Felsenstein-pruning likelihood and
 * CSMC particle loop of amoretti86/phylo (vcsmc.py / csmc.py), behind plain pointers and sizes.
 *
 * The reference has no FFI of its own: the path sits behind Python methods.  Each
 * entry point below names the reference method it stands in for (file:line into the reference);
 * the Python classes in phylo_amd/ (VCSMC, CSMC) keep the reference's names and argument meaning and
 * call these through ctypes (INTEGRATION.md shows the binding).
 *
 * Conventions
 *   - every function returns 0 on success, a negative PHYLO_E* code on failure; the message is
 *     available from phylo_last_error(ctx) (ctx may be NULL for failures of phylo_create);
 *   - the caller owns every host buffer (C-contiguous; double = IEEE binary64, int32/int64 as named);
 *     the library never keeps a host pointer past return;
 *   - the library owns all device memory and releases it in phylo_destroy;
 *   - a ctx is bound to ONE GPU and is not thread-safe; distinct ctxs are independent.  Multi-GPU =
 *     one process (rank) per GPU, joined by phylo_comm_init (RCCL over xGMI);
 *   - calls are synchronous at the boundary unless the name ends in _async;
 *   - no global RNG state: every stochastic entry point takes (seed, step) and follows the
 *     counter-based contract in DESIGN.md (Philox4x32-10).
 *   - there is no CPU fallback: without a usable HIP device every compute entry point fails with
 *     PHYLO_ENODEVICE.
 */
#ifndef PHYLO_HIP_H
#define PHYLO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phylo_ctx phylo_ctx;

enum {
    PHYLO_OK = 0,
    PHYLO_EINVAL = -1,    /* bad argument (shape, NULL pointer, state not set) */
    PHYLO_ENODEVICE = -2, /* no HIP device / device id out of range */
    PHYLO_EHIP = -3,      /* a HIP runtime call failed */
    PHYLO_ENOMEM = -4,    /* device allocation failed */
    PHYLO_ECOMM = -5,     /* RCCL / multi-rank failure */
    PHYLO_ESTATE = -6     /* call order (e.g. sweep before set_leaves/set_model) */
};

/* sweep / model flags */
enum {
    PHYLO_QUIRK_Q1_RAW_Q = 1u << 0,    /* weight subtracts q = 1/C(n,2) itself, not log q (vcsmc.py:298,392).
                                          Set = as the reference.  */
    PHYLO_TWISTING = 1u << 1,          /* twisted/nested proposal of vncsmc.py:295-416 (uses M)          */
    PHYLO_TIME_KERNELS = 1u << 2,      /* bracket the dominant launch of every rank event with HIP events: the merge, or the
                                          look-ahead potentials of a twisted sweep (profiling runs; phylo_stats.merge_ms) */
    PHYLO_EAGER_NODES = 1u << 3,       /* always store every new node's partial likelihoods.  Default with the plain
                                          proposal (one GPU: always; sharded: S >= 8192): only nodes whose creator
                                          survives the next resampling are written (the rest are dead stores);
                                          results are identical either way.
                                          The nodes of the LAST rank event are never read by a merge and are not stored
                                          either (phylo_sweep_node writes them on demand) unless this flag is set */
    PHYLO_KEEP_GRAPH = 1u << 4,        /* keep what phylo_sweep_backward needs (root-table history of every rank
                                          event, every node; with PHYLO_TWISTING also every sub-sample's branch lengths,
                                          transition matrices and potential).  On a sharded context: the plain proposal
                                          with S <= 4096 only (PHYLO_EINVAL otherwise); the sweep then advances all K root
                                          tables on every rank and ends with an exchange that makes the kept graph whole on
                                          every rank.  Nodes are stored eagerly with
                                          PHYLO_TWISTING or more than 4096 sites; otherwise they stay lazy (the reverse pass then
                                          reads no node but the adopted ones) */
    PHYLO_ONE_LAUNCH = 1u << 5,        /* run the whole sweep as ONE launch of resident workgroups (phylo_persist.h) where that
                                          form applies (phylo_sweep_async / phylo_sweep_batch_async on one GPU, plain proposal,
                                          N <= 32, small nodes) instead of launches per rank event (scan, bookkeeping,
                                          materialise, merge).  Same bits either way; PHYLO_ONE_LAUNCH=1 in the environment of
                                          phylo_create sets it for every sweep of the context.  */
    PHYLO_FLAGS_DEFAULT = PHYLO_QUIRK_Q1_RAW_Q
};

typedef struct phylo_stats {
    double sweep_ms;        /* device time of the whole sweep (hipEvents on the ctx stream)            */
    double merge_ms;        /* sum of the launch durations of the rank events' dominant kernel (only with PHYLO_TIME_KERNELS):
                               the merge, or pk_twist_potentials for a twisted sweep.  From phylo_sweep_backward: the
                               host time spent building the integer lists                                  */
    int32_t merge_launches; /* number of launches in that sum                                          */
    int32_t n_launches;     /* kernel launches in the sweep                                            */
    double units;           /* particle-site-likelihoods computed by this rank: K_local * S * (N-1)    */
    double alg_bytes;       /* 96 B * units (two child reads + one parent write, fp64 x 4 states)      */
} phylo_stats;

const char* phylo_version(void);
const char* phylo_last_error(const phylo_ctx* ctx);

/* Number of visible HIP devices (0 if none / no driver).  Does not create a context. */
int phylo_device_count(void);

/* VCSMC.__init__ + the sizes of sample_phylogenies (vcsmc.py:110-118, 406-426): K particles (global
 * count), N taxa, S sites, A = 4 states.  device_ids/n_gpus: this build runs one GPU per process, so
 * n_gpus must be 1; more GPUs join through phylo_comm_init. */
int phylo_create(const int* device_ids, int n_gpus, int K, int N, int S, int A, uint32_t flags,
                 phylo_ctx** out);
int phylo_destroy(phylo_ctx* ctx);

/* The arithmetic contract's site tile (contract v5): sum_s log(pi . x[s]) of compute_forest_posterior
 * (vcsmc.py:240-242) is taken tile by tile -- T sites per tile, 64 log-product columns inside a tile, tile values added left to
 * right -- so that one wavefront owns a (row, tile).  phylo_site_tile(S) is the default T for rows of S sites (the CPU oracle
 * uses the same value); phylo_set_site_tile overrides it for this context (T a multiple of 64 in [64, 4096]; 0 = the default),
 * which changes results in the last bits only and drops the sweep state and its tree summary (call it before the first sweep; PHYLO_ESTATE once a
 * communicator is set).  PHYLO_SITE_TILE=T in the environment of phylo_create does the same.  phylo_get_site_tile returns the
 * context's T. */
int phylo_site_tile(int S);
int phylo_set_site_tile(phylo_ctx* ctx, int T);
int phylo_get_site_tile(const phylo_ctx* ctx);

/* datadict['genome'] [N,S,4] float64 (runner.py:107-115); stored once, not K-replicated
 * (the reference replicates it K-fold at vcsmc.py:479).  Returns when the caller's buffer has been read (small alignments are
 * staged in pinned memory and go up behind the call, ordered before every later call on the context). */
int phylo_set_leaves(phylo_ctx* ctx, const double* genome_NxSxA);

/* Model of VCSMC.__init__ / get_Q / get_stationary_probs (vcsmc.py:119-148), already evaluated by the
 * host: Q row-major 4x4, pi[4], lam_l / lam_r = exp(branch params) [N-1].  jc69_closed_form != 0 uses
 * P_ii = 1/4 + 3/4 e^-t for the JC69 Q instead of the generic Pade expm.  Returns when the 42 numbers are staged;
 * the upload is ordered before every later call on the context. */
int phylo_set_model(phylo_ctx* ctx, const double* Q16, const double* pi4, const double* lam_l,
                    const double* lam_r, int jc69_closed_form);

/* tf.linalg.expm(tensordot(t, Q, 0)) (vcsmc.py:181-184): P[i] = expm(Q * t[i]), [n,4,4].
 * The domain of the matrix function: ||Q||_1 * |t| <= theta_13 * 2^23 = 4.50629e7, Q the model in force.
 * Inside it every entry is within 2^s (8 * 116 + 4) * 2^-53 of the true value, relatively (s squarings; <= 2^-20 at s = 23), no
 * entry is negative and t = +-0 gives the identity; beyond it the squarings lose every digit (a zero matrix from about 1e100
 * on).  A length outside it -- NaN and +-inf included -- is PHYLO_EINVAL naming t[i], the length and the limit, before anything is
 * queued.  The same limit holds for every length (every rate * length) of phylo_tree_loglik and of all phylo_trees_* calls, whose
 * message names tree and row (and category).  Under jc69_closed_form there is no limit: the closed form is right at every length
 * (1/4 everywhere at 1e100), exact in absolute terms (off-diagonal within 0.5 * 2^-53, diagonal within 2 * 2^-53), not in
 * relative ones (off-diagonal within 4 * 2^-53 / min(t, 1) of itself; exactly 0 for t < 2^-54). */
int phylo_expm_batched(phylo_ctx* ctx, const double* t, int n, double* P_nx4x4);

/* VCSMC.broadcast_conditional_likelihood_K (vcsmc.py:180-188) == csmc.conditional_likelihood per
 * particle (csmc.py:300-309): out[k,s,:] = (l[k,s,:] @ P(tl[k])) * (r[k,s,:] @ P(tr[k])). */
int phylo_cond_likelihood_K(phylo_ctx* ctx, const double* l_KxSx4, const double* r_KxSx4,
                            const double* tl_K, const double* tr_K, int K, int S, double* out_KxSx4);

/* VCSMC.compute_forest_posterior (vcsmc.py:231-245): out[k] = sum_x sum_s log(pi . core[k,x,s,:])
 *   - sum_x log (2 max(record[k,x], 2) - 3)!! */
int phylo_forest_loglik(phylo_ctx* ctx, const double* core_KxXxSx4, const int32_t* record_KxX, int K,
                        int X, int S, double* out_K);

/* CSMC.compute_log_conditional_likelihood (csmc.py:318-326) on an explicit binary tree.  Nodes
 * 0..n_leaves-1 are leaves (rows of leaves_LxSx4); node i >= n_leaves has children left[i], right[i]
 * (already-numbered nodes < i or leaves) with branch lengths bl[i], br[i].  prior4 is csmc's
 * `self.prior`.  out_loglik = sum_s log(prior . data_root[s]); root_data_Sx4 may be NULL.  A branch length of a node reachable
 * from root that lies outside the domain of the matrix function (phylo_expm_batched; NaN and inf included) is PHYLO_EINVAL,
 * "tree 0, row <node>: ...", before anything is queued; no limit under jc69_closed_form. */
int phylo_tree_loglik(phylo_ctx* ctx, int n_nodes, int n_leaves, int S, const int32_t* left,
                      const int32_t* right, const double* bl, const double* br, int root,
                      const double* leaves_LxSx4, const double* prior4, double* out_loglik,
                      double* root_data_Sx4);

/* The log-likelihood of T explicit rooted binary trees over the context's N taxa under the context's model (Q and
 * jc69_closed_form of phylo_set_model) and the context's RESIDENT leaves (phylo_set_leaves; nothing is uploaded again) -- what
 * phylo_tree_loglik computes for one tree, in volume.  Numbering: leaves are nodes 0 .. N-1; row i of a
 * tree is internal node N + i with children child[t][i][0], child[t][i][1] (a leaf or a node of an earlier row) and branch
 * lengths blen[t][i][0], blen[t][i][1]; row N-2 is the root.  Every tree is checked on the host before anything is queued: each
 * leaf and each internal node but the root is a child exactly once, branch lengths are finite and >= 0 and, unless the model is
 * the JC69 closed form, inside the domain of the matrix function (phylo_expm_batched: ||Q||_1 * length <= 4.50629e7) (PHYLO_EINVAL
 * naming tree and row); PHYLO_ESTATE before leaves and model are set; T >= 1.
 *   loglik_T[t] = sum_s log(prior . x_root[s]) by the arithmetic contract with the context's site tile: bit for bit what
 *     phylo_tree_loglik returns for the same tree, leaves, prior and site tile.  prior4 == NULL: the context's pi;
 *   site_lik_TxS[t][s] (may be NULL): the factor prior . x_root[s] that entered the product;
 *   perf (may be NULL): sweep_ms = device time (hipEvents), n_launches, units = T S (N-1).
 * Synchronous.  On a sharded context a LOCAL call (every rank holds all leaves), not a collective.  Large T runs in chunks: device
 * scratch is bounded by 64 MiB (PHYLO_TREES_CHUNK=n in the environment of phylo_create: at most n trees per chunk), not by T.
 * The sweep's state, a kept graph and a tree summary are left alone. */
int phylo_trees_loglik(phylo_ctx* ctx, int T, const int32_t* child, const double* blen, const double* prior4, double* loglik_T,
                       double* site_lik_TxS, phylo_stats* perf);
/* phylo_trees_loglik under among-site rate variation: a mixture of C rate categories (rate_C[c],
 * weight_C[c]), 1 <= C <= 16 -- discrete Gamma, +I as a category of rate 0 (expm(0) is the identity), or any other.  Bit level:
 *   the category-c branch lengths are rate_C[c] * blen (one IEEE double multiply, on the host), so the factor f_c[t][s] =
 *     prior . x_root[s] of category c is bit for bit site_lik of phylo_trees_loglik on (child, rate_C[c] * blen);
 *   the site value m = weight_C[0] * f_0, then m = fma(weight_C[c], f_c, m) for c = 1 .. C-1 in ascending order;
 *   loglik_T[t] = sum_s log m[t][s] exactly as phylo_trees_loglik sums log(prior . x_root[s]) (same site tile).
 * The weights are the caller's: finite and >= 0, NOT normalised here (phylo_amd/rates.py builds normalised ones).
 *   site_lik_TxS[t][s] (may be NULL) = m;  cat_lik_TxCxS[t][c][s] (may be NULL) = f_c;
 *   perf (may be NULL): as phylo_trees_loglik, units = T S (N-1) C.
 * State rules, per-tree checks, chunking (the same 64 MiB slab, PHYLO_TREES_CHUNK) and what is left alone are
 * phylo_trees_loglik's; a tree's schedule is built once, not once per category.  PHYLO_EINVAL before anything is queued also for
 * C outside 1 .. 16, a rate or weight that is not finite and >= 0, and a scaled length rate_C[c] * blen that is not finite or lies
 * outside the domain of the matrix function (phylo_expm_batched; the message names tree, row and category).  The other
 * phylo_trees_*_rates calls hold every rate * length to the same limit. */
int phylo_trees_loglik_rates(phylo_ctx* ctx, int T, const int32_t* child, const double* blen, int C, const double* rate_C,
                             const double* weight_C, const double* prior4, double* loglik_T, double* site_lik_TxS,
                             double* cat_lik_TxCxS, phylo_stats* perf);
/* The derivatives of phylo_trees_loglik's log-likelihood with respect to every branch length: for T trees
 * given as phylo_trees_loglik takes them (same numbering, same checks, same state rules),
 *   loglik_T[t]      bit for bit phylo_trees_loglik's value for the same tree, prior and site tile;
 *   grad[t][i][side] = d loglik_T[t] / d blen[t][i][side] = sum_s L'_s / L_s;
 *   curv[t][i][side] (may be NULL) = d^2 loglik_T[t] / d blen[t][i][side]^2 = sum_s (L''_s / L_s - (L'_s / L_s)^2),
 * both shaped [T][N-1][2] as blen.  The sums run in a fixed order (64 sites by the wave's adjacent-pair tree, the steps of a
 * site tile in ascending order, the tiles left to right; no atomics): a call repeats its own bits, and chunking changes none.
 * Against a restatement the derivatives carry a tolerance, not a bit contract.  A tree whose loglik is not finite gets NaN in
 * every derivative entry, and so does a tree with any site factor L_s below 2^-1020 (partials are not rescaled; 1 / L_s is no
 * double there), whose loglik_T stays what phylo_trees_loglik gives.  perf (may be NULL): sweep_ms = device time, n_launches, units = T S (N-1).
 * Synchronous; on a sharded context a LOCAL call.  PHYLO_EINVAL before anything is queued for a bad tree (naming tree and row) and
 * for child, blen, loglik_T or grad == NULL.  Large T runs in chunks (64 MiB; PHYLO_TREES_CHUNK caps the trees of a chunk); the
 * node stores of the resident workgroups take at most 256 MiB more.  Own scratch and events, released with the context: the
 * sweep's state, a pending phylo_sweep_backward, a tree summary and the scratch of phylo_trees_loglik and phylo_rell are left alone. */
int phylo_trees_grad(phylo_ctx* ctx, int T, const int32_t* child, const double* blen, const double* prior4, double* loglik_T,
                     double* grad, double* curv, phylo_stats* perf);
/* phylo_trees_grad under a mixture of C rate categories: the derivatives of phylo_trees_loglik_rates'
 * MIXTURE log-likelihood.  rate and weight are [C] with per_tree == 0 (one mixture for all trees) and [T][C] with per_tree == 1
 * (tree t under its own row), 1 <= C <= 16.  With r = rate[t][c], w = weight[t][c], f_c the factor of category c, m = the site
 * value of phylo_trees_loglik_rates, D1_c (D2_c) the L' (L'') of phylo_trees_grad inside category c (a derivative with respect to
 * the SCALED length r * blen), u_c = w r, v_c = u_c r, a1 = sum_c u_c D1_c and a2 = sum_c v_c D2_c (c ascending from +0.0):
 *   loglik_T[t]      bit for bit phylo_trees_loglik_rates' value for that tree under that tree's mixture (same prior and tile);
 *   grad[t][i][side] = sum_s a1 / m;   curv[t][i][side] (may be NULL) = sum_s (a2 / m - (a1 / m)^2);
 *   drate_TxC[t][c]  (may be NULL) = sum_s sum_b blen_b w D1_{c,b} / m, d loglik / d rate[t][c] at fixed blen;
 *   dweight_TxC[t][c] (may be NULL) = sum_s f_c / m.
 * A rate-0 category, a zero weight and a site with some f_c == 0 are ordinary.  Fixed order of summation, no atomics: a call
 * repeats its own bits; chunking, the grid cap, a tree's place, shared against per-tree passing of the same numbers and the
 * optional outputs change none of grad's.  NaN rule: phylo_trees_grad's, on m.  perf: units = T S (N-1) C.
 * Synchronous; a LOCAL call on a sharded context; state rules, per-tree checks and chunking as phylo_trees_loglik_rates.
 * PHYLO_EINVAL before anything is queued for a bad tree, C outside 1 .. 16, a bad rate, weight or scaled length (the message names
 * tree, row and category), per_tree outside {0, 1}, and for child, blen, rate, weight, loglik_T or grad == NULL.  Own scratch and
 * events, released with the context; everything phylo_trees_grad leaves alone, and phylo_trees_grad's own scratch, is left alone. */
int phylo_trees_grad_rates(phylo_ctx* ctx, int T, const int32_t* child, const double* blen, int C, const double* rate,
                           const double* weight, int per_tree, const double* prior4, double* loglik_T, double* grad, double* curv,
                           double* drate_TxC, double* dweight_TxC, phylo_stats* perf);
/* The derivatives of phylo_trees_loglik's log-likelihood with respect to the substitution model: along P
 * directions in the space of generators (dirs_Px16, row-major 4 x 4 each, 1 <= P <= 16, every entry finite) and with respect to the
 * root distribution.  Trees, prior, state rules and per-tree checks as phylo_trees_grad; one rate only.  With Q_eff the context's Q
 * (under jc69_closed_form the generator 1/4, diagonal -3/4), t_b a branch's length and D_{p,b} = L(Q_eff t_b, dirs[p] t_b) the
 * Frechet derivative of expm (one multiply per entry of either argument; D indexed like the branch's matrix; a zero length gives 0):
 *   loglik_T[t]      bit for bit phylo_trees_loglik's value for the same tree, prior and site tile;
 *   grad[t][i][side] (may be NULL) bit for bit phylo_trees_grad's grad;
 *   dtheta_TxP[t][p] = sum_s sum_b (x_child . D_{p,b} . g_b) / L_s, the derivative of loglik_T[t] along dirs[p] at fixed lengths
 *                      and prior (x_child, g_b and the order of the product as in phylo_trees_grad's L'_s, D in the place of M');
 *   dprior_Tx4[t][j] (may be NULL) = sum_s x_root[s][j] / L_s, the partial derivative with respect to prior[j] at fixed Q.
 * Fixed order of summation, no atomics: per lane and direction the terms of every operation (last to first), side and site step
 * from +0.0, the 64 lanes by the wave's adjacent-pair tree once per (tree, tile), the tiles left to right.  A call repeats its own
 * bits; chunking, the grid cap, a tree's place, the optional outputs and P itself (which other directions ride along) change
 * none.  Against a restatement dtheta and dprior carry a tolerance, not a bit contract.  NaN rule: phylo_trees_grad's, on every
 * entry of grad, dtheta and dprior of the tree.  perf (may be NULL): units = T S (N-1) (1 + P).
 * Synchronous; a LOCAL call on a sharded context.  PHYLO_EINVAL before anything is queued for a bad tree, P outside 1 .. 16, a
 * direction entry that is not finite, and for child, blen, dirs, loglik_T or dtheta == NULL.  Own scratch and events, released
 * with the context; everything phylo_trees_grad leaves alone, and the scratch of its siblings, is left alone. */
int phylo_trees_grad_model(phylo_ctx* ctx, int T, const int32_t* child, const double* blen, int P, const double* dirs_Px16,
                           const double* prior4, double* loglik_T, double* grad, double* dtheta_TxP, double* dprior_Tx4,
                           phylo_stats* perf);
/* Marginal ancestral state posteriors of a scored tree set: which state sat at every internal node at
 * every site, and how sure we are.  T trees given as phylo_trees_grad takes them (same numbering, checks, state rules, prior4 ==
 * NULL).  R = N - 1; row i of the outputs is internal node N + i of the caller's tree, row N - 2 the root.  With x_v = msg_l * msg_r
 * (the upward pass's bits), abar_v the outer partial of section 13 (the prior at the root) and inv = 1 / L_s:
 *   post_TxRxSx4[t][i][s][j] (may be NULL) = (abar_v[j] * x_v[j]) * inv, three IEEE operations each rounded on its own, NOT renormalised;
 *   state_TxRxS[t][i][s]     (may be NULL) = the lowest j whose post is the largest of the four; PHYLO_ANC_NOSTATE if any is NaN;
 *   pmax_TxRxS[t][i][s]      (may be NULL) = post[state], or NaN where there is no state;
 *   loglik_T[t]              bit for bit phylo_trees_loglik's value (required).
 * Not all three of post, state and pmax may be NULL.  NaN rule, per SITE: a site whose L_s lies below 2^-1020 or is not finite
 * gets NaN / PHYLO_ANC_NOSTATE in its own column at every node; every other site of the tree is untouched and loglik_T stays the
 * scoring call's bits.  No sum over sites: the call repeats its own bits, and chunking, the grid cap, a tree's place in the set
 * and which outputs are asked for change none.  perf (may be NULL): sweep_ms = device time, n_launches, units = T S (N-1).
 * Synchronous; on a sharded context a LOCAL call.  PHYLO_EINVAL before anything is queued for a bad tree (naming tree and row),
 * for child, blen or loglik_T == NULL, for all three outputs NULL, and for a single tree whose requested outputs exceed 1 GiB
 * (naming the size).  A chunk is the smallest of: the trees that fit phylo_trees_grad's 64 MiB slab, the trees whose requested
 * outputs (R S (32 + 1 + 8) bytes each, over those asked for) fit a 256 MiB staging region (which grows to one tree's need), and
 * PHYLO_TREES_CHUNK.  Own scratch and events, released with the context; everything phylo_trees_grad leaves alone, and the
 * scratch of its siblings, is left alone. */
#define PHYLO_ANC_NOSTATE 255
int phylo_trees_ancestral(phylo_ctx* ctx, int T, const int32_t* child, const double* blen, const double* prior4, double* loglik_T,
                          double* post_TxRxSx4, uint8_t* state_TxRxS, double* pmax_TxRxS, phylo_stats* perf);
/* phylo_trees_ancestral under a mixture of C rate categories, and the site-rate posteriors beside it.
 * Trees, numbering, per-tree checks, state rules and prior4 == NULL as phylo_trees_grad_rates; rate, weight [C] (per_tree == 0) or
 * [T][C] (per_tree == 1), 1 <= C <= 16, checked as phylo_trees_grad_rates checks them.  Category c of tree t is the tree (child,
 * rate[t][c] blen), one multiply per length on the host.  R = N - 1; rows as phylo_trees_ancestral (row i is node N + i, row N - 2
 * the root).  Inside category c everything is phylo_trees_ancestral's under that category's matrices: x_{v,c} = msg_l * msg_r, the
 * outer partial abar_{v,c} (the prior at the root), f_c = prior . x_root,c.  m_s = w_0 f_0, then fma(w_c, f_c, m) in ascending c
 * (phylo_trees_loglik_rates' site value); inv = 1 / m_s if m_s >= 2^-1020 and finite, else NaN.  Every line one IEEE operation:
 *   loglik_T[t]               bit for bit phylo_trees_loglik_rates' value under that tree's mixture, prior and tile (required);
 *   post_TxRxSx4[t][i][s][j]  (may be NULL) = acc_j * inv with acc_j = +0.0, then acc_j = acc_j + w_c * (abar_{v,c}[j] *
 *                             (msg_l,c[j] * msg_r,c[j])) in ascending c; NOT renormalised;
 *   state_TxRxS, pmax_TxRxS   (may be NULL) phylo_trees_ancestral's rule read from those post bits (PHYLO_ANC_NOSTATE, NaN);
 *   catpost_TxCxS[t][c][s]    (may be NULL) = (w_c * f_c) * inv, the posterior probability that site s evolved in category c
 *                             (f_c bit for bit phylo_trees_loglik_rates' cat_lik);
 *   siterate_TxS[t][s]        (may be NULL) = e with e = +0.0, then e = e + r_c * catpost_c in ascending c: the posterior mean rate.
 * Not all five of them may be NULL.  NaN rule, per SITE: a site whose m_s lies below 2^-1020 or is not finite gets NaN /
 * PHYLO_ANC_NOSTATE in its own column of all five outputs; every other site of the tree is untouched and loglik_T stays the
 * scoring call's bits.  A rate-0 category, a zero weight and a site with some f_c == 0 beside an in-range m_s are ordinary.  No
 * output sums over sites: the call repeats its own bits, and chunking, the grid cap, a tree's place in the set, shared against
 * per-tree passing of the same numbers and which outputs are asked for change none.  perf (may be NULL): units = T S (N-1) C.
 * Synchronous; on a sharded context a LOCAL call.  PHYLO_EINVAL before anything is queued for a bad tree (naming tree and row), C
 * outside 1 .. 16, a bad rate, weight or scaled length (naming tree, row and category), per_tree outside {0, 1}, T < 1, child,
 * blen, rate, weight or loglik_T == NULL, all five outputs NULL, and a single tree whose requested outputs exceed 1 GiB (naming
 * the size); PHYLO_ESTATE before phylo_set_leaves and phylo_set_model.  A chunk is the smallest of: the trees that fit
 * phylo_trees_grad_rates' 64 MiB slab (without M' and M''), the trees whose requested outputs (R S (32 + 1 + 8) + S (8 C + 8) bytes
 * each, over those asked for) fit phylo_trees_ancestral's 256 MiB staging region (which grows to one tree's need), and
 * PHYLO_TREES_CHUNK.  Own scratch and events, released with the context; everything phylo_trees_ancestral leaves alone, and the
 * scratch of every sibling, is left alone. */
int phylo_trees_ancestral_rates(phylo_ctx* ctx, int T, const int32_t* child, const double* blen, int C, const double* rate,
                                const double* weight, int per_tree, const double* prior4, double* loglik_T, double* post_TxRxSx4,
                                uint8_t* state_TxRxS, double* pmax_TxRxS, double* catpost_TxCxS, double* siterate_TxS,
                                phylo_stats* perf);
/* The NNI neighbourhood of every tree of a set, at the tree's current branch lengths: for T trees given as
 * phylo_trees_loglik takes them (same numbering, same checks, same state rules),
 *   loglik_T[t]        bit for bit phylo_trees_loglik's value for the same tree, prior and site tile;
 *   delta[t][i][side]  = sum_s log(L'_s / L_s), L'_s the site factor of one nearest-neighbour interchange, shaped [T][N-1][2] as blen:
 *     row i < N-2 (node v = N + i, parent p, sibling c): v's child on `side` and c change places, every subtree keeping its own
 *       length -- v = (v's other child, c), p = (v, that child); with p the root the move only shifts the root along its edge;
 *     row N-2 (the root, children v = child[N-2][0] and c = child[N-2][1], both internal): v's side-1 child and c's child on `side`
 *       change places -- the two interchanges across the root's edge; NaN in both entries when v or c is a leaf.
 * The neighbour's log-likelihood at the current lengths is loglik_T[t] + delta.  An impossible neighbour (L'_s = 0 at a site)
 * gets -inf.  Fixed order of summation, no atomics: a call repeats its own bits, and chunking changes none; against a
 * restatement delta carries a tolerance, not a bit contract.  A tree whose loglik is not finite, or with a site factor below
 * 2^-1020, gets NaN in every entry (phylo_trees_grad's rule).  perf (may be NULL): sweep_ms = device time, n_launches, units =
 * T S (N-1).  Synchronous; on a sharded context a LOCAL call.  PHYLO_EINVAL before anything is queued for a bad tree (naming tree and
 * row), T < 1, and for child, blen, loglik_T or delta == NULL; PHYLO_ESTATE before phylo_set_leaves and phylo_set_model.  Chunks
 * and node stores as phylo_trees_grad (PHYLO_TREES_CHUNK).  Own scratch and events, released with the context: the sweep's state
 * and the scratch of phylo_trees_loglik, phylo_rell, phylo_trees_grad and phylo_trees_grad_rates are left alone. */
int phylo_trees_nni(phylo_ctx* ctx, int T, const int32_t* child, const double* blen, const double* prior4, double* loglik_T,
                    double* delta, phylo_stats* perf);
/* phylo_trees_nni under a mixture of C rate categories: trees, numbering, checks, prior, state rules, moves,
 * rows, sides and the NaN of a missing root move as phylo_trees_nni; rate, weight [C] (per_tree == 0) or [T][C] (per_tree == 1),
 * 1 <= C <= 16, checked as phylo_trees_grad_rates checks them.  Category c of tree t is the tree (child, rate[t][c] blen), one
 * multiply per length on the host; inside it everything is phylo_trees_nni's under that category's matrices, giving the tree's
 * factor f_c and every neighbour's f'_c per site.  m_s = w_0 f_0, then fma(w_c, f_c, m) in ascending c (phylo_trees_loglik_rates'
 * value); m'_s the same chain over f'_c;
 *   loglik_T[t]        bit for bit phylo_trees_loglik_rates' value for that tree under that tree's mixture (same prior and tile);
 *   delta[t][i][side]  = sum_s log(m'_s (1 / m_s)), shaped [T][N-1][2].
 * The neighbour's mixture log-likelihood at the current lengths is loglik_T[t] + delta.  A neighbour with m'_s = 0 at a site gets
 * -inf; a single f'_c = 0 with m'_s > 0, a zero weight and a rate-0 category are ordinary.  A tree whose loglik is not finite, or
 * with an m_s below 2^-1020 or not finite, gets NaN in every entry.  Fixed order of summation, no atomics: a call repeats its own
 * bits; chunking, the grid cap, a tree's place and shared against per-tree passing of the same numbers change none; against a
 * restatement delta carries a tolerance.  perf (may be NULL): units = T S (N-1) C.  Synchronous; a LOCAL call on a sharded context.
 * PHYLO_EINVAL before anything is queued for a bad tree, C outside 1 .. 16, a bad rate, weight or scaled length (the message names
 * tree, row and category), per_tree outside {0, 1}, T < 1, a tree whose wave would need more than 64 KiB of LDS, and for child,
 * blen, rate, weight, loglik_T or delta == NULL; PHYLO_ESTATE before phylo_set_leaves and phylo_set_model.  Own scratch and events,
 * released with the context: the sweep's state and the scratch of every other tree-set call are left alone. */
int phylo_trees_nni_rates(phylo_ctx* ctx, int T, const int32_t* child, const double* blen, int C, const double* rate,
                          const double* weight, int per_tree, const double* prior4, double* loglik_T, double* delta, phylo_stats* perf);
/* Test hook, no GPU needed: the host half of phylo_trees_loglik on ONE tree -- the checks above (PHYLO_EINVAL, "tree 0, row i")
 * and the slot schedule the kernel walks: ops[N-1][4] = {destination slot, left source, right source, row}, a source >= 0 a
 * leaf, a source < 0 the slot ~source; depth = slots in use (<= floor(log2 N) + 1).  tests/test_trees_host.py replays it. */
int phylo_debug_tree_schedule(int N, const int32_t* child, const double* blen, int32_t* ops, int32_t* depth);

/* VCSMC.resample's index draw (vcsmc.py:284-285) / CSMC.resample (csmc.py:218-228): K iid draws from
 * softmax(logw), by the integer-CDF contract.  idx_K[k] in [0,K). */
int phylo_resample(phylo_ctx* ctx, const double* logw_K, int K, uint64_t seed, uint32_t step,
                   int64_t* idx_K);

/* VCSMC.compute_log_ZSMC (vcsmc.py:270-277): sum_r logsumexp_k(logw[r,k] - log K). */
int phylo_log_zsmc(phylo_ctx* ctx, const double* logw_RxK, int R, int K, double* out);

/* VCSMC.sample_phylogenies (vcsmc.py:406-451): the N-1 rank events, device-resident.  Any output
 * pointer may be NULL.  Shapes (K = this rank's particles when sharded, see phylo_comm_init):
 *   log_weights, log_lik, lbranch, rbranch : [(N-1), K]   (rows 1..N-1 of the reference's tensors)
 *   merges    : [(N-1), K, 2]  root-table slots (left, right) coalesced at each rank event
 *   ancestors : [(N-2), K]     resampling indices drawn before rank events 1..N-2 (global indices)
 *   logZ      : scalar; perf : timing of this sweep
 * M is the number of sub-samples of the twisted proposal (ignored without PHYLO_TWISTING; 1 <= M <= 1024,
 * C(N,2)*M <= 2^20 with it; beyond 8192 sub-samples per particle their weights leave LDS).  With PHYLO_TWISTING the weight subtracts the normalised log-potential of the
 * chosen (pair, sub-sample) (vncsmc.py:315-316,491) and merges[r,k] = (r1 < r2). */
int phylo_sweep(phylo_ctx* ctx, uint64_t seed, uint32_t flags, int M, double* log_weights,
                double* log_lik, double* lbranch, double* rbranch, int32_t* merges, int64_t* ancestors,
                double* logZ, phylo_stats* perf);

/* Same sweep, left on the device (no host copies); phylo_sweep_fetch copies the last sweep's outputs. */
int phylo_sweep_async(phylo_ctx* ctx, uint64_t seed, uint32_t flags, int M);
int phylo_sweep_fetch(phylo_ctx* ctx, double* log_weights, double* log_lik, double* lbranch,
                      double* rbranch, int32_t* merges, int64_t* ancestors, double* logZ,
                      phylo_stats* perf);
int phylo_synchronize(phylo_ctx* ctx);

/* G INDEPENDENT sweeps in one set of launches (throughput form for callers that need many sweeps: minibatches,
 * replicates): the context's K particles are G groups of K/G; group g is exactly the sweep of K/G particles with
 * seeds[g] (own draws, own resampling, own log Z-hat).  Outputs of phylo_sweep_fetch hold group g in columns
 * [g K/G, (g+1) K/G) (ancestors index inside the group); phylo_sweep_fetch_logz returns the G estimates.
 * Plain proposal.  With PHYLO_KEEP_GRAPH (G > 1): one GPU (unsharded context) and S <= 4096 sites -- the batch is then ONE
 * block-diagonal genealogy of K particles that phylo_sweep_backward_batch differentiates; the sweep's bits are those of the
 * batch without the flag (PHYLO_EINVAL names the failed condition: PHYLO_TWISTING, a sharded context, S > 4096).  Without the
 * flag, sharded contexts too: the K = G * (K/G) particle indices are sharded by contiguous ranges as
 * always (a group may straddle ranks), one all-gather per rank event carries all G sweeps.
 * phylo_sweep_batch_begin + phylo_sweep_step(_group) + phylo_sweep_finish is the stepwise form. */
int phylo_sweep_batch_async(phylo_ctx* ctx, const uint64_t* seeds, int G, uint32_t flags);
int phylo_sweep_batch_begin(phylo_ctx* ctx, const uint64_t* seeds, int G, uint32_t flags);
int phylo_sweep_fetch_logz(phylo_ctx* ctx, double* logZ_G, int G);

/* The same sweep issued one rank event at a time: begin (draws, tables), N-1 x step, finish (log Z-hat).
 * phylo_sweep_async is exactly begin + steps + finish.  A caller that keeps several sweeps in flight on sharded
 * contexts interleaves them rank event by rank event (A0 B0 C0 A1 B1 C1 ...), so that the collectives of the
 * shared communicator (phylo_comm_share) are issued in one order on every rank while the kernels of the other
 * sweeps run underneath them. */
int phylo_sweep_begin(phylo_ctx* ctx, uint64_t seed, uint32_t flags, int M);
int phylo_sweep_step(phylo_ctx* ctx);
/* First half of the next rank event on a sharded context with lazy nodes (marking the adopted nodes, the owner's
 * writes, the collective that orders them before the merges); a no-op otherwise.  phylo_sweep_step runs it itself
 * when the caller has not: a caller with several contexts in flight issues the first halves of all of them before
 * the second halves, so that no context's merge waits behind another context's all-gather. */
int phylo_sweep_step_a(phylo_ctx* ctx);
/* One rank event of n sweeps that are at the same rank event and share one communicator: the kernels of each on its
 * own stream, then ONE grouped all-gather for all of them, then each sweep's scan. */
int phylo_sweep_step_group(phylo_ctx** ctxs, int n);
int phylo_sweep_finish(phylo_ctx* ctx);

/* Partial-likelihood vector of the node created at rank event r by particle slot k in the last sweep,
 * [S,4] (test surface for the merge kernel inside the sweep).  After a lazy sweep the missing nodes are
 * written first; when sharded that step is a collective: every rank must make the call.
 * The stored matrices make the call independent of a later phylo_set_model; after phylo_set_leaves it is refused
 * (PHYLO_ESTATE) until the next sweep: the nodes not yet written would come from the new leaves under the old sweep's records. */
int phylo_sweep_node(phylo_ctx* ctx, int r, int k, double* out_Sx4);

/* Reverse pass of the last sweep (which must have run with PHYLO_KEEP_GRAPH): the gradient of log Z-hat with
 * respect to the raw model quantities, d_lam_l[N-1], d_lam_r[N-1], d_pi[4], d_Q[16] (row-major).
 * Replaces the TensorFlow autodiff behind optimizer.minimize(self.cost), vcsmc.py:488-491,534 (cost = -logZ):
 * resampling indices, pair picks and gather indices are constants, branch lengths are reparameterised samples
 * b = -log(U)/lambda (vcsmc.py:353-356), everything else is differentiated.  After a twisted sweep
 * (PHYLO_TWISTING | PHYLO_KEEP_GRAPH) that includes the look-ahead potentials of every (pair, sub-sample), whose normalised
 * value of the chosen one enters the weight (vncsmc.py:399-401, 491; no stop_gradient there).  With jc69_closed_form the Q and pi
 * outputs are still produced (the reference holds them constant; the host ignores them).
 * May be called right after phylo_sweep_async (before the fetch): it is then queued behind the sweep without a host round trip.
 * perf (may be NULL): sweep_ms = device time of the reverse pass, host step included; merge_ms = that host step (building the
 * integer lists of adopters and parents) alone; n_launches.
 * Sharded context (phylo_comm_init / phylo_comm_share): a collective call -- every rank makes it, in the same order, after the
 * same sweep -- that returns the gradient of the GLOBAL log Z-hat, the same bits on every rank (each rank runs the whole pass over
 * the genealogy its sweep gathered, reading node rows from their owners' pools, and ends with a barrier; integer lists by the host
 * builders, a launch per rank event).  Refused there: a sweep with
 * PHYLO_TWISTING | PHYLO_KEEP_GRAPH, batched sweeps with PHYLO_KEEP_GRAPH and more than 4096 sites (PHYLO_EINVAL, at the sweep); a backward without a
 * kept graph is PHYLO_ESTATE as on one GPU. */
int phylo_sweep_backward(phylo_ctx* ctx, double* d_lam_l, double* d_lam_r, double* d_pi, double* d_Q,
                         phylo_stats* perf);
/* The reverse pass of a batched sweep (phylo_sweep_batch_async / _begin ... _finish with PHYLO_KEEP_GRAPH): one set of launches
 * over the block-diagonal genealogy, G gradients out -- d_lam_l[G][N-1], d_lam_r[G][N-1], d_pi[G][4], d_Q[G][16]; row g is the
 * gradient of log Z-hat_g alone (no mean is taken).  May be queued right behind the sweep like phylo_sweep_backward.  G must
 * equal the last sweep's group count (PHYLO_EINVAL); without a kept graph PHYLO_ESTATE.  After a sweep of one group (G = 1, or
 * phylo_sweep_async) it returns phylo_sweep_backward's bits; phylo_sweep_backward itself refuses a sweep of more than one group
 * (PHYLO_ESTATE).  Run to run the same bits (no floating-point atomics). */
int phylo_sweep_backward_batch(phylo_ctx* ctx, double* d_lam_l, double* d_lam_r, double* d_pi, double* d_Q, int G,
                               phylo_stats* perf);

/* The host half of a VI training step in the library (reference: optimizer.minimize(self.cost), vcsmc.py:488-491; the NumPy
 * statement of the same formulas is phylo_amd/train.py).  Variables packed as a_l[N-1] | a_r[N-1] | y_q[16] | y_station[4] (the
 * reference's 'left_branches_param', 'right_branches_param', 'Qmatrix', 'Stationary_probs': log-rates, vcsmc.py:119-124).
 * phylo_vi_gradients: model from the variables (vcsmc.py:133-148; jc != 0: the JC69 constants) -> phylo_set_model -> sweep with
 * PHYLO_KEEP_GRAPH on the context's leaves -> phylo_sweep_backward -> chain rules; grads = d logZ / d variables, packed alike
 * (zeros for y_q, y_station under JC69).  fwd / bwd (may be NULL): phylo_sweep_fetch's and phylo_sweep_backward's stats.
 * Any number of taxa the context accepts (2 ... 512; the twisted proposal: C(N,2) M <= 2^20); the arguments are checked before
 * phylo_set_model and the sweep, so a refused call (PHYLO_EINVAL: NULL vars or grads) leaves nothing in flight.
 * On a sharded context phylo_vi_gradients is a collective call like phylo_sweep_backward (every rank passes the same seed and
 * variables: it is ONE particle system) and every rank receives the same gradient bits.
 * phylo_vi_apply: kind 0 tf.train.GradientDescentOptimizer (var += lr d logZ / d var), 1 tf.train.AdamOptimizer (TF 1.15
 * defaults are beta1 0.9, beta2 0.999, eps 1e-8; t, m, v: its state, m and v packed like the variables, zero at the start). */
int phylo_vi_gradients(phylo_ctx* ctx, uint64_t seed, uint32_t flags, int M, int jc, const double* vars, double* logZ, double* grads,
                       phylo_stats* fwd, phylo_stats* bwd);
/* phylo_vi_gradients for G independent particle systems of K / G particles behind one set of launches (seeds[G]; plain proposal):
 * logZ[G], grads[G][2 (N-1) + 20], row g the gradient of log Z-hat_g with respect to the variables.  2 ... 512 taxa alike. */
int phylo_vi_gradients_batch(phylo_ctx* ctx, const uint64_t* seeds, int G, uint32_t flags, int jc, const double* vars, double* logZ,
                             double* grads, phylo_stats* fwd, phylo_stats* bwd);
int phylo_vi_apply(int n_taxa, int jc, double* vars, const double* grads, int kind, double lr, double beta1, double beta2, double eps,
                   int64_t* t, double* m, double* v);

/* Diagnostics of the one-launch sweep: with PHYLO_PERSIST_STAMPS=1 in the environment when the context is created,
 * workgroup 0 stamps s_memrealtime (100 MHz ticks) at its phase boundaries; out receives [N][16] values (rows 0..N-2: rank
 * events; row N-1: prologue).  No effect on results; not for timed runs. */
int phylo_debug_stamps(phylo_ctx* ctx, uint64_t* out, int n);

/* Test hook, no GPU needed: the host side of phylo_sweep_backward's integer lists (phylo_amd/csrc/phylo_revlists.h), run on
 * caller-supplied ancestors [N-2][K] (int64, as phylo_sweep returns them) and children [N-1][K][2] (node ids: leaf < N, else
 * N + r K + k of an EARLIER rank event: the children of rank event 0 are leaves and are not looked at).  lookahead_nodes: node ids with look-ahead entries (twisted proposal), may be NULL.  lists receives the slab the
 * device reads (ad_off | ad_idx | par_off | par_idx | heavy | chunk_beg | chunk_cnt | slow_flag | slow_idx | adp; R (K+1) + 9 R K
 * + 1 + 2 cap ints, cap = 2 R K / 4 + 1, R = N - 1); meta: n_adp, n_chunks, max_chunks, n_slow, n_par, cap, then ev_adp0[R+1],
 * rank_chunk0[R+1], ev_slow0[R+1].  tests/test_revlists_cpu.py checks it against a restatement in NumPy. */
int phylo_debug_reverse_lists(int N, int K, const int64_t* ancestors, const int32_t* child, int early_free, int rows_form,
                              const int32_t* lookahead_nodes, int n_lookahead, int32_t* lists, int64_t n_lists, int32_t* meta,
                              int n_meta);

/* Test hook, no GPU needed: the twisted proposal's look-ahead lists of phylo_sweep_backward (pg_build_lookahead,
 * phylo_amd/csrc/phylo_revlists.h) on caller-supplied adopted root tables roots_ad [N-1][K][N] (slots 0 .. N-r-1 of rank event r:
 * a leaf id < N or a node id N + r' K + k of an earlier rank event r'; rank event 0 is not looked at).  S shapes the chunks; M (the
 * look-ahead merges per pair) is checked and otherwise unused: the lists do not depend on it.  slow_flag [(N-1) K], in and out:
 * bit 1 is set for every touched node.  image receives xent | xchunk_node | xchunk_beg | xchunk_cnt | xchunk_part | xnode_id |
 * xnode_chunk0 | xnode_nchunks (n_xent + 4 n_xchunks + 3 n_xnodes + 1 ints; PHYLO_EINVAL when n_image is too small); meta: n_xent,
 * n_xchunks, n_xnodes, tw_max_chunks, then ev_chunk0[R+1], ev_node0[R+1] (R = N - 1).  tests/test_revlists_cpu.py. */
int phylo_debug_lookahead_lists(int N, int K, int S, int M, const int32_t* roots_ad, int32_t* slow_flag, int32_t* image,
                                int64_t n_image, int32_t* meta, int n_meta);

/* Test hook, no GPU needed: the form phylo_sweep_backward takes (pg_plan_form + pg_plan_chains, phylo_revlists.h; DESIGN.md
 * section 4b "driver") for a shape, the last sweep's facts (twisted proposal; lazy sweep that left marks), the switches (bit 0
 * PHYLO_REV_HOST_LISTS, 1 PHYLO_GRAD_ONE_STREAM, 2 PHYLO_GRAD_TWO_STREAMS, 3 PHYLO_GRAD_ROWS_CHAIN, 4 PHYLO_GRAD_COEFF_CHAIN) and
 * the lists' counts (flagged nodes, tiles of 256 sites per row, workgroups of the coefficient chain, reverse passes in flight in
 * the process).  mask: bit 0 rows_form, 1 whole, 2 early_free, 3 dev_lists, 4 sort_early, 5 bg_free, 6 two, 7 parents_first,
 * 8 rows_all, 9 rows_overlap, 10 chunks_first, 11 interleave, 12 coeff_all.  tests/test_revplan_cpu.py restates the rules. */
int phylo_debug_reverse_plan(int N, int K, int K_local, int S, int world, int twisted, int marks, uint32_t switches, int64_t n_slow,
                             int TS, int64_t coeff_wgs, int passes_in_flight, uint32_t* mask);
/* Test hook, no GPU needed: the form the forward sweep's launch path takes (sweep_plan_form + sweep_plan_launches,
 * phylo_sweep_plan.h; DESIGN.md section 4 "driver") for a shape, a communicator (transport != 0), the flags of phylo_sweep_begin
 * and the switches: bit 0 PHYLO_EAGER_NODES, 1 PHYLO_REHEARSE_SHARDED, 2 PHYLO_REPLICATED_BOOK (the environment), then three facts
 * of the context: bit 3 a JC69 model, 4 coded leaves, 5 the device-side exchange.  The site tile is the policy's (phylo_site_tile).
 * mask: bit 0 twist, 1 graph, 2 timek, 3 lazy, 4 shard_form, 5 replicated_book, 6 local_book, 7 book_mat, 8 mat_by_draws,
 * 9 want_rdraw, 10 use_rec, 11 sorted_prologue, 12 mat_grouped, 13 mat_draws_grouped, 14 step_a_work, 15 mat_after_book,
 * 16 mat_barrier, 17 fix_rootll, 18 fold_logz, 19 no_store_last, 20 final_missing, 21 last_graph_eager, 22 one_tile, 23 twist_ll,
 * 24 twist_tables, 25 tile_epilogue, 26 batched (the scan strides over the groups' log-normalisers); bits 28..31 book_width / 8.
 * launches[N + 1]: what stats.n_launches counts for the begin ([0]), rank event r ([r + 1]) and the finish ([N]).  Arguments that
 * phylo_sweep_begin refuses are refused with the same code and message.  tests/test_sweepplan_cpu.py restates the rules. */
int phylo_debug_sweep_plan(int N, int K, int K_local, int S, int G, int M, int world, int transport, uint32_t flags, uint32_t switches,
                           uint32_t* mask, int32_t* launches);
/* Test hooks of the chain form of a rank event (sweep_chain_form_of, phylo_sweep_plan.h; DESIGN.md sections 4 and 6b): the scan
 * hands out every particle's ancestor and the list of adopted particles, the bookkeeping reads its ancestor, the adopted nodes are
 * written from the list by item waves inside the bookkeeping's launch.  A decision of its own beside the plan: phylo_debug_sweep_plan's output does not depend on it.
 * phylo_debug_sweep_chain, no GPU needed: the arguments of phylo_debug_sweep_plan, then PHYLO_SCAN_MULTI_MIN and
 * PHYLO_SCAN_ANCESTORS as a context reads them (unset: 4096 and 1).  out[3]: taken (0: the rest is 0), item waves per group, the
 * parts a node's sites are cut into.
 * phylo_debug_sweep_chain_of: 1 if the rank events of the context's last sweep took the chain form, else 0.
 * phylo_debug_scan_ancestors: the scan's tail alone, on G groups of Kg log-weights (host, [G][Kg]) with the groups' seeds for the
 * resampling draws of rank event r_next: anc [G][Kg] (index inside the group), list [G][Kg] (the first cnt[g] entries of a row:
 * the adopted particles, ascending; the rest -1) and cnt [G].  Needs a scan form that keeps the cdf in LDS (else PHYLO_ESTATE).
 * tests/test_sweepchain_cpu.py restates the rule, tests/test_gpu_scan_ancestors.py the tail. */
int phylo_debug_sweep_chain(int N, int K, int K_local, int S, int G, int M, int world, int transport, uint32_t flags, uint32_t switches,
                            int multi_min, int scan_ancestors, int32_t* out);
int phylo_debug_sweep_chain_of(phylo_ctx* ctx, int32_t* taken);
/* Test hooks of how the record-form merge and the chain bookkeeping are launched (phylo_launch_map.h; the plan's launch_xcd and
 * book_xcd; DESIGN.md sections 6b and 8).  Neither changes a bit of a result.
 * phylo_debug_launch_map, no GPU needed: for a launch of n items at W (1, 2 or 4) waves per workgroup, with or without the XCD
 * remap, *grid = the workgroups and, if items is not NULL (cap >= grid W entries), items[b W + w] = the item that wave w of
 * workgroup b takes; an entry >= n is a wave without work.
 * phylo_debug_sweep_launch, no GPU needed: the arguments of phylo_debug_sweep_plan, then PHYLO_LAUNCH_XCD as a context reads it
 * (0 = unset, -1 = off, 1 = on, 2 = the merge alone, 3 = the bookkeeping alone).  out[2]: launch_xcd, book_xcd.
 * phylo_debug_sweep_launch_of: the same two of the context's last sweep.
 * tests/test_launch_map_cpu.py checks the map. */
int phylo_debug_launch_map(int n, int W, int xcd, int32_t* grid, int32_t* items, int64_t cap);
int phylo_debug_sweep_launch(int N, int K, int K_local, int S, int G, int M, int world, int transport, uint32_t flags, uint32_t switches,
                             int launch_xcd, int32_t* out);
int phylo_debug_sweep_launch_of(phylo_ctx* ctx, int32_t* out);
int phylo_debug_scan_ancestors(phylo_ctx* ctx, const double* logw, int Kg, int G, const uint64_t* seeds, uint32_t r_next, int32_t* anc,
                               int32_t* list, int32_t* cnt);
/* Test hook, no GPU needed: the form the resampling scan takes for groups of Kg log-weights (sweep_scan_form_of, phylo_sweep_plan.h;
 * DESIGN.md section 6b): 0 the scan of several workgroups per group (pp_scan_multi_*), 1 pp_resample_scan<512>, 2
 * pp_resample_scan<1024>, 3 pk_resample_scan(_groups); -1 for Kg < 1.  ctx NULL: under PHYLO_SCAN_MULTI_MIN = multi_min; else under
 * the value the context read when it was created (multi_min is ignored).  wanted: the caller asks for a cdf or a log-normaliser
 * (phylo_resample, phylo_log_zsmc and every scan of a sweep do).  tests/test_sweepplan_cpu.py restates the rule. */
int phylo_debug_scan_form(phylo_ctx* ctx, int Kg, int multi_min, int wanted);
/* Test hooks of the one-launch sweep's grid (persist_plan_of, phylo_sweep_plan.h; DESIGN.md sections 4c and 6b).
 * phylo_debug_persist_plan, no GPU needed: the rule for a shape (K: all G groups' particles, K divisible by G), the flags of a sweep,
 * the switches (bit 0 PHYLO_EAGER_NODES, 1 PHYLO_ONE_LAUNCH: the environment), a communicator (transport != 0) and the facts the
 * driver asks the device for: n_cus compute units, blocks_per_cu workgroups the planner may place on one (0: the kernel is not
 * admitted; 1; 2), and the two switches as a context reads them: persist_wgs (PHYLO_PERSIST_WGS, <= 0: unset) and persist_nt
 * (PHYLO_PERSIST_NT: 512, everything else is 256).  out[5]: taken (0: the launch path runs, the rest is 0), Wg workgroups per group,
 * m = K / G / Wg particles per workgroup, threads per workgroup, dynamic LDS bytes per workgroup.
 * phylo_debug_persist_of: threads, Wg, m and LDS bytes of the context's last sweep if it was a one-launch sweep, else PHYLO_ESTATE.
 * tests/test_one_launch_plan_cpu.py restates the rule; tests/test_gpu_one_launch_forms.py asserts the grid before it compares. */
int phylo_debug_persist_plan(int N, int K, int S, int G, uint32_t flags, uint32_t switches, int world, int transport, int n_cus,
                             int blocks_per_cu, int persist_wgs, int persist_nt, int64_t* out);
int phylo_debug_persist_of(phylo_ctx* ctx, int32_t* nt, int32_t* Wg, int32_t* m, int64_t* lds);
/* Test hook, no GPU needed: the packed image of byte codes [N][S] as phylo_set_leaves builds it beside them (pk_pack_leaf_codes,
 * phylo_packed_codes.h): packed[((leaf nC + Jc) 64 + c) 16 + j] = code of site 64 (16 Jc + j) + c with
 * nC = ceil(ceil(S / 64) / 16), sites >= S hold the pad code 5.  *need = N nC 1024, the image's bytes; with packed NULL only
 * *need is set, otherwise cap >= *need is required.  tests/test_packed_codes_cpu.py restates the layout. */
int phylo_debug_pack_leaf_codes(const uint8_t* codes, int N, int S, uint8_t* packed, int64_t cap, int64_t* need);
/* Test hooks of the merge's site-pattern form (phylo_site_patterns.h), the first two without a GPU.
 * phylo_debug_site_patterns: the tables phylo_set_leaves builds from byte codes [N][S].  *U = the number of distinct columns,
 * numbered by first occurrence; rep[u], u < *U: the first site with column u (room for S); image (16 bits per site, room for
 * 2048 ceil(ceil(S / 64) / 16) bytes, written when *U <= 8191): image[((Jc 2 + h) 64 + c) 8 + j] = 8 (column number of site
 * 64 (16 Jc + 8 h + j) + c), 8 *U at sites >= S; rep_off (1024 words, written when *U <= 512): 32 rep[u], 0 from *U on; rep_leaf
 * (written when *U <= 512, rep_leaf_cap >= N 1024 always suffices): the codes [N][*U] of the representative sites as
 * phylo_debug_pack_leaf_codes packs them.  Each output may be NULL.
 * phylo_debug_site_patterns_rule: 1 if a context of S sites in ntiles site tiles whose leaves have U distinct columns and are coded
 * (coded != 0) takes the form under PHYLO_SITE_PATTERNS = 0 (sw 0), unset (1) or force (2), else 0; -1 for bad arguments.
 * phylo_debug_site_patterns_of: *U of the context's current leaves (0: not coded) and whether its record-form merges take the form. */
int phylo_debug_site_patterns(const uint8_t* codes, int N, int S, int32_t* U, int32_t* rep, uint16_t* image, uint32_t* rep_off,
                              uint8_t* rep_leaf, int64_t rep_leaf_cap);
int phylo_debug_site_patterns_rule(int S, int U, int coded, int ntiles, int sw);
int phylo_debug_site_patterns_of(phylo_ctx* ctx, int32_t* U, int32_t* taken);
/* Test hooks of the clade tables of the site-pattern form (phylo_site_patterns.h), the first two without a GPU.
 * phylo_debug_clade_patterns_rule: 1 if leaves of N taxa, S sites and U distinct columns whose merges take the pattern form
 * (pat_taken != 0) get clade tables under PHYLO_CLADE_PATTERNS = 0 (sw 0), unset (1) or force (2), else 0; -1 for bad arguments.
 * *bytes (may be NULL) = the tables' size.
 * phylo_debug_clade_tables: the tables of byte codes [N][S], N <= 12.  *U as above; layout[5] = the bytes of the strided byte
 * codes, of a block's representatives, of its site image, a block's stride, the whole buffer.  With tables NULL nothing else is
 * written; otherwise cap >= layout[4] and U <= 512 are required, block Z lies at layout[0] + Z layout[3] (header word 0 = U_Z at
 * +0, representatives at +256, image behind them; blocks of fewer than three leaves are not written) and cls, if given, receives
 * [2^N][U] 16-bit class numbers (every bitset, the small ones included).
 * phylo_debug_clade_patterns_of: whether the context's current leaves have tables that a record-form sweep would use, whether the
 * last sweep begun on the launch path took them (the plan's clade_pat), and the tables' bytes (0: none).
 * phylo_debug_sweep_plan: bit 6 of `switches` states that the tables are there; the plan's clade_pat is bit 27 of *mask. */
int phylo_debug_clade_patterns_rule(int pat_taken, int N, int S, int U, int sw, int64_t* bytes);
int phylo_debug_clade_tables(const uint8_t* codes, int N, int S, int32_t* U, int64_t* layout, uint8_t* tables, int64_t cap, uint16_t* cls);
int phylo_debug_clade_patterns_of(phylo_ctx* ctx, int32_t* eligible, int32_t* taken, int64_t* bytes);
/* ... after a batched sweep of G groups (K the total): the device lists' limit is per group (K / G <= 8192), every other
 * limit sees the totals.  G = 1 is phylo_debug_reverse_plan. */
int phylo_debug_reverse_plan_batch(int N, int K, int G, int S, uint32_t switches, int64_t n_slow, int TS, int64_t coeff_wgs,
                                   int passes_in_flight, uint32_t* mask);
/* No GPU and no context needed: the form of phylo_tree_summary and phylo_tree_branches (pt_plan_form / pb_plan_form of
 * phylo_trees_plan.h; DESIGN.md section 10 "driver") for a sweep of G groups on `world` ranks, a summary of n_clades and
 * n_topologies rows, whether the sweep kept whole-K branch lengths, whether PHYLO_TREE_WIDE_KEYS is set (force_wide: the 64-bit
 * keys of the branch pass at any size), and rocPRIM's temporary-storage bytes of either pass (facts).
 * scalars[13]: R, L, W, E, Emax, Kg, cbits, tbits, wide, gather, the number of sort passes, the buffers of slot 12, of slot 13.
 * summary_slab / branches_slab [2 n + 1]: the n buffers' offsets, their bytes, the slab's total (order: TREE_SUMMARY_BUFS /
 * TREE_BRANCHES_BUFS of phylo_amd/_ffi.py).  sort_bits[17]: the radix bits of the summary's sort passes in issue order.
 * launches[2]: what stats.n_launches of the two calls counts.  What the calls refuse is refused with the same code and message
 * (the summary's first).  tests/test_treeplan_cpu.py restates the rules.
 * phylo_debug_tree_branches_of: the plan the context's last phylo_tree_branches took: *wide (1: the 64-bit keys), *cbits, *tbits.
 * PHYLO_ESTATE when no branch pass has run on the context. */
int phylo_debug_tree_plan(int N, int K, int G, int world, int64_t n_clades, int64_t n_topologies, int kept_whole, int force_wide,
                          int64_t summary_temp, int64_t branches_temp, int64_t* scalars, int64_t* summary_slab, int64_t* branches_slab,
                          int32_t* sort_bits, int32_t* launches);
int phylo_debug_tree_branches_of(phylo_ctx* ctx, int32_t* wide, int32_t* cbits, int32_t* tbits);

/* The same lists built by the device kernels (phylo_revlists_dev.h) from the graph of the preceding lazy sweep with
 * PHYLO_KEEP_GRAPH, copied back in the same layout (what the builders do not write reads -1; heavy[] holds GLOBAL chunk indices,
 * rank_chunk0 in meta is zero), plus, when not NULL, the ancestors [N-2][K] and children [N-1][K][2] they were built from:
 * tests/test_gpu_grad.py compares them with phylo_debug_reverse_lists on those. */
int phylo_debug_device_lists(phylo_ctx* ctx, int32_t* lists, int64_t n_lists, int32_t* meta, int n_meta, int64_t* ancestors,
                             int32_t* child);
/* ... and from a genealogy the caller gives (the context's N and K; it replaces the last sweep's: sweep again before the next
 * phylo_sweep_backward): tests/test_gpu_grad.py replays the cases of tests/test_revlists_cpu.py through the device builders. */
int phylo_debug_device_lists_of(phylo_ctx* ctx, const int64_t* ancestors, const int32_t* child, int32_t* lists, int64_t n_lists,
                                int32_t* meta, int n_meta);

/* Tree posterior of the last sweep (what get_tree_prob, csmc.py:335-349, is to the CSMC path): every final
 * particle's tree as its N-2 non-trivial clades (taxon bitsets, W = ceil(N/64) uint64 words, taxon i = bit i % 64 of word i / 64),
 * weighted by the resampling contract's integer weights u_k = floor(exp(logw[N-2][k] - max) 2^44) of the last rank event (same
 * NaN / all-bad rules as the scan), U = sum u_k per group.  Clade weight C = sum of u_k over the particles whose tree holds the clade,
 * topology (= clade set) weight T = sum of u_k over its particles; integer sums, exact.  All G groups of a batched sweep, each on
 * its own: group g's rows equal the summary of the sweep of K/G particles with seeds[g].  Runs after the sweep on the context's
 * stream and leaves the sweep's state alone (the next sweep's bits do not change).  Sharded context: a collective call (every rank
 * gathers the children records) that returns the same tables on every rank, equal to the unsharded sweep's.
 * phylo_tree_summary: counts n_clades <= K (N-2), n_topologies <= K, n_groups (may be NULL) = G; perf (may be NULL): sweep_ms = the
 * summary's device time (hipEvents), n_launches.  Needs N >= 3.  PHYLO_ESTATE before any sweep; PHYLO_EHIP (message in
 * phylo_last_error) when the summarised sweep timed out in a bounded wait, or when two different topologies share a 64-bit routing
 * hash (never merged: the summary is refused).
 * phylo_tree_summary_fetch copies the last summary's tables (any pointer may be NULL), rows group-major:
 *   clade_bits [n_clades][W], clade_weight [n_clades], clade_group [n_clades]: per group by C descending, then bitset ascending
 *     (as an unsigned integer, word W-1 most significant);
 *   topo_weight, topo_count (particles), topo_rep (smallest particle inside its group), topo_group [n_topologies]: per group by
 *     T descending, then representative ascending;
 *   particle_topo [K]: the row of particle k's topology counted from its group's first row; u [K]; U [G]. */
int phylo_tree_summary(phylo_ctx* ctx, int64_t* n_clades, int32_t* n_topologies, int32_t* n_groups, phylo_stats* perf);
int phylo_tree_summary_fetch(phylo_ctx* ctx, uint64_t* clade_bits, uint64_t* clade_weight, int32_t* clade_group, uint64_t* topo_weight,
                             int32_t* topo_count, int32_t* topo_rep, int32_t* topo_group, int32_t* particle_topo, uint64_t* u, uint64_t* U);

/* Branch lengths of that tree posterior.  The node a particle's tree holds for a rank event has a left
 * and a right child with their own sampled lengths (lbranch / rbranch of phylo_sweep_fetch): 2N-2 branches per tree, one above
 * every leaf and every non-trivial clade.  Per segment of particles the pass returns four doubles, never a quotient:
 *   S1 = sum of x, x = (double) u_k * b;  S2 = sum of x * b;  min b;  max b
 * by the canonical segment sum (element j to column j mod 64, columns added in increasing j from +0.0, the 64 columns by the
 * adjacent-pair tree): the host divides by the clade weight C (U_g for a leaf, T for a topology's branches); C = 0 has no mean.
 * phylo_tree_branches runs the pass for the last phylo_tree_summary of the last sweep on the context's stream; perf (may be NULL):
 * sweep_ms = device time, n_launches.  PHYLO_ESTATE when there is no summary of the current sweep (a newer sweep invalidates it).
 * Collective on a sharded context (the branch lengths are all-gathered; every rank returns the unsharded tables).  The sweep's and
 * the summary's state are left alone.
 * phylo_tree_branches_fetch (any pointer may be NULL; row order that of phylo_tree_summary_fetch):
 *   clade_stats [n_clades][4]: over the particles of the row's group that hold the clade, in ascending entry r K + k;
 *   leaf_stats [G][N][4]: the branch above leaf i over all particles of group g, in ascending k;
 *   topo_clades [n_topologies][N-2]: the topology's clade rows, ascending, counted from its group's first clade row;
 *   topo_stats [n_topologies][2N-2][4]: over the topology's particles in ascending k, the N leaves in taxon order, then the
 *     branches above its N-2 clades in the order of topo_clades. */
int phylo_tree_branches(phylo_ctx* ctx, phylo_stats* perf);
int phylo_tree_branches_fetch(phylo_ctx* ctx, double* clade_stats, double* leaf_stats, int32_t* topo_clades, double* topo_stats);

/* RELL bootstrap over the per-site factors of a scored tree set: which of T trees are significantly worse
 * than the best one?  site_lik_TxS is what phylo_trees_loglik / phylo_trees_loglik_rates return (every entry finite and > 0); S is
 * the call's own (no leaves are read, it need not be the context's).  Bit level:
 *   x[t][s] = log(site_lik[t][s]) (the contract's log, phylo_math_probe op 1);
 *   replicate b (its GLOBAL index, whatever the chunking) draws S sites: draw j is word j & 3 of the Philox4x32-10 block with key
 *     seed and counter (b, 0, 4, j >> 2) -- stream 4 --, the site is (word * S) >> 32 as a 64-bit product; cnt[b][s] counts them;
 *   rl[t][b]: acc = +0.0, then acc = fma((double)cnt[b][s], x[t][s], acc) for s = 0 .. S-1 in ascending order, ONE chain;
 *   obs[t]: the same chain with every count 1 (last bits off loglik_T of the scoring call, which multiplies site factors: the
 *     statistics use obs, which is consistent with the replicates);
 *   best[b] = the t of the greatest rl[t][b], ties to the lowest t;  wins[t] = #{b : best[b] = t}.
 * Outputs: obs_T [T], best_B [B], wins_T [T]; may be NULL: rep_loglik_TxB [T][B] = rl, counts_BxS [B][S] = cnt, site_loglik_TxS
 * [T][S] = x, perf (sweep_ms = device time by hipEvents, n_launches, units = T S B).
 * Synchronous; on a sharded context a local call, not a collective.  x stays on the device for the call (PHYLO_ENOMEM if it cannot
 * be allocated); replicates run in chunks whose counts (uint16) and scores stay within 256 MiB (PHYLO_RELL_CHUNK=n in the
 * environment of phylo_create caps the replicates per chunk; no bit depends on it).  The call has its own scratch and events,
 * released with the context, and leaves alone the sweep's state, a kept graph, a tree summary and phylo_trees_loglik's scratch.
 * PHYLO_EINVAL, before anything is queued: a NULL required pointer, T < 1, S outside 1 .. 65535, B outside 1 .. 2^20, an entry of
 * site_lik that is not finite and > 0 (the message names tree and site). */
int phylo_rell(phylo_ctx* ctx, int T, int S, const double* site_lik_TxS, int B, uint64_t seed, double* obs_T, int32_t* best_B,
               int64_t* wins_T, double* rep_loglik_TxB, int32_t* counts_BxS, double* site_loglik_TxS, phylo_stats* perf);
/* Test hook, no GPU and no context needed: phylo_rell's contract as a loop on the host over the same functions the kernels call,
 * for replicates b0 .. b0 + nB - 1: counts [nB][S], x [T][S], rl [T][nB]; any output may be NULL (site_lik too when only counts
 * are asked for). */
int phylo_debug_rell_host(int T, int S, const double* site_lik_TxS, int b0, int nB, uint64_t seed, int32_t* counts, double* x,
                          double* rl);
/* The multiscale RELL bootstrap behind Shimodaira's approximately unbiased (AU) test: K scales, B
 * replicates each; replicate b of scale k draws draws[k] sites, not S.  x and obs_T are phylo_rell's, bit for bit.  Counts: draw j
 * (0 <= j < draws[k]) is word j & 3 of the Philox4x32-10 block with key = seed and counter (b, k, 4, j >> 2) -- counter word 1,
 * which is 0 in phylo_rell, carries the scale --, the site (word * S) >> 32; cnt[k][b][s] is uint16 and a row sums to draws[k]; b
 * and k are global indices, chunking changes no bit.  rl[k][t][b] is phylo_rell's single fma chain over ascending s with these
 * counts; it is NOT rescaled by S / draws[k] (the factor is the same for every tree of a column).  best[k][b] is the lexicographic
 * maximum of (rl[k][t][b], -t) over t: the greatest score, ties to the lowest t, in any order of reduction.  wins[k][t] =
 * #{b : best[k][b] = t}; every row of wins sums to B.  K = 1 with draws = {S} returns phylo_rell's obs, best and wins bit for bit
 * for the same seed and B: scale 0 shares its Philox stream with phylo_rell, so samples of the two calls are not independent.
 * The score matrix is never stored unless rep_loglik_KxTxB is given (tests and probes); best_KxB and counts_KxBxS may be NULL too.
 * perf (may be NULL): sweep_ms = device time by events, n_launches, units = T S K B.  Synchronous; on a sharded context a LOCAL
 * call.  Columns (k, b) run in chunks whose counts, partial maxima and, when asked for, scores stay within 256 MiB; a chunk may
 * straddle scales (PHYLO_RELL_CHUNK=n caps its columns; no bit depends on it).  Own scratch and events, released with the context:
 * the sweep's state, a kept graph, a tree summary and every other call's scratch are left alone.  PHYLO_EINVAL, before anything is
 * queued: phylo_rell's refusals (T < 1, S outside 1 .. 65535, B outside 1 .. 2^20 per scale, a site factor that is not finite and
 * > 0), K outside 1 .. 64, draws, obs or wins == NULL, a draws[k] outside 1 .. 65535, the uint16 count bound (the message names k). */
int phylo_rell_multiscale(phylo_ctx* ctx, int T, int S, const double* site_lik_TxS, int K, const int32_t* draws_K, int B, uint64_t seed,
                          double* obs_T, int64_t* wins_KxT, int32_t* best_KxB, double* rep_loglik_KxTxB, int32_t* counts_KxBxS,
                          phylo_stats* perf);
/* Test hook, no GPU and no context needed: phylo_rell_multiscale's contract as a loop on the host over the same functions the
 * kernels call, for scale k0 and replicates b0 .. b0 + nB - 1: counts [nB][S], rl [T][nB], best [nB]; any output may be NULL
 * (site_lik too when only counts are asked for). */
int phylo_debug_rell_multiscale_host(int T, int S, const double* site_lik_TxS, int K, const int32_t* draws_K, int k0, int b0, int nB,
                                     uint64_t seed, int32_t* counts, double* rl, int32_t* best);

/* Bit-level probe of the device arithmetic contract: op 0 exp(x), 1 log(x), 2 x/y, 3 fma(x,y,x), 4 exp(x) for x <= 0 (the scan's);
 * op 5 is outside that contract: the reverse pass's reciprocal of a site likelihood (pg_rcp, an ulp or two off 1/x). */
int phylo_math_probe(phylo_ctx* ctx, int op, const double* x, const double* y, int n, double* out);

/* Test hook: the reverse pass's Frechet derivative of expm (a scaled Taylor series, phylo_grad.h) on n caller-given pairs of
 * row-major 4x4 matrices, L = d/dt exp(A + t E) at t = 0.  form 0: one thread per matrix (pg_expm4_frechet, as pg_twist_finish
 * runs it); form 1: four lanes per matrix, one row each (pg_expm4_frechet_row, as pg_node_finish runs it).  The kernels call
 * the functions the pass calls; tests/test_gpu_grad_schemes.py compares both with a high-precision evaluation. */
int phylo_debug_frechet(phylo_ctx* ctx, int form, const double* A_nx16, const double* E_nx16, int n, double* L_nx16);

/* Test hook: the two statements of the site-product update (phylo_amd/csrc/phylo_math.h) on n caller-given
 * triples (p in [1,2), any x1, any x2), each from a fresh {p, 0, 0.0}: row 0 of the outputs [2][n] is the state (p', E', extra')
 * after pm_lp_mul2(x1, x2) -- the pair form of the merge kernels --, row 1 after pm_lp_mul(x1); pm_lp_mul(x2) -- the contract's
 * statement, what the oracle does.  ctx == NULL: a loop on the host, no GPU needed; otherwise one thread per triple on the
 * context's device (n <= 2^22 per call: the 64 n bytes of device scratch stay with the context until it is destroyed, so use a
 * throw-away context).  Both run the same functions the kernels call.  tests/test_site_product_host.py and
 * tests/test_gpu_site_product_edges.py compare them with a restatement in Python. */
int phylo_debug_site_product(phylo_ctx* ctx, const double* p, const double* x1, const double* x2, int n, double* out_p, int32_t* out_E,
                             double* out_extra);

/* ---- multi-GPU: one process per GPU, particles sharded by contiguous ranges ------------------- */
#define PHYLO_COMM_ID_BYTES 128
/* rank 0 makes the id (ncclGetUniqueId) and hands it to the other ranks out of band. */
int phylo_comm_unique_id(char id[PHYLO_COMM_ID_BYTES]);
/* Join `world` ranks.  The ctx must have been created with the GLOBAL K; afterwards this rank owns
 * particles [rank*K/world, (rank+1)*K/world) and sweep outputs are this shard's columns. */
int phylo_comm_init(phylo_ctx* ctx, int rank, int world, const char id[PHYLO_COMM_ID_BYTES]);
/* A further context of this process joins `owner`'s communicator (same rank, same world) instead of creating its
 * own: all collectives of the process then run on one stream of one communicator, in host issue order.  Collective
 * (peer pools are mapped); every rank makes the call for its contexts in the same order.  `owner` must outlive ctx. */
int phylo_comm_share(phylo_ctx* ctx, phylo_ctx* owner);
/* All-gather of a host blob of `bytes` bytes per rank (all = world * bytes, rank order): how a sharded caller
 * assembles per-particle outputs (ancestors, merges, branches) for host-side tree reconstruction. */
int phylo_comm_allgather(phylo_ctx* ctx, const void* mine, size_t bytes, void* all);
/* barrier + max over ranks of *value: an RCCL all-reduce (ncclMax) of one double on the communicator's stream (the
 * host-mediated test transport gathers and takes the max on the host); identity when no communicator is set. */
int phylo_comm_max(phylo_ctx* ctx, double* value);
int phylo_comm_barrier(phylo_ctx* ctx);
/* How this context exchanges the K-vectors of a rank event with the other ranks: 0 not sharded; 1 RCCL all-gather; 2 the
 * host-mediated test transport (PHYLO_COMM=hostshm); 3 the device-side exchange (every rank writes into the peers' hipIpc-mapped
 * slabs and raises a flag: no collective call per rank event; the default when sharded, PHYLO_P2P=0 turns it off). */
int phylo_comm_exchange_kind(const phylo_ctx* ctx);
/* Sharded contexts keep the remote nodes their particles merge in a local cache, fetched once per sweep over the peer mapping
 * (pk_pull_remote_children; PHYLO_NO_REMOTE_CACHE=1: every remote child is read in place, PHYLO_REMOTE_CACHE_CAP: slots).
 * used: slots claimed by the last sweep (more than cap: the rest was read in place); cap: slots (0: no cache). */
int phylo_debug_remote_cache(phylo_ctx* ctx, int* used, int* cap);

#ifdef __cplusplus
}
#endif
#endif /* PHYLO_HIP_H */
