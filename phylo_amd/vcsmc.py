"""VCSMC: the reference's class surface (vcsmc.py:103-645) over the MI355X library.

Same constructor, attribute names and method names/argument meaning as the reference.  Where the reference
builds TensorFlow graph nodes, these methods take and return NumPy arrays and run the computation on the
GPU through the C ABI (phylo_amd/_ffi.py).  No TensorFlow, no PyTorch, no CPU fallback for the hot ops.

Differences that are deliberate:
  * randomness is the counter-based contract of DESIGN.md (`seed` attribute; the reference sets no seed);
  * jump chains are rebuilt on the host from integer merge records, with the correct per-particle gather
    (the reference's vcsmc.py:306-307 gathers without the row offset, fixed in vncsmc.py);
  * train() takes the reference's optimiser steps (vcsmc.py:488-491, 532-536) with the gradient of the device's
    reverse pass (phylo_amd/train.py) instead of TensorFlow autodiff; with args.nested that is the reverse pass of the
    twisted proposal (vncsmc.py:568-640), every look-ahead potential differentiated.
"""
from __future__ import annotations

from datetime import datetime
from types import SimpleNamespace

import numpy as np

from . import _ffi, model, rng, treepost
from . import train as train_mod


def ncr(n, r):
    """vcsmc.py:23-27: n choose r as product / product (true division -> float)."""
    numer = np.prod(np.arange(n - r + 1, n + 1), dtype=np.int64) if r > 0 else 1
    denom = np.prod(np.arange(1, r + 1), dtype=np.int64) if r > 0 else 1
    return numer / denom


def log_double_factorial(n):
    """vcsmc.py:40-57: log n!! via the loop n, n-2, ... while >= 2; works on arrays."""
    n = np.asarray(n, dtype=np.float64).copy()
    result = np.zeros_like(n)
    while np.count_nonzero(n >= 2):
        result = np.where(n >= 2, result + np.log(np.where(n >= 2, n, 1.0)), result)
        n = n - 2
    return result


def gather_across_2d(a, idx, a_shape_1=None, idx_shape_1=None):
    """vcsmc.py:60-77: [a[k][idx[k]] for k]."""
    a, idx = np.asarray(a), np.asarray(idx)
    return a[np.arange(a.shape[0])[:, None], idx]


def gather_across_core(a, idx, a_shape_1=None, idx_shape_1=None, A=4):
    """vcsmc.py:80-97: per-particle row gather of a [K,N,S,A] core."""
    a, idx = np.asarray(a), np.asarray(idx)
    return a[np.arange(a.shape[0])[:, None], idx]


def default_args(**kw):
    """The reference's argparse defaults (runner.py:12-58) as a namespace."""
    d = dict(dataset='primate_data', n_particles=10, batch_size=256, learning_rate=0.001, num_epoch=100,
             optimizer='GradientDescentOptimizer', branch_prior=np.log(10), M=10, nested=False, jcmodel=False,
             memory_optimization='on', seed=0, n_gpus=1)
    d.update(kw)
    return SimpleNamespace(**d)


class VCSMC:
    """
    VCSMC takes as input a dictionary (datadict) with two keys:
     taxa: a list of n strings denoting taxa
     genome_NxSxA: a 3 tensor of genomes for the n taxa one hot encoded
    """

    def __init__(self, datadict, K, args=None, device=0):
        self.args = args if args is not None else default_args()
        self.taxa = datadict['taxa']
        self.genome_NxSxA = np.asarray(datadict['genome'], dtype=np.float64)
        self.K = K
        self.M = self.args.M
        self.N = len(self.genome_NxSxA)
        self.S = len(self.genome_NxSxA[0])
        self.A = len(self.genome_NxSxA[0, 0])
        self.seed = int(getattr(self.args, 'seed', 0) or 0)
        # the trainable variables (vcsmc.py:119-130) and what the graph derives from them
        self.variables = train_mod.Variables(self.N, self.args.branch_prior, self.args.jcmodel, self.A)
        self._sync_from_variables()
        self._device = device
        self._ctx = None
        self._sweeps = 0

    def _sync_from_variables(self):
        v = self.variables
        self.left_branches_param = np.exp(v.a_l)                                         # vcsmc.py:119
        self.right_branches_param = np.exp(v.a_r)                                        # vcsmc.py:120
        self.y_q, self.y_station = v.y_q, v.y_station
        self.Qmatrix = model.jc_Q(self.A) if v.jc else self.get_Q()                      # vcsmc.py:122-129
        self.stationary_probs = self.get_stationary_probs()

    # ---- device context -----------------------------------------------------------------------------
    def _context(self):
        if self._ctx is None:
            n_gpus = int(getattr(self.args, 'n_gpus', 1) or 1)
            if n_gpus > 1:
                # one process per GPU (python -m torch.distributed.run --nproc-per-node N runner.py --n_gpus N ...):
                # the K particles are sharded over the ranks, resampling stays global
                import os
                from .rendezvous import exchange_comm_id
                world, rank = int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('RANK', '0'))
                if world != n_gpus:
                    raise RuntimeError("--n_gpus %d needs %d ranks (python -m torch.distributed.run --nproc-per-node %d ...), "
                                       "found WORLD_SIZE=%d" % (n_gpus, n_gpus, n_gpus, world))
                self._device = int(os.environ.get('LOCAL_RANK', '0')) % max(_ffi.device_count(), 1)
                self._rank, self._world = rank, world
            ctx = _ffi.Context(self.K, self.N, self.S, self.A, device=self._device)
            ctx.set_leaves(self.genome_NxSxA)
            if n_gpus > 1:
                cid = exchange_comm_id(self._rank, self._world, _ffi.comm_unique_id if self._rank == 0 else None)
                ctx.comm_init(self._rank, self._world, cid)
            self._ctx = ctx
        self._ctx.set_model(self.Qmatrix, self.stationary_probs, self.left_branches_param, self.right_branches_param,
                            jc69_closed_form=bool(self.args.jcmodel))
        return self._ctx

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    # ---- model (vcsmc.py:133-148) -------------------------------------------------------------------
    def get_stationary_probs(self):
        """ Compute stationary probabilities of the Q matrix """
        return model.get_stationary_probs(self.y_station)

    def get_Q(self):
        """Off-diagonal terms by the softmax function, diagonal = -row sum (vcsmc.py:138-148)."""
        return model.get_Q(self.y_q)

    # ---- per-rank ops -------------------------------------------------------------------------------
    def conditional_likelihood(self, l_data, r_data, l_branch, r_branch):
        """vcsmc.py:150-161: (l_data @ expm(Q l_branch)) * (r_data @ expm(Q r_branch)), [S,A]."""
        l = np.asarray(l_data, dtype=np.float64)[None]
        r = np.asarray(r_data, dtype=np.float64)[None]
        return self._context().cond_likelihood_K(l, r, np.array([l_branch], dtype=np.float64),
                                                 np.array([r_branch], dtype=np.float64))[0]

    def broadcast_conditional_likelihood_K(self, l_data_KxSxA, r_data_KxSxA, l_branch_samples_K, r_branch_samples_K):
        """vcsmc.py:180-188."""
        return self._context().cond_likelihood_K(l_data_KxSxA, r_data_KxSxA, l_branch_samples_K, r_branch_samples_K)

    def compute_forest_posterior(self, data_KxXxSxA, leafnode_num_record, r=None):
        """vcsmc.py:231-245 (r only fixes the reshape in the reference; shapes are taken from the data)."""
        return self._context().forest_loglik(data_KxXxSxA, leafnode_num_record)

    def overcounting_correct(self, leafnode_num_record):
        """vcsmc.py:247-252."""
        rec = np.asarray(leafnode_num_record)
        return np.sum(rec - (rec == 1).astype(np.int32), axis=1)

    def compute_log_ZSMC(self, log_weights):
        """vcsmc.py:270-277."""
        return self._context().log_zsmc(np.atleast_2d(log_weights))

    def resample(self, core, leafnode_num_record, JC_K, log_weights, step=1):
        """vcsmc.py:279-289: indices ~ Categorical(softmax(log_weights)), K draws; gathers core / record /
        jump chains by them.  `step` is the rank event the draw belongs to (RNG counter)."""
        indices = self._context().resample(log_weights, self.seed, step)
        return (np.asarray(core)[indices], np.asarray(leafnode_num_record)[indices], np.asarray(JC_K)[indices],
                indices)

    def extend_partial_state(self, JCK, r):
        """vcsmc.py:291-316: two root slots to coalesce per particle, the remaining slots, q = 1/C(N-r,2)
        and the new jump-chain strings."""
        n = self.N - r
        q = 1 / ncr(n, 2)
        coalesced_indices, remaining_indices = rng.pair_order(self.K, n, self.seed, r)
        JCK = np.asarray(JCK, dtype=object)
        keep = gather_across_2d(JCK, remaining_indices)
        particles = gather_across_2d(JCK, coalesced_indices)
        coalesced = np.array([a + '+' + b for a, b in particles], dtype=object)
        return coalesced_indices, remaining_indices, q, np.concatenate([keep, coalesced[:, None]], axis=1)

    def get_log_likelihood(self, log_likelihood):
        """vcsmc.py:254-268, including its use of the LEFT rates for the right multiplier (quirk Q8)."""
        l_exponent = self.left_branches.T * self.left_branches_param[None, :]
        r_exponent = self.right_branches.T * self.right_branches_param[None, :]
        l_multiplier = np.log(self.left_branches_param)[None, :]
        r_multiplier = np.log(self.left_branches_param)[None, :]
        left_branches_logprior = np.sum(l_multiplier - l_exponent, axis=1)
        right_branches_logprior = np.sum(r_multiplier - r_exponent, axis=1)
        return log_likelihood[self.N - 2] + log_double_factorial(2 * self.N - 3) - left_branches_logprior \
            - right_branches_logprior

    # ---- the sweep ----------------------------------------------------------------------------------
    def sample_phylogenies(self, seed=None, flags=None):
        """vcsmc.py:406-451 (vncsmc.py:505-560 with args.nested): the N-1 rank events on the device.  Sets
        the reference's attributes and returns the ELBO (log Z-hat)."""
        if flags is None:
            flags = _ffi.FLAGS_DEFAULT | (_ffi.TWISTING if getattr(self.args, 'nested', False) else 0)
        self._twisted = bool(flags & _ffi.TWISTING)
        seed = self.seed + self._sweeps if seed is None else int(seed)
        self._sweeps += 1
        ctx = self._context()
        out = ctx.sweep(seed, flags=flags, M=self.M)
        if ctx.K_local != ctx.K:                         # sharded: every rank assembles all K particles' outputs
            for key in ('log_weights', 'log_likelihood', 'left_branches', 'right_branches', 'ancestors'):
                out[key] = ctx.comm_allgather_columns(out[key])
            out['merges'] = np.ascontiguousarray(
                np.moveaxis(ctx.comm_allgather_columns(np.moveaxis(out['merges'], 1, 2)), 2, 1))
        self.log_weights = out['log_weights']            # rows 1..N-1 of the reference's tensor
        self.log_likelihood = out['log_likelihood']
        self.left_branches = out['left_branches']
        self.right_branches = out['right_branches']
        self.merges = out['merges']
        self.ancestors = out['ancestors']
        self.elbo = out['logZ']
        self.cost = -self.elbo
        self.log_likelihood_R = self.get_log_likelihood(self.log_likelihood)
        self.stats = out['stats']
        self._last_seed = seed
        anc = out['ancestors']
        self.log_likelihood_tilde = (out['log_likelihood'][self.N - 3, anc[self.N - 3]] if self.N > 2
                                     else np.zeros(self.K) + np.log(1 / self.K))
        self.jump_chain_tensor, self.v_minus = self._final_tables()
        return self.elbo

    def _final_tables(self):
        """Root-table strings and v_minus after the last rank event, replayed on the host from the
        integer records (ancestors, merges) and the pair-order contract."""
        K, N = self.K, self.N
        jc = np.array([list(self.taxa)] * K, dtype=object)
        rec = np.ones((K, N), dtype=np.int64)
        for r in range(N - 1):
            if r > 0:
                idx = self.ancestors[r - 1]
                jc, rec = jc[idx], rec[idx]
            if self._twisted:                      # chosen pair from the device; the rest in descending slot order
                co = self.merges[r]
                rem = np.array([[i for i in range(N - r - 1, -1, -1) if i != a and i != b] for a, b in co],
                               dtype=np.int64).reshape(K, N - r - 2)
            else:
                co, rem = rng.pair_order(K, N - r, self._last_seed, r)
                assert np.array_equal(co, self.merges[r]), "host replay of the pair pick disagrees with the device"
            new = np.array([a + '+' + b for a, b in gather_across_2d(jc, co)], dtype=object)
            jc = np.concatenate([gather_across_2d(jc, rem), new[:, None]], axis=1)
            rec = np.concatenate([gather_across_2d(rec, rem), gather_across_2d(rec, co).sum(axis=1)[:, None]], axis=1)
        return jc, self.overcounting_correct(rec)

    @property
    def jump_chains(self):
        return self.jump_chain_tensor

    def batch_slices(self, data, batch_size):
        """Site minibatches (vcsmc.py:453-464): S // batch_size draws of batch_size sites without replacement from the
        sites not used yet, then the leftover sites as a last slice.  Draws come from python's global RNG by
        random.sample over the unused-site list in CPython set-difference order, so a seeded `random` reproduces the
        reference's slices."""
        import random
        unused = list(range(data.shape[2]))
        out = []
        for _ in range(len(unused) // batch_size):
            picked = random.sample(unused, batch_size)
            out.append(picked)
            unused = list(set(unused) - set(picked))
        return out + [unused] if unused else out

    def newick(self, k=0):
        """Newick string of particle k's final tree, rebuilt from the integer merge records of the last
        sweep (branch lengths = the sampled left/right branches of each coalescence)."""
        return self._newick_table()[k] + ';'

    def tree_posterior(self, threshold=0.5, branch_lengths=False):
        """Summary of the last sweep's tree posterior (the K weighted final particles; the counterpart of the CSMC path's
        get_tree_prob, csmc.py:335-349): clades with their support, topologies with probability, particle count,
        representative and its Newick, the majority-rule consensus (clades with support > threshold, supports as labels), the
        MAP topology and credible_set(p).  Clades, weights and topologies come from the device (phylo_tree_summary) in exact
        integer weights; with --n_gpus > 1 a collective call that every rank makes, and every rank holds the same table.
        branch_lengths=True adds (phylo_tree_branches, no particle replayed): clade_branches (mean, sd, min, max of the branch
        above every clade, conditional on the clade), leaf_branches by taxon name, per topology its `clades` rows and mean
        lengths, consensus_bl (the consensus with :mean on every edge) and map_newick (the MAP topology with its mean lengths)."""
        if self._ctx is None or not hasattr(self, '_last_seed'):
            raise RuntimeError("tree_posterior summarises the last sweep: call sample_phylogenies first")
        tab = self._ctx.tree_summary()
        if branch_lengths:
            tab.update(self._ctx.tree_branches(tab))
        table = treepost.group_table(tab, 0)
        trees = self._newick_table()
        newicks = {int(r): trees[int(r)] + ';' for r in table['topo_rep']}
        return treepost.TreePosterior(self.taxa, table, newicks, threshold)

    def _newick_table(self):
        """the final Newick strings (without ';') of all K particles"""
        K, N = self.K, self.N
        tab = [[str(t) for t in self.taxa] for _ in range(K)]
        for r in range(N - 1):
            if r > 0:
                idx = self.ancestors[r - 1]
                tab = [list(tab[i]) for i in idx]
            if self._twisted:
                rems = [[i for i in range(N - r - 1, -1, -1) if i != a and i != b] for a, b in self.merges[r]]
            else:
                rems = rng.pair_order(K, N - r, self._last_seed, r)[1]
            new = []
            for kk in range(K):
                a, b = self.merges[r][kk]
                node = '(%s:%.6g,%s:%.6g)' % (tab[kk][a], self.left_branches[r, kk], tab[kk][b], self.right_branches[r, kk])
                new.append([tab[kk][i] for i in rems[kk]] + [node])
            tab = new
        return [row[0] for row in tab]

    def score_trees(self, newicks, rates=None, want_sites=False, optimize=False, fit=(), search=None, search_rounds=20, fit_model=(),
                    fit_on=None, fit_rounds=20, ancestral=0, ancestral_rates=0):
        """Log-likelihoods of rooted Newick trees over the taxon names under the current model, the model's stationary
        distribution at the root (phylo_trees_loglik on the resident alignment: one call for all of them).  rates: a
        (rates, weights) pair, e.g. phylo_amd.rates.rate_model's -- the trees are then scored under that mixture of site
        rates (phylo_trees_loglik_rates).  Returns a list of floats -- with want_sites, that list and the site factors [T][S] the
        call returned --; a local call on every rank when sharded.
        optimize=True: the branch lengths of every tree are first climbed to their maximum-likelihood values
        (phylo_amd.treeopt.optimize_branches over phylo_trees_grad, or with rates over phylo_trees_grad_rates under that
        mixture); the scores, and the site factors of a final scoring call, are at those lengths, and self.last_tree_opt holds
        'newicks' (the trees at those lengths), 'loglik_given', 'iterations' and 'converged' per tree.
        fit (with optimize and rates): ('alpha',) or ('alpha', 'pinv') -- every tree also climbs its own Gamma shape (and share
        of invariant sites) from the model's values (phylo_amd.treeopt.optimize_rates); rates is then what
        phylo_amd.rates.parse_spec returns (it knows alpha, C and p_inv), the final scores come from one trees_loglik_rates per
        tree under that tree's fitted mixture, and self.last_tree_opt also holds 'alpha' and 'pinv' (None without the class).
        search='nni' (with optimize): after the climb every tree is hill-climbed over nearest-neighbour interchanges
        (phylo_amd.treesearch.nni_search over phylo_trees_nni and phylo_trees_grad, at most search_rounds rounds); the scores and
        site factors are those of the trees found, and self.last_tree_search holds 'newicks' (those trees), 'loglik_ml' (of the
        given topologies at their ML lengths), 'nni_moves', 'rounds' and 'converged' per tree.  With rates the search runs under
        the mixture (phylo_trees_nni_rates and phylo_trees_grad_rates).  With fit as well, every tree is searched with ITS fitted
        alpha (and p_inv) held fixed -- a mixture per tree, which follows its tree through the search --, then one more
        optimize_rates runs on the trees found from the found lengths and those values; self.last_tree_search then also holds
        the final 'alpha' and 'pinv' (self.last_tree_opt keeps those of the given topologies).
        fit_model (with optimize; one rate, no search): ('q',) or ('q', 'pi') -- ONE substitution model shared by all trees is
        fitted (at most fit_rounds rounds; CAVEAT: under the project's pruning convention the fitted function has no interior
        maximum over an asymmetric Q, so this is not a maximum-likelihood model estimate: DESIGN.md section 13c) on the trees fit_on (default: the best tree at its ML lengths under the current model)
        together with every tree's lengths (phylo_amd.treeopt.optimize_model over phylo_trees_grad_model and phylo_trees_grad,
        from y_q and y_station; never the JC69 closed form).  The fit calls set_model between device calls; the context's
        model is put back before this returns, and the fitted one is handed to the caller in self.last_model_fit ('Q', 'pi',
        'y_q', 'y_station', 'fit_on', 'rounds', 'objective_start', 'objective', 'history').  The scores and site factors come
        from one trees_loglik under the fitted model; self.last_tree_opt is as with optimize alone ('loglik_given' under the
        model given, 'newicks' at the lengths climbed under the fitted model).
        ancestral=k (one rate only): after everything else asked for, and before a fitted model is put back, the k best trees by
        the final score are reconstructed at the final lengths and model (phylo_trees_ancestral): self.last_ancestral holds
        'trees' (their indices, best first), 'newicks', 'child', 'loglik', 'state' and 'pmax' [k][N-1][S].
        ancestral_rates=k (with rates): the same under the mixture (phylo_trees_ancestral_rates) -- after everything else asked
        for (fit, search, refit) the k best trees by the final score are reconstructed under each tree's own final mixture (the
        fitted alpha and p_inv where fit gave them, passed per tree); self.last_ancestral holds ancestral=k's dictionary and
        'catpost' [k][C][S] (every category's posterior per site), 'siterate' [k][S] (the posterior mean rate of the site),
        'rates' and 'weights' [k][C] (the mixtures used) and 'alpha', 'pinv' (per tree where fitted, else None)."""
        ancestral = int(ancestral or 0)
        if ancestral < 0 or (ancestral and rates is not None):
            raise ValueError("score_trees: ancestral=%r needs k >= 1 and no rates (the posteriors are not built for mixtures; "
                             "ancestral_rates=k reconstructs under them)" % (ancestral,))
        ancestral_rates = int(ancestral_rates or 0)
        if ancestral_rates < 0 or (ancestral_rates and (rates is None or ancestral)):
            raise ValueError("score_trees: ancestral_rates=%r needs k >= 1, rates, and no ancestral=" % (ancestral_rates,))
        self.last_ancestral = None

        def reconstruct_rates(ctx, child, blen, loglik, r, w, alpha=None, pinv=None):
            if not ancestral_rates:
                return
            order = np.argsort(-np.asarray(loglik, dtype=np.float64), kind='stable')[:ancestral_rates]
            r, w = np.asarray(r, dtype=np.float64), np.asarray(w, dtype=np.float64)
            if r.ndim == 1:                                 # one mixture for all trees
                r, w = np.broadcast_to(r, (child.shape[0], r.size)), np.broadcast_to(w, (child.shape[0], w.size))
            r, w = np.ascontiguousarray(r[order]), np.ascontiguousarray(w[order])
            ll, state, pmax, catpost, siterate = ctx.trees_ancestral_rates(child[order], blen[order], r, w, want_post=False, want_state=True,
                                                                           want_pmax=True, want_catpost=True, want_siterate=True)
            self.last_ancestral = {'trees': [int(t) for t in order], 'child': child[order].copy(), 'loglik': [float(x) for x in ll],
                                   'newicks': [treepost.rows_to_newick(c, b, self.taxa) for c, b in zip(child[order], blen[order])],
                                   'state': state, 'pmax': pmax, 'catpost': catpost, 'siterate': siterate, 'rates': r, 'weights': w,
                                   'alpha': None if alpha is None else [float(alpha[t]) for t in order],
                                   'pinv': None if pinv is None else [float(pinv[t]) for t in order]}

        def reconstruct(ctx, child, blen, loglik):
            if not ancestral:
                return
            order = np.argsort(-np.asarray(loglik, dtype=np.float64), kind='stable')[:ancestral]
            ll, state, pmax = ctx.trees_ancestral(child[order], blen[order], want_post=False, want_state=True, want_pmax=True)
            self.last_ancestral = {'trees': [int(t) for t in order], 'child': child[order].copy(), 'loglik': [float(x) for x in ll],
                                   'newicks': [treepost.rows_to_newick(c, b, self.taxa) for c, b in zip(child[order], blen[order])],
                                   'state': state, 'pmax': pmax}

        fit = tuple(fit)
        fit_model = tuple(fit_model)
        if fit_model and (not optimize or rates is not None or fit or search is not None):
            raise ValueError("score_trees: fit_model=%r needs optimize=True and neither rates, fit nor search" % (fit_model,))
        if search is not None and (search != 'nni' or not optimize):
            raise ValueError("score_trees: search=%r needs search='nni' and optimize=True" % (search,))
        spec = rates if isinstance(rates, dict) else None
        if spec is not None:
            rates = (spec['rates'], spec['weights'])
        if fit and not (optimize and spec is not None):
            raise ValueError("score_trees: fit=%r needs optimize=True and rates as phylo_amd.rates.parse_spec gives them" % (fit,))
        rows = [treepost.newick_to_rows(nw, self.taxa) for nw in newicks]
        if not rows:
            return ([], np.empty((0, self.S))) if want_sites else []
        ctx = self._context()
        child, blen = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        if optimize and rates is not None:
            from . import treeopt
            given = ctx.trees_loglik_rates(child, blen, rates[0], rates[1])
            if fit:
                opt = treeopt.optimize_rates(lambda b, r, w: ctx.trees_grad_rates(child, b, r, w, want_curv=True, want_params=True),
                                             child, blen, spec['alpha'], spec['C'], pinv0=spec['pinv'], fit=fit)
            else:
                opt = treeopt.optimize_branches(lambda b: ctx.trees_grad_rates(child, b, rates[0], rates[1], want_curv=True), child, blen)
            blen = opt['blen']
            self.last_tree_opt = {'newicks': [treepost.rows_to_newick(c, b, self.taxa) for c, b in zip(child, blen)],
                                  'loglik_given': [float(x) for x in given], 'iterations': [int(i) for i in opt['iterations']],
                                  'converged': [bool(v) for v in opt['converged']]}
            if fit:
                self.last_tree_opt['alpha'] = [float(a) for a in opt['alpha']]
                self.last_tree_opt['pinv'] = None if opt['pinv'] is None else [float(p) for p in opt['pinv']]
            if search:
                from . import treesearch
                if fit:                                     # every tree under its own fitted mixture, held fixed while it is searched
                    r_t, w_t = np.array(opt['rates'], dtype=np.float64), np.array(opt['weights'], dtype=np.float64)
                    found = treesearch.nni_search(lambda c, b, i: ctx.trees_grad_rates(c, b, r_t[i], w_t[i], want_curv=True),
                                                  lambda c, b, i: ctx.trees_nni_rates(c, b, r_t[i], w_t[i]), child, blen,
                                                  max_rounds=search_rounds, with_index=True)
                else:
                    found = treesearch.nni_search(lambda c, b: ctx.trees_grad_rates(c, b, rates[0], rates[1], want_curv=True),
                                                  lambda c, b: ctx.trees_nni_rates(c, b, rates[0], rates[1]), child, blen,
                                                  max_rounds=search_rounds)
                ml_scores = [float(x) for x in opt['loglik']]
                child, blen = found['child'], found['blen']
                if fit:                                     # the model of the trees found, from the found lengths and the values held
                    opt = treeopt.optimize_rates(lambda b, r, w: ctx.trees_grad_rates(child, b, r, w, want_curv=True, want_params=True),
                                                 child, blen, opt['alpha'], spec['C'],
                                                 pinv0=spec['pinv'] if opt['pinv'] is None else opt['pinv'], fit=fit)
                    blen = opt['blen']
                self.last_tree_search = {'newicks': [treepost.rows_to_newick(c, b, self.taxa) for c, b in zip(child, blen)],
                                         'loglik_ml': ml_scores, 'nni_moves': [len(m) for m in found['moves']],
                                         'rounds': [int(r) for r in found['rounds']], 'converged': [bool(v) for v in found['converged']]}
                if fit:
                    self.last_tree_search['alpha'] = [float(a) for a in opt['alpha']]
                    self.last_tree_search['pinv'] = None if opt['pinv'] is None else [float(p) for p in opt['pinv']]
            if fit:
                per = [ctx.trees_loglik_rates(child[t], blen[t], opt['rates'][t], opt['weights'][t], want_sites=True)
                       for t in range(child.shape[0])]
                res = (np.array([p[0][0] for p in per]), np.array([p[1][0] for p in per]))
                reconstruct_rates(ctx, child, blen, res[0], opt['rates'], opt['weights'], opt['alpha'], opt['pinv'])
            else:
                res = ctx.trees_loglik_rates(child, blen, rates[0], rates[1], want_sites=True)
                reconstruct_rates(ctx, child, blen, res[0], rates[0], rates[1])
            res = res if want_sites else res[0]
        elif optimize and fit_model:
            from . import treeopt
            given = ctx.trees_loglik(child, blen)
            lam_l, lam_r = self.left_branches_param, self.right_branches_param

            def under(Q, pi):
                ctx.set_model(Q, pi, lam_l, lam_r, jc69_closed_form=False)

            def grad_fn(b, Q, pi):
                under(Q, pi)
                return ctx.trees_grad(child, b, want_curv=True)

            def grad_model_fn(idx, b, Q, pi, dirs):
                under(Q, pi)
                return ctx.trees_grad_model(child[idx], b, dirs)

            try:
                mf = treeopt.optimize_model(grad_model_fn, grad_fn, child, blen, self.y_q, np.asarray(self.y_station).reshape(-1),
                                            fit=fit_model, fit_on=fit_on, max_rounds=fit_rounds)
                blen = mf['blen']
                under(mf['Q'], mf['pi'])
                res = ctx.trees_loglik(child, blen, want_sites=True)
                reconstruct(ctx, child, blen, res[0])       # under the fitted model, before the context's own is put back
            finally:
                self._context()                             # the context's model again, from the same numbers: the same bits
            opt = mf['branches']
            self.last_tree_opt = {'newicks': [treepost.rows_to_newick(c, b, self.taxa) for c, b in zip(child, blen)],
                                  'loglik_given': [float(x) for x in given], 'iterations': [int(i) for i in opt['iterations']],
                                  'converged': [bool(v) for v in opt['converged']]}
            self.last_model_fit = {'Q': mf['Q'].tolist(), 'pi': mf['pi'].tolist(), 'y_q': mf['y_q'].tolist(),
                                   'y_station': mf['y_station'].tolist(), 'fit': list(fit_model), 'fit_on': mf['fit_on'],
                                   'rounds': int(mf['rounds']), 'objective_start': float(mf['objective_start']),
                                   'objective': float(mf['objective']), 'history': [float(h) for h in mf['history']],
                                   'converged': bool(mf['converged'])}
            res = res if want_sites else res[0]
        elif optimize:
            from . import treeopt
            given = ctx.trees_loglik(child, blen)
            opt = treeopt.optimize_branches(lambda b: ctx.trees_grad(child, b, want_curv=True), child, blen)
            blen = opt['blen']
            self.last_tree_opt = {'newicks': [treepost.rows_to_newick(c, b, self.taxa) for c, b in zip(child, blen)],
                                  'loglik_given': [float(x) for x in given], 'iterations': [int(i) for i in opt['iterations']],
                                  'converged': [bool(v) for v in opt['converged']]}
            if search:
                from . import treesearch
                found = treesearch.nni_search(lambda c, b: ctx.trees_grad(c, b, want_curv=True), ctx.trees_nni, child, blen,
                                              max_rounds=search_rounds)
                self.last_tree_search = {'newicks': [treepost.rows_to_newick(c, b, self.taxa) for c, b in zip(found['child'], found['blen'])],
                                         'loglik_ml': [float(x) for x in opt['loglik']], 'nni_moves': [len(m) for m in found['moves']],
                                         'rounds': [int(r) for r in found['rounds']], 'converged': [bool(v) for v in found['converged']]}
                child, blen = found['child'], found['blen']
            res = ctx.trees_loglik(child, blen, want_sites=True)
            reconstruct(ctx, child, blen, res[0])
            res = res if want_sites else res[0]
        elif rates is None:
            res = ctx.trees_loglik(child, blen, want_sites=want_sites)
            reconstruct(ctx, child, blen, res[0] if want_sites else res)
        else:
            res = ctx.trees_loglik_rates(child, blen, rates[0], rates[1], want_sites=want_sites)
            reconstruct_rates(ctx, child, blen, res[0] if want_sites else res, rates[0], rates[1])
        if want_sites:
            return [float(x) for x in res[0]], res[1]
        return [float(x) for x in res]

    def tree_tests(self, site_lik, B, seed, au=None):
        """tree_tests.json of --tree_tests: the RELL bootstrap (phylo_rell) over the site factors of the scored trees and the
        statistics phylo_amd.treetests reads off it; with au (--tree_tests_au: 'default' or r1,r2,...) also the AU test, from
        the multiscale bootstrap (phylo_rell_multiscale) on the same site factors, B and seed"""
        from . import treetests
        out = self._context().rell(site_lik, B, seed, want_reps=True)
        st = treetests.tree_tests(out['obs'], out['wins'], B, reps=out['rep_loglik'])
        res = {'B': int(B), 'seed': int(seed), 'best': int(st['best']), 'obs': out['obs'].tolist(), 'bp': st['bp'].tolist(),
               'p_kh': st['p_kh'].tolist(), 'p_sh': st['p_sh'].tolist(), 'c_elw': st['c_elw'].tolist()}
        if au:                                             # (absent without the flag: the file is what it was before it existed)
            sc = treetests.au_scales(np.asarray(site_lik).shape[1], au)
            ms = self._context().rell_multiscale(site_lik, sc['draws'], B, seed)
            fit = treetests.au_test(ms['wins'], sc['sigma2'], B)
            nn = lambda a: [None if x != x else float(x) for x in a]       # NaN (no fit for that tree) is null in JSON
            res.update(p_au=fit['p_au'].tolist(), se_au=nn(fit['se_au']), au_d=nn(fit['d']), au_c=nn(fit['c']),
                       au_ok=[bool(x) for x in fit['au_ok']],
                       au_scales={'r': sc['r'].tolist(), 'draws': sc['draws'].tolist(), 'sigma2': sc['sigma2'].tolist()},
                       bp_scales=fit['bp'].tolist())
        return res

    def _tree_scores(self, path):
        """tree_scores.json of --score_trees: the file's trees, and with branch lengths in the posterior also map.tre,
        consensus_bl.tre and the ten most probable topologies at their mean lengths (None where a branch has no estimate);
        with --score_rates every one of these scores is under that rate model, which the file then names"""
        with open(path) as f:
            newicks = [line.strip() for line in f if line.strip()]
        spec = getattr(self.args, 'score_rates', None)
        rm = None
        if spec:
            from . import rates as rates_mod
            rm = rates_mod.parse_spec(spec)
        mix = None if rm is None else (rm['rates'], rm['weights'])
        tests = getattr(self.args, 'tree_tests', None)
        ml = bool(getattr(self.args, 'score_opt', False)) and bool(newicks)   # --score_opt: at maximum-likelihood branch lengths
        mode = getattr(self.args, 'score_fit', None)       # --score_fit: the same under the rate model, and its parameters fitted
        fit = tuple(mode.split('+')[1:]) if mode and newicks else None
        self.tree_test_results = None
        self.trees_ml = None
        self.trees_search = None
        self.model_ml = None
        self.ancestral_results = None
        anc = int(getattr(self.args, 'score_ancestral', None) or 0) if newicks else 0   # --score_ancestral K: the K best trees reconstructed
        ancr = int(getattr(self.args, 'score_ancestral_rates', None) or 0) if newicks else 0   # --score_ancestral_rates K: under the rate model
        mfit = getattr(self.args, 'score_model_fit', None) if ml else None  # --score_model_fit q | q+pi: one ML model for all trees
        mfit = tuple(mfit.split('+')) if mfit else None
        srch = getattr(self.args, 'score_search', None) if ml else None     # --score_search nni[:ROUNDS]: then an NNI search from there
        fsrch = getattr(self.args, 'score_fit_search', None) if fit is not None else None   # --score_fit_search: the same under the rate model
        if fsrch:
            ll_search, sites = self.score_trees(newicks, rates=rm, want_sites=True, optimize=True, fit=fit, search=fsrch[0],
                                                search_rounds=fsrch[1], ancestral_rates=ancr)
            opt, found = self.last_tree_opt, self.last_tree_search
            ll, ll_ml = opt['loglik_given'], found['loglik_ml']
            self.trees_ml, self.trees_search = opt['newicks'], found['newicks']
            srch, ml = fsrch, True
        elif srch:
            ll_search, sites = self.score_trees(newicks, want_sites=True, optimize=True, search=srch[0], search_rounds=srch[1], ancestral=anc)
            opt, found = self.last_tree_opt, self.last_tree_search
            ll, ll_ml = opt['loglik_given'], found['loglik_ml']
            self.trees_ml, self.trees_search = opt['newicks'], found['newicks']
        elif ml and mfit:
            ll_ml, sites = self.score_trees(newicks, want_sites=True, optimize=True, fit_model=mfit, ancestral=anc)
            opt = self.last_tree_opt
            ll = opt['loglik_given']
            self.trees_ml = opt['newicks']
            self.model_ml = self.last_model_fit
        elif ml:
            ll_ml, sites = self.score_trees(newicks, want_sites=True, optimize=True, ancestral=anc)
            opt = self.last_tree_opt
            ll = opt['loglik_given']
            self.trees_ml = opt['newicks']
        elif fit is not None:
            ll_ml, sites = self.score_trees(newicks, rates=rm, want_sites=True, optimize=True, fit=fit, ancestral_rates=ancr)
            opt = self.last_tree_opt
            ll = opt['loglik_given']
            self.trees_ml = opt['newicks']
            ml = True
        elif tests and newicks:                            # --tree_tests: from the site factors of this very scoring call
            ll, sites = self.score_trees(newicks, rates=mix, want_sites=True, ancestral=anc, ancestral_rates=ancr)
        else:
            ll = self.score_trees(newicks, rates=mix, ancestral=anc, ancestral_rates=ancr)
        if anc or ancr:                                    # (absent without --score_ancestral / --score_ancestral_rates)
            self.ancestral_results = self.last_ancestral
        if tests and newicks:                              # (with --score_opt: the site factors at the ML lengths)
            from . import treetests
            self.tree_test_results = self.tree_tests(sites, *treetests.parse_spec(tests), au=getattr(self.args, 'tree_tests_au', None))
        out = {'model': {'Q': np.asarray(self.Qmatrix, dtype=np.float64).tolist(),
                         'pi': np.asarray(self.stationary_probs, dtype=np.float64).reshape(-1).tolist(),
                         'jc69_closed_form': bool(self.args.jcmodel)},
               'trees': [{'newick': nw, 'loglik': x} for nw, x in zip(newicks, ll)],
               'best': int(np.argmax(ll)) if ll else None}
        if ml:                                             # (absent without --score_opt: the file is what it was before the flag)
            for t, x, it, cv in zip(out['trees'], ll_ml, opt['iterations'], opt['converged']):
                t.update(loglik_ml=x, iterations=it, converged=cv)
            if srch:                                       # (absent without --score_search)
                for t, x, nm, rd in zip(out['trees'], ll_search, found['nni_moves'], found['rounds']):
                    t.update(loglik_search=x, nni_moves=nm, search_rounds=rd)
            if fit:                                        # --score_fit with a fitted model: every tree's own values
                for i, t in enumerate(out['trees']):
                    t['alpha'] = opt['alpha'][i]
                    if opt['pinv'] is not None:
                        t['pinv'] = opt['pinv'][i]
                    if fsrch:                              # (absent without --score_fit_search) the values of the tree found
                        t['alpha_search'] = found['alpha'][i]
                        if found['pinv'] is not None:
                            t['pinv_search'] = found['pinv'][i]
        if rm is not None:                                 # (absent without --score_rates: the file is what it was before the flag)
            out['rates'] = {'spec': rm['spec'], 'rates': rm['rates'].tolist(), 'weights': rm['weights'].tolist()}
        post = self.posterior
        if post is not None and getattr(post, 'map_newick', None) is not None:
            def scored(nw):
                try:
                    return {'newick': nw, 'loglik': self.score_trees([nw], rates=mix)[0]}
                except ValueError as e:                    # a branch held only by particles of weight 0 has no mean length
                    return {'newick': nw, 'loglik': None, 'error': str(e)}

            tops = []
            for i, t in enumerate(post.topologies[:10]):
                nw = treepost.tree_newick(post.taxa, [(post.clade_sets[j][0], m) for j, m in zip(t['clades'], t['clade_means'])],
                                          t['leaf_means'])
                tops.append(dict(scored(nw), rank=i, probability=t['probability']))
            out['summary'] = {'map': scored(post.map_newick), 'consensus_bl': scored(post.consensus_bl), 'topologies': tops}
        return out

    def _save_ancestral(self, save_dir, res):
        """ancestral.fa and ancestral.json of --score_ancestral: per reconstructed tree one FASTA record per internal node
        ('>tree{t}_node{N+i} clade=a,b,c', the most probable states as letters), and its index, Newick string and per node the
        numbers of phylo_amd.ancestral.summarise.  Under --score_ancestral_rates every tree of ancestral.json also carries the
        mixture used ('rates', 'weights', and 'alpha' / 'pinv' where fitted) and 'site_rates' (phylo_amd.ancestral.summarise_rates'
        numbers), and site_rates.tsv holds every site's posterior mean rate and category posteriors (write_site_rates)"""
        import json
        import os
        from . import ancestral as anc
        taxa = [str(t) for t in self.taxa]
        records, trees = [], []
        nn = lambda a: [None if x != x else float(x) for x in a]           # NaN (a node without a usable site) is null in JSON
        for t, child, nw, ll, state, pmax in zip(res['trees'], res['child'], res['newicks'], res['loglik'], res['state'], res['pmax']):
            records += anc.fasta_records(state, child, taxa, tree=t)
            sm = anc.summarise(pmax)
            trees.append({'tree': t, 'newick': nw, 'loglik': ll,
                          'nodes': [{'node': self.N + i, 'clade': cl, 'mean_pmax': m, 'share_below_0.9': sh, 'n_nan': int(k)}
                                    for i, (cl, m, sh, k) in enumerate(zip(anc.node_clades(child, taxa), nn(sm['mean_pmax']),
                                                                           nn(sm['share_below']), sm['n_nan']))]})
        if res.get('catpost') is not None:                 # (absent without --score_ancestral_rates)
            sr = anc.summarise_rates(res['siterate'], res['catpost'])
            for k, tree in enumerate(trees):
                tree['rates'], tree['weights'] = [float(x) for x in res['rates'][k]], [float(x) for x in res['weights'][k]]
                if res['alpha'] is not None:
                    tree['alpha'] = res['alpha'][k]
                if res['pinv'] is not None:
                    tree['pinv'] = res['pinv'][k]
                tree['site_rates'] = {'mean_rate': nn([sr['mean_rate'][k]])[0], 'quantile_levels': list(sr['q']),
                                      'quantiles': nn(sr['quantiles'][k]), 'category_share': nn(sr['cat_share'][k]),
                                      'n_nan': int(sr['n_nan'][k])}
            anc.write_site_rates(os.path.join(save_dir, 'site_rates.tsv'), res['trees'], res['siterate'], res['catpost'])
        anc.write_fasta(os.path.join(save_dir, 'ancestral.fa'), records)
        with open(os.path.join(save_dir, 'ancestral.json'), 'w') as f:
            json.dump({'trees': trees}, f, indent=1)

    def _save_results(self, save_dir, initial, history):
        """run_parameters.txt and results.p with the reference's keys (vcsmc.py:503-516, 618-642); no plots."""
        import os
        import pickle
        os.makedirs(save_dir, exist_ok=True)
        with open(os.path.join(save_dir, "run_parameters.txt"), "w") as rp:
            rp.write('Initial evaluation of ELBO : ' + str(initial) + '\n')
            for key, v in vars(self.args).items():
                if key in ('tree_branches', 'score_trees', 'score_rates', 'tree_tests', 'tree_tests_au', 'score_opt', 'score_fit', 'score_search', 'score_fit_search', 'score_model_fit', 'score_ancestral', 'score_ancestral_rates') and not v:   # (off: the file is what it was before the flag existed)
                    continue
                rp.write(str(key) + ' : ' + str(v) + '\n')
            rp.write(str(getattr(self, 'optimizer', '')))
        elbos = np.asarray(history['cost'])
        best = int(np.argmax(elbos)) if len(elbos) else 0
        resultDict = {'cost': elbos, 'nParticles': self.K, 'nTaxa': self.N, 'lr': self.lr,
                      'log_weights': np.asarray(history['log_weights']), 'Qmatrices': np.asarray(history['Qmatrices']),
                      'left_branches': history['left_branches'], 'right_branches': history['right_branches'],
                      'log_lik': np.asarray(history['log_lik']), 'll_tilde': np.asarray(history['ll_tilde']),
                      'log_lik_R': np.asarray(history['log_lik_R']),
                      'jump_chain_evolution': history['jump_chain_evolution'], 'best_epoch': best,
                      'best_log_lik': history['log_lik_R'][best] if len(elbos) else None,
                      'best_jump_chain': history['jump_chain_evolution'][best] if len(elbos) else None,
                      'best_newick': history['newick'][best] if len(elbos) else None}
        with open(os.path.join(save_dir, 'results.p'), 'wb') as f:
            pickle.dump(resultDict, f)
        return resultDict

    def train(self, epochs=100, batch_size=128, learning_rate=0.001, memory_optimization='on', save_dir='auto'):
        """vcsmc.py:466-645: per epoch, one optimiser step per site minibatch (all slices but the last,
        vcsmc.py:533), then the full-S evaluation sweep the reference reports (vcsmc.py:538-551); same printed
        lines and result artefacts (results/<dataset>/<nested>/<K>/<timestamp>/{run_parameters.txt,results.p};
        save_dir=None to skip; no plots).  Returns the per-epoch ELBOs."""
        self.lr = learning_rate
        data_view = np.broadcast_to(self.genome_NxSxA, (1,) + self.genome_NxSxA.shape)
        slices = self.batch_slices(data_view, batch_size)
        print('================= Dataset shape: KxNxSxA =================')
        print((self.K, self.N, self.S, self.A))
        print('==========================================================')
        ctx = self._context()                              # fixes the device (and joins the ranks when --n_gpus > 1)
        world, rank = getattr(self, '_world', 1), getattr(self, '_rank', 0)
        # --train_parallel replicas (the default with --n_gpus > 1): data-parallel training -- on every minibatch each rank sweeps
        # its OWN K-particle system(s) (own seeds) on its own GPU and the optimiser steps on the mean of all gradients, i.e.
        # world x grad_samples independent ELBO samples per step.  redundant: every rank takes the identical step.
        # sharded: ONE K-particle system per step split over the ranks (same seeds everywhere), every rank the same gradient bits.
        mode = str(getattr(self.args, 'train_parallel', 'replicas') or 'replicas')
        replicas = world > 1 and mode == 'replicas'
        sharded = world > 1 and mode == 'sharded'
        n_local = max(1, int(getattr(self.args, 'grad_samples', 1) or 1))   # particle systems per step and rank
        if world > 1:
            # all ranks must train on the SAME site minibatches; python's
            # global RNG (unseeded, like the reference) differs from process to process: rank 0's slices are everybody's
            flat = ctx.comm_allgather_blob(np.asarray(sum(slices, []), dtype=np.int32))[0]
            cuts = np.cumsum([len(sl) for sl in slices])[:-1]
            slices = [[int(v) for v in part] for part in np.split(flat, cuts)]
        self.optimizer = train_mod.make_optimizer(getattr(self.args, 'optimizer', ''), self.lr)   # vcsmc.py:488-491
        nested = bool(getattr(self.args, 'nested', False))
        trainer = None
        # --grad_batched true: the n_local systems of a step share one batched sweep and one reverse pass (train.Trainer, batched)
        batched = n_local if bool(getattr(self.args, 'grad_batched', False)) and n_local > 1 else 1
        if len(slices) > 1:
            trainer = train_mod.Trainer(self.genome_NxSxA, self.K, self.variables, self.optimizer, len(slices[0]),
                                        device=self._device, nested=nested, M=self.M, shard_with=ctx if sharded else None,
                                        batched=batched)
        initial = self.sample_phylogenies()
        print('===================\nInitial evaluation of ELBO:', round(initial, 3))
        print('Initial jump chain:')
        print(self.jump_chains[0])
        print('===================')
        print('Training begins --')
        elbos = []
        hist = {k: [] for k in ('cost', 'log_weights', 'Qmatrices', 'left_branches', 'right_branches', 'log_lik', 'll_tilde',
                                'log_lik_R', 'jump_chain_evolution', 'newick')}
        self.minibatch_costs = []
        try:
            for i in range(epochs):
                bt = datetime.now()
                if trainer is not None:
                    for j in range(len(slices) - 1):                       # vcsmc.py:533 (the last slice is never used)
                        seed = self.seed + self._sweeps
                        self._sweeps += 1
                        # sample i of the step (i = rank * grad_samples + g when the ranks train as replicas) draws from seed + i 2^32:
                        # seeds are 64-bit, so 2 ranks x 1 sample and 1 rank x 2 samples are the same training run bit for bit
                        first = rank * n_local if replicas else 0
                        seeds = [seed + ((first + g) << 32) for g in range(n_local)]
                        self.minibatch_costs.append(trainer.step(slices[j], seeds[0], seeds[1:], ctx if replicas else None))
                    self._sync_from_variables()
                elbo = self.sample_phylogenies()
                best_k = int(np.argmax(self.log_likelihood_R))
                for key, val in (('cost', elbo), ('log_weights', self.log_weights), ('Qmatrices', self.Qmatrix),
                                 ('left_branches', self.left_branches), ('right_branches', self.right_branches),
                                 ('log_lik', self.log_likelihood), ('ll_tilde', self.log_likelihood_tilde),
                                 ('log_lik_R', self.log_likelihood_R), ('jump_chain_evolution', self.jump_chains),
                                 ('newick', self.newick(best_k))):
                    hist[key].append(val)
                print('Epoch', i + 1)
                print('ELBO\n', round(elbo, 3))
                print('Stationary probabilities\n', self.stationary_probs)
                print('Q-matrix\n', self.Qmatrix)
                print('LB param:\n', self.left_branches_param)
                print('RB param:\n', self.right_branches_param)
                elbos.append(elbo)
                at = datetime.now()
                print('Time spent\n', at - bt, '\n-----------------------------------------')
        finally:
            if trainer is not None:
                trainer.close()
        print("Done training.")
        self.elbos = np.asarray(elbos)
        # --tree_summary: the final evaluation sweep's tree posterior (a collective when sharded: every rank summarises)
        self.posterior = None
        if getattr(self.args, 'tree_summary', False):
            self.posterior = self.tree_posterior(branch_lengths=bool(getattr(self.args, 'tree_branches', False)))
        scores = None
        if getattr(self.args, 'score_trees', None):        # --score_trees: explicit trees under the final model
            scores = self._tree_scores(self.args.score_trees)
        if save_dir is not None and getattr(self, '_rank', 0) == 0:   # sharded: every rank holds the same results; rank 0 writes
            if save_dir == 'auto':                   # vcsmc.py:504-507
                tm = str(datetime.now())
                save_dir = './results/' + str(getattr(self.args, 'dataset', 'data')) + '/' + str(getattr(self.args, 'nested', False)) + \
                    '/' + str(getattr(self.args, 'n_particles', self.K)) + '/' + (tm[:10] + '-' + tm[11:13] + tm[14:16] + tm[17:19]) + '/'
            self.results = self._save_results(save_dir, initial, hist)
            if self.posterior is not None:
                self.posterior.write(save_dir)             # tree_posterior.json, consensus.tre
                if getattr(self.args, 'tree_branches', False):
                    self.posterior.write_branches(save_dir)    # consensus_bl.tre, map.tre, tree_branches.json
            if scores is not None:
                import json
                import os
                with open(os.path.join(save_dir, 'tree_scores.json'), 'w') as f:
                    json.dump(scores, f, indent=1)
                if getattr(self, 'trees_ml', None) is not None:
                    with open(os.path.join(save_dir, 'trees_ml.nwk'), 'w') as f:
                        f.write('\n'.join(self.trees_ml) + '\n')
                if getattr(self, 'model_ml', None) is not None:
                    with open(os.path.join(save_dir, 'model_ml.json'), 'w') as f:
                        json.dump(self.model_ml, f, indent=1)
                if getattr(self, 'trees_search', None) is not None:
                    with open(os.path.join(save_dir, 'trees_search.nwk'), 'w') as f:
                        f.write('\n'.join(self.trees_search) + '\n')
                if getattr(self, 'tree_test_results', None) is not None:
                    with open(os.path.join(save_dir, 'tree_tests.json'), 'w') as f:
                        json.dump(self.tree_test_results, f, indent=1)
                if getattr(self, 'ancestral_results', None) is not None:
                    self._save_ancestral(save_dir, self.ancestral_results)
            self.save_dir = save_dir
            print("Finished...")
        return self.elbos
