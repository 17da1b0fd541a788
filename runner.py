#!/usr/bin/env python3
"""runner.py -- the reference's CLI (runner.py:12-58, 61-212) over the MI355X library.

Same flags and defaults.  Differences: datasets come from an explicit table
(phylo_amd/datasets.py) instead of `exec(args.dataset + ' = True')`; `--twisting` is accepted as an alias of
`--nested` (the reference's README advertises it, its parser lacks it); `--seed`, `--n_gpus`, `--train_parallel`,
`--grad_samples`, `--grad_batched`, `--tree_summary`, `--tree_branches`, `--score_trees`, `--score_rates`, `--score_opt`, `--score_fit`, `--score_search`, `--score_fit_search`, `--score_model_fit`, `--score_ancestral`, `--score_ancestral_rates`, `--tree_tests`, `--tree_tests_au` and `--ambiguity` (default: the reference's KeyError on characters such as DS7's 'N'; `iupac`
encodes them) are new.
"""
import argparse
import sys

import numpy as np


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Variational Combinatorial Sequential Monte Carlo')
    parser.add_argument('--dataset', help='benchmark dataset to use.', default='primate_data')
    parser.add_argument('--n_particles', type=int, help='number of SMC samples.', default=10)
    parser.add_argument('--batch_size', type=int, help='number of sites on genome per batch.', default=256)
    parser.add_argument('--learning_rate', type=float, help='Learning rate.', default=0.001)
    parser.add_argument('--num_epoch', type=int, help='number of epoches to train.', default=100)
    parser.add_argument('--optimizer', type=str, help='Optimizer for Training', default='GradientDescentOptimizer')
    parser.add_argument('--branch_prior', type=float, help='Hyperparameter for branch length initialization.',
                        default=np.log(10))
    parser.add_argument('--M', type=int, help='number of subparticles to compute look-ahead particles', default=10)
    parser.add_argument('--nested', default=False, type=lambda x: (str(x).lower() == 'true'))
    parser.add_argument('--twisting', default=None, type=lambda x: (str(x).lower() == 'true'),
                        help='alias of --nested (README.md:28 of the reference)')
    parser.add_argument('--jcmodel', default=False, type=lambda x: (str(x).lower() == 'true'))
    parser.add_argument('--memory_optimization', help='Use memory optimization?', default='on')
    parser.add_argument('--seed', type=int, default=0, help='seed of the counter-based RNG contract')
    parser.add_argument('--n_gpus', type=int, default=1,
                        help='one process per GPU (python -m torch.distributed.run --nproc-per-node N runner.py --n_gpus N ...): the '
                             'particles of the EVALUATION sweeps are sharded over the ranks (global resampling, same bits as one GPU); '
                             'training: see --train_parallel')
    parser.add_argument('--train_parallel', choices=('replicas', 'redundant', 'sharded'), default='replicas',
                        help='with --n_gpus N > 1: replicas = data-parallel training, every rank sweeps its own n_particles-particle '
                             'system per minibatch (own seed) and the optimiser steps on the mean gradient of the N ranks; '
                             'redundant = every rank takes the identical step (equals the one-process run bit for bit); '
                             'sharded = ONE n_particles-particle system per minibatch split over the ranks, its reverse pass on every '
                             'rank over the gathered genealogy (plain proposal only)')
    parser.add_argument('--grad_samples', type=int, default=1,
                        help='independent particle systems swept per optimiser step (and per rank with --train_parallel replicas); the '
                             'step is taken on their mean gradient')
    parser.add_argument('--grad_batched', default=False, type=lambda x: (str(x).lower() == 'true'),
                        help='with --grad_samples G > 1: the G particle systems of a step share ONE batched sweep and ONE reverse pass '
                             '(every rank batches its own G systems under --train_parallel replicas) instead of G sweep-and-reverse-pass '
                             'pairs one after the other; same seeds, same sweeps, gradients equal to rounding.  Plain proposal, not '
                             'with --train_parallel sharded')
    parser.add_argument('--ambiguity', choices=('error', 'iupac'), default='error',
                        help="characters outside the dataset's alphabet: KeyError like the reference, or IUPAC indicator rows")
    parser.add_argument('--tree_summary', default=False, type=lambda x: (str(x).lower() == 'true'),
                        help="after training, summarise the final evaluation sweep's tree posterior (clade supports, topology "
                             "probabilities, majority-rule consensus) into tree_posterior.json and consensus.tre in the results directory")
    parser.add_argument('--tree_branches', default=False, type=lambda x: (str(x).lower() == 'true'),
                        help="with --tree_summary true: also the branch lengths of that posterior (mean, sd, min, max above every "
                             "clade and leaf) into tree_branches.json, consensus_bl.tre (consensus with mean lengths) and map.tre "
                             "(the most probable topology with its mean lengths)")
    parser.add_argument('--score_trees', default=None, metavar='FILE',
                        help="a file of rooted Newick trees over the dataset's taxon names, one per line, every branch with its "
                             "length: after training, their log-likelihoods under the final model (with the model's stationary "
                             "distribution at the root) go into tree_scores.json in the results directory, with the index of the "
                             "best one; with --tree_branches true also the scores of map.tre, consensus_bl.tre and the ten most "
                             "probable topologies at their mean branch lengths")
    parser.add_argument('--score_rates', default=None, metavar='gamma:ALPHA:C[:PINV]',
                        help="with --score_trees: score under among-site rate variation -- C discrete Gamma categories of shape "
                             "ALPHA (Yang 1994, mean rates), and with PINV > 0 a class of invariant sites of that proportion (the "
                             "rates of the variable sites are not rescaled); every score in tree_scores.json is then under that "
                             "model, and the file names its rates and weights")
    parser.add_argument('--score_opt', default=False, type=lambda x: (str(x).lower() == 'true'),
                        help="with --score_trees: first climb every tree's branch lengths to their maximum-likelihood values "
                             "(phylo_trees_grad on the device, phylo_amd/treeopt.py); writes trees_ml.nwk (the trees at those "
                             "lengths), adds loglik_ml, iterations and converged to every tree of tree_scores.json, and gives "
                             "--tree_tests the site likelihoods at those lengths.  Not with --score_rates: under a rate model "
                             "--score_fit does this")
    parser.add_argument('--score_fit', default=None, choices=['branches', 'branches+alpha', 'branches+alpha+pinv'],
                        help="with --score_trees and --score_rates: climb every tree's branch lengths to their maximum-likelihood "
                             "values UNDER that rate model (phylo_trees_grad_rates on the device), and with +alpha (+pinv) also "
                             "every tree's own Gamma shape (and share of invariant sites), starting from the model's values; "
                             "writes trees_ml.nwk, adds loglik_ml, iterations, converged (and alpha, pinv where fitted) to every "
                             "tree of tree_scores.json, and gives --tree_tests the site likelihoods at the fitted values.  Not "
                             "with --score_opt true")
    parser.add_argument('--score_search', default=None, metavar='nni[:ROUNDS]',
                        help="with --score_trees and --score_opt true: after the climb, hill-climb every tree over nearest-neighbour "
                             "interchanges (phylo_trees_nni on the device, phylo_amd/treesearch.py), at most ROUNDS rounds (default "
                             "20); writes trees_search.nwk (the trees found), adds loglik_search, nni_moves and search_rounds to "
                             "every tree of tree_scores.json, and gives --tree_tests the site likelihoods of the trees found.  Not "
                             "with --score_rates or --score_fit: --score_fit_search does this under a rate model")
    parser.add_argument('--score_model_fit', default=None, choices=['q', 'q+pi'],
                        help="with --score_trees and --score_opt true: fit ONE substitution model for all trees by climbing the "
                             "log-likelihood -- the row-softmax Q (q), and the root distribution too (q+pi) -- on the best tree, "
                             "together with every tree's branch lengths (phylo_trees_grad_model).  Writes model_ml.json (Q, pi, "
                             "y_q, y_station, fit_on, rounds, the objective before and after); loglik_ml of tree_scores.json, "
                             "trees_ml.nwk and the site likelihoods of --tree_tests are then under the fitted model.  Not with "
                             "--score_rates, --score_fit or --score_search.  CAVEAT: under the project's pruning convention (a message is x.M) the "
                             "site factors of an asymmetric Q are not probabilities and the climb ends on the boundary of the "
                             "softmax: the fitted model is NOT a maximum-likelihood estimate of a substitution model, and tree tests "
                             "under it are tests under a degenerate model (DESIGN.md section 13c)")
    parser.add_argument('--score_fit_search', default=None, metavar='nni[:ROUNDS]',
                        help="with --score_trees, --score_rates and --score_fit: after the fit, hill-climb every tree over "
                             "nearest-neighbour interchanges UNDER the rate model (phylo_trees_nni_rates on the device), every tree "
                             "with its own fitted alpha (and p_inv) held fixed, at most ROUNDS rounds (default 20), then fit the "
                             "trees found once more; writes trees_search.nwk, adds loglik_search, nni_moves and search_rounds (and "
                             "alpha_search, pinv_search where fitted) to every tree of tree_scores.json, and gives --tree_tests the "
                             "site likelihoods of the trees found")
    parser.add_argument('--score_ancestral', default=None, type=int, metavar='K',
                        help="with --score_trees: reconstruct the marginal ancestral states of the K best trees by their final score "
                             "(K >= 1; phylo_trees_ancestral on the device), at the final lengths and model (after --score_opt, "
                             "--score_search and --score_model_fit where given); writes ancestral.fa (one record per internal node, "
                             "'>tree{t}_node{n} clade=a,b,c', the most probable state of every site as a letter, '?' where a site "
                             "has none) and ancestral.json (per tree its index, its Newick string and per node the mean posterior "
                             "of the most probable state and the share of sites below 0.9).  Not with --score_rates, --score_fit "
                             "or --score_fit_search")
    parser.add_argument('--score_ancestral_rates', default=None, type=int, metavar='K',
                        help="with --score_trees and --score_rates: --score_ancestral UNDER the rate model "
                             "(phylo_trees_ancestral_rates on the device) -- the K best trees by their final score (after --score_fit "
                             "and --score_fit_search where given), every tree under its own final mixture (the fitted alpha and "
                             "p_inv where --score_fit gave them); writes ancestral.fa and ancestral.json as --score_ancestral does "
                             "(ancestral.json also carries per tree the mixture used -- rates, weights, and alpha / pinv where "
                             "fitted -- and the mean and quantiles of the posterior mean site rate and the share of sites per most "
                             "probable category) and site_rates.tsv (tree, site, rate, cat, p0 .. p{C-1}: the empirical-Bayes rate "
                             "of every site, its most probable category and every category's posterior).  Not with --score_ancestral")
    parser.add_argument('--tree_tests', default=None, metavar='B[:SEED]',
                        help="with --score_trees: which of those trees are significantly worse than the best one?  A RELL bootstrap "
                             "of B replicates (seed SEED, default 0) over the site likelihoods of that scoring call (under "
                             "--score_rates if given) writes tree_tests.json beside tree_scores.json: per tree the observed score, "
                             "the bootstrap proportion, the p-values of the KH and SH tests and the expected likelihood weight")
    parser.add_argument('--tree_tests_au', default=None, metavar='default|r1,r2,...',
                        help="with --tree_tests: also Shimodaira's approximately unbiased (AU) test, from a multiscale RELL bootstrap "
                             "on the same site likelihoods, B and SEED -- B replicates of r_k S sites at every scale r_k "
                             "('default': 0.5, 0.6, ..., 1.4); adds p_au, se_au, au_d, au_c, au_ok, au_scales and bp_scales to "
                             "tree_tests.json")
    args = parser.parse_args(argv)
    if args.tree_tests_au is not None:
        if args.tree_tests is None:
            parser.error('--tree_tests_au needs --tree_tests B[:SEED] (it adds the AU test to the tests made there)')
        from phylo_amd import treetests
        try:
            treetests.au_ratios(args.tree_tests_au)
        except ValueError as e:
            parser.error('--tree_tests_au: %s' % e)
    if args.score_fit_search is not None:
        kind, _, rounds = str(args.score_fit_search).partition(':')
        if kind != 'nni' or (rounds and not (rounds.isdigit() and int(rounds) >= 1)):
            parser.error('--score_fit_search: nni or nni:ROUNDS with ROUNDS >= 1, not %r' % args.score_fit_search)
        if not args.score_trees or args.score_rates is None or args.score_fit is None:
            parser.error('--score_fit_search needs --score_trees, --score_rates and --score_fit (it searches from the trees fitted '
                         'there, under their fitted rate models)')
        args.score_fit_search = ('nni', int(rounds) if rounds else 20)
    if args.tree_tests is not None:
        if not args.score_trees:
            parser.error('--tree_tests needs --score_trees FILE (it tests the trees scored there)')
        from phylo_amd import treetests
        try:
            treetests.parse_spec(args.tree_tests)
        except ValueError as e:
            parser.error('--tree_tests: %s' % e)
    if args.score_rates is not None:
        if not args.score_trees:
            parser.error('--score_rates needs --score_trees FILE (it is the rate model those trees are scored under)')
        from phylo_amd import rates
        try:
            rates.parse_spec(args.score_rates)
        except ValueError as e:
            parser.error('--score_rates: %s' % e)
    if args.score_search is not None:
        kind, _, rounds = str(args.score_search).partition(':')
        if kind != 'nni' or (rounds and not (rounds.isdigit() and int(rounds) >= 1)):
            parser.error('--score_search: nni or nni:ROUNDS with ROUNDS >= 1, not %r' % args.score_search)
        if args.score_rates is not None or args.score_fit is not None:
            parser.error('--score_search nni: the NNI neighbourhood is not built for rate mixtures (not with --score_rates or '
                         '--score_fit); --score_fit_search nni searches under the rate model')
        if not args.score_trees or not args.score_opt:
            parser.error('--score_search needs --score_trees and --score_opt true (it searches from the trees scored there, at '
                         'their maximum-likelihood lengths)')
        args.score_search = ('nni', int(rounds) if rounds else 20)
    if args.score_opt:
        if not args.score_trees:
            parser.error('--score_opt true needs --score_trees FILE (it optimises the branch lengths of the trees scored there)')
        if args.score_rates is not None:
            parser.error('--score_opt true: the one-rate branch-length gradient is not built for rate mixtures (not with '
                         '--score_rates); --score_fit branches climbs the lengths under the rate model')
    if args.score_model_fit is not None:
        if args.score_rates is not None or args.score_fit is not None:
            parser.error('--score_model_fit: the model gradient is not built for rate mixtures (not with --score_rates or --score_fit)')
        if args.score_search is not None:
            parser.error('--score_model_fit: the NNI search runs under the model given, not a fitted one (not with --score_search)')
        if not args.score_trees or not args.score_opt:
            parser.error('--score_model_fit needs --score_trees and --score_opt true (it fits the model on the trees scored there, '
                         'at their maximum-likelihood branch lengths)')
    if args.score_fit is not None:
        if not args.score_trees or args.score_rates is None:
            parser.error('--score_fit needs --score_trees FILE and --score_rates gamma:ALPHA:C[:PINV] (it fits the trees scored there '
                         'under that rate model, from its values)')
        if args.score_opt:
            parser.error('--score_fit and --score_opt true exclude one another (--score_fit branches is --score_opt under the rate model)')
        if 'alpha' in args.score_fit and rates.parse_spec(args.score_rates)['C'] < 2:
            parser.error('--score_fit %s: one category has no shape to fit (--score_rates with C >= 2)' % args.score_fit)
    if args.score_ancestral is not None:
        if args.score_ancestral < 1:
            parser.error('--score_ancestral: K >= 1 trees to reconstruct, not %d' % args.score_ancestral)
        if not args.score_trees:
            parser.error('--score_ancestral needs --score_trees FILE (it reconstructs the best of the trees scored there)')
        if args.score_ancestral_rates is not None:
            parser.error('--score_ancestral_rates and --score_ancestral exclude one another (one rate, or the rate model)')
        if args.score_rates is not None or args.score_fit is not None or args.score_fit_search is not None:
            parser.error('--score_ancestral: the ancestral posteriors are not built for rate mixtures (not with --score_rates, '
                         '--score_fit or --score_fit_search); use --score_ancestral_rates K')
    if args.score_ancestral_rates is not None:
        if args.score_ancestral_rates < 1:
            parser.error('--score_ancestral_rates: K >= 1 trees to reconstruct, not %d' % args.score_ancestral_rates)
        if not args.score_trees:
            parser.error('--score_ancestral_rates needs --score_trees FILE (it reconstructs the best of the trees scored there)')
        if args.score_rates is None:
            parser.error('--score_ancestral_rates needs --score_rates gamma:ALPHA:C[:PINV] (it reconstructs under that rate model; '
                         'under one rate --score_ancestral does this)')
    if args.tree_branches and not args.tree_summary:
        parser.error('--tree_branches true needs --tree_summary true (it adds branch lengths to that summary)')
    if args.twisting is not None:
        args.nested = args.twisting
    if args.train_parallel == 'sharded' and args.nested:
        parser.error('--train_parallel sharded trains the plain proposal only: the reverse pass of a twisted sweep needs the '
                     'whole particle system on one GPU (use --train_parallel replicas or redundant with --nested true)')
    if args.grad_batched and args.nested:
        parser.error('--grad_batched true batches the plain proposal only: not with --nested true (the twisted proposal trains '
                     'its --grad_samples systems one after the other)')
    if args.grad_batched and args.train_parallel == 'sharded':
        parser.error('--grad_batched true needs every particle system whole on one GPU: not with --train_parallel sharded (use '
                     '--train_parallel replicas or redundant)')
    return args


def main(argv=None):
    args = parse_args(argv)
    from phylo_amd.datasets import load_dataset
    from phylo_amd.vcsmc import VCSMC
    datadict = load_dataset(args.dataset, ambiguity=args.ambiguity)
    vcsmc = VCSMC(datadict, K=args.n_particles, args=args)
    from phylo_amd.treeopt import OutOfRangeError
    try:
        return vcsmc.train(epochs=args.num_epoch, batch_size=args.batch_size, learning_rate=args.learning_rate,
                           memory_optimization=args.memory_optimization)
    except OutOfRangeError as e:                           # --score_opt / --score_fit on a tree that cannot be climbed: a message, no traceback
        flag = '--score_fit' if args.score_fit else '--score_opt'
        sys.exit("runner.py %s: %s (trees are numbered from 0 in the order of %s; score it without %s, "
                 "or give it branch lengths under which every site has a likelihood above 2^-1020)"
                 % (flag, e, args.score_trees, '--score_fit' if args.score_fit else '--score_opt true'))


if __name__ == "__main__":
    main()
