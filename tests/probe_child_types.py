#!/usr/bin/env python3
"""What the merges of a workload's sweeps merge -- no GPU: the C oracle's sweeps replayed through the root tables' leaf counts
(cpu_ref.extend_partial_state gives the slots that remain), every merge classed by its two children.  A child with one leaf is a
coded leaf (pk_rank_merge_nostore reads its codes), one with two a cherry.  Run by tools/child_types.sh:
    python tests/probe_child_types.py [--dataset primate_data] [--K 2048] [--seeds 0 1 2]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import c_oracle as CO                          # noqa: E402
from oracle import cpu_ref as O                            # noqa: E402
from phylo_amd.datasets import load_dataset                # noqa: E402


def child_counts(g, Q, pi, lam, K, seed):
    """[R][K][2] leaf counts of the two children of every merge of one sweep"""
    N = g.shape[0]
    out = CO.sweep(g, Q, pi, lam, lam, K, seed)
    record = np.ones((K, N), dtype=np.int64)
    ar = np.arange(K)
    counts = np.zeros((N - 1, K, 2), dtype=np.int64)
    for r in range(N - 1):
        if r > 0:
            record = record[out['ancestors'][r - 1]]
        coalesced, remaining, _ = O.extend_partial_state(K, N - r, seed, r)
        assert np.array_equal(coalesced, out['merges'][r])
        counts[r, :, 0] = record[ar, coalesced[:, 0]]
        counts[r, :, 1] = record[ar, coalesced[:, 1]]
        record = np.concatenate([record[ar[:, None], remaining], counts[r].sum(axis=1)[:, None]], axis=1)
    return counts


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--dataset', default='primate_data')
    p.add_argument('--K', type=int, default=2048)
    p.add_argument('--seeds', type=int, nargs='+', default=[0, 1, 2])
    a = p.parse_args()
    g = load_dataset(a.dataset)['genome']
    N, S, _ = g.shape
    Q, pi, lam = O.get_Q(O.init_y_q()), np.full((1, 4), 0.25), np.full(N - 1, 10.0)
    c = np.concatenate([child_counts(g, Q, pi, lam, a.K, s) for s in a.seeds], axis=1)
    leaf = c == 1
    n = float(leaf[..., 0].size)
    print("%s %d x %d, GTR-init, K = %d, seeds %s: %d merges" % (a.dataset, N, S, a.K, a.seeds, int(n)))
    print("| Quantity | Share |\n|---|---|")
    for what, v in (("Child slots that are coded leaves", leaf.mean()),
                    ("Merges leaf x leaf", (leaf[..., 0] & leaf[..., 1]).sum() / n),
                    ("Merges leaf x internal", (leaf[..., 0] ^ leaf[..., 1]).sum() / n),
                    ("Merges internal x internal", (~leaf[..., 0] & ~leaf[..., 1]).sum() / n),
                    ("Child slots that are cherries", (c == 2).mean())):
        print("| %s | %.1f %% |" % (what, 100.0 * v))
    print("leaf x leaf by rank event: " + " ".join("%.2f" % x for x in (leaf[..., 0] & leaf[..., 1]).mean(axis=1)))


if __name__ == "__main__":
    main()
