"""stats.n_launches of phylo_tree_summary and phylo_tree_branches equals what the plan (phylo_trees_plan.h, through
debug_tree_plan) says, at the smallest shapes where the count changes: L = 1, one bitset word, a batch, two and three words."""
import pytest

from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset, synthetic_alignment
from test_gpu_tree_summary import make_ctx

pytestmark = pytest.mark.gpu


def genome(N):
    return load_dataset('primate_data_wang')['genome'] if N is None else synthetic_alignment(N, 40, seed=N)['genome']


@pytest.mark.parametrize("N,K,G,summary_launches", [
    (3, 64, 1, 28),       # L = 1: one clade entry per particle
    (None, 64, 1, 28),    # primates_small, N = 9
    (None, 256, 4, 36),   # ... as a batch of 4 x 64: the four group passes
    (70, 64, 1, 30),      # W = 2
    (130, 16, 1, 32),     # W = 3
])
def test_launch_counts_equal_the_plan(N, K, G, summary_launches):
    g = genome(N)
    N = g.shape[0]
    ctx = make_ctx(g, K)
    if G > 1:
        ctx.sweep_batch_async([11 * (i + 1) for i in range(G)])
    else:
        ctx.sweep(7)
    tab = ctx.tree_summary()
    br = ctx.tree_branches(tab)
    ctx.close()
    plan = _ffi.debug_tree_plan(N, K, G=G, n_clades=len(tab['clade_weight']), n_topologies=len(tab['topo_weight']))
    print("N=%d K=%d G=%d: summary %d (plan %d), branches %d (plan %d)"
          % (N, K, G, tab['summary_launches'], plan['summary_launches'], br['branches_launches'], plan['branches_launches']))
    assert tab['summary_launches'] == plan['summary_launches'] == summary_launches
    assert br['branches_launches'] == plan['branches_launches'] == 11
    assert tab['G'] == G
