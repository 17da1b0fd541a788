"""The reverse pass of a batched sweep treats its G particle systems as ONE K-particle genealogy with global indices in which
adoption never crosses a group.  No GPU: the index convention the device builders must meet (phylo_revlists_dev.h adds g K/G to
the group-local ancestors) is pinned on the host builders through phylo_debug_reverse_lists -- the lists of the block-diagonal
genealogy are, entry by entry, the per-group lists shifted by g K/G; the plan of the batched pass; the runner's refusals."""
import numpy as np
import pytest

import runner
from phylo_amd import _ffi
from tests.test_revlists_cpu import _random_genealogy

FREE = 1 << 30


def _block_diagonal(N, Kg, groups):
    """groups: [(anc [N-2][Kg], child [N-1][Kg][2])] -> the K = G Kg genealogy with global particle and node indices"""
    R, G = N - 1, len(groups)
    K = G * Kg
    anc = np.zeros((max(R - 1, 0), K), dtype=np.int64)
    child = np.zeros((R, K, 2), dtype=np.int32)
    for g, (a, c) in enumerate(groups):
        anc[:, g * Kg:(g + 1) * Kg] = a + g * Kg
        c = c.astype(np.int64)
        rp, kp = (c - N) // Kg, (c - N) % Kg
        child[:, g * Kg:(g + 1) * Kg] = np.where(c >= N, N + rp * K + g * Kg + kp, c)
    return anc, child


def _shift_entry(e, Kg, K, g):
    """a parent entry (node * 2 + side | FREE) of group g's own lists as an entry of the whole genealogy"""
    free, e = e & FREE, e & (FREE - 1)
    node, side = e >> 1, e & 1
    r, k = node // Kg, node % Kg
    return ((r * K + g * Kg + k) * 2 + side) | free


@pytest.mark.parametrize("N,Kg,G,survivors,early,seed", [
    (3, 4, 2, 2, True, 0), (6, 32, 3, 3, True, 1), (6, 64, 5, 64, True, 2), (7, 50, 4, 5, True, 3), (8, 129, 2, 12, False, 4),
    (12, 256, 4, 4, True, 5), (5, 512, 20, 2, True, 6),
])
def test_block_diagonal_lists_are_the_groups_lists_shifted(N, Kg, G, survivors, early, seed):
    rng = np.random.default_rng(seed)
    R, K = N - 1, G * Kg
    groups = [_random_genealogy(rng, N, Kg, survivors) for _ in range(G)]
    anc, child = _block_diagonal(N, Kg, groups)
    whole = _ffi.debug_reverse_lists(N, K, anc, child, early_free=early, rows_form=True)
    adp_whole = [whole['adp'][whole['ev_adp0'][r]:whole['ev_adp0'][r + 1]] for r in range(R)]
    slow_whole = [whole['slow_idx'][whole['ev_slow0'][r]:whole['ev_slow0'][r + 1]] for r in range(R)]
    for g, (a, c) in enumerate(groups):
        own = _ffi.debug_reverse_lists(N, Kg, a, c, early_free=early, rows_form=True)
        lo, hi = g * Kg, (g + 1) * Kg
        for r in range(1, R):
            # adopters: offsets and indices of the group's particles, both shifted by g Kg
            assert np.array_equal(whole['ad_off'][r, lo:hi + 1], own['ad_off'][r] + lo), (g, r)
            assert np.array_equal(whole['ad_idx'][r, lo:hi], own['ad_idx'][r] + lo), (g, r)
        for r in range(R):
            # the adopted particles and the flagged nodes of a rank event: the group's, in order, inside the rank event's run
            mine = adp_whole[r][(adp_whole[r] % K >= lo) & (adp_whole[r] % K < hi)]
            theirs = own['adp'][own['ev_adp0'][r]:own['ev_adp0'][r + 1]]
            assert np.array_equal(mine, r * K + lo + theirs % Kg), (g, r)
            mine = slow_whole[r][(slow_whole[r] % K >= lo) & (slow_whole[r] % K < hi)]
            theirs = own['slow_idx'][own['ev_slow0'][r]:own['ev_slow0'][r + 1]]
            assert np.array_equal(mine, r * K + lo + theirs % Kg), (g, r)
            for k in range(Kg):
                xo, xw = r * Kg + k, r * K + lo + k
                assert (whole['slow_flag'][xw] & 7) == (own['slow_flag'][xo] & 7), (g, r, k)
                assert (whole['heavy'][xw] >= 0) == (own['heavy'][xo] >= 0), (g, r, k)
                po = own['par_idx'][own['par_off'][xo]:own['par_off'][xo + 1]]
                pw = whole['par_idx'][whole['par_off'][xw]:whole['par_off'][xw + 1]]
                assert np.array_equal(pw, [_shift_entry(int(e), Kg, K, g) for e in po]), (g, r, k)
    # nothing crosses a group: every adopter list lies inside its group
    for r in range(1, R):
        for g in range(G):
            run = whole['ad_idx'][r, whole['ad_off'][r, g * Kg]:whole['ad_off'][r, (g + 1) * Kg]]
            assert run.size == Kg and run.min() >= g * Kg and run.max() < (g + 1) * Kg


def test_plan_of_a_batched_pass():
    """The device lists' limit is per group; every other limit sees the totals; one group is the plan of the single pass."""
    for N, K, S in ((8, 2048, 256), (12, 4096, 898), (6, 16384, 70), (27, 8192, 1949)):
        for sw in ((), ('rev_host_lists',), ('one_stream',), ('rows_chain', 'coeff_chain')):
            for n_slow, wgs in ((0, 0), (300, 900), (20000, 5000)):
                one = _ffi.debug_reverse_plan(N, K, S, switches=sw, n_slow=n_slow, coeff_wgs=wgs)
                assert _ffi.debug_reverse_plan_batch(N, K, 1, S, switches=sw, n_slow=n_slow, coeff_wgs=wgs)['mask'] == one['mask']
    # total K beyond one workgroup's sort, every group within it: the device builders apply
    assert not _ffi.debug_reverse_plan(5, 20 * 512, 40)['dev_lists']
    p = _ffi.debug_reverse_plan_batch(5, 20 * 512, 20, 40, n_slow=100, coeff_wgs=500)
    assert p['dev_lists'] and p['early_free'] and p['rows_all'] and p['coeff_all']
    assert not _ffi.debug_reverse_plan_batch(5, 2 * 16384, 2, 40)['dev_lists']            # K / G = 16384 > 8192
    assert not _ffi.debug_reverse_plan_batch(5, 20 * 512, 20, 40, switches=('rev_host_lists',))['dev_lists']
    # the one-launch chains keep their limits on the totals
    assert not _ffi.debug_reverse_plan_batch(5, 20 * 512, 20, 40, n_slow=100, coeff_wgs=2049)['coeff_all']
    assert not _ffi.debug_reverse_plan_batch(5, 20 * 512, 20, 40, n_slow=16385, coeff_wgs=500)['rows_all']
    with pytest.raises(_ffi.PhyloError):
        _ffi.debug_reverse_plan_batch(5, 100, 3, 40)                                     # K not divisible by G


def test_runner_refuses_batched_with_nested_or_sharded(capsys):
    assert runner.parse_args([]).grad_batched is False
    assert runner.parse_args(['--grad_samples', '3', '--grad_batched', 'true']).grad_batched is True
    for extra, word in ((['--nested', 'true'], '--nested'), (['--twisting', 'true'], '--nested'),
                        (['--train_parallel', 'sharded'], '--train_parallel sharded')):
        with pytest.raises(SystemExit) as e:
            runner.parse_args(['--grad_samples', '3', '--grad_batched', 'true'] + extra)
        assert e.value.code != 0
        err = capsys.readouterr().err
        assert '--grad_batched' in err and word in err


def test_trainer_refuses_batched_with_nested_or_sharded():
    """before any device work: the arguments alone decide"""
    from phylo_amd import train
    v = train.Variables(5, np.log(10.0), False)
    genome = np.ones((5, 8, 4))
    with pytest.raises(ValueError, match="batched"):
        train.Trainer(genome, 8, v, train.GradientDescent(0.01), 8, nested=True, batched=3)
    with pytest.raises(ValueError, match="batched"):
        train.Trainer(genome, 8, v, train.GradientDescent(0.01), 8, shard_with=object(), batched=3)
