"""What keeps tests/test_gpu_context_reuse.py from going vacuous, without a GPU: the walks of tests/context_reuse_cases.py take
every ordered pair they claim, the sweep's plan accepts every form at the walks' shape, the plan refuses what the refusals walk
expects it to, and the inputs discriminate by the oracle alone -- a context that answered from a stale cache (the previous leaves,
model or site tile) could not reproduce the right result by accident."""
import numpy as np
import pytest

import context_reuse_cases as C
from phylo_amd import _ffi


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_form_walk_takes_all_169_ordered_pairs():
    n = len(C.FORMS)
    assert n == 13 and len(C.REFERENCES) == 13 and len(set(C.NAMES)) == 13
    assert C.FORM_WALK[0] == C.FORM_WALK[-1] and len(C.FORM_WALK) == n * n + 1
    assert C.pairs_of(C.FORM_WALK) == {(a, b) for a in range(n) for b in range(n)}
    # the four quarters: consecutive, each begins on the form the one before ended on, together all the pairs once
    quarters = [C.form_walk_quarter(q) for q in range(4)]
    taken = []
    for q, steps in enumerate(quarters):
        forms = [f for f, _ in steps]
        if q:
            assert forms[0] == quarters[q - 1][-1][0]
        taken += list(zip(forms[:-1], forms[1:]))
        assert all(a[1] != b[1] for a, b in zip(steps[:-1], steps[1:])), "the seed changes at every step"
    assert len(taken) == n * n and set(taken) == C.pairs_of(C.FORM_WALK)


@pytest.mark.parametrize("walk,states", [(C.LEAVES_WALK, tuple(C.LEAF_STATES)), (C.MODEL_WALK, tuple(C.MODELS)), (C.TILE_WALK, C.TILES)])
def test_state_walks_take_every_ordered_pair(walk, states):
    assert C.pairs_of(walk) == {(a, b) for a in states for b in states}
    assert len(walk) == len(states) ** 2 + 1


def test_the_plan_accepts_every_form_and_refuses_the_refusals():
    assert len(C.FORMS) == 13
    for name, _, ask in C.FORMS:
        plan = _ffi.debug_sweep_plan(C.N, C.K, C.S, switches=('coded_leaves',), **ask)
        assert plan['launches'][0] >= 1, name
        assert plan['twist'] == bool(ask['flags'] & _ffi.TWISTING) and plan['graph'] == bool(ask['flags'] & _ffi.KEEP_GRAPH), name
        assert plan['batched'] == (ask['G'] > 1) or ask['flags'] & _ffi.ONE_LAUNCH, name
    # the shape takes the merge-record path, lazy nodes by default, and at tiles 64 and 128 a row has several tiles
    plain = _ffi.debug_sweep_plan(C.N, C.K, C.S, switches=('coded_leaves',), flags=C.DEFAULT)
    assert plain['use_rec'] and plain['lazy'] and C.K % 4 == 0
    assert all(-(-C.S // T) > 1 for T in C.TILES if T)
    for name, ask, _ in C.REFUSED_SWEEPS:
        with pytest.raises(_ffi.PhyloError) as e:
            _ffi.debug_sweep_plan(C.N, C.K, C.S, **ask)
        assert e.value.code == C.EINVAL, name


def test_leaf_states_discriminate():
    a, b = C.LEAVES['A'], C.LEAVES['B']
    assert (a != b).any() and (b.sum(axis=2) == 4).all(axis=0).sum() >= 9            # B has all-gap columns
    assert ((a == 0) | (a == 1)).all() and not ((C.LEAVES['generic'] == 0) | (C.LEAVES['generic'] == 1)).all()
    assert (C.LEAVES['A_broken'][2] != a[2]).any() and np.array_equal(np.delete(C.LEAVES['A_broken'], 2, 0), np.delete(a, 2, 0))
    i, seed = C.F['twisted_m3'], C.state_seed(C.F['twisted_m3'])                   # the form that reads the code-pair histogram
    ra, rb, rg = (C.reference(i, C.Env(s), seed) for s in ('A', 'B', 'generic'))
    assert (bits(ra['log_weights']) != bits(rb['log_weights'])).any()
    assert (bits(ra['log_weights']) != bits(rg['log_weights'])).any() and (bits(rb['log_weights']) != bits(rg['log_weights'])).any()
    assert C.reference(i, C.Env('A_restored'), seed) is ra                           # the same alignment: the same reference


def test_models_discriminate():
    i = C.F['plain']
    z = [float(C.reference(i, C.Env('A', m), C.state_seed(i))['logZ']) for m in C.MODELS]
    assert len(C.MODELS) == 3 and len(set(z)) == 3, z


def test_tiles_discriminate():
    i = C.F['plain']
    base = C.reference(i, C.Env('A', 'gtr_init', 0), C.state_seed(i))['log_weights']
    for T in (64, 128):
        assert (bits(C.reference(i, C.Env('A', 'gtr_init', T), C.state_seed(i))['log_weights']) != bits(base)).any(), T
    assert (bits(C.reference(i, C.Env('A', 'gtr_init', 64), C.state_seed(i))['log_weights'])
            != bits(C.reference(i, C.Env('A', 'gtr_init', 128), C.state_seed(i))['log_weights'])).any()


def _finite(d):
    return all(np.isfinite(np.asarray(d[k], dtype=np.float64)).all() for k in ('logZ', 'logZ_groups', 'trees_loglik') if k in d)


def test_every_memoised_oracle_logz_of_the_walks_is_finite():
    """every (form, state) the leaves, model and tile walks visit, and every (form, seed) of the form walk"""
    for s in C.LEAF_STATES:
        for i in C.LEAVES_FORMS:
            assert _finite(C.reference(i, C.Env(s), C.state_seed(i))), (s, C.NAMES[i])
    for m in C.MODELS:
        for i in C.MODEL_FORMS:
            assert _finite(C.reference(i, C.Env('A', m), C.state_seed(i))), (m, C.NAMES[i])
    for T in C.TILES:
        for i in C.TILE_FORMS:
            assert _finite(C.reference(i, C.Env('A', 'gtr_init', T), C.state_seed(i))), (T, C.NAMES[i])
    for q in range(4):
        for i, seed in C.form_walk_quarter(q):
            assert _finite(C.reference(i, C.Env(), seed)), (C.NAMES[i], seed)
    assert all(_finite(d) for d in C.ORACLE_MEMO.values()) and len(C.ORACLE_MEMO) > 60


def test_scratch_walk_sizes_go_small_large_small_larger():
    names = [op[0] for op in C.SCRATCH_OPS]
    assert [n for n in names if n.startswith('expm')] == ['expm_batched n=%d' % n for n in (3, 5000, 3, 20000)]
    assert [n for n in names if n.startswith('cond')] == ['cond_likelihood_K %s' % s for s in ('2x16', '40x898', '2x16')]
    assert [n for n in names if n.startswith('resample')] == ['resample n=%d' % n for n in (64, 9000, 64)]
    assert [n for n in names if n.startswith('trees')] == ['trees_loglik T=2', 'trees_loglik T=37']
    assert 'forest_loglik' in names and 'log_zsmc' in names


def test_training_steps_differ():
    steps = C.training_steps()
    assert len(steps) == 6 and [M for _, _, _, M, _ in steps] == [1, 2, 1, 2, 1, 2]
    for a, b in zip(steps[:-1], steps[1:]):
        assert (a[0] != b[0]).any() and a[4] != b[4]
        assert (a[1] != b[1]).sum() == a[1].size - 4                              # every variable but the diagonal of y_q (zeros)
