"""Long-lived contexts: every state change of a context held to the bits of a fresh one ("driver": the reuse
contract; INTEGRATION.md: the stale-read rule).

A Trainer keeps one context for hundreds of set_leaves / set_model / sweep / reverse-pass cycles, bench.py re-uses its contexts,
runner.py follows training with a tree summary and a branch pass -- and a context caches a great deal between calls.  The walks
of tests/context_reuse_cases.py put every form of the sweep behind every other one, change leaves, model and site tile under
them, grow and shrink the scratch slots between them, train, and make the calls the plan refuses; every step is compared with
its reference (the C oracle, cpu_grad, the tree posterior's references) and with the same call on a fresh context, bit for bit
(gradients against cpu_grad: RTOL).  tests/test_context_reuse_cpu.py checks that the walks and inputs are what they claim."""
import numpy as np
import pytest

import context_reuse_cases as C
from oracle import cpu_grad as G
from phylo_amd import _ffi

pytestmark = pytest.mark.gpu


def new_ctx(env=None):
    ctx = _ffi.Context(C.K, C.N, C.S)
    if env is not None:
        try:
            env.apply(ctx)
        except Exception:
            ctx.close()
            raise
    return ctx


# ---- the form walk: 169 transitions in four quarters ----------------------------------------------------------------------------
@pytest.mark.parametrize("quarter", range(4))
def test_form_walk(quarter):
    env = C.Env()
    ctx = new_ctx(env)
    try:
        w = C.Walker(ctx, "form (quarter %d)" % quarter)
        for i, seed in C.form_walk_quarter(quarter):
            w.step(i, env, seed)
    finally:
        ctx.close()


# ---- leaves, model, site tile -----------------------------------------------------------------------------------------------------
def test_leaves_walk():
    """every ordered pair of: coded A, coded B (other codes, gap columns), generic rows (no codes), A after a generic row was in it"""
    ctx = new_ctx(C.Env())
    try:
        w = C.Walker(ctx, "leaves")
        before = 'nothing'
        for state in C.LEAVES_WALK:
            for name in C.LEAF_STATES[state][0]:
                ctx.set_leaves(C.LEAVES[name])
            w.state, before = "leaves %s -> %s" % (before, state), state
            env = C.Env(state)
            for i in C.LEAVES_FORMS:
                w.step(i, env, C.state_seed(i))
    finally:
        ctx.close()


def test_model_walk():
    ctx = new_ctx(C.Env())
    try:
        w = C.Walker(ctx, "model")
        before = 'nothing'
        for m in C.MODEL_WALK:
            Q, pi, ll, lr, jc = C.MODELS[m]
            ctx.set_model(Q, pi, ll, lr, jc69_closed_form=jc)
            w.state, before = "model %s -> %s" % (before, m), m
            env = C.Env('A', m)
            for i in C.MODEL_FORMS:
                w.step(i, env, C.state_seed(i))
    finally:
        ctx.close()


def test_tile_walk():
    """(the oracle's tile is set around every reference call and reset to 0 behind it: context_reuse_cases.reference)"""
    ctx = new_ctx(C.Env())
    try:
        w = C.Walker(ctx, "tile")
        before = 'the default'
        for T in C.TILE_WALK:
            ctx.set_site_tile(T)
            w.forget_sweep()
            w.state, before = "tile %s -> %d" % (before, T), T
            env = C.Env('A', 'gtr_init', T)
            assert ctx.site_tile() == (T or _ffi.load().phylo_site_tile(C.S))
            for i in C.TILE_FORMS:
                w.step(i, env, C.state_seed(i))
    finally:
        C.CO.set_site_tile(0)
        ctx.close()


# ---- scratch slots that grow, shrink and grow again between sweeps ------------------------------------------------------------------
def test_scratch_walk():
    env = C.Env()
    ctx = new_ctx(env)
    try:
        w = C.Walker(ctx, "scratch")

        def tree_with_calls_between(c, seed):
            def between(cc):
                for op in C.SCRATCH_BETWEEN:
                    C.check_op(op, cc, env, "between tree_summary and tree_branches, step %d" % w.step_index)
            return C.form_tree(c, seed, between)

        for t, op in enumerate(C.SCRATCH_OPS):
            w.state = "after %s" % op[0]
            C.check_op(op, ctx, env, "scratch walk, call %d" % t)
            w.step(C.F['plain'], env, C.form_seed(C.F['plain'], t))
            last = t == len(C.SCRATCH_OPS) - 1               # ... whose slots the calls between summary and branch pass outgrow once more
            w.step(C.F['tree'], env, C.form_seed(C.F['tree'], t), run=tree_with_calls_between if last else None)
    finally:
        ctx.close()


# ---- training: plain and nested steps in turn on one context ------------------------------------------------------------------------
def _vi_step(ctx, g, packed, flags, M, seed):
    ctx.set_leaves(g)
    z, grads, _, _ = ctx.vi_gradients(seed, flags, M, False, packed)
    sweep = ctx.sweep_fetch()
    d = {k: sweep[k] for k in C.ARRAYS}
    d['logZ'], d['grads'] = np.float64(z), grads
    return d


def test_training_walk():
    ctx = new_ctx()
    try:
        for t, (g, packed, flags, M, seed) in enumerate(C.training_steps()):
            what = "training walk, step %d (%s)" % (t, "nested, M = %d" % M if flags & _ffi.TWISTING else "plain")
            got = _vi_step(ctx, g, packed, flags, M, seed)
            with new_ctx() as one:
                alone = _vi_step(one, g, packed, flags, M, seed)
            diff = C.first_difference(got, alone)
            assert diff is None, "%s against a fresh context: %s" % (what, diff)
            Q, pi, ll, lr = C.variables_model(packed)
            raw = C.grad_reference(g, Q, pi, ll, lr, C.K, seed, got, M if flags & _ffi.TWISTING else 0)
            assert abs(raw['logZ'] - got['logZ']) < 1e-9 * max(1.0, abs(got['logZ'])), what
            ref = G.to_variables(Q, pi, ll, lr, raw)
            R = C.R
            blocks = {'a_l': (got['grads'][:R], ref['d_loglam_l']), 'a_r': (got['grads'][R:2 * R], ref['d_loglam_r']),
                      'y_q': (got['grads'][2 * R:2 * R + 16].reshape(4, 4), ref['d_y_q']), 'y_station': (got['grads'][2 * R + 16:], ref['d_y_station'])}
            for name, (mine, theirs) in blocks.items():
                err = np.max(np.abs(mine - theirs)) / max(np.max(np.abs(theirs)), 1e-300)
                print("%s %s rel err %.3e" % (what, name, err))
                assert err < C.RTOL, (what, name, err)
    finally:
        ctx.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _refused(call, ctx, code, what):
    with pytest.raises(_ffi.PhyloError) as e:
        call(ctx)
    assert e.value.code == code, "%s: code %d, expected %d (%s)" % (what, e.value.code, code, e.value)


def test_refusals_leave_the_context_as_it_was():
    """A refused call raises with the documented code, the sweep before it can still be fetched with its bits, and the next valid
    step has the bits of a fresh context."""
    env = C.Env()
    ctx = new_ctx(env)
    try:
        w = C.Walker(ctx, "refusals")
        plain, graph, tree = C.F['plain'], C.F['graph'], C.F['tree']
        # (the valid step before, the refused call, its code, the valid step after)
        cases = [(plain, name, call, C.EINVAL, nxt) for (name, _, call), nxt in zip(C.REFUSED_SWEEPS, (C.F['batch_g2'], C.F['twisted_m1'], C.F['twisted_m3']))]
        cases += [(plain, 'sweep_backward after a sweep without KEEP_GRAPH', lambda c: c.sweep_backward(), C.ESTATE, graph),
                  (graph, 'sweep_backward_batch of 2 after a sweep of one group', lambda c: c.sweep_backward_batch(2), C.EINVAL, C.F['batch_g4_graph']),
                  (plain, 'tree_branches without a summary', lambda c: c.tree_branches(), C.ESTATE, tree)]
        for t, (first, name, call, code, nxt) in enumerate(cases):
            w.state = name
            w.step(first, env, C.form_seed(first, 2 * t))
            _refused(call, ctx, code, name)
            w.step(C.F['trees_loglik'], env, 0)             # fetches the sweep before the refusal again: its bits
            w.step(nxt, env, C.form_seed(nxt, 2 * t + 1))
        # a kept graph outlives a refused phylo_sweep_backward_batch: the reverse pass still returns its gradient
        got = w.step(graph, env, C.form_seed(graph, 1))
        _refused(lambda c: c.sweep_backward_batch(2), ctx, C.EINVAL, 'sweep_backward_batch of 2')
        again = ctx.sweep_backward()
        assert C.first_difference({k: again[k] for k in C.GRADS}, {k: got[k] for k in C.GRADS}) is None
    finally:
        ctx.close()


# ---- stale reads ------------------------------------------------------------------------------------------------------------------
def _raw_summary_fetch(ctx, counts):
    nc, nt, Gn = counts
    W = (C.N + 63) // 64
    out = {'clade_bits': np.empty((nc, W), dtype=np.uint64), 'clade_weight': np.empty(nc, dtype=np.uint64),
           'clade_group': np.empty(nc, dtype=np.int32), 'topo_weight': np.empty(nt, dtype=np.uint64), 'topo_count': np.empty(nt, dtype=np.int32),
           'topo_rep': np.empty(nt, dtype=np.int32), 'topo_group': np.empty(nt, dtype=np.int32), 'particle_topo': np.empty(C.K, dtype=np.int32),
           'u': np.empty(C.K, dtype=np.uint64), 'U': np.empty(Gn, dtype=np.uint64)}
    ctx._check(ctx._lib.phylo_tree_summary_fetch(ctx._h, *[_ffi._ptr(a) for a in out.values()]))
    return out


def _raw_branches_fetch(ctx, counts):
    nc, nt, Gn = counts
    out = {'clade_stats': np.empty((nc, 4)), 'leaf_stats': np.empty((Gn, C.N, 4)), 'topo_clades': np.empty((nt, C.N - 2), dtype=np.int32),
           'topo_stats': np.empty((nt, 2 * C.N - 2, 4))}
    ctx._check(ctx._lib.phylo_tree_branches_fetch(ctx._h, *[_ffi._ptr(a) for a in out.values()]))
    return out


SUMMARY = ('clade_bits', 'clade_weight', 'topo_weight', 'topo_count', 'topo_rep', 'particle_topo', 'u')
BRANCHES = ('clade_stats', 'leaf_stats', 'topo_stats', 'topo_clades')
SEED, SEED2 = 4100, 4200
BASES = {'lazy': C.DEFAULT, 'eager': C.DEFAULT | _ffi.EAGER_NODES, 'kept graph': C.DEFAULT | _ffi.KEEP_GRAPH}
OLD, NEW, REFUSE, OLD_OR_REFUSE, GRAPH = 'old', 'new', 'refuse', 'old or refuse', 'old if the graph was kept'


def _mutators():
    B, rnd = C.LEAVES['B'], C.MODELS['random']
    return {
        'nothing': lambda c: None,
        'set_leaves': lambda c: c.set_leaves(B),
        'set_model': lambda c: c.set_model(*rnd[:4], jc69_closed_form=rnd[4]),
        'set_site_tile': lambda c: c.set_site_tile(64),
        'a new sweep': lambda c: c.sweep_async(SEED2),
        'a refused call': lambda c: _refused(C.REFUSED_SWEEPS[0][2], c, C.EINVAL, 'a batch of 5'),
    }


# reader -> what it does after each mutator: the old sweep's bits, the new sweep's, or PHYLO_ESTATE; nothing else
#                              nothing  set_leaves  set_model  set_site_tile  a new sweep     a refused call
RULE = {
    'sweep_fetch':            (OLD,    OLD,        OLD,       REFUSE,        NEW,            OLD),
    'sweep_fetch_logz':       (OLD,    OLD,        OLD,       REFUSE,        NEW,            OLD),
    'tree_branches (old summary)': (OLD, OLD,      OLD,       REFUSE,        REFUSE,         OLD),
    'tree_summary_fetch':     (OLD,    OLD,        OLD,       REFUSE,        OLD_OR_REFUSE,  OLD),
    'tree_branches_fetch':    (OLD,    OLD,        OLD,       REFUSE,        REFUSE,         OLD),
    'tree_summary':           (OLD,    OLD,        OLD,       REFUSE,        NEW,            OLD),
    'tree_branches':          (OLD,    OLD,        OLD,       REFUSE,        NEW,            OLD),
    'sweep_backward':         (GRAPH,  REFUSE,     REFUSE,    REFUSE,        REFUSE,         GRAPH),
    'sweep_node':             (OLD,    REFUSE,     OLD,       REFUSE,        NEW,            OLD),
}


def test_a_reader_returns_the_last_sweeps_bits_or_refuses():
    """Every (sweep: lazy, eager, kept graph) x (mutator) x (reader): the reader returns the bits of the sweep it belongs to, or it
    raises PHYLO_ESTATE -- RULE says which, and nothing else may happen.  Readers of stored tables survive set_leaves and set_model;
    the reverse pass does not; phylo_sweep_node survives set_model (the matrices are stored) and refuses after set_leaves (the nodes a
    lazy sweep did not write would come from the new leaves).  A reader called twice returns the same bits twice, also
    sweep_backward -> sweep_node -> sweep_backward, where phylo_sweep_node widens the marks the reverse pass reads."""
    env = C.Env()
    want = {}
    for tag, seed in ((OLD, SEED), (NEW, SEED2)):
        want[tag] = dict(C.reference(C.F['tree'], env, seed))
        want[tag].update(C.reference(C.F['plain'], env, seed))             # the three nodes
    want[OLD].update({k: C.fresh(C.F['graph'], env, SEED)[k] for k in C.GRADS})   # (held to cpu_grad by the form walk)
    ref_grads = C.reference(C.F['graph'], env, SEED)
    assert C.first_difference({k: want[OLD][k] for k in C.GRADS}, {k: ref_grads[k] for k in C.GRADS}, tolerant=C.GRADS) is None
    mutators = _mutators()
    assert list(mutators) == ['nothing', 'set_leaves', 'set_model', 'set_site_tile', 'a new sweep', 'a refused call']

    problems = []                                            # every combination is looked at: each has a context of its own
    for base, flags in BASES.items():
        for col, (mname, mutate) in enumerate(mutators.items()):
            ctx = new_ctx(env)
            try:
                ctx.sweep_async(SEED, flags)
                ctx.tree_summary()                           # a summary of the old sweep, for the branch pass behind the mutator
                counts = ctx._last_counts
                mutate(ctx)

                def check(reader, call, keys):
                    rule = RULE[reader][col]
                    if rule == GRAPH:
                        rule = OLD if base == 'kept graph' else REFUSE
                    what = "%s sweep, %s, then %s" % (base, mname, reader)
                    try:
                        got = call()
                    except _ffi.PhyloError as e:
                        if e.code != C.ESTATE:
                            problems.append("%s: error %d, not PHYLO_ESTATE (%s)" % (what, e.code, e))
                        elif rule not in (REFUSE, OLD_OR_REFUSE):
                            problems.append("%s: refused (%s), expected the %s sweep's bits" % (what, e, rule))
                        return
                    if rule == REFUSE:
                        problems.append("%s: returned something, expected PHYLO_ESTATE" % what)
                        return
                    exp = want[NEW if rule == NEW else OLD]
                    diff = C.first_difference({k: got[k] for k in keys}, {k: exp[k] for k in keys})
                    if diff:
                        problems.append("%s: neither the %s sweep's bits nor a refusal: %s" % (what, rule, diff))

                def fetch():
                    out = ctx.sweep_fetch()
                    out['logZ'] = np.float64(out['logZ'])
                    return out

                def summary():
                    tab = ctx.tree_summary()
                    counts[:] = ctx._last_counts
                    return dict(C.TP.group_table(tab, 0), U=np.asarray(int(tab['U'][0])))

                def branches():                              # (one group: the rows are the group's; the summary only gives the counts)
                    out = ctx.tree_branches({'clade_weight': np.empty(counts[0]), 'topo_weight': np.empty(counts[1]), 'G': 1})
                    return dict(out, leaf_stats=out['leaf_stats'][0])

                def branches_fetch():
                    out = _raw_branches_fetch(ctx, counts)
                    return dict(out, leaf_stats=out['leaf_stats'][0])

                def nodes():
                    return {name: ctx.sweep_node(r, k) for name, (r, k) in C.pick_nodes(want[NEW if RULE['sweep_node'][col] == NEW else OLD]['ancestors']).items()}

                counts = list(counts)
                grads = lambda: ctx.sweep_backward()
                check('sweep_fetch', fetch, C.ARRAYS + ('logZ',))
                check('sweep_fetch_logz', lambda: {'logZ': ctx.sweep_fetch_logz(1)[0]}, ('logZ',))
                check('tree_branches (old summary)', branches, BRANCHES)
                check('tree_summary_fetch', lambda: _raw_summary_fetch(ctx, counts), SUMMARY)
                check('tree_branches_fetch', branches_fetch, BRANCHES)
                check('tree_summary', summary, SUMMARY + ('U',))
                check('tree_branches', branches, BRANCHES)
                check('sweep_backward', grads, C.GRADS)
                check('sweep_backward', grads, C.GRADS)      # twice: the same bits
                check('sweep_node', nodes, ('node_dead', 'node_adopted', 'node_last'))
                check('sweep_backward', grads, C.GRADS)      # ... and behind phylo_sweep_node, which widened the marks
                check('sweep_node', nodes, ('node_dead', 'node_adopted', 'node_last'))
                check('sweep_fetch', fetch, C.ARRAYS + ('logZ',))
                check('tree_summary', summary, SUMMARY + ('U',))
            finally:
                ctx.close()
    assert not problems, "\n".join(problems)
