"""Long-lived contexts ("driver": the reuse contract): the forms a context is driven through, their
references, and the walks that put every form behind every other one on ONE context.  No GPU is needed to import this module or to
compute a reference; tests/test_context_reuse_cpu.py checks the walks and the inputs, tests/test_gpu_context_reuse.py runs them.

A form is a function of (ctx, seed) that returns a dict of arrays; reference(i, env, seed) returns the same dict from the C oracle
(oracle/c_oracle.py), the gradient oracle (oracle/cpu_grad.py) and the tree posterior's references (tests/tree_posterior_ref.py,
tests/tree_branches_ref.py).  Everything is compared bit for bit except the gradients against cpu_grad (RTOL, the figure of
tests/test_gpu_grad.py for exactly this comparison); against the same call on a fresh context the gradients are bits too.
A step of a walk is checked twice: against the reference, and against the same form on a fresh context (fresh())."""
import numpy as np

import tree_branches_ref as BR
import trees_cases as TC
from oracle import c_oracle as CO
from oracle import cpu_grad as G
from oracle import cpu_ref as O
from phylo_amd import _ffi, model
from phylo_amd import treepost as TP

N, K, S = 6, 64, 200          # the merge-record path (tests/test_gpu_merge_fast_rows.py: RN, RS, RK); several tiles at 64 and 128
R = N - 1
RTOL = 1e-9                   # tests/test_gpu_grad.py: relative to the largest entry of each gradient block
DEFAULT = _ffi.FLAGS_DEFAULT
ARRAYS = ('log_weights', 'log_likelihood', 'left_branches', 'right_branches', 'merges', 'ancestors')
GRADS = ('d_lam_l', 'd_lam_r', 'd_pi', 'd_Q')
TABLES = ('clade_bits', 'clade_weight', 'topo_weight', 'topo_count', 'topo_rep', 'particle_topo', 'u', 'U', 'clade_stats', 'leaf_stats',
          'topo_stats', 'topo_clades')
EINVAL, ESTATE = -1, -6       # include/phylo_hip.h


# ---- inputs --------------------------------------------------------------------------------------------------------------------
def _one_hot(codes):
    g = np.zeros(codes.shape + (4,))
    for a in range(4):
        g[..., a] = (codes == a) | (codes == 4)             # code 4: a gap, all ones
    return g


def _alignment(seed, gap_columns):
    """taxa that differ from one random sequence at 30 % of the sites, 5 % scattered gaps, `gap_columns` all-gap columns"""
    rng = np.random.default_rng(seed)
    root = rng.integers(0, 4, S)
    codes = np.where(rng.random((N, S)) < 0.3, rng.integers(0, 4, (N, S)), root[None, :])
    codes[rng.random((N, S)) < 0.05] = 4
    if gap_columns:
        codes[:, rng.choice(S, gap_columns, replace=False)] = 4
    return _one_hot(codes)


def _leaves():
    a = _alignment(61, 0)
    rng = np.random.default_rng(63)
    broken = a.copy()
    broken[2] = rng.uniform(0.05, 1.0, (S, 4))              # one generic row: the whole alignment loses its codes
    return {'A': a, 'B': _alignment(62, 9), 'generic': rng.uniform(0.05, 1.0, (N, S, 4)), 'A_broken': broken}


LEAVES = _leaves()
# a leaf state: the set_leaves calls that enter it, and the alignment the context then holds
LEAF_STATES = {'A': (('A',), 'A'), 'B': (('B',), 'B'), 'generic': (('generic',), 'generic'), 'A_restored': (('A_broken', 'A'), 'A')}


def _random_model(seed):
    rng = np.random.default_rng(seed)
    e = np.exp(rng.normal(size=(4, 4)) * 0.3)
    np.fill_diagonal(e, 0.0)
    Q = e / e.sum(axis=1, keepdims=True)
    np.fill_diagonal(Q, -Q.sum(axis=1))
    p = np.exp(rng.normal(size=4) * 0.3)
    return Q, (p / p.sum())[None, :], np.exp(rng.normal(2.0, 0.3, R)), np.exp(rng.normal(2.0, 0.3, R)), False


# (Q, pi [1, 4], lam_l, lam_r, jc69_closed_form)
MODELS = {'gtr_init': (model.get_Q(model.init_y_q()), np.full((1, 4), 0.25), np.full(R, 10.0), np.full(R, 10.0), False),
          'jc69': (model.jc_Q(), np.full((1, 4), 0.25), np.linspace(6.0, 9.0, R), np.linspace(9.0, 7.0, R), True),
          'random': _random_model(64)}
TILES = (0, 64, 128)


def _trees(n, seed):
    rng = np.random.default_rng(seed)
    rows = [TC.random_rows(N, rng), TC.caterpillar_rows(N, rng), TC.balanced_rows(N, rng), TC.random_rows(N, rng, zeros=False)]
    while len(rows) < n:
        rows.append(TC.random_rows(N, rng))
    rows = rows[:n]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


TREES = _trees(5, 65)


class Env:
    """What a context holds when a form runs: leaves, model, site tile"""

    def __init__(self, leaves='A', model_name='gtr_init', tile=0):
        self.leaves, self.model_name, self.tile = LEAF_STATES[leaves][1] if leaves in LEAF_STATES else leaves, model_name, int(tile)
        self.genome = LEAVES[self.leaves]
        self.Q, self.pi, self.ll, self.lr, self.jc = MODELS[model_name]
        self.key = (self.leaves, model_name, self.tile)

    def apply(self, ctx):
        if self.tile:
            ctx.set_site_tile(self.tile)
        ctx.set_leaves(self.genome)
        ctx.set_model(self.Q, self.pi, self.ll, self.lr, jc69_closed_form=self.jc)

    def model_args(self):
        return self.genome, self.Q, self.pi, self.ll, self.lr

    def __repr__(self):
        return "leaves %s, model %s, tile %d" % self.key


# ---- the forms -----------------------------------------------------------------------------------------------------------------
def _sweep_dict(out):
    d = {k: out[k] for k in ARRAYS}
    d['logZ'] = np.float64(out['logZ'])
    return d


def pick_nodes(ancestors):
    """(r, k) of a node nobody adopted, of an adopted one and of the last rank event's last node (never stored by a lazy sweep)"""
    adopted = np.unique(ancestors[1])
    dead = np.setdiff1d(np.arange(ancestors.shape[1]), adopted)
    return {'node_dead': (1, int(dead[0]) if dead.size else 0), 'node_adopted': (1, int(adopted[0])), 'node_last': (R - 1, K - 1)}


def _with_nodes(ctx, d):
    for name, (r, k) in pick_nodes(d['ancestors']).items():
        d[name] = ctx.sweep_node(r, k)
    return d


def _grads(raw):
    return {k: raw[k] for k in GRADS}


def form_plain(ctx, seed):
    return _with_nodes(ctx, _sweep_dict(ctx.sweep(seed)))


def form_eager(ctx, seed):
    return _with_nodes(ctx, _sweep_dict(ctx.sweep(seed, DEFAULT | _ffi.EAGER_NODES)))


def form_graph(ctx, seed):
    d = _sweep_dict(ctx.sweep(seed, DEFAULT | _ffi.KEEP_GRAPH))
    d.update(_grads(ctx.sweep_backward()))
    return d


def _form_twisted(M):
    def form(ctx, seed):
        return _sweep_dict(ctx.sweep(seed, DEFAULT | _ffi.TWISTING, M))
    return form


def form_twisted_graph(ctx, seed):
    d = _sweep_dict(ctx.sweep(seed, DEFAULT | _ffi.TWISTING | _ffi.KEEP_GRAPH, 2))
    d.update(_grads(ctx.sweep_backward()))
    return d


def group_seeds(seed, Gn):
    return [seed + 7919 * g for g in range(Gn)]


def _form_batch(Gn, flags):
    def form(ctx, seed):
        ctx.sweep_batch_async(group_seeds(seed, Gn), flags)
        z = ctx.sweep_fetch_logz(Gn)
        out = ctx.sweep_fetch()
        d = {k: out[k] for k in ARRAYS}
        d['logZ_groups'] = z
        if flags & _ffi.KEEP_GRAPH:
            d.update(_grads(ctx.sweep_backward_batch(Gn)))
        return d
    return form


def form_one_launch(ctx, seed):
    out = ctx.sweep(seed, DEFAULT | _ffi.ONE_LAUNCH)
    d = _sweep_dict(out)
    d['n_launches'] = np.int64(out['stats']['n_launches'])
    return d


def form_stepwise(ctx, seed):
    ctx.sweep_begin(seed)
    for _ in range(R):
        ctx.sweep_step()
    ctx.sweep_finish()
    return _sweep_dict(ctx.sweep_fetch())


def form_tree(ctx, seed, between=None):
    """between(ctx): calls made between the summary and the branch pass (the scratch walk's)"""
    d = _sweep_dict(ctx.sweep(seed))
    tab = ctx.tree_summary()
    if between is not None:
        between(ctx)
    tab.update(ctx.tree_branches(tab))
    got = TP.group_table(tab, 0)
    for k in TABLES:
        d[k] = np.asarray(got[k])
    return d


def form_trees_loglik(ctx, seed):
    """... then the previous sweep once more ('re_' keys; none when the context has not swept yet: the fetch must then refuse)"""
    d = {'trees_loglik': ctx.trees_loglik(*TREES)}
    try:
        out = ctx.sweep_fetch()
    except _ffi.PhyloError as e:
        assert e.code == ESTATE, e
        return d
    for k in ARRAYS:
        d['re_' + k] = out[k]
    return d


# (name, form, what debug_sweep_plan is asked: G, M, flags)
FORMS = (
    ('plain', form_plain, dict(G=1, M=1, flags=DEFAULT)),
    ('eager', form_eager, dict(G=1, M=1, flags=DEFAULT | _ffi.EAGER_NODES)),
    ('graph', form_graph, dict(G=1, M=1, flags=DEFAULT | _ffi.KEEP_GRAPH)),
    ('twisted_m1', _form_twisted(1), dict(G=1, M=1, flags=DEFAULT | _ffi.TWISTING)),
    ('twisted_m3', _form_twisted(3), dict(G=1, M=3, flags=DEFAULT | _ffi.TWISTING)),
    ('twisted_graph_m2', form_twisted_graph, dict(G=1, M=2, flags=DEFAULT | _ffi.TWISTING | _ffi.KEEP_GRAPH)),
    ('batch_g2', _form_batch(2, DEFAULT), dict(G=2, M=1, flags=DEFAULT)),
    ('batch_g4_graph', _form_batch(4, DEFAULT | _ffi.KEEP_GRAPH), dict(G=4, M=1, flags=DEFAULT | _ffi.KEEP_GRAPH)),
    ('one_launch', form_one_launch, dict(G=1, M=1, flags=DEFAULT | _ffi.ONE_LAUNCH)),
    ('one_launch_batch_g2', _form_batch(2, DEFAULT | _ffi.ONE_LAUNCH), dict(G=2, M=1, flags=DEFAULT | _ffi.ONE_LAUNCH)),
    ('stepwise', form_stepwise, dict(G=1, M=1, flags=DEFAULT)),
    ('tree', form_tree, dict(G=1, M=1, flags=DEFAULT)),
    ('trees_loglik', form_trees_loglik, dict(G=1, M=1, flags=DEFAULT)),
)
NAMES = tuple(f[0] for f in FORMS)
F = {name: i for i, name in enumerate(NAMES)}       # the issue's form k is index k - 1


# ---- the references ------------------------------------------------------------------------------------------------------------
def grad_reference(genome, Q, pi, ll, lr, Kp, seed, sweep, M=0):
    """cpu_grad's gradient on the discrete structure of a fetched (or oracle) sweep of Kp particles, as tests/test_gpu_grad.py
    builds it: M = 0 the plain proposal, M >= 1 the twisted one"""
    if M == 0:
        st = G.forward(genome, Q, pi, ll, lr, Kp, seed)['struct']
        for r in range(1, R):
            st['anc'][r] = sweep['ancestors'][r - 1].astype(np.int64)
        return G.sweep_grad(genome, Q, pi, ll, lr, Kp, seed, struct=st)
    st = G.forward_twisted(genome, Q, pi, ll, lr, Kp, M, seed)['struct']
    for r in range(R):
        if r > 0:
            st['anc'][r] = sweep['ancestors'][r - 1].astype(np.int64)
        pairs = O.pair_list(N - r)
        b_l = -np.log(st['Ul'][r]) / ll[r]
        js = np.zeros(Kp, dtype=np.int64)
        for k in range(Kp):
            t = pairs.index((int(sweep['merges'][r, k, 0]), int(sweep['merges'][r, k, 1])))
            js[k] = t * M + int(np.argmin(np.abs(b_l[k, t * M:(t + 1) * M] - sweep['left_branches'][r, k])))
        st['js'][r] = js
    return G.sweep_grad_twisted(genome, Q, pi, ll, lr, Kp, M, seed, struct=st)


def _ref_sweep(env, seed, nodes=False, Kp=K):
    ref = CO.sweep(*env.model_args(), Kp, seed, jc=env.jc, want_nodes=nodes)
    d = _sweep_dict(ref)
    if nodes:
        for name, (r, k) in pick_nodes(ref['ancestors']).items():
            d[name] = ref['nodes'][r, k].copy()
    return d


def _ref_graph(env, seed):
    d = _ref_sweep(env, seed)
    d.update(_grads(grad_reference(*env.model_args(), K, seed, d)))
    return d


def _ref_twisted(M, graph=False):
    def ref(env, seed):
        d = _sweep_dict(CO.sweep_twisted(*env.model_args(), K, M, seed, jc=env.jc))
        if graph:
            d.update(_grads(grad_reference(*env.model_args(), K, seed, d, M)))
        return d
    return ref


def _ref_batch(Gn, graph=False):
    def ref(env, seed):
        Kg = K // Gn
        groups = [_ref_sweep(env, sd, Kp=Kg) for sd in group_seeds(seed, Gn)]
        d = {k: np.concatenate([g[k] for g in groups], axis=1) for k in ARRAYS}
        d['logZ_groups'] = np.array([g['logZ'] for g in groups])
        if graph:
            gr = [grad_reference(*env.model_args(), Kg, sd, g) for sd, g in zip(group_seeds(seed, Gn), groups)]
            d.update({k: np.stack([x[k] for x in gr]) for k in GRADS})
        return d
    return ref


def _ref_one_launch(env, seed):
    d = _ref_sweep(env, seed)
    d['n_launches'] = np.int64(1)
    return d


def _ref_tree(env, seed):
    d = _ref_sweep(env, seed)
    summary, exp, _, _ = BR.expected(d, N, K, seed)
    for k in TABLES:
        d[k] = np.asarray(summary[k] if k in summary else exp[k])
    return d


def _ref_trees_loglik(env, seed):
    out = []
    for c, b in zip(*TREES):
        left, right, bl, br = TC.rows_to_nodes(c, b)
        out.append(CO.tree_loglik(env.Q, env.pi.reshape(-1), left, right, bl, br, 2 * N - 2, env.genome, jc=env.jc)[0])
    return {'trees_loglik': np.array(out)}


REFERENCES = (lambda e, s: _ref_sweep(e, s, nodes=True), lambda e, s: _ref_sweep(e, s, nodes=True), _ref_graph, _ref_twisted(1),
              _ref_twisted(3), _ref_twisted(2, graph=True), _ref_batch(2), _ref_batch(4, graph=True), _ref_one_launch, _ref_batch(2),
              _ref_sweep, _ref_tree, _ref_trees_loglik)
ORACLE_MEMO, FRESH_MEMO = {}, {}


def reference(i, env, seed):
    """the reference's dict of form i, memoised by (form, leaves, model, tile, seed); the oracle's site tile is set for the call"""
    key = (i,) + env.key + (seed,)
    if key not in ORACLE_MEMO:
        CO.set_site_tile(env.tile)
        try:
            ORACLE_MEMO[key] = REFERENCES[i](env, seed)
        finally:
            CO.set_site_tile(0)
    return ORACLE_MEMO[key]


def fresh(i, env, seed):
    """form i on a context that has done nothing else, memoised alike"""
    key = (i,) + env.key + (seed,)
    if key not in FRESH_MEMO:
        with _ffi.Context(K, N, S) as ctx:
            env.apply(ctx)
            FRESH_MEMO[key] = FORMS[i][1](ctx, seed)
    return FRESH_MEMO[key]


# ---- comparison ----------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def first_difference(got, want, tolerant=(), skip=()):
    """None, or what the first differing array is.  Keys of `tolerant` (gradients against cpu_grad) within RTOL of the block's
    largest entry, everything else bit for bit; keys of `skip` (what the reference does not model) and 're_' keys are left out"""
    keys = [k for k in got if not k.startswith('re_') and k not in skip]
    missing = sorted(set(want) - set(skip) - set(keys)) + sorted(set(keys) - set(want))
    if missing:
        return "the key sets differ: %s" % missing
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.shape != w.shape:
            return "%s: shape %r against %r" % (k, g.shape, w.shape)
        if k in tolerant:
            err = np.max(np.abs(g - w)) / max(np.max(np.abs(w)), 1e-300)
            if not err < RTOL:
                return "%s: relative error %.3e >= %.0e" % (k, err, RTOL)
        elif not np.array_equal(_bits(g), _bits(w)):
            bad = np.flatnonzero(_bits(g).reshape(-1) != _bits(w).reshape(-1))
            return "%s: %d of %d values differ, the first at %d: %r against %r" % (k, bad.size, g.size, bad[0], g.reshape(-1)[bad[0]],
                                                                                w.reshape(-1)[bad[0]])
    return None


class Walker:
    """Runs steps on one context and checks each against the reference and against a fresh context; remembers the last sweep's
    arrays for the form that fetches them again.  A failure names the walk, the step, the transition, the seed and the array, and
    ends the walk (AssertionError): the later steps would run on a context already known to be wrong."""

    def __init__(self, ctx, walk):
        self.ctx, self.walk = ctx, walk
        self.step_index, self.prev, self.last_sweep = 0, 'a fresh context', None
        self.state = ''                                     # what the walk changed last, for the report

    def fail(self, name, seed, env, against, what):
        raise AssertionError("%s walk, step %d%s, %s -> %s, seed %d (%s), against %s: %s"
                             % (self.walk, self.step_index, self.state and " (%s)" % self.state, self.prev, name, seed, env, against, what))

    def step(self, i, env, seed, run=None):
        """form i (or run(ctx, seed) in its place: the same form with calls in between)"""
        name = NAMES[i]
        got = (run or FORMS[i][1])(self.ctx, seed)
        jc_skip = tuple(k for k in ('d_pi', 'd_Q') if env.jc and k in got)      # held constant under JC69: cpu_grad differs by design
        ref = reference(i, env, seed)
        what = first_difference(got, {k: v for k, v in ref.items() if k not in jc_skip}, tolerant=GRADS, skip=jc_skip)
        if what:
            self.fail(name, seed, env, "the reference", what)
        what = first_difference(got, fresh(i, env, seed))
        if what:
            self.fail(name, seed, env, "a fresh context", what)
        re = {k[3:]: v for k, v in got.items() if k.startswith('re_')}
        if i == F['trees_loglik'] and (self.last_sweep is None) != (not re):
            self.fail(name, seed, env, "the previous step", "sweep_fetch %s" % ("refused" if not re else "returned a sweep nobody ran"))
        if re:
            what = first_difference(re, self.last_sweep)
            if what:
                self.fail(name, seed, env, "the previous step's sweep, fetched again", what)
        if 'log_weights' in got:
            self.last_sweep = {k: got[k] for k in ARRAYS}
        self.prev = name
        self.step_index += 1
        return got

    def forget_sweep(self):
        """the context dropped its sweep (phylo_set_site_tile)"""
        self.last_sweep = None


# ---- the walks -----------------------------------------------------------------------------------------------------------------
def closed_walk(n):
    """A closed walk through the complete directed graph on n nodes with self-loops that takes every one of the n * n edges exactly
    once (Hierholzer; the graph is Eulerian: in-degree = out-degree = n): n * n + 1 nodes, the first one again at the end"""
    nxt = [0] * n
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < n:
            stack.append((v + nxt[v]) % n)                  # the self-loop first
            nxt[v] += 1
        else:
            out.append(stack.pop())
    return out[::-1]


def pairs_of(seq):
    return {(a, b) for a, b in zip(seq[:-1], seq[1:])}


FORM_WALK = closed_walk(len(FORMS))


def form_seed(i, step):
    """a seed that differs between consecutive steps whatever the forms, from three per form: the references are memoised"""
    return 1000 + 31 * i + step % 3


def form_walk_quarter(q):
    """[(form, seed)] of quarter q of the 169 transitions: its first entry repeats the last form of the quarter before, so that the
    transition across the cut is taken too (the context of a quarter is fresh: that first entry only sets the state)"""
    n = len(FORM_WALK) - 1
    lo, hi = q * n // 4, (q + 1) * n // 4
    return [(FORM_WALK[t], form_seed(FORM_WALK[t], t)) for t in range(lo, hi + 1)]


def state_walk(states):
    return [states[j] for j in closed_walk(len(states))]


LEAVES_WALK = state_walk(tuple(LEAF_STATES))
LEAVES_FORMS = (F['plain'], F['twisted_m3'], F['graph'], F['one_launch'], F['trees_loglik'])
MODEL_WALK = state_walk(tuple(MODELS))
MODEL_FORMS = (F['plain'], F['twisted_m1'], F['graph'], F['batch_g2'], F['one_launch'])
TILE_WALK = state_walk(TILES)
TILE_FORMS = (F['plain'], F['eager'], F['graph'], F['twisted_m1'], F['tree'])


def state_seed(i):
    """the leaves, model and tile walks change the state, not the seed: one seed per form"""
    return 2000 + 31 * i


# ---- the scratch walk's op-level calls: (name, call(ctx, env) -> array, oracle(env) -> array), sizes small, large, small, larger ----
def _op_expm(n):
    t = np.random.default_rng(70 + n).exponential(0.1, n)
    return ('expm_batched n=%d' % n, lambda ctx, env: ctx.expm_batched(t), lambda env: CO.expm_batched(env.Q, t, jc=env.jc))


def _op_cond(Kc, Sc):
    rng = np.random.default_rng(71 + Kc)
    l, r = rng.uniform(0.1, 1.0, (Kc, Sc, 4)), rng.uniform(0.1, 1.0, (Kc, Sc, 4))
    tl, tr = rng.exponential(0.1, Kc), rng.exponential(0.1, Kc)
    return ('cond_likelihood_K %dx%d' % (Kc, Sc), lambda ctx, env: ctx.cond_likelihood_K(l, r, tl, tr),
            lambda env: CO.cond_likelihood_K(env.Q, l, r, tl, tr, jc=env.jc))


def _op_forest():
    rng = np.random.default_rng(72)
    core = rng.uniform(1e-3, 1.0, (9, 5, S, 4))
    rec = rng.integers(1, 6, (9, 5)).astype(np.int32)
    return ('forest_loglik', lambda ctx, env: ctx.forest_loglik(core, rec), lambda env: CO.forest_loglik(env.pi, core, rec))


def _op_resample(n):
    lw = np.random.default_rng(73 + n).normal(scale=30.0, size=n) - 6000.0
    return ('resample n=%d' % n, lambda ctx, env: ctx.resample(lw, 11, 3), lambda env: CO.resample(lw, 11, 3))


def _op_log_zsmc():
    lw = np.random.default_rng(74).normal(scale=20.0, size=(11, 777)) - 500.0
    return ('log_zsmc', lambda ctx, env: np.float64(ctx.log_zsmc(lw)), lambda env: np.float64(CO.log_zsmc(lw)))


def _op_trees(n):
    child, blen = _trees(n, 75 + n)

    def ora(env):
        out = []
        for c, b in zip(child, blen):
            left, right, bl, br = TC.rows_to_nodes(c, b)
            out.append(CO.tree_loglik(env.Q, env.pi.reshape(-1), left, right, bl, br, 2 * N - 2, env.genome, jc=env.jc)[0])
        return np.array(out)
    return ('trees_loglik T=%d' % n, lambda ctx, env: ctx.trees_loglik(child, blen), ora)


SCRATCH_OPS = (_op_expm(3), _op_cond(2, 16), _op_forest(), _op_resample(64), _op_log_zsmc(), _op_trees(2),
               _op_expm(5000), _op_cond(40, 898), _op_resample(9000), _op_trees(37),
               _op_expm(3), _op_cond(2, 16), _op_resample(64), _op_expm(20000))
SCRATCH_BETWEEN = (_op_expm(30000), _op_trees(64))          # between the summary and the branch pass of the last tree step: larger again


def check_op(op, ctx, env, where):
    name, call, ora = op
    got, want = np.asarray(call(ctx, env)), np.asarray(ora(env))
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want)), "%s: %s differs from the C oracle" % (where, name)


# ---- the training walk: six steps, plain and nested in turn, each on its own minibatch and variables --------------------------------
TRAIN_SITES = 3 * S


def training_steps():
    """[(minibatch [N][S][4], packed variables, flags, M, seed)]"""
    rng = np.random.default_rng(66)
    root = rng.integers(0, 4, TRAIN_SITES)
    codes = np.where(rng.random((N, TRAIN_SITES)) < 0.3, rng.integers(0, 4, (N, TRAIN_SITES)), root[None, :])
    genome = _one_hot(codes)
    steps = []
    for t in range(6):
        nested = t % 2 == 1
        y_q = rng.normal(size=(4, 4)) * 0.2
        np.fill_diagonal(y_q, 0.0)
        packed = np.concatenate([np.log(10.0) + rng.normal(size=R) * 0.1, np.log(10.0) + rng.normal(size=R) * 0.1, y_q.reshape(-1),
                                 0.25 + rng.normal(size=4) * 0.2])
        sites = np.sort(rng.permutation(TRAIN_SITES)[:S])
        steps.append((genome[:, sites, :], packed, DEFAULT | _ffi.KEEP_GRAPH | (_ffi.TWISTING if nested else 0), 2 if nested else 1, 3000 + t))
    return steps


def variables_model(packed):
    """(Q, pi, lam_l, lam_r) of packed variables a_l | a_r | y_q | y_station, as phylo_amd/train.py evaluates them"""
    return (model.get_Q(packed[2 * R:2 * R + 16].reshape(4, 4)), model.get_stationary_probs(packed[2 * R + 16:]), np.exp(packed[:R]),
            np.exp(packed[R:2 * R]))


# ---- what the plan refuses: (name, call(ctx), code); the three sweeps are refused by debug_sweep_plan with the same code ------------
REFUSED_SWEEPS = (
    ('a batch of 5 on K = 64', dict(G=5, M=1, flags=DEFAULT), lambda ctx: ctx.sweep_batch_async([1, 2, 3, 4, 5])),
    ('a batch with TWISTING', dict(G=2, M=1, flags=DEFAULT | _ffi.TWISTING), lambda ctx: ctx.sweep_batch_async([1, 2], DEFAULT | _ffi.TWISTING)),
    ('M = 0', dict(G=1, M=0, flags=DEFAULT | _ffi.TWISTING), lambda ctx: ctx.sweep_async(1, DEFAULT | _ffi.TWISTING, 0)),
)
