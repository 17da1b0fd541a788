"""The one-launch sweep (phylo_persist.h) in the forms no default reaches: pp_sweep<512> (PHYLO_PERSIST_NT=512: eight waves per
chunk of 16 particles, the merge's pipeline at BS = 2, pp_scan<512> inside the sweep, loops strided by 512) and grids forced with
PHYLO_PERSIST_WGS (m = one chunk, a chunk and one particle, PP_MAX_M, one workgroup per group, fewer workgroups than groups).

Both switches are read when a context is created, so they are set before it is made.  Every grid computes the launch path's bits,
and a refused grid falls back to the launch path, so a switch that is not read passes every comparison.  Hence every test, in this
order: runs the sweep; asserts stats['n_launches'] == 1; asserts through phylo_debug_persist_of that threads, Wg and m are the
ones the case claims (tests/one_launch_cases.py; tests/test_one_launch_plan_cpu.py pins the claims to the rule); compares with the
C oracle bit for bit (log-weights, log-likelihoods, branch lengths, ancestors, merges, log Z); compares with the launch path of the
same context.  The grids are stated for an MI355X (256 compute units).

No case aims at the time-out path of the kernel's bounded waits: forced grids are smaller than the device, so every workgroup is
resident.  A time-out error here is a finding about the kernel."""
import functools

import numpy as np
import pytest

import one_launch_cases as OC
from oracle import c_oracle as CO
from oracle import cpu_ref as O
from phylo_amd import _ffi
from phylo_amd.datasets import load_dataset, synthetic_alignment

pytestmark = pytest.mark.gpu
PI = np.full((1, 4), 0.25)
ONE = _ffi.FLAGS_DEFAULT | _ffi.ONE_LAUNCH
ESTATE = -6
KEYS = ('log_weights', 'log_likelihood', 'left_branches', 'right_branches')


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b, nan_ok=False):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    eq = bits(a) == bits(b)
    return bool((eq | (np.isnan(a) & np.isnan(b))).all()) if nan_ok else bool(eq.all())


def check(out, ref, what, nan_ok=False):
    np.testing.assert_array_equal(out['ancestors'], ref['ancestors'], err_msg=what + ": resampling indices")
    np.testing.assert_array_equal(out['merges'], ref['merges'], err_msg=what + ": merges")
    for key in KEYS:
        assert out[key].shape == ref[key].shape and same_bits(out[key], ref[key], nan_ok), "%s: %s differs" % (what, key)
    if ref['logZ'] is not None:
        assert same_bits(out['logZ'], ref['logZ'], nan_ok), (what, out['logZ'], ref['logZ'])


def joined(refs):
    """G oracle sweeps side by side, as a batch returns them (ancestors count inside their group; the G log Z are fetched apart)"""
    if len(refs) == 1:
        return refs[0]
    out = {key: np.concatenate([r[key] for r in refs], axis=1) for key in KEYS + ('ancestors', 'merges')}
    out['logZ'] = None
    return out


def took(ctx, name_or_grid, nt, Kg):
    """the grid the context's last sweep took is the claimed one"""
    Wg, m = name_or_grid
    assert Wg * m == Kg
    assert ctx.debug_persist() == {'nt': nt, 'Wg': Wg, 'm': m, 'lds': OC.lds_bytes(ctx.N, m, Kg)}


def took_launches(ctx, out):
    assert out['stats']['n_launches'] > 1
    with pytest.raises(_ffi.PhyloError) as e:
        ctx.debug_persist()
    assert e.value.code == ESTATE


def one_launch(ctx, seed, grid, nt, flags=ONE):
    out = ctx.sweep(seed, flags=flags)
    assert out['stats']['n_launches'] == 1, "the one-launch form did not run"
    took(ctx, grid, nt, ctx.K)
    return out


def one_launch_batch(ctx, seeds, grid, nt):
    G = len(seeds)
    ctx.sweep_batch_async(seeds, flags=ONE)
    logz = ctx.sweep_fetch_logz(G)
    out = ctx.sweep_fetch()
    assert out['stats']['n_launches'] == 1, "the one-launch form did not run"
    took(ctx, grid, nt, ctx.K // G)
    return out, list(logz)


def launches_batch(ctx, seeds):
    ctx.sweep_batch_async(seeds, flags=_ffi.FLAGS_DEFAULT)
    logz = ctx.sweep_fetch_logz(len(seeds))
    out = ctx.sweep_fetch()
    took_launches(ctx, out)
    return out, list(logz)


def make_ctx(g, K, Q, pi=PI, lam_l=None, lam_r=None, jc=False):
    N, S, _ = g.shape
    ctx = _ffi.Context(K, N, S)
    ctx.set_leaves(g)
    ctx.set_model(Q, pi, np.full(N - 1, 10.0) if lam_l is None else lam_l, np.full(N - 1, 10.0) if lam_r is None else lam_r,
                  jc69_closed_form=jc)
    return ctx


def gtr():
    return O.get_Q(O.init_y_q())


@functools.lru_cache(maxsize=None)
def primate():
    g = load_dataset('primate_data')['genome']
    g.setflags(write=False)
    return g


def claim(name, N, G, Kg):
    c = OC.DEFAULT_GRID[name]
    assert (c["N"], c["G"], c["Kg"]) == (N, G, Kg), "the case and its claim are out of step"
    return c["Wg"], c["m"]


@pytest.fixture
def nt512(monkeypatch):
    monkeypatch.setenv('PHYLO_PERSIST_NT', '512')
    monkeypatch.delenv('PHYLO_PERSIST_WGS', raising=False)
    monkeypatch.delenv('PHYLO_NO_LEAF_CODES', raising=False)
    return 512


# ---- part A: PHYLO_PERSIST_NT=512 on the default grid ------------------------------------------------------------------------------

def _shape(name):
    if name == "k16":
        return load_dataset('primate_data_wang')['genome'], 16, True
    if name == "ds1-k300":
        return load_dataset('hohna_data_1')['genome'][:, :400], 300, False
    if name == "n32-k96":
        return synthetic_alignment(32, 200)['genome'], 96, False
    K, S = {"k257": (257, 898), "k5000": (5000, 256), "k8192": (8192, 192)}[name]
    return primate()[:, :S], K, False


@pytest.mark.parametrize("name", ["k16", "k257", "k5000", "k8192", "ds1-k300", "n32-k96"])
def test_512_threads_particle_and_group_shapes(nt512, name):
    g, K, jc = _shape(name)
    N = g.shape[0]
    Q = O.jc_Q() if jc else gtr()
    lam = np.full(N - 1, 10.0)
    grid = claim(name, N, 1, K)
    with make_ctx(g, K, Q, jc=jc) as ctx:
        out = one_launch(ctx, 4, grid, 512)
        ref = CO.sweep(g, Q, PI, lam, lam, K, 4, jc=jc, want_nodes=(K <= 300))
        check(out, ref, "%s, one launch of 512 threads" % name)
        if K <= 300:
            # nodes on demand behind a one-launch sweep: an adopted one (the pool holds it), a dead one, the last rank event's, others
            adopted = int(out['ancestors'][1, 0])
            dead = sorted(set(range(K)) - set(out['ancestors'][0].tolist()))
            assert dead, "no dead node at rank event 0"
            for (r, k) in [(1, adopted), (0, dead[0]), (0, dead[-1]), (N - 2, K - 1), (N - 2, 0), (0, 0), (N // 2, K // 3)]:
                assert same_bits(ctx.sweep_node(r, k), ref['nodes'][r, k]), "node (%d,%d)" % (r, k)
            took(ctx, grid, 512, K)                        # (fetching nodes is not a sweep)
        four = ctx.sweep(4)
        took_launches(ctx, four)
        check(four, out, "%s, launches against one launch" % name)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 129, 256, 257, 513])
def test_512_threads_merge_loop_edges(nt512, S):
    """The merge's ping-pong loop at BS = 2 advances 4 site steps a turn; ceil(S / 64) = 1, 1, 1, 2, 3, 4, 5, 9 steps: less than one
    block, one block exactly, a turn exactly, a turn and one step, two turns and one.  Coded leaves (byte codes) and, with one generic
    leaf row, the row loads; later rank events merge internal nodes in both."""
    N, K = 5, 64
    Q = gtr()
    lam = np.full(N - 1, 10.0)
    grid = claim("edges-k64", N, 1, K)
    for variant in ('coded', 'generic'):
        g = primate()[:N, 100:100 + S].copy()
        if variant == 'generic':
            g[1, S // 2] = [0.25, 0.5, 0.125, 0.125]
        with make_ctx(g, K, Q) as ctx:
            out = one_launch(ctx, 7, grid, 512)
            check(out, CO.sweep(g, Q, PI, lam, lam, K, 7), "S = %d, %s leaves" % (S, variant))
            check(ctx.sweep(7), out, "S = %d, %s leaves: launches against one launch" % (S, variant))


def test_512_threads_uneven_site_tiles(nt512):
    """S = 300 in site tiles of 128: tiles of 128, 128 and 44 sites, i.e. 2, 2 and 1 site steps, summed left to right"""
    N, K, S, T = 6, 80, 300, 128
    g = primate()[:N, 200:200 + S]
    Q = gtr()
    lam = np.full(N - 1, 10.0)
    try:
        CO.set_site_tile(T)
        with make_ctx(g, K, Q) as ctx:
            ctx.set_site_tile(T)
            out = one_launch(ctx, 3, claim("tiles-k80", N, 1, K), 512)
            check(out, CO.sweep(g, Q, PI, lam, lam, K, 3), "site tiles of %d" % T)
            check(ctx.sweep(3), out, "site tiles of %d: launches against one launch" % T)
    finally:
        CO.set_site_tile(0)
    with make_ctx(g, K, Q) as ctx:                            # (the tile mattered: one tile of 300 sites sums in another order)
        assert not same_bits(ctx.sweep(3, flags=ONE)['log_weights'], out['log_weights'])


@pytest.mark.parametrize("variant", ['coded', 'generic', 'no-codes', 'zero-row'])
def test_512_threads_leaf_forms_special_values_and_models(nt512, monkeypatch, variant):
    """The four CL / CR instantiations of the merge at BS = 2 under an asymmetric Q, a non-uniform pi and per-rank rates, with the Q1
    quirk on and off.  coded: leaf children go through byte codes (two leaves: the 25 memoised likelihoods), internal children
    through rows, so all four variants run; generic (one leaf row neither one-hot nor all-ones) and no-codes (PHYLO_NO_LEAF_CODES):
    every merge takes the uncoded loads; zero-row: a site likelihood of 0, the merge flags the particle and pp_merge_slow redoes
    it (NaN is matched as NaN)."""
    N, K = 7, 128
    g = primate()[:N, 100:500].copy()
    if variant == 'generic':
        g[3, 5] = [0.5, 0.5, 0.0, 0.0]
    if variant == 'zero-row':
        g[2, 7] = [0.0, 0.0, 0.0, 0.0]
    if variant == 'no-codes':
        monkeypatch.setenv('PHYLO_NO_LEAF_CODES', '1')
    rng = np.random.default_rng(9)
    Q = O.get_Q(rng.normal(size=(4, 4)))
    pi = O.get_stationary_probs(rng.normal(size=4))
    lam_l, lam_r = rng.uniform(3, 20, N - 1), rng.uniform(3, 20, N - 1)
    grid = claim("variants-k128", N, 1, K)
    with make_ctx(g, K, Q, pi, lam_l, lam_r) as ctx:
        for q1 in (_ffi.QUIRK_Q1_RAW_Q, 0):
            out = one_launch(ctx, 21, grid, 512, flags=q1 | _ffi.ONE_LAUNCH)
            ref = CO.sweep(g, Q, pi, lam_l, lam_r, K, 21, flags=q1)
            check(out, ref, "%s, quirk %d" % (variant, q1), nan_ok=True)
            assert np.isfinite(ref['log_weights']).all() == (variant != 'zero-row')      # the special values really occurred
            check(ctx.sweep(21, flags=q1), out, "%s, quirk %d: launches against one launch" % (variant, q1), nan_ok=True)
            if q1:
                with_quirk = ref['log_weights']
        if variant != 'zero-row':                              # (the quirk is not a no-op under this Q; the zero row leaves -inf and NaN only)
            assert not same_bits(with_quirk, ref['log_weights'])


@pytest.mark.parametrize("K,name", [(64, "flat-k64"), (1000, "flat-k1000"), (4096, "flat-k4096")])
def test_512_threads_flat_weights_most_nodes_are_adopted(nt512, K, name):
    """All-gap rows: weights differ only through the priors, most nodes of a rank event are adopted: written by loops strided by the
    512 threads and read behind their marks by merges of the same rank event.  Nodes too."""
    N, S = 9, 333
    g = np.ones((N, S, 4))
    Q = gtr()
    lam = np.full(N - 1, 10.0)
    with make_ctx(g, K, Q) as ctx:
        out = one_launch(ctx, 2, claim(name, N, 1, K), 512)
        ref = CO.sweep(g, Q, PI, lam, lam, K, 2, want_nodes=True)
        check(out, ref, "flat K = %d" % K)
        assert len(np.unique(out['ancestors'][0])) > K // 3        # the regime this test is about
        for r in range(N - 1):
            ks = {0, K // 2, K - 1}
            if r < N - 2:
                ks |= {int(k) for k in out['ancestors'][r, :3]}     # adopted nodes of rank event r: the pool holds them
            for k in sorted(ks):
                assert same_bits(ctx.sweep_node(r, k), ref['nodes'][r, k]), "node (%d,%d)" % (r, k)
        check(ctx.sweep(2), out, "flat K = %d: launches against one launch" % K)


@pytest.mark.parametrize("G,Kg,name", [(3, 32, "batch-3x32"), (5, 7, "batch-5x7"), (8, 256, "batch-8x256")])
def test_512_threads_batches(nt512, G, Kg, name):
    """every group carries the bits of the Kg-particle sweep of its own seed, its log Z included"""
    g = primate()[:, :300]
    N = g.shape[0]
    Q = gtr()
    lam = np.full(N - 1, 10.0)
    seeds = [100 + 7 * i for i in range(G)]
    refs = [CO.sweep(g, Q, PI, lam, lam, Kg, s) for s in seeds]
    with make_ctx(g, G * Kg, Q) as ctx:
        out, logz = one_launch_batch(ctx, seeds, claim(name, N, G, Kg), 512)
        check(out, joined(refs), "batch %d x %d" % (G, Kg))
        assert logz == [r['logZ'] for r in refs]
        four, logz4 = launches_batch(ctx, seeds)
        check(four, out, "batch %d x %d: launches against one launch" % (G, Kg))
        assert logz4 == logz


def test_512_threads_one_context_through_every_path(nt512):
    """one launch, launches, one launch, a batch of another G, one launch again on ONE context: the groups' arrival counters are
    monotone across launches of a grid and start again from 0 when the grid or the number of groups changes"""
    g = primate()[:8, 300:500]
    N, K = 8, 192
    Q = gtr()
    lam = np.full(N - 1, 10.0)
    grid1, grid4 = claim("reuse-k192", N, 1, K), claim("reuse-4x48", N, 4, K // 4)
    oracle = lambda Kg, seed: CO.sweep(g, Q, PI, lam, lam, Kg, seed)
    with make_ctx(g, K, Q) as ctx:
        check(one_launch(ctx, 1, grid1, 512), oracle(K, 1), "first one-launch sweep")
        four = ctx.sweep(2)
        took_launches(ctx, four)
        check(four, oracle(K, 2), "launches between one-launch sweeps")
        check(one_launch(ctx, 3, grid1, 512), oracle(K, 3), "one launch behind the launch path (the counters carried over)")
        check(one_launch(ctx, 1, grid1, 512), oracle(K, 1), "one launch behind one launch")
        seeds = [31, 32, 33, 34]
        out, logz = one_launch_batch(ctx, seeds, grid4, 512)
        refs = [oracle(K // 4, s) for s in seeds]
        check(out, joined(refs), "a batch of 4 behind single sweeps (another grid: the counters start again)")
        assert logz == [r['logZ'] for r in refs]
        out, logz = one_launch_batch(ctx, seeds[::-1], grid4, 512)
        check(out, joined(refs[::-1]), "the batch again")
        assert logz == [r['logZ'] for r in refs[::-1]]
        check(one_launch(ctx, 5, grid1, 512), oracle(K, 5), "a single sweep behind the batches")


# ---- part B: PHYLO_PERSIST_WGS forced, at both thread counts -----------------------------------------------------------------------

def forced_leaves():
    return primate()[:OC.FORCED_N, 50:50 + OC.FORCED_S]


@functools.lru_cache(maxsize=None)
def forced_refs(G, Kg):
    g = forced_leaves()
    lam = np.full(OC.FORCED_N - 1, 10.0)
    return [CO.sweep(g, gtr(), PI, lam, lam, Kg, s) for s in range(50, 50 + G)]


def run_forced(ctx, G, Kg, grid, nt):
    """(the sweep's arrays, its G log Z), one launch when `grid` is a grid and the launch path when it is None"""
    seeds = list(range(50, 50 + G))
    if G == 1:
        if grid is not None:
            out = one_launch(ctx, seeds[0], grid, nt)
        else:
            out = ctx.sweep(seeds[0], flags=ONE)
            took_launches(ctx, out)
        return out, [out['logZ']]
    if grid is not None:
        return one_launch_batch(ctx, seeds, grid, nt)
    ctx.sweep_batch_async(seeds, flags=ONE)
    logz = ctx.sweep_fetch_logz(G)
    out = ctx.sweep_fetch()
    took_launches(ctx, out)
    return out, list(logz)


@pytest.mark.parametrize("nt", [256, 512])
@pytest.mark.parametrize("case", OC.FORCED, ids=OC.forced_id)
def test_forced_grids(monkeypatch, case, nt):
    wgs, G, Kg, grid = case
    monkeypatch.setenv('PHYLO_PERSIST_WGS', str(wgs))
    monkeypatch.setenv('PHYLO_PERSIST_NT', str(nt))
    g = forced_leaves()
    refs = forced_refs(G, Kg)
    what = "PHYLO_PERSIST_WGS=%d, %d x %d, %d threads" % (wgs, G, Kg, nt)
    with make_ctx(g, G * Kg, gtr()) as ctx:
        out, logz = run_forced(ctx, G, Kg, grid, nt)
        check(out, joined(refs), what)
        assert logz == [r['logZ'] for r in refs], what
        if grid is not None:                                # the launch path of the same context
            if G == 1:
                four = ctx.sweep(50)
                took_launches(ctx, four)
            else:
                four, _ = launches_batch(ctx, list(range(50, 50 + G)))
            check(four, out, what + ": launches against one launch")
            out2, logz2 = run_forced(ctx, G, Kg, grid, nt)  # ... and the grid again behind it
            check(out2, out, what + ": again")
            assert logz2 == logz
        report = ctx.debug_persist() if grid is not None else None
    if wgs > OC.N_CUS * 2:                                  # clamped to the device: what an unforced context reports
        monkeypatch.delenv('PHYLO_PERSIST_WGS')
        with make_ctx(g, G * Kg, gtr()) as ctx:
            ctx.sweep(50, flags=ONE)
            assert ctx.debug_persist() == report
