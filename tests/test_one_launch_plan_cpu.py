"""The grid of the one-launch sweep (persist_plan_of, phylo_amd/csrc/phylo_sweep_plan.h) against a restatement in Python, condition
by condition, and the grids the GPU cases of tests/one_launch_cases.py claim.  Every grid (and the launch path a refusal falls back
to) computes the same bits, so a rule that moves passes every comparison on the device: it has to fail HERE instead of leaving
tests/test_gpu_one_launch_forms.py vacuous.  No GPU: phylo_debug_persist_plan calls the function the driver calls."""
import itertools

import pytest

import one_launch_cases as OC
from phylo_amd import _ffi

ONE = _ffi.FLAGS_DEFAULT | _ffi.ONE_LAUNCH
EINVAL = -1


def _rule(N, K, S, G, flags, sw, world, transport, n_cus, blocks, wgs, nt):
    """persist_plan as the driver spelled it before there was persist_plan_of"""
    env_eager, env_one = ("eager_nodes" in sw), ("one_launch" in sw)
    if not (env_one or flags & _ffi.ONE_LAUNCH):
        return None
    if world != 1 or transport:
        return None
    if flags & (_ffi.TWISTING | _ffi.KEEP_GRAPH | _ffi.TIME_KERNELS):
        return None
    if flags & _ffi.EAGER_NODES or env_eager:
        return None
    if N > 32 or N < 2:
        return None
    Kg = K // G
    if Kg > OC.PP_MAX_KG:
        return None
    if S * 32.0 > 256.0 * 1024.0:
        return None
    if blocks < 1 or n_cus < 1:
        return None
    Wt = wgs if wgs > 0 else n_cus
    Wt = min(Wt, n_cus * blocks)
    if Wt < G:
        return None
    Wg = min(Wt // G, Kg)
    while Wg > 1 and Kg % Wg:
        Wg -= 1
    m = Kg // Wg
    if m > OC.PP_MAX_M:
        return None
    lds = OC.lds_bytes(N, m, Kg)
    if lds > OC.MAX_LDS:
        return None
    return {'nt': 512 if nt == 512 else 256, 'Wg': Wg, 'm': m, 'lds': lds}


def _ask(N, K, S, G=1, flags=ONE, sw=(), world=1, transport=False, n_cus=OC.N_CUS, blocks=OC.BLOCKS_PER_CU, wgs=0, nt=256):
    got = _ffi.debug_persist_plan(N, K, S, G=G, flags=flags, switches=sw, world=world, transport=transport, n_cus=n_cus,
                                  blocks_per_cu=blocks, persist_wgs=wgs, persist_nt=nt)
    assert got == _rule(N, K, S, G, flags, sw, world, transport, n_cus, blocks, wgs, nt), \
        (N, K, S, G, flags, sw, world, transport, n_cus, blocks, wgs, nt, got)
    return got


KGS = (1, 7, 16, 17, 64, 68, 257, 2048, 5000, 8191, 8192, 8193)
WGS = (0, 1, 2, 4, 7, 40, 64, 255, 256, 257, 512, 513, 1000000, -3)


def test_the_grid_over_shapes_devices_and_switches():
    """N x Kg x G x the device's facts x PHYLO_PERSIST_WGS x PHYLO_PERSIST_NT"""
    n = 0
    for N, Kg, G, n_cus, blocks, wgs, nt in itertools.product((1, 2, 12, 32, 33), KGS, (1, 3, 5, 8, 64), (1, 8, 256), (0, 1, 2), WGS,
                                                              (256, 512)):
        n += _ask(N, G * Kg, 130, G=G, n_cus=n_cus, blocks=blocks, wgs=wgs, nt=nt) is not None
    assert n > 10000                                       # (the grid is not all refusals)


def test_sites_flags_switches_and_communicators():
    for S in (1, 8191, 8192, 8193, 50000):
        assert (_ask(12, 2048, S) is not None) == (S <= 8192)
    took = _ask(12, 2048, 898)
    assert took == {'nt': 256, 'Wg': 256, 'm': 8, 'lds': OC.lds_bytes(12, 8, 2048)}
    # opt-in: the flag or the environment
    assert _ask(12, 2048, 898, flags=_ffi.FLAGS_DEFAULT) is None
    assert _ask(12, 2048, 898, flags=_ffi.FLAGS_DEFAULT, sw=("one_launch",)) == took
    assert _ask(12, 2048, 898, flags=0, sw=("one_launch",)) == took        # (the Q1 quirk is not the plan's business)
    # twisting, a kept graph, timing and eager nodes (flag or switch) each refuse, alone and together
    for k in range(1, 5):
        for bits in itertools.combinations((_ffi.TWISTING, _ffi.KEEP_GRAPH, _ffi.TIME_KERNELS, _ffi.EAGER_NODES), k):
            assert _ask(12, 2048, 898, flags=ONE | sum(bits)) is None, bits
    assert _ask(12, 2048, 898, sw=("eager_nodes",)) is None
    assert _ask(12, 2048, 898, sw=("eager_nodes", "one_launch")) is None
    # sharded, or a communicator on one rank
    assert _ask(12, 2048, 898, world=2) is None and _ask(12, 2048, 898, transport=True) is None
    # PHYLO_PERSIST_NT: 512 and nothing else selects the 512-thread form
    assert [_ask(12, 2048, 898, nt=v)['nt'] for v in (512, 256, 0, 1024, 511, -512)] == [512, 256, 256, 256, 256, 256]
    for bad in (dict(K=2047, G=2), dict(K=0), dict(S=0), dict(G=0), dict(world=0)):
        args = dict(N=12, K=2048, S=898, G=1, world=1)
        args.update(bad)
        with pytest.raises(_ffi.PhyloError) as e:
            _ffi.debug_persist_plan(**args)
        assert e.value.code == EINVAL


def test_the_lds_refusal_is_out_of_reach():
    """pp_layout(...).total > 150 KiB cannot happen for a shape the refusals above let through (N <= 32, m <= PP_MAX_M,
    Kg <= PP_MAX_KG): the largest layout is 94 240 bytes.  The layout grows with each of the three, so the corner is the maximum."""
    worst = OC.lds_bytes(OC.MAX_TAXA, OC.PP_MAX_M, OC.PP_MAX_KG)
    assert worst == 94240 and worst < OC.MAX_LDS
    for N, m, Kg in itertools.product((2, 31, 32), (1, 1023, 1024), (1024, 8191, 8192)):
        assert OC.lds_bytes(N, m, Kg) <= worst
    # ... and the library's layout is the restated one at that corner (Wg = 8: m = 1024)
    assert _ask(32, 8192, 8192, wgs=8) == {'nt': 256, 'Wg': 8, 'm': 1024, 'lds': worst}


@pytest.mark.parametrize("name", list(OC.DEFAULT_GRID))
def test_default_grid_cases_claim_their_grid(name):
    c = OC.DEFAULT_GRID[name]
    got = _ask(c["N"], c["G"] * c["Kg"], 130, G=c["G"], nt=512)
    assert got is not None and (got['nt'], got['Wg'], got['m']) == (512, c["Wg"], c["m"])


def test_default_grid_cases_cover_the_chunk_shapes_of_eight_waves():
    """what part A is for: m = 1 (seven idle waves), a last chunk of one particle, a second chunk shorter than the waves, m exactly
    one chunk, m of two chunks"""
    ms = {c["m"] for c in OC.DEFAULT_GRID.values()}
    assert 1 in ms and OC.PP_CHUNK in ms and 2 * OC.PP_CHUNK in ms
    assert any(m > OC.PP_CHUNK and m % OC.PP_CHUNK == 1 for m in ms)
    assert any(m > OC.PP_CHUNK and 1 < m % OC.PP_CHUNK < 8 for m in ms)


@pytest.mark.parametrize("nt", [256, 512])
@pytest.mark.parametrize("case", OC.FORCED, ids=OC.forced_id)
def test_forced_cases_claim_their_grid(case, nt):
    wgs, G, Kg, claim = case
    got = _ask(OC.FORCED_N, G * Kg, OC.FORCED_S, G=G, wgs=wgs, nt=nt)
    if claim is None:
        assert got is None
    else:
        assert (got['nt'], got['Wg'], got['m']) == (nt, claim[0], claim[1])
        assert got['Wg'] * got['m'] == Kg and G * got['Wg'] <= OC.N_CUS * OC.BLOCKS_PER_CU


def test_forced_cases_are_what_they_say():
    F = {OC.forced_id(c): c[3] for c in OC.FORCED}
    assert F["wgs4-1x64"][1] == OC.PP_CHUNK and F["wgs4-1x68"][1] == OC.PP_CHUNK + 1 and F["wgs2-1x2048"][1] == OC.PP_MAX_M
    assert 2048 % 7 != 0 and F["wgs7-1x2048"][0] == 4       # the walk down to a divisor
    assert 2048 > OC.PP_MAX_M and F["wgs1-1x2048"] is None
    # the clamp: a request above the device gives the unforced grid with one workgroup per CU admitted, and twice the grid with two
    unforced = _ask(OC.FORCED_N, 2048, OC.FORCED_S)
    assert _ask(OC.FORCED_N, 2048, OC.FORCED_S, wgs=1000000) == unforced
    assert (unforced['Wg'], unforced['m']) == F["wgs1000000-1x2048"]
    assert _ask(OC.FORCED_N, 2048, OC.FORCED_S, wgs=1000000, blocks=2)['Wg'] == 2 * unforced['Wg']
