"""The chain form of a rank event (sweep_chain_form_of, phylo_sweep_plan.h), restated: the scan hands out
ancestors and adopted particles, the bookkeeping reads its ancestor, the adopted nodes are written from the list.  No GPU: the rule
through phylo_debug_sweep_chain at both sides of every condition, and phylo_debug_sweep_plan's output for the same facts, which
the switch must not move."""
import pytest

from phylo_amd import _ffi

S = 898


def restated(N, K, S, G=1, world=1, K_local=None, transport=False, flags=0, switches=(), multi_min=4096, scan_ancestors=1):
    plan = _ffi.debug_sweep_plan(N, K, S, K_local=K_local, G=G, world=world, transport=transport, flags=flags, switches=switches)
    taken = (scan_ancestors != 0 and plan['use_rec'] and plan['mat_after_book'] and not plan['mat_barrier'] and N - 1 >= 2
             and _ffi.debug_scan_form(K // G, multi_min=multi_min) in ('lds512', 'lds1024'))
    if not taken:
        return {'taken': False, 'item_waves': 0, 'parts': 0}
    q = min(-(-S // 128), 8)
    return {'taken': True, 'item_waves': min((K // G) * q, 128), 'parts': q}


def both(**kw):
    got = _ffi.debug_sweep_chain(**kw)
    assert got == restated(**kw), kw
    return got


def test_the_flagship_takes_it():
    got = both(N=12, K=40960, S=S, G=20)
    assert got == {'taken': True, 'item_waves': 128, 'parts': 8}


def test_one_group_small_and_large():
    # a single small sweep writes its adopted nodes in the bookkeeping launch (book_mat): today's launches
    assert not both(N=12, K=2048, S=S)['taken']
    assert not both(N=12, K=8192, S=S)['taken']
    # above 8192 particles the separate launch is back, but one group of that size is scanned by several workgroups ...
    assert not both(N=12, K=8256, S=S)['taken']
    # ... unless PHYLO_SCAN_MULTI_MIN says otherwise: pp_resample_scan<1024> holds the cdf in LDS up to 16384 weights
    assert both(N=12, K=8256, S=S, multi_min=1 << 20)['taken']
    assert both(N=12, K=16384, S=S, multi_min=1 << 20)['taken']
    assert not both(N=12, K=16385, S=S, multi_min=1 << 20)['taken']          # staged in the cdf buffer itself


def test_batched():
    for G, Kg in ((2, 64), (3, 96), (16, 512), (20, 2048), (64, 1)):
        assert both(N=12, K=G * Kg, S=S, G=G)['taken'], (G, Kg)


def test_group_size_at_the_scan_threshold():
    assert both(N=12, K=2 * 4096, S=S, G=2)['taken']
    assert not both(N=12, K=2 * 4097, S=S, G=2)['taken']
    assert both(N=12, K=2 * 4097, S=S, G=2, multi_min=8192)['taken']
    assert not both(N=12, K=2 * 2048, S=S, G=2, multi_min=2047)['taken']


def test_everything_else_keeps_its_launches():
    assert not both(N=12, K=4096, S=S, G=2, transport=True)['taken']
    assert not both(N=12, K=4096, S=S, G=2, transport=True, switches=('rehearse_sharded',))['taken']
    assert not both(N=12, K=16384, S=S, world=2, K_local=8192, transport=True)['taken']
    assert not both(N=12, K=16384, S=S, flags=_ffi.TWISTING)['taken']
    assert not both(N=12, K=4096, S=S, G=2, flags=_ffi.EAGER_NODES)['taken']
    assert not both(N=12, K=4096, S=S, G=2, switches=('eager_nodes',))['taken']
    assert not both(N=2, K=4096, S=S, G=2)['taken']                           # one rank event: nothing is resampled
    # a kept graph of one site tile stays lazy and takes it; longer rows are stored by their merges
    assert both(N=12, K=4096, S=S, G=2, flags=_ffi.KEEP_GRAPH)['taken']
    assert not both(N=12, K=16384, S=5000, flags=_ffi.KEEP_GRAPH, multi_min=1 << 20)['taken']


def test_the_switch():
    for sw in (0, 1, 2):                                   # PHYLO_SCAN_ANCESTORS=0 alone switches it off
        assert both(N=12, K=40960, S=S, G=20, scan_ancestors=sw)['taken'] == (sw != 0)


@pytest.mark.parametrize("S_, parts", [(1, 1), (128, 1), (129, 2), (256, 2), (257, 3), (898, 8), (1024, 8), (5000, 8)])
def test_parts_of_a_node(S_, parts):
    assert both(N=12, K=4096, S=S_, G=2)['parts'] == parts
    assert both(N=12, K=2 * 3, S=S_, G=2)['item_waves'] == 3 * parts           # never more waves than items


def test_the_plan_does_not_know_the_switch(monkeypatch):
    """phylo_debug_sweep_plan has no argument for it; the environment must not reach it either"""
    cases = [dict(N=12, K=40960, S=S, G=20), dict(N=12, K=2048, S=S), dict(N=50, K=4096, S=300, G=2), dict(N=12, K=4096, S=S, G=2, flags=_ffi.KEEP_GRAPH)]
    before = [_ffi.debug_sweep_plan(**c) for c in cases]
    for v in ('0', '1'):
        monkeypatch.setenv('PHYLO_SCAN_ANCESTORS', v)
        assert [_ffi.debug_sweep_plan(**c) for c in cases] == before
    assert before[0]['mat_after_book'] and before[0]['use_rec'] and before[0]['book_width'] == 8
    assert before[0]['launches'][2] == 4                                       # bookkeeping, adopted nodes, merge, scan: the stages
