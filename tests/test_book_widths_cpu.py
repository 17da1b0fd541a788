"""What tests/test_gpu_book_widths.py stands on, checked without a GPU: the plan gives every case of tests/book_width_cases.py the
bookkeeping kernel at 64 lanes per particle and not the combined launch (a threshold that moves later fails HERE instead of
leaving the GPU test green and no longer reaching the kernel), the sharded case advances owner-held tables, the 257-taxon cases
meet more key blocks than a wave has lanes to spare, and the oracle's sweep there is a usable reference."""
import numpy as np
import pytest

import book_width_cases as BC
from phylo_amd import _ffi


@pytest.mark.parametrize("name", BC.NAMES)
def test_cases_take_the_bookkeeping_kernel_at_64_lanes(name):
    c = BC.CASES[name]
    flag_sets = (0, _ffi.EAGER_NODES, _ffi.KEEP_GRAPH) if name == "key-loop" else (0,)
    for flags in flag_sets:
        p = _ffi.debug_sweep_plan(c["N"], c["G"] * c["Kg"], BC.S, G=c["G"], flags=flags)
        assert p["book_width"] == 64 and not p["book_mat"] and not p["twist"] and not p["shard_form"], (name, flags, p)
        assert p["batched"] == (c["G"] > 1)
        assert p["lazy"] == (flags != _ffi.EAGER_NODES) and p["graph"] == (flags == _ffi.KEEP_GRAPH)


def test_the_limit_of_the_combined_launch_lies_between_the_cases():
    """one sweep alone: 64 taxa share a launch with the adopted nodes, 65 do not; 33 taxa would, but for the batch"""
    assert _ffi.debug_sweep_plan(64, 16, BC.S)["book_mat"] and not _ffi.debug_sweep_plan(65, 16, BC.S)["book_mat"]
    assert _ffi.debug_sweep_plan(33, 16, BC.S)["book_mat"] and not _ffi.debug_sweep_plan(33, 16, BC.S, G=2)["book_mat"]
    assert _ffi.debug_sweep_plan(32, 16, BC.S, G=2)["book_width"] == 32


def test_sharded_case_advances_owner_held_tables_at_64_lanes():
    c = BC.SHARDED
    p = _ffi.debug_sweep_plan(c["N"], c["K"], c["S"], K_local=c["K"] // c["world"], world=c["world"], transport=True)
    assert p["local_book"] and p["shard_form"] and p["lazy"] and not p["replicated_book"] and not p["book_mat"]
    assert p["book_width"] == 64


def test_twisted_case_launches_no_bookkeeping():
    c = BC.TWISTED
    p = _ffi.debug_sweep_plan(c["N"], c["K"], c["S"], M=c["M"], flags=_ffi.TWISTING)
    assert p["twist"] and p["book_width"] == 0


def test_key_blocks_of_257_taxa():
    """rank event r has n = N - r root slots and (n + 3) // 4 key blocks; 63 fit beside the resampling counter of a wave"""
    blocks = [(257 - r + 3) // 4 for r in range(256)]
    assert blocks[:6] == [65, 64, 64, 64, 64, 63] and max(blocks[5:]) == 63
    assert all((N - r + 3) // 4 <= 63 for N in (33, 65) for r in range(N - 1))


def test_oracle_sweep_of_257_taxa_is_a_usable_reference():
    ref, = BC.reference("key-loop")
    assert np.isfinite(ref["logZ"]) and np.isfinite(ref["log_weights"]).all() and np.isfinite(ref["log_likelihood"]).all()
    assert ref["ancestors"].shape == (255, 8)
    distinct = [len(np.unique(row)) for row in ref["ancestors"]]
    assert 1 <= min(distinct) and max(distinct) > 1
    # adoption is exercised inside the key loop's rank events: some particle there takes another one's table
    assert (ref["ancestors"][:4] != np.arange(8)).any()
