"""More than 65 taxa without a GPU: the host builders of the reverse pass's lists (phylo_debug_reverse_lists) against the NumPy
restatement of tests/test_revlists_cpu.py on random genealogies of 66, 130 and 512 taxa; the plan rules unchanged at 66 and 130
taxa (pg_nodes_rows_all may be taken, the one-launch coefficient chain is not: it stops at 65 taxa, so above that the coefficients
run as a launch per rank event beside or ahead of it); and the Python layer sizes nothing for 65 taxa."""
import numpy as np
import pytest

from phylo_amd import _ffi
from phylo_amd import train as T
from test_revlists_cpu import FREE, HCHUNK, PCHUNK, _random_genealogy, _reference      # (pytest puts tests/ on sys.path)


@pytest.mark.parametrize("N,K,survivors,early,rows,seed", [
    (66, 24, 3, True, True, 0), (66, 24, 24, True, True, 1), (130, 16, 5, True, True, 2), (130, 16, 16, False, True, 3),
    (512, 6, 2, True, True, 4), (512, 6, 6, True, False, 5),
])
def test_host_lists_match_the_restatement_above_65_taxa(N, K, survivors, early, rows, seed):
    rng = np.random.default_rng(seed)
    R, nn = N - 1, (N - 1) * K
    anc, child = _random_genealogy(rng, N, K, survivors)
    lookahead = [] if seed % 2 else [int(N + x) for x in rng.choice(nn, size=5, replace=False)]
    out = _ffi.debug_reverse_lists(N, K, anc, child, early, rows, lookahead)
    adopters, parents, flags, slow_lists = _reference(N, K, anc, child, early, rows, lookahead)
    assert len(out["ev_adp0"]) == R + 1 == len(out["ev_slow0"])
    n_adp = 0
    for r in range(1, R):
        off = out["ad_off"][r]
        assert off[0] == 0 and off[K] == K
        for k in range(K):
            assert list(out["ad_idx"][r][off[k]:off[k + 1]]) == adopters[r][k], (r, k)
    for r in range(R):
        ev = [r * K + k for k in range(K) if r + 1 < R and adopters[r + 1][k]]
        assert list(out["adp"][out["ev_adp0"][r]:out["ev_adp0"][r + 1]]) == ev, r
        assert (len(ev) > 0) == (r + 1 < R)                  # every rank event but the last has adopted nodes: also 64 and above
        n_adp += len(ev)
    assert out["n_adp"] == n_adp == out["ev_adp0"][R]
    po = out["par_off"]
    assert po[0] == 0 and po[nn] == out["n_par"] == sum(len(p) for p in parents)
    for x in range(nn):
        got = out["par_idx"][po[x]:po[x + 1]]
        if rows and early:
            want = [e for e in parents[x] if flags[e >> 1] == 0] + [e for e in parents[x] if flags[e >> 1] != 0][::-1]
        else:
            want = parents[x]
        assert list(got & (FREE - 1)) == want, x
        for e in got:
            assert bool(e & FREE) == (rows and flags[(int(e) & (FREE - 1)) >> 1] == 0)
    ns = nch = 0
    for r in range(R):
        assert out["ev_slow0"][r] == ns and out["rank_chunk0"][r] == nch
        for x in slow_lists[r]:
            assert out["slow_idx"][ns] == x and out["slow_flag"][x] == (ns << 3 | flags[x])
            ns += 1
        for k in range(K):
            x = r * K + k
            if flags[x] == 0:
                assert out["slow_flag"][x] == 0
            if len(parents[x]) > PCHUNK:
                assert out["heavy"][x] == nch - out["rank_chunk0"][r]
                for b in range(0, len(parents[x]), HCHUNK):
                    assert out["chunk_beg"][nch] == po[x] + b and out["chunk_cnt"][nch] == min(HCHUNK, len(parents[x]) - b)
                    nch += 1
            else:
                assert out["heavy"][x] == -1
    assert out["ev_slow0"][R] == ns == out["n_slow"] and out["rank_chunk0"][R] == nch == out["n_chunks"]


@pytest.mark.parametrize("N", [66, 130])
def test_plan_rules_unchanged_above_65_taxa(N):
    """A small lazy plain sweep with device-built lists: pg_nodes_rows_all is taken (beside the coefficient launches when it is
    small), the one-launch coefficient chain only up to R - 1 = 64."""
    p = _ffi.debug_reverse_plan(N, 24, 40, n_slow=300, coeff_wgs=1500)
    assert p["dev_lists"] and p["rows_all"] and p["rows_overlap"] and not p["interleave"]
    assert p["coeff_all"] == (N - 2 <= 64)
    assert N == 66 or not p["coeff_all"]
    big = _ffi.debug_reverse_plan(N, 24, 40, n_slow=3000, coeff_wgs=1500)
    assert big["rows_all"] and not big["rows_overlap"] and big["coeff_all"] == (N - 2 <= 64)
    assert not _ffi.debug_reverse_plan(N, 24, 40, n_slow=300, coeff_wgs=1500, switches=("rows_chain",))["rows_all"]
    assert not _ffi.debug_reverse_plan(67, 24, 40, n_slow=300, coeff_wgs=1500)["coeff_all"]


def test_python_layer_sizes_nothing_for_65_taxa():
    """Variables, the packed layout and the optimisers for N = 512; a Trainer needs a device and is built in the GPU tests."""
    N = 512
    v = T.Variables(N, np.log(10.0), jcmodel=False)
    p = v.pack()
    assert p.shape == (2 * (N - 1) + 20,)
    g = np.linspace(-1.0, 1.0, p.size)
    un = v.unpack_grads(g)
    assert un['a_l'].shape == (N - 1,) and un['a_r'].shape == (N - 1,) and un['y_q'].shape == (4, 4)
    Q, pi, ll, lr = v.evaluate()
    assert ll.shape == lr.shape == (N - 1,)
    raw = {'d_lam_l': np.ones(N - 1), 'd_lam_r': np.ones(N - 1), 'd_pi': np.ones(4), 'd_Q': np.ones((4, 4))}
    cr = T.chain_rules(v, Q, pi, ll, lr, raw)
    assert cr['a_l'].shape == (N - 1,)
    # the library's optimiser step on 1042 packed variables against the NumPy statement
    v2 = T.Variables(N, np.log(10.0), jcmodel=False)
    a, b = T.Adam(0.02), T.Adam(0.02)
    for _ in range(2):
        a.apply_packed(v, g)
        b.apply(v2, v2.unpack_grads(g))
    np.testing.assert_allclose(v.pack(), v2.pack(), rtol=1e-12, atol=1e-15)


def test_trainer_constructs_for_512_taxa_or_names_the_missing_device():
    """Trainer(...) for N = 512 sizes its context from N alone; without a device the library says so (no refusal of the shape)."""
    N, S = 512, 8
    v = T.Variables(N, np.log(10.0), jcmodel=False)
    if _ffi.device_count() < 1:                              # (the library's own count: 0 without the hardware, and it does not raise)
        with pytest.raises(_ffi.PhyloError) as e:
            T.Trainer(np.ones((N, S, 4)), 4, v, T.GradientDescent(0.0), S)
        assert 'taxa' not in str(e.value) and 'exceeds' not in str(e.value)
        return
    tr = T.Trainer(np.ones((N, S, 4)), 4, v, T.GradientDescent(0.0), S)
    tr.close()
