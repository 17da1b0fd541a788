"""phylo_amd.treetests (bootstrap proportions, KH, SH, c-ELW from a RELL replicate matrix) against loop restatements
(tests/rell_ref.py) on hand-made matrices.  ImportError without the module."""
import numpy as np
import pytest

import rell_ref
from phylo_amd.treetests import tree_tests

TOL = 1e-12


def wins_of(R):
    return np.bincount(rell_ref.first_argmax(np.asarray(R)), minlength=len(R)).astype(np.int64)


def check(obs, R):
    obs, R = np.asarray(obs, dtype=float), np.asarray(R, dtype=float)
    B = R.shape[1]
    got = tree_tests(obs, wins_of(R), B, reps=R)
    want = rell_ref.tree_tests_loops(obs.tolist(), R.tolist())
    for key in ('bp', 'p_kh', 'p_sh', 'c_elw'):
        np.testing.assert_allclose(got[key], want[key], rtol=0, atol=TOL, err_msg=key)
    assert got['bp'].sum() == pytest.approx(1.0, abs=TOL) and got['c_elw'].sum() == pytest.approx(1.0, abs=TOL)
    assert got['best'] == int(np.argmax(obs))
    assert got['p_kh'][got['best']] == 1.0 and got['p_sh'][got['best']] == 1.0
    assert ((got['p_sh'] >= got['p_kh'] - TOL)).all()                      # SH is the more conservative test
    only = tree_tests(obs, wins_of(R), B)
    assert list(only) == ['bp']
    np.testing.assert_array_equal(only['bp'], got['bp'])
    return got


def test_random_matrices():
    r = np.random.default_rng(3)
    for T, B in ((1, 1), (2, 5), (5, 40), (9, 200)):
        obs = -1000.0 - np.sort(r.uniform(0, 12, size=T))
        R = obs[:, None] + r.normal(scale=4.0, size=(T, B)) + r.normal(scale=20.0, size=(1, B))
        check(obs, R)


def test_hand_made_numbers():
    obs = [-10.0, -12.0, -11.0]
    R = [[-10.0, -13.0, -9.0, -12.0],
         [-12.5, -12.0, -12.0, -13.0],
         [-11.0, -12.5, -11.5, -11.0]]
    got = check(obs, R)
    np.testing.assert_array_equal(got['bp'], [0.5, 0.25, 0.25])
    # KH for tree 1: d = [2.5, -1, 3, 1], mean 1.375, centred [1.125, -2.375, 1.625, -0.375] >= 2 never
    np.testing.assert_array_equal(got['p_kh'], [1.0, 0.0, 0.25])
    np.testing.assert_array_equal(got['delta'], [0.0, 2.0, 1.0])


def test_a_duplicated_best_tree_and_a_tree_that_never_wins():
    r = np.random.default_rng(8)
    B = 50
    row = -500.0 + r.normal(scale=3.0, size=B)
    R = np.stack([row, row, row - 1.0 - r.uniform(0, 2, size=B), row + r.normal(scale=3.0, size=B) - 2.0])
    obs = np.array([-500.0, -500.0, -502.0, -502.5])
    got = check(obs, R)
    assert got['best'] == 0
    assert got['p_kh'][1] == 1.0 and got['p_sh'][1] == 1.0               # the copy of the best tree is never rejected
    assert got['bp'][1] == 0.0 and got['bp'][0] > 0                       # ... and every tie of the two goes to the lower index
    assert got['bp'][2] == 0.0 and wins_of(R)[2] == 0                     # tree 2 is below tree 0 in every replicate
    assert got['c_elw'][0] == got['c_elw'][1] > got['c_elw'][2] > 0


def test_bad_arguments():
    with pytest.raises(ValueError):
        tree_tests([-1.0, -2.0], [3, 1], 5)
    with pytest.raises(ValueError):
        tree_tests([-1.0, -2.0], [3, 2], 5, reps=np.zeros((2, 4)))
    with pytest.raises(ValueError):
        tree_tests([-1.0, -2.0], [5], 5)


def test_runner_parses_tree_tests(capsys):
    import runner
    from phylo_amd.treetests import parse_spec
    assert parse_spec('200') == (200, 0) and parse_spec('200:3') == (200, 3) and parse_spec('1:18446744073709551615')[1] == 2 ** 64 - 1
    for bad in ('', '0', 'x', '5:y', '1:2:3', '1048577', '5:-1'):
        with pytest.raises(ValueError):
            parse_spec(bad)
    a = runner.parse_args(['--score_trees', 'trees.nwk', '--tree_tests', '200:3'])
    assert a.tree_tests == '200:3'
    assert runner.parse_args(['--score_trees', 'trees.nwk']).tree_tests is None and runner.parse_args([]).tree_tests is None
    for argv, what in ((['--tree_tests', '200'], '--score_trees'), (['--score_trees', 'trees.nwk', '--tree_tests', '0'], 'B must be')):
        with pytest.raises(SystemExit):
            runner.parse_args(argv)
        assert what in capsys.readouterr().err
