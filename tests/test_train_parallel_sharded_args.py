"""runner.py --train_parallel sharded: parsing, and its refusal together with the twisted proposal (no GPU needed)."""
import pytest

import runner


def test_sharded_parses():
    args = runner.parse_args(['--n_gpus', '2', '--train_parallel', 'sharded'])
    assert args.train_parallel == 'sharded' and not args.nested


def test_replicas_stays_the_default():
    assert runner.parse_args([]).train_parallel == 'replicas'


@pytest.mark.parametrize("flag", ['--nested', '--twisting'])
def test_sharded_with_the_twisted_proposal_is_refused(flag, capsys):
    with pytest.raises(SystemExit) as e:
        runner.parse_args(['--n_gpus', '2', '--train_parallel', 'sharded', flag, 'true'])
    assert e.value.code == 2
    assert 'plain proposal' in capsys.readouterr().err
