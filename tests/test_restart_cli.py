"""Restarting a replica farm, without a device: the command line refuses --restart-from / --audit without --replicas, and
run_replicas refuses a restart with a reservoir or from a directory that lacks a replica, naming the cause, before any
engine exists."""
import os
import shutil

import pytest

from maniac_mc_amd import run
from maniac_mc_amd.replicas import run_replicas
from tests.util import GOLDEN

RUNS = os.path.join(GOLDEN, "runs")


def _inputs(case):
    d = os.path.join(RUNS, case, "inputs")
    return os.path.join(d, "system.maniac"), os.path.join(d, "system.data"), os.path.join(d, "system.inc")


@pytest.mark.parametrize("argv", [["--restart-from", "somewhere"], ["--audit"], ["--restart-from", "somewhere", "--audit"]])
def test_cli_needs_replicas(argv, capsys):
    with pytest.raises(SystemExit) as ex:
        run.main(["-i", "a.maniac", "-d", "a.data", "-p", "a.inc"] + argv)
    assert ex.value.code == 2
    assert "need --replicas" in capsys.readouterr().err


def _restart_dir(tmp_path, replicas):
    """A directory as run_replicas leaves it, as far as a restart reads it: replica_NNNN/topology.data"""
    src = os.path.join(RUNS, "co2_gcmc", "expected", "topology.data")
    root = tmp_path / "earlier"
    for r in replicas:
        os.makedirs(root / f"replica_{r:04d}")
        shutil.copy(src, root / f"replica_{r:04d}" / "topology.data")
    return str(root)


def test_restart_with_a_reservoir_is_refused(tmp_path):
    maniac, data, inc = _inputs("co2_gcmc")
    root = _restart_dir(tmp_path, range(3))
    rsv = os.path.join(RUNS, "dumbbell_gcmc_reservoir", "inputs", "reservoir.data")
    with pytest.raises(ValueError, match="reservoir"):
        run_replicas(maniac, data, inc, str(tmp_path / "out"), replicas=3, restart_from=root, reservoir_path=rsv)
    assert not os.path.exists(tmp_path / "out")


def test_a_missing_replica_is_named(tmp_path):
    maniac, data, inc = _inputs("co2_gcmc")
    root = _restart_dir(tmp_path, (0, 1))
    with pytest.raises(ValueError, match="replica_0002") as ex:
        run_replicas(maniac, data, inc, str(tmp_path / "out"), replicas=3, restart_from=root)
    assert os.path.join(root, "replica_0002", "topology.data") in str(ex.value)
    # the directory without its file
    os.makedirs(os.path.join(root, "replica_0002"))
    with pytest.raises(ValueError, match="replica_0002"):
        run_replicas(maniac, data, inc, str(tmp_path / "out"), replicas=3, restart_from=root)
    assert not os.path.exists(tmp_path / "out")


def test_counts_above_the_capacity_are_refused(tmp_path):
    maniac, data, inc = _inputs("co2_gcmc")
    root = _restart_dir(tmp_path, range(2))
    with pytest.raises(ValueError, match="capacity"):
        run_replicas(maniac, data, inc, str(tmp_path / "out"), replicas=2, restart_from=root, mol_capacity=[1])
