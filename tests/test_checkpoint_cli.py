"""Checkpointing a replica farm, without a device: the command line takes --checkpoint-every / --resume only with --replicas
and refuses --resume with --restart-from; run_replicas refuses the same pair, a resume without a checkpoint and a resume of
another run, naming the cause, before any engine exists."""
import os

import numpy as np
import pytest

from maniac_mc_amd import _lib, checkpoint, run
from maniac_mc_amd.replicas import run_replicas
from tests.util import GOLDEN

RUNS = os.path.join(GOLDEN, "runs")


def _inputs(case):
    d = os.path.join(RUNS, case, "inputs")
    return os.path.join(d, "system.maniac"), os.path.join(d, "system.data"), os.path.join(d, "system.inc")


@pytest.mark.parametrize("argv", [["--checkpoint-every", "2"], ["--resume"], ["--checkpoint-every", "1", "--resume"]])
def test_cli_needs_replicas(argv, capsys):
    with pytest.raises(SystemExit) as ex:
        run.main(["-i", "a.maniac", "-d", "a.data", "-p", "a.inc"] + argv)
    assert ex.value.code == 2
    assert "need --replicas" in capsys.readouterr().err


@pytest.mark.parametrize("argv,said", [(["--resume", "--restart-from", "somewhere"], "--restart-from"),
                                       (["--checkpoint-every", "-1"], "--checkpoint-every"),
                                       (["--checkpoint-every", "often"], "--checkpoint-every")])
def test_cli_refusals(argv, said, capsys):
    with pytest.raises(SystemExit) as ex:
        run.main(["-i", "a.maniac", "-d", "a.data", "-p", "a.inc", "--replicas", "3"] + argv)
    assert ex.value.code == 2
    assert said in capsys.readouterr().err


def test_cli_passes_the_flags_on(monkeypatch, tmp_path):
    seen = {}

    def fake(*args, **kw):
        seen.update(kw)
        return dict(mode="windows", accepted=0)
    from maniac_mc_amd import replicas
    monkeypatch.setattr(replicas, "run_replicas", fake)
    maniac, data, inc = _inputs("co2_gcmc")
    base = ["-i", maniac, "-d", data, "-p", inc, "-o", str(tmp_path / "o"), "--replicas", "3"]
    assert run.main(base) == 0
    assert seen["checkpoint_every"] == 0 and seen["resume"] is False, "both are off by default"
    assert run.main(base + ["--checkpoint-every", "2", "--resume"]) == 0
    assert seen["checkpoint_every"] == 2 and seen["resume"] is True


def test_resume_with_restart_from_is_refused(tmp_path):
    maniac, data, inc = _inputs("co2_gcmc")
    with pytest.raises(ValueError, match="restart_from"):
        run_replicas(maniac, data, inc, str(tmp_path / "out"), replicas=3, resume=True, restart_from=str(tmp_path))
    with pytest.raises(ValueError, match="checkpoint_every"):
        run_replicas(maniac, data, inc, str(tmp_path / "out"), replicas=3, checkpoint_every=-2)
    assert not os.path.exists(tmp_path / "out")


def test_resume_without_a_checkpoint_is_named(tmp_path):
    maniac, data, inc = _inputs("co2_gcmc")
    with pytest.raises(ValueError, match="no checkpoint") as ex:
        run_replicas(maniac, data, inc, str(tmp_path / "out"), replicas=3, resume=True)
    assert checkpoint.path_of(str(tmp_path / "out")) in str(ex.value)
    assert not os.path.exists(tmp_path / "out")


def test_resume_of_another_run_is_named(tmp_path):
    """a checkpoint of 3 replicas at seed 5, 40 steps a block, with a reservoir: every other run is told what differs"""
    maniac, data, inc = _inputs("dumbbell_gcmc_reservoir")
    rsv = os.path.join(RUNS, "dumbbell_gcmc_reservoir", "inputs", "reservoir.data")
    out = str(tmp_path / "out")
    ident = checkpoint.identity(_lib.ABI_VERSION, 40, 5, "auto", 3, None, (0,), maniac, data, inc, rsv)
    ident["recalibrate"] = 1
    checkpoint.save(out, ident, 3, 4, "windows", [np.zeros(8, np.uint8)], np.zeros(8, np.uint8), {})
    kw = dict(replicas=3, seed=5, nb_step=40, nb_block=4, reservoir_path=rsv, resume=True)
    for change, named in ((dict(replicas=4), "R"), (dict(seed=6), "seed"), (dict(nb_step=50), "nb_step"), (dict(mode="host"), "mode"),
                          (dict(reservoir_path=None), "reservoir"), (dict(frames=(0, 1)), "frames"), (dict(nb_block=1), "nb_block"),
                          (dict(fugacities=[1.0, 2.0]), "fugacities"), (dict(recalibrate_moves=False), "recalibrate_moves")):
        with pytest.raises(ValueError, match=named):
            run_replicas(maniac, data, inc, out, **{**kw, **change})
    other = tmp_path / "system.maniac"                           # the same input with one more line feed: other bytes
    other.write_bytes(open(maniac, "rb").read() + b"\n")
    with pytest.raises(ValueError, match="digest"):
        run_replicas(str(other), data, inc, out, **kw)
    ident["abi_version"] = _lib.ABI_VERSION + 1
    checkpoint.save(out, ident, 3, 4, "windows", [np.zeros(8, np.uint8)], np.zeros(8, np.uint8), {})
    with pytest.raises(ValueError, match="ABI version"):
        run_replicas(maniac, data, inc, out, **kw)
    assert sorted(os.listdir(out)) == ["checkpoint"], "nothing was created beside the checkpoint"
