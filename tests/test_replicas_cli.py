"""CPU checks of the replica front end (maniac_mc_amd.replicas, run.py --replicas): argument parsing and its refusals."""
import os
import subprocess
import sys

import pytest

from maniac_mc_amd import replicas, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_frames():
    assert replicas.parse_frames("0,3,7", 8) == (0, 3, 7)
    assert replicas.parse_frames("7,0,0", 8) == (0, 7)
    assert replicas.parse_frames("all", 3) == (0, 1, 2)
    assert replicas.parse_frames("none", 3) == ()
    for bad in ("0,8", "-1", "x", "1,,2"):
        with pytest.raises(ValueError):
            replicas.parse_frames(bad, 8)


def test_parse_fugacities():
    assert replicas.parse_fugacities("1,2.5,1e3") == [1.0, 2.5, 1000.0]
    for bad in ("1,0", "-2", "a,b", ""):
        with pytest.raises(ValueError):
            replicas.parse_fugacities(bad)


@pytest.mark.parametrize("argv, message", [
    (["--replicas", "4", "--as-written"], "--as-written cannot be combined with --replicas"),
    (["--replicas", "4", "--frames", "0,4"], "--frames"),
    (["--replicas", "4", "--frames", "some"], "--frames"),
    (["--replicas", "0"], "--replicas must be at least 1"),
    (["--replicas", "2", "--fugacities", "1,-1"], "--fugacities"),
    (["--frames", "1"], "need --replicas"),
    (["--farm-mode", "host"], "need --replicas"),
    (["--replicas", "2", "--farm-mode", "fast"], "invalid choice"),
])
def test_cli_refusals(argv, message, capsys):
    with pytest.raises(SystemExit) as ex:
        run.main(["-i", "a.maniac", "-d", "a.data", "-p", "a.inc"] + argv)
    assert ex.value.code == 2
    assert message in capsys.readouterr().err


def test_cli_refusal_in_a_child_process():
    p = subprocess.run([sys.executable, "-m", "maniac_mc_amd.run", "-i", "a", "-d", "b", "-p", "c", "--replicas", "2",
                        "--as-written"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--as-written cannot be combined with --replicas" in p.stderr
