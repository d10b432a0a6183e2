"""Checkpoint a replica farm and resume it bit for bit (run_replicas(checkpoint_every=..., resume=True)): run A does four
blocks in one go; run B does two with a checkpoint after each, and a SECOND run_replicas with a new engine and a new farm
finishes it in the same directory.  The trees of A and B are the same bytes file for file (checkpoint/ and the lines that name
the directory aside), the results' energies, counts and chain counters are equal, and so are the engines' final state blocks.
Windows (NVT at depth 2 and grand-canonical), a reservoir, the host-built farm `auto` picks for a triclinic input, the explicit
device-built and device-decided modes, and a run whose step sizes are recalibrated before the checkpoint.

Sizes as tests/test_gpu_farm_restart.py's (R = 3, 40 steps a block); the recalibrated case takes 200 steps a block, the fewest
with which the pooled counters pass the reference's 500 trials before the checkpoint."""
import os

import numpy as np
import pytest

from maniac_mc_amd import checkpoint, replicas
from maniac_mc_amd.fortran_host import FortranFarm
from maniac_mc_amd.replicas import run_replicas
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "runs")
R, BLOCKS, CUT, STEPS = 3, 4, 2, 40

# name -> (fixture, keyword arguments of run_replicas)
CASES = {
    "spce_nvt": ("spce_nvt", {}),
    "co2_gcmc": ("co2_gcmc", {}),
    "dumbbell_gcmc_reservoir": ("dumbbell_gcmc_reservoir", {}),
    "spce_triclinic_nvt": ("spce_triclinic_nvt", {}),
    "co2_gcmc_device": ("co2_gcmc", dict(mode="device")),
    "co2_gcmc_device_accept": ("co2_gcmc", dict(mode="device_accept")),
    "spce_nvt_recalibrated": ("spce_nvt", dict(recalibrate_moves=True, nb_step=200)),
}
MODE_RAN = {"spce_nvt": "windows", "co2_gcmc": "windows", "dumbbell_gcmc_reservoir": "windows", "spce_triclinic_nvt": "host",
            "co2_gcmc_device": "device", "co2_gcmc_device_accept": "device_accept", "spce_nvt_recalibrated": "windows"}


def _args(name):
    fixture, kw = CASES[name]
    d = os.path.join(RUNS, fixture, "inputs")
    kw = dict(dict(replicas=R, seed=5, nb_step=STEPS), **kw)
    if os.path.isfile(os.path.join(d, "reservoir.data")):
        kw["reservoir_path"] = os.path.join(d, "reservoir.data")
    return (os.path.join(d, "system.maniac"), os.path.join(d, "system.data"), os.path.join(d, "system.inc")), kw


def _tree(path):
    out = {}
    for base, dirs, files in os.walk(path):
        dirs[:] = [d for d in dirs if not (base == path and d == checkpoint.DIR_NAME)]
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, path)] = open(p, "rb").read()
    return out


def _without_dir(data, root):
    return b"\n".join(ln for ln in data.split(b"\n") if str(root).encode() not in ln)


def _same_trees(a_dir, b_dir, parent, what):
    ta, tb = _tree(a_dir), _tree(b_dir)
    print(what, "files", len(ta), len(tb), "bytes", sum(map(len, ta.values())), sum(map(len, tb.values())))
    assert sorted(ta) == sorted(tb), (what, sorted(set(ta) ^ set(tb)))
    for name in sorted(ta):
        x, y = _without_dir(ta[name], parent), _without_dir(tb[name], parent)
        if x != y:
            k = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
            raise AssertionError(f"{what}: {name} differs: {len(x)} and {len(y)} bytes, first difference at byte {k}: "
                                 f"{x[max(0, k - 60): k + 60]!r} | {y[max(0, k - 60): k + 60]!r}")


def _same_results(a, b, what):
    for key in ("energy", "counts", "chain_counters"):
        assert np.array_equal(a[key], b[key]), (what, key, a[key], b[key])
    assert a["counters"] == b["counters"] and a["mode"] == b["mode"]
    assert len(a["state"]) == len(b["state"])
    for x, y in zip(a["state"], b["state"]):
        diff = np.nonzero(x[: min(len(x), len(y))] != y[: min(len(x), len(y))])[0]
        assert len(x) == len(y) and not len(diff), f"{what}: engine blocks of {len(x)} and {len(y)} bytes, first difference at byte {diff[:1]}"


@pytest.fixture(autouse=True)
def _final_engine_state(monkeypatch):
    """run_replicas closes its farm: the engine's final state block is taken just before, into the result"""
    taken = []
    close = FortranFarm.close

    def closing(self):
        if getattr(self, "slot", -1) in FortranFarm._slots and self.eng.h:
            taken.append(self.checkpoint_state()["engine"])
        close(self)
    monkeypatch.setattr(FortranFarm, "close", closing)
    run = replicas.run_replicas

    def _run(*args, **kw):
        res = run(*args, **kw)
        res["state"] = taken.pop()
        return res
    yield _run


def _counts_at_checkpoint(out):
    """molecule counts per replica in the engine blocks of the checkpoint of `out`"""
    from maniac_mc_amd.engine import state_unpack
    ck = checkpoint.load(out)
    return [tuple(rep["n"]) for blk in ck["engine"] for rep in state_unpack(blk)], ck


@pytest.mark.parametrize("name", sorted(CASES))
def test_a_resumed_run_is_the_uninterrupted_one(name, tmp_path, _final_engine_state):
    run = _final_engine_state
    inputs, kw = _args(name)
    a_dir, b_dir = str(tmp_path / "A"), str(tmp_path / "B")
    a = run(*inputs, a_dir, nb_block=BLOCKS, **kw)
    assert a["mode"] == MODE_RAN[name]
    assert not os.path.exists(os.path.join(a_dir, checkpoint.DIR_NAME)), "a default run writes no checkpoint"
    run(*inputs, b_dir, nb_block=CUT, checkpoint_every=1, **kw)
    counts, ck = _counts_at_checkpoint(b_dir)
    assert int(ck["next_block"]) == CUT + 1 and str(ck["mode_ran"]) == MODE_RAN[name]
    print(name, "counts at the checkpoint", counts)
    if name == "co2_gcmc":
        assert len(set(counts)) > 1, "the replicas' counts differ at the checkpoint"
    b = run(*inputs, b_dir, nb_block=BLOCKS, resume=True, **kw)
    _same_trees(a_dir, b_dir, str(tmp_path), name)
    _same_results(a, b, name)
    if name == "spce_nvt_recalibrated":
        # the step sizes the checkpoint carries (the two words behind the fugacities of the driver's block: mc_farm.f90,
        # state_walk) are no longer the input's: 1200 pooled trials had passed the reference's threshold of 500 translations
        from maniac_mc_amd import io_maniac
        inp = io_maniac.load_system(*inputs)[1]
        at = 16 + 3 * 1 + 4 * R + R + 5 * R + R
        steps = np.frombuffer(ck["driver"], np.float64)[at: at + 2]
        print(name, "carried steps", steps, "input", inp.translation_step, inp.rotation_step_angle)
        assert 1e-3 <= steps[0] <= 3.0 and steps[0] != inp.translation_step


def test_a_killed_run_is_cut_back_to_its_checkpoint(tmp_path, _final_engine_state):
    """after run B's checkpoint: garbage appended to two output files and a stray temporary checkpoint -- what a run killed
    in its third block leaves -- and the resume still reproduces A; with --audit it reports the carried running energies"""
    run = _final_engine_state
    inputs, kw = _args("co2_gcmc")
    a_dir, b_dir = str(tmp_path / "A"), str(tmp_path / "B")
    a = run(*inputs, a_dir, nb_block=BLOCKS, **kw)
    run(*inputs, b_dir, nb_block=CUT, checkpoint_every=2, **kw)
    for name in (os.path.join("replica_0001", "energy.dat"), "replicas.dat"):
        with open(os.path.join(b_dir, name), "ab") as f:
            f.write(b"         3   garbage of a block that never finished\n")
    with open(os.path.join(b_dir, checkpoint.DIR_NAME, checkpoint.TMP_NAME), "wb") as f:
        f.write(b"torn")
    b = run(*inputs, b_dir, nb_block=BLOCKS, resume=True, audit=True, **kw)
    assert np.array_equal(b["audit"]["running"], a["energy"])
    os.remove(os.path.join(b_dir, "audit.dat"))
    _same_trees(a_dir, b_dir, str(tmp_path), "killed")
    _same_results(a, b, "killed")
    # once more from the same checkpoint: the finished run is cut back to it and finished again, the same files
    c = run(*inputs, b_dir, nb_block=BLOCKS, resume=True, **kw)
    _same_trees(a_dir, b_dir, str(tmp_path), "resumed twice")
    _same_results(a, c, "resumed twice")


def test_a_default_run_creates_no_checkpoint(tmp_path):
    inputs, kw = _args("spce_nvt")
    out = str(tmp_path / "Z")
    run_replicas(*inputs, out, nb_block=1, **kw)
    assert sorted(os.listdir(out)) == sorted(["replicas.dat"] + [f"replica_{r:04d}" for r in range(R)])
