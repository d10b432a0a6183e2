"""Every mode of the single-chain driver (mc_chain.f90: draw -> evaluate -> resolve) at the edges where a step draws fewer
numbers or none: an emptied one-site type (lj_gcmc at a fugacity of 1e-7), an emptied two-site type (dumbbell_gcmc at the same
fugacity: the rotation of an empty type, and the chain run's rule that such a type keeps its last molecule for the windows), a
two-site type that empties and refills (dumbbell_gcmc at a fugacity of 0.3) and a creation into a full type (lj_gcmc with two
free slots, as it is and at a fugacity that fills them).

The yardstick of the emptied and the refilled runs is tests/golden/modes_agree: the files, counters and counts that the driver
wrote when each mode still had its own copy of the step (the seams mode's for the emptied inputs; results.json holds the
counters and counts), so a mistake in a routine that all modes now share cannot move them together unnoticed.  A creation into
a full type ends every mode with the seams mode's error and files."""
import json
import os
import shutil

import pytest

from maniac_mc_amd import _lib
from tests.test_gpu_chain_run_gcmc_files import RUNS, _identical_dirs, _run
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

MODES = {
    "seams": dict(seams=True),
    "fused": dict(speculate=1, chain_windows=False),
    "batched2": dict(speculate=2, chain_windows=False),
    "batched8": dict(speculate=8, chain_windows=False),
    "chain1": dict(speculate=1, chain_windows=True),
    "default": dict(speculate=4, chain_windows=True),
    "run": dict(chain_run=(4, 3), chain_run_gcmc=True),
    "run_plain_fallback": dict(chain_run=(4, 3), chain_run_gcmc=True, speculate=1, chain_windows=False),
}
KEPT = os.path.join(GOLDEN, "modes_agree")
RESULTS = json.load(open(os.path.join(KEPT, "results.json")))
EMPTIED = {"lj_gcmc": ("fugacity 30.0", "number_Ar.dat", 108), "dumbbell_gcmc": ("fugacity 20.0", "number_N2.dat", 30)}
# A step at a time (the seams, one batched call per step) the driver builds an insertion's trial in the mirror's slot count + 1, as
# InsertAndOrientMolecule does, and a rejection leaves it there; the windows build it beside the mirror.  For an EMPTY type of more
# than one site that slot is slot 1, whose geometry the next insertion copies -- so after a rejected insertion into an empty
# dumbbell type the two groups insert differently oriented molecules (trajectory.lammpstrj differs; energies, counters and counts
# do not).  The first group is the reference's behaviour.  Each mode is held to what it did before the copies were folded.
REFILL_GROUP = {"seams": "plain", "fused": "plain", "run_plain_fallback": "plain",
                "batched2": "windows", "batched8": "windows", "chain1": "windows", "default": "windows", "run": "windows"}
# lj_gcmc's 108 molecules in 110 slots.  At the input's own fugacity the first exchange is an accepted deletion and the count only
# falls from there (to 38), so no mode meets the edge and all must write the same run; at a fugacity of 1e6 insertions are
# accepted wherever there is room, deletions never, and the third insertion's successor is the creation into a full type.
FULL = {"fugacity 30.0": False, "fugacity 1e6": True}
_seams = {}


def _inputs_with(case, tmp, fugacity, new):
    inputs = tmp / "inputs"
    shutil.copytree(os.path.join(RUNS, case, "inputs"), inputs)
    text = open(inputs / "system.maniac").read()
    assert fugacity in text
    open(inputs / "system.maniac", "w").write(text.replace(fugacity, new))
    return str(inputs)


def _run_capped(inputs, out, **kw):
    """lj_gcmc with 110 slots for its 108 molecules: (the error's code and text, or None; the output directory)"""
    err = None
    try:
        _run(inputs, out, "lj_gcmc", mol_capacity=[110], **kw)
    except _lib.MgpuError as e:
        err = (e.code, str(e))
    return err, str(out) + "/"


def _as_kept(name, res, out):
    assert res["counters"].tolist() == RESULTS[name]["counters"] and res["n_mol"].tolist() == RESULTS[name]["n_mol"]
    _identical_dirs(out, os.path.join(KEPT, name))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(EMPTIED))
def test_an_emptied_type_gives_every_mode_the_same_run(case, mode, tmp_path):
    kept = case + "_emptied"
    counts = [int(ln.split()[1]) for ln in open(os.path.join(KEPT, kept, EMPTIED[case][1])).read().split("\n")[1:] if ln.strip()]
    # the edge is reached: the type starts full of its molecules and ends with one or none
    assert counts[0] == EMPTIED[case][2] and RESULTS[kept]["n_mol"][0] <= 1
    inputs = _inputs_with(case, tmp_path, EMPTIED[case][0], "fugacity 1e-7")
    res, out = _run(inputs, tmp_path / "out", case, **MODES[mode])
    cr = res["chain_run"]
    print(f"{case} {mode}: {cr}, windows {res['chain_windows']}, counters {res['counters'].tolist()}, n_mol {res['n_mol'].tolist()}")
    if mode.startswith("run"):
        assert cr["on"] and cr["gcmc"] and cr["fallback_steps"] > 0 and cr["steps"] > 0
    else:
        assert not cr["on"]
    _as_kept(kept, res, out)


@pytest.mark.parametrize("mode", list(MODES))
def test_a_type_that_empties_and_refills_keeps_each_modes_run(mode, tmp_path):
    # the edge is reached: insertions were accepted (61 of 231) in a run whose box was empty at a block's end and at the last step,
    # and the two groups' files differ
    r = RESULTS["dumbbell_refill_plain"]
    assert r["counters"][5] > 0 and r["n_mol"] == [0] and r == RESULTS["dumbbell_refill_windows"]
    f = "trajectory.lammpstrj"
    assert open(os.path.join(KEPT, "dumbbell_refill_plain", f)).read() != open(os.path.join(KEPT, "dumbbell_refill_windows", f)).read()
    inputs = _inputs_with("dumbbell_gcmc", tmp_path, "fugacity 20.0", "fugacity 0.3")
    res, out = _run(inputs, tmp_path / "out", "dumbbell_gcmc", **MODES[mode])
    print(f"refill {mode}: {res['chain_run']}, counters {res['counters'].tolist()}, n_mol {res['n_mol'].tolist()}")
    _as_kept("dumbbell_refill_" + REFILL_GROUP[mode], res, out)


@pytest.fixture(scope="module")
def seams_runs(tmp_path_factory):
    """the seams mode's run of each capped input, made once"""
    def get(fugacity):
        if fugacity not in _seams:
            tmp = tmp_path_factory.mktemp("seams")
            inputs = _inputs_with("lj_gcmc", tmp, "fugacity 30.0", fugacity)
            _seams[fugacity] = (inputs,) + _run_capped(inputs, tmp / "out", **MODES["seams"])
        return _seams[fugacity]
    yield get
    _seams.clear()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("fugacity", list(FULL))
def test_a_creation_into_a_full_type_ends_every_mode_alike(fugacity, mode, seams_runs, tmp_path):
    inputs, err_ref, out_ref = seams_runs(fugacity)
    print(f"{fugacity}, seams: {err_ref}")
    assert (err_ref is not None) == FULL[fugacity]              # the edge is reached where the input can reach it
    err, out = _run_capped(inputs, tmp_path / "out", **MODES[mode])
    print(f"{fugacity}, {mode}: {err}")
    assert err == err_ref
    _identical_dirs(out, out_ref)
