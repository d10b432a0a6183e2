"""The single-chain driver's grand-canonical chain runs on TRICLINIC inputs (run_simulation(chain_run=(k, depth),
chain_run_triclinic=True, chain_run_gcmc=True), mc_chain.f90 run_block by count): with BOTH switches a block with insertions and
deletions in a tilted cell is drawn ahead as by-count records and run as launches queued back to back, which build the
inserted centres (lo + box%matrix u) and wrap the translations on the device.  It must write the reference's files character
for character (tests/golden/runs_triclinic_gcmc, made by tests/golden/make_triclinic_gcmc_fixtures.py: the dumbbell_gcmc
inputs with a tilt line, run by the compiled reference) -- which also holds the default windows of such an input to the
reference -- or, for a charged input, the files of the default-window run of the same input.  Either switch alone, a
reservoir and an as-written run keep the windows."""
import json
import os
import shutil

import pytest

from tests.golden.make_triclinic_gcmc_fixtures import TILT, tilted
from tests.test_gpu_chain_run_gcmc_files import _identical_dirs, _is_a_gc_run, _n_steps, _run
from tests.util import GOLDEN, blank_output_path

RUNS = os.path.join(GOLDEN, "runs")
TRI = os.path.join(GOLDEN, "runs_triclinic_gcmc")
CASE = "dumbbell_tri_gcmc"
SUMMARY = json.load(open(os.path.join(TRI, "summary.json")))
BOTH = dict(chain_run=(4, 3), chain_run_triclinic=True, chain_run_gcmc=True)
pytestmark = pytest.mark.gpu


def _same_files(out):
    """tests/test_gpu_chain_run_files.py's comparison, against this directory's expected files"""
    expected = os.path.join(TRI, CASE, "expected")
    produced = sorted(os.listdir(out))
    assert produced == sorted(SUMMARY[CASE]["files"]) and "log.maniac" in produced
    for f in SUMMARY[CASE]["files"]:
        want = open(os.path.join(expected, f)).read().split("\n")
        got = open(os.path.join(out, f)).read().split("\n")
        if f == "log.maniac":
            got = blank_output_path(got, out)
        assert len(got) == len(want), f
        bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
        assert not bad, f"{f}: first differing line {bad[0] + 1}: {got[bad[0]]!r} vs {want[bad[0]]!r} ({len(bad)} lines differ)"


def _tilted_inputs(case, tmp_path, tilt=TILT):
    """the committed inputs of tests/golden/runs/<case> with a tilt line in system.data (the reservoir's box stays as it is)"""
    inputs = tmp_path / "inputs"
    shutil.copytree(os.path.join(RUNS, case, "inputs"), inputs)
    text = open(inputs / "system.data").read()
    open(inputs / "system.data", "w").write(tilted(text, tilt))
    return str(inputs)


def _kept_its_windows(res):
    cr = res["chain_run"]
    assert not cr["on"] and not cr["gcmc"] and cr["launches"] == 0 and cr["fallback_steps"] == 0
    assert res["chain_windows"][0] > 0


# 7. reference files
def test_a_triclinic_gc_chain_run_writes_the_reference_files(tmp_path):
    inputs = os.path.join(TRI, CASE, "inputs")
    res, out = _run(inputs, tmp_path / "out", "dumbbell_gcmc", **BOTH)
    cr = res["chain_run"]
    print(f"{CASE}: {cr}, windows {res['chain_windows']}")
    _is_a_gc_run(res, _n_steps(inputs))
    if cr["fallback_steps"] == 0:
        assert res["chain_windows"][0] == 0                            # no window was launched
    _same_files(out)


def test_the_default_windows_of_a_triclinic_gc_input_write_the_reference_files(tmp_path):
    res, out = _run(os.path.join(TRI, CASE, "inputs"), tmp_path / "out", "dumbbell_gcmc")
    _kept_its_windows(res)
    _same_files(out)


# 8. charged input
def test_a_charged_triclinic_gc_chain_run_writes_the_window_runs_files(tmp_path):
    """co2_gcmc tilted, as_written=False (the intended physics): the default windows of the same input are the yardstick."""
    inputs = _tilted_inputs("co2_gcmc", tmp_path, "4.0 -3.0 2.0 xy xz yz")
    ref, out_ref = _run(inputs, tmp_path / "windows", "co2_gcmc", as_written=False)
    res, out = _run(inputs, tmp_path / "run", "co2_gcmc", as_written=False, **BOTH)
    cr = res["chain_run"]
    print(f"co2_gcmc tilted: {cr}, counters {res['counters'].tolist()}")
    _kept_its_windows(ref)
    _is_a_gc_run(res, _n_steps(inputs))
    if cr["fallback_steps"] == 0:
        assert res["chain_windows"][0] == 0
    assert res["counters"].tolist() == ref["counters"].tolist() and res["n_mol"].tolist() == ref["n_mol"].tolist()
    _identical_dirs(out, out_ref)


# 9. single switches
@pytest.mark.parametrize("switch", ["chain_run_triclinic", "chain_run_gcmc"])
def test_one_switch_alone_keeps_the_windows(switch, tmp_path):
    res, out = _run(os.path.join(TRI, CASE, "inputs"), tmp_path / "out", "dumbbell_gcmc", chain_run=(4, 3), **{switch: True})
    _kept_its_windows(res)
    _same_files(out)


# 10. reservoirs and as-written
def test_a_triclinic_reservoir_input_keeps_its_windows(tmp_path):
    inputs = _tilted_inputs("dumbbell_gcmc_reservoir", tmp_path)
    ref, out_ref = _run(inputs, tmp_path / "windows", "dumbbell_gcmc_reservoir")
    res, out = _run(inputs, tmp_path / "run", "dumbbell_gcmc_reservoir", **BOTH)
    _kept_its_windows(res)
    _identical_dirs(out, out_ref)


def test_a_triclinic_as_written_run_keeps_its_windows(tmp_path):
    inputs = _tilted_inputs("co2_gcmc", tmp_path, "4.0 -3.0 2.0 xy xz yz")
    ref, out_ref = _run(inputs, tmp_path / "windows", "co2_gcmc", as_written=True)
    res, out = _run(inputs, tmp_path / "run", "co2_gcmc", as_written=True, **BOTH)
    _kept_its_windows(res)
    _identical_dirs(out, out_ref)


# the fallback in a tilted cell
def test_the_ahead_of_outcome_rule_bites_in_a_triclinic_cell(tmp_path):
    """tests/test_gpu_chain_run_gcmc_files.py's emptying box, tilted: lj_gcmc at a fugacity of 1e-7 loses its molecules, and from
    a count of 1 on the run draws nothing ahead of a deletion's outcome: those steps go through the windows such a cell takes
    without runs -- rows built by the loop's own ApplyPBC, on an engine whose frames were dropped -- and the run reopens from
    the frames the loop uploads.  Same files as the default windows."""
    inputs = _tilted_inputs("lj_gcmc", tmp_path, "2.0 -1.5 1.0 xy xz yz")
    text = open(os.path.join(inputs, "system.maniac")).read()
    assert "fugacity 30.0" in text
    open(os.path.join(inputs, "system.maniac"), "w").write(text.replace("fugacity 30.0", "fugacity 1e-7"))
    ref, out_ref = _run(inputs, tmp_path / "windows", "lj_gcmc")
    res, out = _run(inputs, tmp_path / "run", "lj_gcmc", **BOTH)
    cr = res["chain_run"]
    print(f"lj_gcmc tilted, emptying: {cr}, final count {ref['n_mol'].tolist()}")
    _kept_its_windows(ref)
    assert int(ref["n_mol"][0]) <= 1
    assert cr["on"] and cr["gcmc"] and cr["fallback_steps"] > 0 and cr["steps"] > 0
    assert cr["steps"] + cr["fallback_steps"] == _n_steps(inputs)
    assert res["chain_windows"][0] > 0
    assert res["counters"].tolist() == ref["counters"].tolist() and res["n_mol"].tolist() == ref["n_mol"].tolist()
    _identical_dirs(out, out_ref)
