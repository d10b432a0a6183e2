"""The single-chain driver on TRICLINIC inputs with rigid molecules of 6 and 24 sites (run_simulation(wide_triclinic=True): the
one-launch windows under wide_chain_windows, the chain runs under chain_run_triclinic + chain_run_wide, grand-canonical with
chain_run_gcmc).  tests/golden/runs_wide_triclinic (made by tests/golden/make_wide_triclinic_fixtures.py: the runs_wide inputs with
a tilt line, run by the compiled reference) must be written character for character by the default batched windows -- which
nothing pinned for such an input before -- by the WIDE one-launch windows and by the chain runs; the charged 24-site input not as
written (the intended physics, where the reference's files do not apply) writes the files of its own default windows.  Without
wide_triclinic every variant keeps the path it always had and still writes the same files."""
import json
import os

import pytest

from tests.test_gpu_chain_run_gcmc_files import _identical_dirs
from tests.util import GOLDEN, TOL_K, blank_output_path

TRI = os.path.join(GOLDEN, "runs_wide_triclinic")
SUMMARY = json.load(open(os.path.join(TRI, "summary.json")))
N_STEPS = 450
RUNS6 = dict(chain_run=(4, 3), chain_run_triclinic=True, chain_run_wide=True)
RUNS24 = dict(RUNS6, chain_run_gcmc=True)
pytestmark = pytest.mark.gpu


def _run(case, out, as_written=None, **kw):
    from maniac_mc_amd import run
    out = str(out) + "/"
    if as_written is None:
        as_written = bool(SUMMARY[case]["as_written"])
    cwd = os.getcwd()
    os.chdir(os.path.join(TRI, case, "inputs"))    # the log echoes the file names as given: the fixtures used relative ones
    try:
        res = run.run_simulation("system.maniac", "system.data", "system.inc", out, seed=SUMMARY[case]["seed"], as_written=as_written, **kw)
    finally:
        os.chdir(cwd)
    if not as_written:          # (the deletion as written leaves A(k) with the swapped-in molecule's terms: SURVEY F3)
        for k, v in res["energy"].items():
            assert abs(v - res["recomputed_energy"][k]) <= 1e-9 * max(1.0, abs(v)) + 50 * TOL_K, k
    return res, out


def _same_files(case, out):
    """tests/test_gpu_chain_run_files.py's comparison, against this directory's expected files"""
    expected = os.path.join(TRI, case, "expected")
    produced = sorted(os.listdir(out))
    assert produced == sorted(SUMMARY[case]["files"]) and "log.maniac" in produced
    for f in SUMMARY[case]["files"]:
        want = open(os.path.join(expected, f)).read().split("\n")
        got = open(os.path.join(out, f)).read().split("\n")
        if f == "log.maniac":
            got = blank_output_path(got, out)
        assert len(got) == len(want), f
        bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
        assert not bad, f"{f}: first differing line {bad[0] + 1}: {got[bad[0]]!r} vs {want[bad[0]]!r} ({len(bad)} lines differ)"


def _kept_todays_path(res):
    """batched windows: no one-launch window, no run"""
    cr = res["chain_run"]
    assert not cr["on"] and cr["launches"] == 0 and cr["fallback_steps"] == 0
    assert res["chain_windows"][0] == 0


def test_cage6_default_batched_windows_write_the_reference_files(tmp_path):
    res, out = _run("cage6_tri_nvt", tmp_path / "out")
    _kept_todays_path(res)
    _same_files("cage6_tri_nvt", out)


def test_cage6_wide_triclinic_windows_write_the_reference_files(tmp_path):
    res, out = _run("cage6_tri_nvt", tmp_path / "out", wide_chain_windows=True, wide_triclinic=True)
    windows, undecided = res["chain_windows"]
    print(f"cage6_tri_nvt WIDE TRI windows: {windows} windows, {undecided} left to the host")
    assert windows > 0 and undecided == 0 and not res["chain_run"]["on"]
    _same_files("cage6_tri_nvt", out)


def test_cage6_wide_triclinic_chain_runs_write_the_reference_files(tmp_path):
    res, out = _run("cage6_tri_nvt", tmp_path / "out", wide_triclinic=True, **RUNS6)
    cr = res["chain_run"]
    print(f"cage6_tri_nvt runs: {cr}, windows {res['chain_windows']}")
    assert cr["on"] and not cr["gcmc"] and (cr["k"], cr["depth"]) == (4, 3) and cr["steps"] == N_STEPS and cr["fallback_steps"] == 0
    assert 0 < cr["launches"] - cr["void_launches"] <= cr["steps"] and res["chain_windows"][0] == 0
    _same_files("cage6_tri_nvt", out)


def test_cage24_as_written_wide_triclinic_windows_write_the_reference_files(tmp_path):
    res, out = _run("cage24_tri_gcmc", tmp_path / "out", wide_chain_windows=True, wide_triclinic=True)
    windows, undecided = res["chain_windows"]
    print(f"cage24_tri_gcmc as written, WIDE TRI windows: {windows} windows, {undecided} left to the host")
    assert SUMMARY["cage24_tri_gcmc"]["as_written"] and windows > 0 and not res["chain_run"]["on"]
    _same_files("cage24_tri_gcmc", out)


def test_cage24_default_batched_windows_write_the_reference_files(tmp_path):
    res, out = _run("cage24_tri_gcmc", tmp_path / "out")
    _kept_todays_path(res)
    _same_files("cage24_tri_gcmc", out)


def test_cage24_gc_chain_runs_write_the_default_windows_files(tmp_path):
    """not as written (the intended physics): the default windows of the same input are the yardstick"""
    ref, out_ref = _run("cage24_tri_gcmc", tmp_path / "windows", as_written=False)
    res, out = _run("cage24_tri_gcmc", tmp_path / "run", as_written=False, wide_triclinic=True, **RUNS24)
    cr = res["chain_run"]
    print(f"cage24_tri_gcmc not as written, runs: {cr}, windows {res['chain_windows']}, counters {res['counters'].tolist()}")
    _kept_todays_path(ref)
    assert cr["on"] is True or cr["on"] == 1
    assert cr["gcmc"] and cr["steps"] + cr["fallback_steps"] == N_STEPS and cr["steps"] > 0
    assert res["counters"].tolist() == ref["counters"].tolist() and res["n_mol"].tolist() == ref["n_mol"].tolist()
    _identical_dirs(out, out_ref)


@pytest.mark.parametrize("case,kw", [("cage6_tri_nvt", dict(wide_chain_windows=True)), ("cage6_tri_nvt", RUNS6),
                                     ("cage24_tri_gcmc", dict(wide_chain_windows=True)), ("cage24_tri_gcmc", RUNS24)],
                         ids=["cage6-windows", "cage6-runs", "cage24-windows", "cage24-runs"])
def test_without_wide_triclinic_every_variant_keeps_todays_path(case, kw, tmp_path):
    res, out = _run(case, tmp_path / "out", **kw)
    _kept_todays_path(res)
    _same_files(case, out)
