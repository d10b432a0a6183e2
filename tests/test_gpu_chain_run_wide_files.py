"""The single-chain driver's chain runs of rigid molecules of 6 to 63 sites (run_simulation(chain_run=(k, depth),
chain_run_wide=True), Engine.chain_run_set_wide): the 6-site NVT fixture of tests/golden/runs_wide runs its blocks as chain runs
and writes the reference's files character for character; the 24-site grand-canonical fixture, run NOT as written and with
chain_run_gcmc as well, writes the files its default windows write -- also where a count reaches an edge and the loop takes steps
through its windows (fallback).  The same input as written, chain_run without chain_run_wide, and an input with a reservoir keep
their windows."""
import filecmp
import json
import os

import pytest

from tests.util import GOLDEN, TOL_K, blank_output_path

RUNS = os.path.join(GOLDEN, "runs_wide")
SUMMARY = json.load(open(os.path.join(RUNS, "summary.json")))
pytestmark = pytest.mark.gpu


def _run(case, out, runs=RUNS, summary=SUMMARY, **kw):
    from maniac_mc_amd import run
    inputs = os.path.join(runs, case, "inputs")
    out = str(out) + "/"
    kw.setdefault("as_written", bool(summary[case].get("as_written")))
    reservoir = "reservoir.data" if summary[case]["reservoir"] else None
    cwd = os.getcwd()
    os.chdir(inputs)                    # the log echoes the file names as given: the fixtures used relative ones
    try:
        res = run.run_simulation("system.maniac", "system.data", "system.inc", out, seed=summary[case]["seed"], reservoir_path=reservoir, **kw)
    finally:
        os.chdir(cwd)
    return res, out


def _reference_files(case, out, runs=RUNS, summary=SUMMARY):
    expected = os.path.join(runs, case, "expected")
    assert sorted(os.listdir(out)) == sorted(summary[case]["files"])
    for f in summary[case]["files"]:
        want = open(os.path.join(expected, f)).read().split("\n")
        got = open(os.path.join(out, f)).read().split("\n")
        if f == "log.maniac":
            got = blank_output_path(got, out)
        assert len(got) == len(want), f
        bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
        assert not bad, f"{f}: first differing line {bad[0] + 1}: {got[bad[0]]!r} vs {want[bad[0]]!r} ({len(bad)} lines differ)"


def _same_files(out_a, out_b):
    """every file but the log, which names its own output directory and its mode"""
    names = sorted(os.listdir(out_a))
    assert names == sorted(os.listdir(out_b)) and "moves.dat" in names
    for f in names:
        if f != "log.maniac":
            assert filecmp.cmp(os.path.join(out_a, f), os.path.join(out_b, f), shallow=False), f


def test_the_6_site_nvt_fixture_runs_as_chain_runs_and_writes_the_reference_files(tmp_path):
    res, out = _run("cage6_nvt", tmp_path / "out", chain_run=(4, 3), chain_run_wide=True)
    cr = res["chain_run"]
    print(f"cage6_nvt: {cr}")
    assert cr["on"] and (cr["k"], cr["depth"]) == (4, 3)
    assert 0 < cr["launches"] - cr["void_launches"] <= cr["launches"] and cr["steps"] > 0
    assert cr["undecided"] == 0 and res["chain_windows"][0] == 0
    for k, v in res["energy"].items():
        assert abs(v - res["recomputed_energy"][k]) <= 1e-9 * max(1.0, abs(v)) + 50 * TOL_K, k
    _reference_files("cage6_nvt", out)


def test_the_24_site_gcmc_fixture_not_as_written_writes_its_windows_files(tmp_path):
    """The fixture's count falls from six to the edge in its first block (number_CAGE.dat: 6, 5, ...; the type is emptied on the
    way), so the loop also takes steps through its windows: no variant with a lowered count is needed to see the fallback.  The last
    molecule of the type is left to the window path (mc_chain.f90 ahead_ok): the insertion that refills the type copies its
    geometry from the mirror."""
    kw = dict(as_written=False)
    ref, out_ref = _run("cage24_gcmc", tmp_path / "windows", **kw)
    res, out = _run("cage24_gcmc", tmp_path / "runs", chain_run=(4, 3), chain_run_gcmc=True, chain_run_wide=True, **kw)
    cr = res["chain_run"]
    work = max(1, cr["launches"] - cr["void_launches"])
    print(f"cage24_gcmc: steps per working launch {cr['steps'] / work:.2f}, fallback_steps {cr['fallback_steps']}, {cr}")
    assert not ref["chain_run"]["on"] and ref["chain_run"]["launches"] == 0
    assert cr["on"] and cr["gcmc"] and cr["steps"] > 0 and cr["launches"] > cr["void_launches"]
    assert cr["fallback_steps"] > 0 and cr["steps"] + cr["fallback_steps"] == 3 * 150
    assert cr["undecided"] == 0
    for k, v in res["energy"].items():
        assert abs(v - res["recomputed_energy"][k]) <= 1e-9 * max(1.0, abs(v)) + 50 * TOL_K, k
    assert list(res["counters"]) == list(ref["counters"]) and list(res["n_mol"]) == list(ref["n_mol"])
    _same_files(out_ref, out)


def test_what_keeps_its_windows(tmp_path):
    # the same input as written
    res, out = _run("cage24_gcmc", tmp_path / "as_written", chain_run=(4, 3), chain_run_gcmc=True, chain_run_wide=True)
    assert not res["chain_run"]["on"] and res["chain_run"]["launches"] == 0
    _reference_files("cage24_gcmc", out)
    # chain_run without chain_run_wide
    res, out = _run("cage6_nvt", tmp_path / "narrow_only", chain_run=(4, 3))
    assert not res["chain_run"]["on"] and res["chain_run"]["launches"] == 0
    _reference_files("cage6_nvt", out)
    # an input with a reservoir
    runs = os.path.join(GOLDEN, "runs")
    summary = json.load(open(os.path.join(runs, "summary.json")))
    case = "dumbbell_gcmc_reservoir"
    res, out = _run(case, tmp_path / "reservoir", runs=runs, summary=summary, chain_run=(4, 3), chain_run_gcmc=True, chain_run_wide=True)
    assert not res["chain_run"]["on"] and res["chain_run"]["launches"] == 0
    _reference_files(case, out, runs=runs, summary=summary)
