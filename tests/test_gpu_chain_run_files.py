"""The single-chain driver's chain-run mode (run_simulation(chain_run=(k, depth)), mc_chain.f90 run_block): NVT inputs run
each block as launches queued back to back that continue from the step cursor on the device, and must still write the
reference's files character for character -- the comparison tests/test_gpu_run.py makes; a grand-canonical input keeps its
windows by itself."""
import json
import os

import pytest

from tests.util import GOLDEN, TOL_K, blank_output_path

RUNS = os.path.join(GOLDEN, "runs")
SUMMARY = json.load(open(os.path.join(RUNS, "summary.json")))
pytestmark = pytest.mark.gpu


def _run(case, tmp_path, **kw):
    from maniac_mc_amd import run
    inputs = os.path.join(RUNS, case, "inputs")
    out = str(tmp_path / "out") + "/"
    reservoir = "reservoir.data" if SUMMARY[case]["reservoir"] else None
    cwd = os.getcwd()
    os.chdir(inputs)                    # the log echoes the file names as given: the fixtures used relative ones
    try:
        res = run.run_simulation("system.maniac", "system.data", "system.inc", out, seed=SUMMARY[case]["seed"],
                                 reservoir_path=reservoir, as_written=bool(SUMMARY[case].get("as_written")), **kw)
    finally:
        os.chdir(cwd)
    return res, out


def _same_files(case, out):
    expected = os.path.join(RUNS, case, "expected")
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


@pytest.mark.parametrize("case", ["argon_nvt", "spce_nvt", "framework_water_nvt"])
def test_a_chain_run_writes_the_reference_files(case, tmp_path):
    res, out = _run(case, tmp_path, chain_run=(4, 3))
    cr = res["chain_run"]
    print(f"{case}: {cr}")
    assert cr["on"] and (cr["k"], cr["depth"]) == (4, 3)
    assert 0 < cr["launches"] - cr["void_launches"] <= cr["launches"] < cr["steps"]    # some launch consumed more than one step
    assert cr["undecided"] == 0                                        # no step fell inside the 16-ulp margin
    assert res["chain_windows"][0] == 0                                # no window was launched
    for k, v in res["energy"].items():
        assert abs(v - res["recomputed_energy"][k]) <= 1e-9 * max(1.0, abs(v)) + 50 * TOL_K, k
    _same_files(case, out)


def test_a_grand_canonical_input_keeps_its_windows(tmp_path):
    res, out = _run("lj_gcmc", tmp_path, chain_run=(4, 3))
    assert not res["chain_run"]["on"] and res["chain_run"]["launches"] == 0
    assert res["chain_windows"][0] > 0
    _same_files("lj_gcmc", out)
