"""The single-chain driver's grand-canonical chain runs (run_simulation(chain_run=(k, depth), chain_run_gcmc=True), mc_chain.f90
run_block by count): a block with insertions and deletions is drawn ahead as BY-COUNT records -- while no molecule count can reach 0
or the capacity -- and run as launches queued back to back.  It must still write the reference's files character for character
(the comparison tests/test_gpu_run.py makes) or, for the charged inputs whose fixtures are the as-written runs, the files of
the default-window run of the same input; as-written runs and inputs with a reservoir keep their windows."""
import json
import os
import shutil

import pytest

from tests.test_gpu_chain_run_files import _same_files
from tests.util import GOLDEN, TOL_K, blank_output_path

RUNS = os.path.join(GOLDEN, "runs")
SUMMARY = json.load(open(os.path.join(RUNS, "summary.json")))
pytestmark = pytest.mark.gpu


def _run(inputs, out, case, as_written=None, **kw):
    from maniac_mc_amd import run
    out = str(out) + "/"
    reservoir = "reservoir.data" if SUMMARY[case]["reservoir"] else None
    if as_written is None:
        as_written = bool(SUMMARY[case].get("as_written"))
    cwd = os.getcwd()
    os.chdir(inputs)                    # the log echoes the file names as given: the fixtures used relative ones
    try:
        res = run.run_simulation("system.maniac", "system.data", "system.inc", out, seed=SUMMARY[case]["seed"],
                                 reservoir_path=reservoir, as_written=as_written, **kw)
    finally:
        os.chdir(cwd)
    return res, out


def _n_steps(inputs):
    words = dict(ln.split()[:2] for ln in open(os.path.join(str(inputs), "system.maniac")) if ln.split()[:1] in (["nb_block"], ["nb_step"]))
    return int(words["nb_block"]) * int(words["nb_step"])


def _identical_dirs(a, b):
    """every file of run a equals the file of run b, but for the output path the log echoes"""
    assert sorted(os.listdir(a)) == sorted(os.listdir(b))
    for f in sorted(os.listdir(a)):
        la = open(os.path.join(a, f)).read().split("\n")
        lb = open(os.path.join(b, f)).read().split("\n")
        if f == "log.maniac":
            la, lb = blank_output_path(la, a), blank_output_path(lb, b)
        assert len(la) == len(lb), f
        bad = [i for i, (x, y) in enumerate(zip(la, lb)) if x != y]
        assert not bad, f"{f}: first differing line {bad[0] + 1}: {la[bad[0]]!r} vs {lb[bad[0]]!r} ({len(bad)} lines differ)"


def _is_a_gc_run(res, steps):
    cr = res["chain_run"]
    assert cr["on"] and cr["gcmc"] and (cr["k"], cr["depth"]) == (4, 3)
    assert cr["steps"] + cr["fallback_steps"] == steps
    assert 0 < cr["launches"] - cr["void_launches"] < cr["steps"]      # some launch consumed more than one step
    for k, v in res["energy"].items():
        assert abs(v - res["recomputed_energy"][k]) <= 1e-9 * max(1.0, abs(v)) + 50 * TOL_K, k


@pytest.mark.parametrize("case", ["lj_gcmc", "dumbbell_gcmc"])
def test_a_gc_chain_run_writes_the_reference_files(case, tmp_path):
    res, out = _run(os.path.join(RUNS, case, "inputs"), tmp_path / "out", case, chain_run=(4, 3), chain_run_gcmc=True)
    cr = res["chain_run"]
    print(f"{case}: {cr}, windows {res['chain_windows']}")
    _is_a_gc_run(res, _n_steps(os.path.join(RUNS, case, "inputs")))
    if cr["fallback_steps"] == 0:
        assert res["chain_windows"][0] == 0                            # no window was launched
    _same_files(case, out)


@pytest.mark.parametrize("case", ["co2_gcmc", "framework_water_gcmc"])
def test_a_charged_gc_chain_run_writes_the_window_runs_files(case, tmp_path):
    """as_written=False (the intended physics; the fixture is the as-written run): the default windows are the yardstick."""
    inputs = os.path.join(RUNS, case, "inputs")
    ref, out_ref = _run(inputs, tmp_path / "windows", case, as_written=False)
    res, out = _run(inputs, tmp_path / "run", case, as_written=False, chain_run=(4, 3), chain_run_gcmc=True)
    cr = res["chain_run"]
    print(f"{case}: {cr}, counters {res['counters'].tolist()}")
    assert not ref["chain_run"]["on"] and ref["chain_windows"][0] > 0
    _is_a_gc_run(res, _n_steps(inputs))
    if cr["fallback_steps"] == 0:
        assert res["chain_windows"][0] == 0
    assert res["counters"].tolist() == ref["counters"].tolist() and res["n_mol"].tolist() == ref["n_mol"].tolist()
    _identical_dirs(out, out_ref)


@pytest.mark.parametrize("case", ["co2_gcmc", "framework_water_gcmc", "dumbbell_gcmc_reservoir"])
def test_as_written_runs_and_reservoirs_keep_their_windows(case, tmp_path):
    res, out = _run(os.path.join(RUNS, case, "inputs"), tmp_path / "out", case, chain_run=(4, 3), chain_run_gcmc=True)
    cr = res["chain_run"]
    assert not cr["on"] and not cr["gcmc"] and cr["launches"] == 0 and cr["fallback_steps"] == 0
    assert res["chain_windows"][0] > 0
    _same_files(case, out)


def test_the_ahead_of_outcome_rule_bites(tmp_path):
    """lj_gcmc at a fugacity of 1e-7: nearly every deletion is accepted and the box empties: number_Ar.dat of the default-window
    run shows the count falling from 108 to 2 or fewer at a block's end, and the run ends with at most one molecule.  From a count
    of 1 on the run can draw nothing ahead of a deletion's outcome, from 0 nothing at all: those steps go through the windows.
    Same files as the default windows."""
    inputs = tmp_path / "inputs"
    shutil.copytree(os.path.join(RUNS, "lj_gcmc", "inputs"), inputs)
    text = open(inputs / "system.maniac").read()
    assert "fugacity 30.0" in text
    open(inputs / "system.maniac", "w").write(text.replace("fugacity 30.0", "fugacity 1e-7"))
    ref, out_ref = _run(str(inputs), tmp_path / "windows", "lj_gcmc")
    res, out = _run(str(inputs), tmp_path / "run", "lj_gcmc", chain_run=(4, 3), chain_run_gcmc=True)
    counts = [int(ln.split()[1]) for ln in open(os.path.join(out_ref, "number_Ar.dat")).read().split("\n")[1:] if ln.strip()]
    cr = res["chain_run"]
    print(f"counts per block {counts}; {cr}")
    assert counts[0] == 108 and min(counts) <= 2 and int(ref["n_mol"][0]) <= 1
    assert cr["on"] and cr["gcmc"] and cr["fallback_steps"] > 0 and cr["steps"] > 0
    assert cr["steps"] + cr["fallback_steps"] == _n_steps(inputs)
    assert res["chain_windows"][0] > 0
    assert res["counters"].tolist() == ref["counters"].tolist() and res["n_mol"].tolist() == ref["n_mol"].tolist()
    _identical_dirs(out, out_ref)


def test_without_the_switch_a_gc_input_keeps_its_windows(tmp_path):
    res, out = _run(os.path.join(RUNS, "lj_gcmc", "inputs"), tmp_path / "out", "lj_gcmc", chain_run=(4, 3))
    cr = res["chain_run"]
    assert not cr["on"] and not cr["gcmc"] and cr["launches"] == 0 and cr["fallback_steps"] == 0
    assert res["chain_windows"][0] > 0
    with pytest.raises(ValueError):
        _run(os.path.join(RUNS, "lj_gcmc", "inputs"), tmp_path / "out2", "lj_gcmc", chain_run_gcmc=True)
    from maniac_mc_amd import run
    with pytest.raises(SystemExit):
        run.main(["-i", "a", "-d", "b", "-p", "c", "--chain-run-gcmc"])
