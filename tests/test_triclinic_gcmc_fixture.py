"""The whole-run fixture of a grand-canonical run in a triclinic cell (tests/golden/runs_triclinic_gcmc, made by
tests/golden/make_triclinic_gcmc_fixtures.py), without a GPU: its inputs are the committed dumbbell_gcmc inputs plus the tilt
line, and the log header the front end builds for them is the head of the reference's log character for character -- the two
"COM outside simulation box" warnings included, which the reference's reader prints for every centre that ApplyPBC wraps to
outside xlo..zhi (data_parser.f90:1465-1478, check_utils.f90:23-33) and which only a tilted cell can draw."""
import json
import os

import pytest

from maniac_mc_amd import io_maniac
from tests.golden.make_triclinic_gcmc_fixtures import CASE, TILT, tilted
from tests.util import GOLDEN

RUNS = os.path.join(GOLDEN, "runs")
TRI = os.path.join(GOLDEN, "runs_triclinic_gcmc")


def test_the_inputs_are_the_tilted_dumbbell_inputs():
    inputs = os.path.join(TRI, CASE, "inputs")
    for f in ("system.maniac", "system.inc"):
        assert open(os.path.join(inputs, f)).read() == open(os.path.join(RUNS, "dumbbell_gcmc", "inputs", f)).read()
    plain = open(os.path.join(RUNS, "dumbbell_gcmc", "inputs", "system.data")).read()
    assert open(os.path.join(inputs, "system.data")).read() == tilted(plain)
    assert TILT in tilted(plain).split("\n") and TILT.endswith("xy xz yz")
    summary = json.load(open(os.path.join(TRI, "summary.json")))
    assert sorted(os.listdir(os.path.join(TRI, CASE, "expected"))) == summary[CASE]["files"]


def test_log_header_is_the_references(tmp_path):
    """tests/test_run_fixtures.py's comparison for this fixture"""
    import ctypes as C
    from maniac_mc_amd import fortran_host, run
    from maniac_mc_amd.engine import box_prepare, ewald_setup
    if not os.path.exists(fortran_host.LIB_PATH):
        pytest.skip("Fortran host library not built")
    cwd = os.getcwd()
    os.chdir(os.path.join(TRI, CASE, "inputs"))   # the fixture was generated with relative file names
    try:
        system, inp, dat = io_maniac.load_system("system.maniac", "system.data", "system.inc", with_data=True)
        _, _, _, metrics = box_prepare(dat["matrix"])
        ew = ewald_setup(metrics, inp.real_space_cutoff, inp.ewald_tolerance)
        text = run.header_text(inp, dat, "system.maniac", "system.data", "system.inc", ew, None, None)
    finally:
        os.chdir(cwd)
    assert system.is_triclinic()
    H = fortran_host.lib()
    H.mchain_set_log_header(text, C.c_int(len(text)))
    out = tmp_path / "header.txt"
    H.mchain_write_log_header(str(out).encode())
    H.mchain_set_log_header(b"", C.c_int(0))
    got = open(out).read().split("\n")
    want = open(os.path.join(TRI, CASE, "expected", "log.maniac")).read().split("\n")
    stop = next(i for i, ln in enumerate(want) if "Started Monte Carlo Loop" in ln) - 2
    assert got[-1] == "" and got[:-1] == want[:stop], next(
        (i, a, b) for i, (a, b) in enumerate(zip(got + [None] * 400, want[:stop] + [None])) if a != b)
    n = sum("COM outside simulation box" in ln for ln in got)
    assert n > 0 and n == 2 * sum(ln == " Molecule COM outside simulation box" for ln in got)
