"""The whole-run fixtures of rigid molecules of 6 and 24 sites in a triclinic cell (tests/golden/runs_wide_triclinic, made by
tests/golden/make_wide_triclinic_fixtures.py), without a GPU: their inputs are the committed runs_wide inputs plus the tilt
line, io_maniac loads them as triclinic systems of those molecules, and the log header the front end builds for them is the head
of the reference's log character for character (tests/test_triclinic_gcmc_fixture.py's comparison)."""
import json
import os

import pytest

from maniac_mc_amd import io_maniac
from tests.golden.make_triclinic_gcmc_fixtures import tilted
from tests.golden.make_wide_triclinic_fixtures import CASES, TILT
from tests.util import GOLDEN

WIDE = os.path.join(GOLDEN, "runs_wide")
TRI = os.path.join(GOLDEN, "runs_wide_triclinic")
SITES = {"cage6_tri_nvt": 6, "cage24_tri_gcmc": 24}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_inputs_are_the_tilted_parents(case):
    inputs = os.path.join(TRI, case, "inputs")
    parent = os.path.join(WIDE, CASES[case], "inputs")
    for f in ("system.maniac", "system.inc"):
        assert open(os.path.join(inputs, f)).read() == open(os.path.join(parent, f)).read()
    plain = open(os.path.join(parent, "system.data")).read()
    assert open(os.path.join(inputs, "system.data")).read() == tilted(plain, TILT)
    assert TILT in tilted(plain, TILT).split("\n") and TILT.endswith("xy xz yz")
    summary = json.load(open(os.path.join(TRI, "summary.json")))
    parents = json.load(open(os.path.join(WIDE, "summary.json")))
    assert sorted(os.listdir(os.path.join(TRI, case, "expected"))) == summary[case]["files"]
    assert summary[case]["as_written"] == parents[CASES[case]]["as_written"] and summary[case]["seed"] == parents[CASES[case]]["seed"]
    # same step counts as the parent: 3 blocks of 150 steps, and the run accepted something
    last = summary[case]["last_moves_record"]
    assert last[0] == "3" and sum(int(x) for x in last[2::2]) > 0


@pytest.mark.parametrize("case", sorted(CASES))
def test_io_maniac_loads_it_and_the_log_header_is_the_references(case, tmp_path):
    import ctypes as C
    from maniac_mc_amd import fortran_host, run
    from maniac_mc_amd.engine import box_prepare, ewald_setup
    assert os.path.exists(fortran_host.LIB_PATH), "the Fortran host library is part of the build"
    cwd = os.getcwd()
    os.chdir(os.path.join(TRI, case, "inputs"))   # the fixture was generated with relative file names
    try:
        system, inp, dat = io_maniac.load_system("system.maniac", "system.data", "system.inc", with_data=True)
        _, _, _, metrics = box_prepare(dat["matrix"])
        ew = ewald_setup(metrics, inp.real_space_cutoff, inp.ewald_tolerance)
        text = run.header_text(inp, dat, "system.maniac", "system.data", "system.inc", ew, None, None)
    finally:
        os.chdir(cwd)
    assert system.is_triclinic()
    xy, xz, yz = (float(x) for x in TILT.split()[:3])
    assert (system.box_matrix[1, 0], system.box_matrix[2, 0], system.box_matrix[2, 1]) == (xy, xz, yz)
    assert [int(x) for x in system.topo.atoms_in_res] == [SITES[case]] and inp.nb_block == 3 and inp.nb_step == 150
    H = fortran_host.lib()
    H.mchain_set_log_header(text, C.c_int(len(text)))
    out = tmp_path / "header.txt"
    H.mchain_write_log_header(str(out).encode())
    H.mchain_set_log_header(b"", C.c_int(0))
    got = open(out).read().split("\n")
    want = open(os.path.join(TRI, case, "expected", "log.maniac")).read().split("\n")
    stop = next(i for i, ln in enumerate(want) if "Started Monte Carlo Loop" in ln) - 2
    assert got[-1] == "" and got[:-1] == want[:stop], next(
        (i, a, b) for i, (a, b) in enumerate(zip(got + [None] * 400, want[:stop] + [None])) if a != b)
