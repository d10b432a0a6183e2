"""The switch of the single-chain one-launch paths for rigid molecules of 6 to 63 sites in a triclinic box, without a device:
the C header, the Fortran binding and the Python loader name mgpu_chain_set_wide_triclinic with the same argument list
(tests/test_chain_run_abi.py's comparison), the ABI version is unchanged (an export was added, no signature or struct of the
interface changed), the built library and the Fortran host library resolve it, the Engine class and run_simulation carry the
switch, and the command line names --wide-triclinic."""
import ctypes as C
import inspect
import os
import subprocess
import sys

from tests.test_chain_run_abi import ROOT, _c_args, _f_args

NAME = "mgpu_chain_set_wide_triclinic"


def test_header_binding_and_loader_agree():
    from maniac_mc_amd import _lib
    header = open(os.path.join(ROOT, "include", "maniac_gpu.h")).read()
    f90 = open(os.path.join(ROOT, "maniac_mc_amd", "fortran", "maniac_gpu.f90")).read()
    assert NAME in _lib.EXPORTS
    c, f = _c_args(header, NAME), _f_args(f90, NAME)
    assert [(ct, cptr) for _, ct, cptr in c] == [("ptr", True), ("int", False)], c
    assert len(c) == len(f), (c, f)
    for (cn, ct, cptr), (fn, ft, fref) in zip(c, f):
        if ct == "ptr":
            assert ft == "ptr" and not fref, (cn, fn)
        else:
            assert ct == ft and cptr == fref, (cn, fn)
    assert "MGPU_ABI_VERSION 2" in " ".join(header.split())
    assert _lib.ABI_VERSION == 2
    # the header's comment says what the switch stands for, with the reference's routines, and what it refuses
    at = header.index("mgpu_chain_set_wide_triclinic(e, 1):")
    text = header[at:header.index("int mgpu_chain_window_capacity", at)]
    for word in ("energy_utils.f90", "geometry_utils.f90", "never the", "farm windows", "orthorhombic box", "mgpu_chain_run_set_wide",
                 "MGPU_ERR_STATE", "Drains"):
        assert word in text, word
    # the two set_wide entries say where a triclinic box stands now
    at = header.index("set_wide    on:")
    assert NAME in header[at:header.index("An open run does not lock the engine", at)]
    at = header.index("mgpu_chain_set_wide(e, 1):")
    assert NAME in header[at:header.index("mgpu_chain_set_wide_triclinic(e, 1):", at)]


def test_the_libraries_and_the_engine_class_carry_it():
    from maniac_mc_amd import _lib
    from maniac_mc_amd.engine import Engine
    assert hasattr(_lib.lib(), NAME)
    H = C.CDLL(os.path.join(ROOT, "maniac_mc_amd", "libmaniac_host.so"))
    assert hasattr(H, NAME)                                      # (through the engine library the host library is linked to)
    assert list(inspect.signature(Engine.chain_set_wide_triclinic).parameters) == ["self", "on"]
    assert inspect.signature(Engine.chain_set_wide_triclinic).parameters["on"].default is True


def test_the_command_line_names_the_flag():
    from maniac_mc_amd import run
    assert inspect.signature(run.run_simulation).parameters["wide_triclinic"].default is False
    p = subprocess.run([sys.executable, "-m", "maniac_mc_amd.run", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0 and "--wide-triclinic" in p.stdout, p.stdout + p.stderr
    # the parser takes the flag alone and beside the others (the run stops at the missing input file, after parsing)
    assert run.main(["-i", "/nonexistent.maniac", "-d", "x", "-p", "y", "--wide-triclinic"]) == 1
    assert run.main(["-i", "/nonexistent.maniac", "-d", "x", "-p", "y", "--chain-run", "4,3", "--chain-run-triclinic", "--chain-run-wide",
                     "--wide-chain-windows", "--wide-triclinic"]) == 1


def test_the_speed_tool_has_the_tilted_workloads():
    text = open(os.path.join(ROOT, "tools", "chain_run_speed.py")).read()
    for word in ("adsorbate24_triclinic", "adsorbate24_gcmc_triclinic", "wide_triclinic", "tilt_of(60.0)"):
        assert word in text, word
