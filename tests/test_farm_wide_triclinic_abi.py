"""The switch of the farm windows for rigid molecules of 6 to 63 sites in a triclinic box, without a device: the C header, the
Fortran binding and the Python loader name mgpu_farm_set_wide_triclinic with the same argument list
(tests/test_wide_triclinic_abi.py's comparison), the ABI version is unchanged (an export was added, no signature or struct of the
interface changed), the built library and the Fortran host library resolve it, the Engine class, FortranFarm and run_replicas
carry the parameter with its default off, the command line hands --wide-triclinic to the replica farm, and the speed tool names
the sheared workloads."""
import ctypes as C
import inspect
import os
import subprocess
import sys

from tests.test_chain_run_abi import ROOT, _c_args, _f_args

NAME = "mgpu_farm_set_wide_triclinic"


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
    at = header.index("mgpu_farm_set_wide_triclinic(e, 1):")
    text = header[at:header.index("int mgpu_farm_set_wide_triclinic", at)]
    for word in ("energy_utils.f90:374-442", "geometry_utils.f90:167-220", "geometry_utils.f90:359-415", "mgpu_set_triclinic_moves",
                 "mgpu_chain_set_wide_triclinic", "orthorhombic box", "uncollected", "MGPU_ERR_STATE", "Drains"):
        assert word in text, word
    # the chain switch's comment stands as it was
    at = header.index("mgpu_chain_set_wide_triclinic(e, 1):")
    text = header[at:header.index("int mgpu_chain_window_capacity", at)]
    assert "never the" in text and "farm windows" in text


def test_the_libraries_and_the_engine_class_carry_it():
    from maniac_mc_amd import _lib
    from maniac_mc_amd.engine import Engine
    assert hasattr(_lib.lib(), NAME)
    H = C.CDLL(os.path.join(ROOT, "maniac_mc_amd", "libmaniac_host.so"))
    assert hasattr(H, NAME)                                      # (through the engine library the host library is linked to)
    assert list(inspect.signature(Engine.farm_set_wide_triclinic).parameters) == ["self", "on"]
    assert inspect.signature(Engine.farm_set_wide_triclinic).parameters["on"].default is True


def test_the_farm_and_the_replica_runs_carry_the_parameter_default_off():
    from maniac_mc_amd import replicas, run
    from maniac_mc_amd.fortran_host import FortranFarm
    assert inspect.signature(FortranFarm.__init__).parameters["wide_triclinic"].default is False
    assert inspect.signature(replicas.run_replicas).parameters["wide_triclinic"].default is False
    text = " ".join(open(os.path.join(ROOT, "maniac_mc_amd", "run.py")).read().split())
    call = text[text.index("farm_run.run_replicas("):]
    assert "wide_triclinic=a.wide_triclinic" in call[:call.index("except ValueError")]
    p = subprocess.run([sys.executable, "-m", "maniac_mc_amd.run", "--help"], capture_output=True, text=True, cwd=ROOT)
    assert p.returncode == 0 and "--wide-triclinic" in p.stdout and "--farm-mode windows" in " ".join(p.stdout.split()), p.stdout + p.stderr
    # the parser takes the flag beside --replicas (the run stops at the missing input file, after parsing)
    assert run.main(["-i", "/nonexistent.maniac", "-d", "x", "-p", "y", "--replicas", "4", "--farm-mode", "windows", "--wide-triclinic"]) == 1


def test_the_speed_tool_has_the_sheared_workloads():
    text = open(os.path.join(ROOT, "tools", "farm_window_speed.py")).read()
    for word in ("adsorbate24_triclinic", "adsorbate24_gcmc_triclinic", "--wide-triclinic", "wide_triclinic", "tilt_of(60.0)", "--repeats"):
        assert word in text, word
