"""WIDE chain runs' interface without a device: the C header, the Fortran binding and the Python loader name
mgpu_chain_run_set_wide with the same argument list (tests/test_chain_run_abi.py's comparison), the ABI version is unchanged
(an export was added, no signature or struct of the interface changed), the Engine class and run_simulation carry the switch,
and the command line takes --chain-run-wide together with --chain-run only."""
import inspect
import os

import pytest

from tests.test_chain_run_abi import ROOT, _c_args, _f_args

NAME = "mgpu_chain_run_set_wide"


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
    # the header's comment says what the switch stands for, with the reference's routines
    at = header.index("set_wide    on:")
    text = header[at:header.index("An open run does not lock the engine", at)]
    for word in ("energy_utils.f90", "ewald_energy.f90", "triclinic", "reservoir", "MGPU_ERR_STATE"):
        assert word in text, word


def test_the_library_and_the_engine_class_carry_it():
    from maniac_mc_amd import _lib
    from maniac_mc_amd.engine import Engine
    assert hasattr(_lib.lib(), NAME)
    assert list(inspect.signature(Engine.chain_run_set_wide).parameters) == ["self", "on"]
    assert inspect.signature(Engine.chain_run_set_wide).parameters["on"].default is True


def test_the_command_line_flag_parses():
    from maniac_mc_amd import run
    assert inspect.signature(run.run_simulation).parameters["chain_run_wide"].default is False
    # with --chain-run the parser takes the flag (the run stops at the missing input file, after parsing)
    assert run.main(["-i", "/nonexistent.maniac", "-d", "x", "-p", "y", "--chain-run", "4,3", "--chain-run-wide"]) == 1
    assert run.main(["-i", "/nonexistent.maniac", "-d", "x", "-p", "y", "--chain-run", "4", "--chain-run-wide", "--chain-run-gcmc"]) == 1
    # alone it is an argument error
    with pytest.raises(SystemExit) as ei:
        run.main(["-i", "/nonexistent.maniac", "-d", "x", "-p", "y", "--chain-run-wide"])
    assert ei.value.code == 2


def test_the_speed_tool_takes_the_switch_and_the_workloads():
    import importlib.util
    spec = importlib.util.spec_from_file_location("chain_run_speed", os.path.join(ROOT, "tools", "chain_run_speed.py"))
    text = open(spec.origin).read()
    for word in ("--chain-run-wide", "adsorbate24", "adsorbate24_gcmc", "--wide-chain-windows"):
        assert word in text, word
