"""Grand-canonical chain runs' interface without a device: the C header, the Fortran binding and the Python loader name
mgpu_chain_run_set_gc and mgpu_chain_run_push_gc with the same argument lists (tests/test_chain_run_abi.py's comparison), the ABI
version is unchanged, the host library carries the driver's switch, and the command line takes --chain-run-gcmc together with
--chain-run only."""
import inspect
import os

import pytest

from tests.test_chain_run_abi import ROOT, _c_args, _f_args

SHAPES = {
    "mgpu_chain_run_set_gc": [("ptr", True), ("int", False)],
    "mgpu_chain_run_push_gc": [("ptr", True), ("int", False), ("int", True), ("int", True), ("double", True), ("double", True),
                               ("double", True), ("double", True)],
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_header_binding_and_loader_agree(name):
    from maniac_mc_amd import _lib
    header = open(os.path.join(ROOT, "include", "maniac_gpu.h")).read()
    f90 = open(os.path.join(ROOT, "maniac_mc_amd", "fortran", "maniac_gpu.f90")).read()
    assert name in _lib.EXPORTS
    c, f = _c_args(header, name), _f_args(f90, name)
    assert [(ct, cptr) for _, ct, cptr in c] == SHAPES[name], c
    assert len(c) == len(f), (c, f)
    for (cn, ct, cptr), (fn, ft, fref) in zip(c, f):
        if ct == "ptr":
            assert ft == "ptr" and not fref, (cn, fn)
        else:
            assert ct == ft and cptr == fref, (cn, fn)
    assert "MGPU_ABI_VERSION 2" in " ".join(header.split())
    assert _lib.ABI_VERSION == 2


def test_the_libraries_and_the_engine_class_carry_them():
    from maniac_mc_amd import _lib, fortran_host
    from maniac_mc_amd.engine import Engine
    for name in SHAPES:
        assert hasattr(_lib.lib(), name)
    assert list(inspect.signature(Engine.chain_run_set_gc).parameters) == ["self", "on"]
    assert list(inspect.signature(Engine.chain_run_push_gc).parameters) == ["self", "t", "move", "u", "accept_u", "sel_u", "phi_v"]
    fortran_host.set_chain_run_gcmc(True)
    fortran_host.set_chain_run_gcmc(False)
    assert fortran_host.chain_run_gcmc_mode() == (False, 0)


def test_the_command_line_flag_parses():
    from maniac_mc_amd import run
    assert inspect.signature(run.run_simulation).parameters["chain_run_gcmc"].default is False
    # with --chain-run the parser takes the flag (the run stops at the missing input file, after parsing)
    assert run.main(["-i", "/nonexistent.maniac", "-d", "x", "-p", "y", "--chain-run", "4,3", "--chain-run-gcmc"]) == 1
    # alone it is an argument error
    with pytest.raises(SystemExit) as ei:
        run.main(["-i", "/nonexistent.maniac", "-d", "x", "-p", "y", "--chain-run-gcmc"])
    assert ei.value.code == 2
