"""The many-replica energy calls' interface without a device: the C header declares mgpu_system_energy_replicas and
mgpu_init_structure_factor_replicas with the argument lists the engine implements, the Python loader and the Fortran binding
name them, and the ABI version did not move (additions only)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "mgpu_system_energy_replicas": ["mgpu_engine *e", "int n", "const int *replicas", "int chunk", "double *out", "double *a_deviation"],
    "mgpu_init_structure_factor_replicas": ["mgpu_engine *e", "int n", "const int *replicas", "int mode"],
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_header_declares_the_signature(name):
    header = _read("include", "maniac_gpu.h")
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/maniac_gpu.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == SIGNATURES[name]


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_loader_and_fortran_binding_name_it(name):
    from maniac_mc_amd import _lib
    assert name in _lib.EXPORTS
    f90 = _read("maniac_mc_amd", "fortran", "maniac_gpu.f90")
    m = re.search(r"function\s+" + name + r"\s*\(([^)]*)\)\s*&?\s*bind\(C,\s*name=\"" + name + r"\"\)(.*?)end function", f90, re.S)
    assert m, f"{name} has no interface in maniac_gpu.f90"
    names = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    assert names == [a.split()[-1].lstrip("*") for a in SIGNATURES[name]]
    body = m.group(2)
    # scalars by value, the lists by reference, the optional deviation block a C pointer by value (c_null_ptr: not wanted)
    assert re.search(r"integer\(c_int\),\s*value\s*::\s*n\b", body)
    assert re.search(r"integer\(c_int\),\s*intent\(in\)\s*::\s*replicas\(\*\)", body)
    if name == "mgpu_system_energy_replicas":
        assert re.search(r"real\(c_double\),\s*intent\(out\)\s*::\s*out\(6,\s*\*\)", body)
        assert re.search(r"type\(c_ptr\),\s*value\s*::\s*a_deviation", body)


def test_abi_version_is_unchanged():
    from maniac_mc_amd import _lib
    header = _read("include", "maniac_gpu.h")
    assert "MGPU_ABI_VERSION 2" in " ".join(header.split())
    assert _lib.ABI_VERSION == 2


def test_the_library_exports_them():
    from maniac_mc_amd import _lib
    L = _lib.lib()
    for name in SIGNATURES:
        assert hasattr(L, name)
    import ctypes as C
    H = C.CDLL(os.path.join(ROOT, "maniac_mc_amd", "libmaniac_host.so"))
    assert hasattr(H, "mfarm_set_replica")


def test_python_wrappers_exist_with_the_stated_defaults():
    import inspect
    from maniac_mc_amd.engine import Engine
    from maniac_mc_amd.fortran_host import FortranFarm
    from maniac_mc_amd.replicas import run_replicas
    p = inspect.signature(Engine.system_energy_replicas).parameters
    assert p["replicas"].default is None and p["chunk"].default is None and p["a_deviation"].default is False
    p = inspect.signature(Engine.init_structure_factor_replicas).parameters
    assert p["replicas"].default is None and p["full"].default is True
    assert inspect.signature(FortranFarm.__init__).parameters["initial"].default is None
    assert inspect.signature(FortranFarm.audit).parameters["replicas"].default is None
    p = inspect.signature(run_replicas).parameters
    assert p["restart_from"].default is None and p["audit"].default is False
