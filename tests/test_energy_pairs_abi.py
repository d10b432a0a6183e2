"""The energy decomposition's interface without a device: the C header declares mgpu_energy_pairs_replicas with the argument
list the engine implements, the Python loader and the Fortran binding name it, the built library exports it, the ABI version
did not move (an addition), and the Python wrappers exist with the stated defaults."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "mgpu_energy_pairs_replicas"
SIGNATURE = ["mgpu_engine *e", "int n", "const int *replicas", "int chunk", "int n_sel", "const int *res_a", "const int *res_b",
             "double *out"]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_signature():
    header = _read("include", "maniac_gpu.h")
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{NAME} is not declared in include/maniac_gpu.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == SIGNATURE


def test_loader_and_fortran_binding_name_it():
    from maniac_mc_amd import _lib
    assert NAME in _lib.EXPORTS
    f90 = _read("maniac_mc_amd", "fortran", "maniac_gpu.f90")
    m = re.search(r"function\s+" + NAME + r"\s*\(([^)]*)\)\s*&?\s*bind\(C,\s*name=\"" + NAME + r"\"\)(.*?)end function", f90, re.S)
    assert m, f"{NAME} has no interface in maniac_gpu.f90"
    assert [a.strip() for a in m.group(1).replace("&", " ").split(",")] == [a.split()[-1].lstrip("*") for a in SIGNATURE]
    body = m.group(2)
    assert re.search(r"type\(c_ptr\),\s*value\s*::\s*e\b", body)
    assert re.search(r"integer\(c_int\),\s*value\s*::\s*n,\s*chunk,\s*n_sel", body)
    assert re.search(r"integer\(c_int\),\s*intent\(in\)\s*::\s*replicas\(\*\),\s*res_a\(\*\),\s*res_b\(\*\)", body)
    assert re.search(r"real\(c_double\),\s*intent\(out\)\s*::\s*out\(\*\)", body)


def test_fortran_wrapper_and_integration_row():
    f90 = _read("maniac_mc_amd", "fortran", "maniac_gpu.f90")
    doc = _read("INTEGRATION.md")
    assert re.search(r"subroutine\s+GpuEnergyPairs\s*\(engine,\s*n,\s*replicas,\s*n_sel,\s*res_a,\s*res_b,\s*out,\s*stat\)", f90)
    assert re.search(r"int\(res_a - 1, c_int\)", f90), "residue types are 1-based in the wrapper"
    assert len([ln for ln in doc.splitlines() if "GpuEnergyPairs" in ln and f"`{NAME}`" in ln]) == 1


def test_abi_version_is_unchanged():
    from maniac_mc_amd import _lib
    header = _read("include", "maniac_gpu.h")
    assert "MGPU_ABI_VERSION 2" in " ".join(header.split())
    assert _lib.ABI_VERSION == 2


def test_the_library_exports_it():
    from maniac_mc_amd import _lib
    assert hasattr(_lib.lib(), NAME)


def test_the_kernel_header_is_a_dependency_of_the_build():
    from maniac_mc_amd import _lib
    assert "mgpu_kernels_epairs.h" in _lib.HEADERS
    assert os.path.isfile(os.path.join(_lib.CSRC, "mgpu_kernels_epairs.h"))
    assert _lib.SOURCES == ["mgpu_engine.hip", "mgpu_launch.hip", "mgpu_lanes.hip", "mgpu_windows.hip", "mgpu_replicas.hip",
                            "mgpu_host_setup.cpp", "mgpu_comm.cpp"], "the build recipe did not change"


def test_python_wrappers_exist_with_the_stated_defaults():
    import inspect
    from maniac_mc_amd import energy_pairs
    from maniac_mc_amd.engine import Engine
    from maniac_mc_amd.fortran_host import FortranFarm
    from maniac_mc_amd.replicas import run_replicas
    p = inspect.signature(Engine.energy_pairs_replicas).parameters
    assert list(p)[1:] == ["pairs", "replicas", "chunk"] and p["replicas"].default is None and p["chunk"].default is None
    p = inspect.signature(FortranFarm.energy_pairs_sample).parameters
    assert list(p)[1:] == ["pairs", "replicas", "chunk"] and p["replicas"].default is None and p["chunk"].default is None
    assert inspect.signature(run_replicas).parameters["energy_pairs"].default is None
    for f in ("parse_spec", "parse_select", "default_pairs", "identity_array", "start_replica_file", "append_replica_file",
              "read_replica_file", "write_pooled_file", "read_pooled_file"):
        assert callable(getattr(energy_pairs, f))
