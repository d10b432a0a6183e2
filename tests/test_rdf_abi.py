"""The radial distribution functions' interface without a device: the C header declares the five mgpu_rdf_* entry points with
the argument lists the engine implements, the Python loader and the Fortran binding name them, the ABI version did not move
(additions only), and the Python wrappers exist with the stated defaults."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULL = "unsigned long long"
SIGNATURES = {
    "mgpu_rdf_configure": ["mgpu_engine *e", "int n_bins", "double r_max", "int n_pairs", "const int *type_a", "const int *type_b",
                           "int include_intra"],
    "mgpu_rdf_accumulate_replicas": ["mgpu_engine *e", "int n", "const int *replicas", "int chunk"],
    "mgpu_rdf_read": ["mgpu_engine *e", "int n", "const int *replicas", f"{ULL} *hist", f"{ULL} *eligible", f"{ULL} *samples"],
    "mgpu_rdf_load": ["mgpu_engine *e", "int n", "const int *replicas", f"const {ULL} *hist", f"const {ULL} *eligible",
                      f"const {ULL} *samples"],
    "mgpu_rdf_reset": ["mgpu_engine *e", "int n", "const int *replicas"],
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
    # the engine by value, scalars by value, the lists by reference, the counts 64-bit integers
    assert re.search(r"type\(c_ptr\),\s*value\s*::\s*e\b", body)
    if name == "mgpu_rdf_configure":
        assert re.search(r"real\(c_double\),\s*value\s*::\s*r_max", body)
        assert re.search(r"integer\(c_int\),\s*value\s*::\s*n_bins,\s*n_pairs,\s*include_intra", body)
        assert re.search(r"integer\(c_int\),\s*intent\(in\)\s*::\s*type_a\(\*\),\s*type_b\(\*\)", body)
    else:
        assert re.search(r"integer\(c_int\),\s*intent\(in\)\s*::\s*replicas\(\*\)", body)
    if name in ("mgpu_rdf_read", "mgpu_rdf_load"):
        intent = "out" if name == "mgpu_rdf_read" else "in"
        assert re.search(r"integer\(c_long_long\),\s*intent\(" + intent + r"\)\s*::\s*hist\(\*\),\s*eligible\(\*\),\s*samples\(\*\)", body)


def test_fortran_wrappers_and_integration_rows():
    f90 = _read("maniac_mc_amd", "fortran", "maniac_gpu.f90")
    doc = _read("INTEGRATION.md")
    for wrapper, entry in (("GpuRdfConfigure", "mgpu_rdf_configure"), ("GpuRdfAccumulate", "mgpu_rdf_accumulate_replicas"),
                           ("GpuRdfRead", "mgpu_rdf_read"), ("GpuRdfLoad", "mgpu_rdf_load"), ("GpuRdfReset", "mgpu_rdf_reset")):
        assert re.search(r"subroutine\s+" + wrapper + r"\s*\(engine,", f90), wrapper
        assert len([ln for ln in doc.splitlines() if wrapper in ln and f"`{entry}`" in ln]) == 1, f"one line for {entry} in INTEGRATION.md"


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


def test_the_kernel_header_is_a_dependency_of_the_build():
    from maniac_mc_amd import _lib
    assert "mgpu_kernels_rdf.h" in _lib.HEADERS
    assert os.path.isfile(os.path.join(_lib.CSRC, "mgpu_kernels_rdf.h"))
    assert _lib.SOURCES == ["mgpu_engine.hip", "mgpu_launch.hip", "mgpu_lanes.hip", "mgpu_windows.hip", "mgpu_replicas.hip",
                            "mgpu_host_setup.cpp", "mgpu_comm.cpp"], "the build recipe did not change"


def test_python_wrappers_exist_with_the_stated_defaults():
    import inspect
    from maniac_mc_amd import checkpoint, rdf
    from maniac_mc_amd.engine import Engine
    from maniac_mc_amd.fortran_host import FortranFarm
    from maniac_mc_amd.replicas import run_replicas
    p = inspect.signature(Engine.rdf_configure).parameters
    assert list(p)[1:] == ["n_bins", "r_max", "pairs", "include_intra"] and p["include_intra"].default is False
    p = inspect.signature(Engine.rdf_accumulate).parameters
    assert p["replicas"].default is None and p["chunk"].default is None
    assert inspect.signature(Engine.rdf_read).parameters["replicas"].default is None
    assert inspect.signature(Engine.rdf_reset).parameters["replicas"].default is None
    assert list(inspect.signature(Engine.rdf_load).parameters)[1:4] == ["hist", "eligible", "samples"]
    assert callable(FortranFarm.rdf_sample)
    assert inspect.signature(run_replicas).parameters["rdf"].default is None
    assert inspect.signature(checkpoint.save).parameters["extra"].default is None
    for f in ("parse_spec", "half_width", "normalise", "eligible_pairs", "write_dat", "write_counts"):
        assert callable(getattr(rdf, f))
