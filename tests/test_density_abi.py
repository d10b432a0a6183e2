"""The density maps' interface without a device: the C header declares the five mgpu_density_* entry points with the argument
lists the engine implements, the Python loader and the Fortran binding name them, the ABI version did not move (additions only),
the argument checks that come before any device work refuse with their codes, and the Python wrappers exist with the stated
defaults."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULL = "unsigned long long"
SIGNATURES = {
    "mgpu_density_configure": ["mgpu_engine *e", "const int *n", "int n_channels", "const int *types", "int n_groups",
                               "const int *group_of"],
    "mgpu_density_accumulate_replicas": ["mgpu_engine *e", "int n", "const int *replicas", "int chunk"],
    "mgpu_density_read": ["mgpu_engine *e", "int n", "const int *groups", f"{ULL} *hist", f"{ULL} *samples"],
    "mgpu_density_load": ["mgpu_engine *e", "int n", "const int *groups", f"const {ULL} *hist", f"const {ULL} *samples"],
    "mgpu_density_reset": ["mgpu_engine *e", "int n", "const int *groups"],
}
WRAPPERS = (("GpuDensityConfigure", "mgpu_density_configure"), ("GpuDensityAccumulate", "mgpu_density_accumulate_replicas"),
            ("GpuDensityRead", "mgpu_density_read"), ("GpuDensityLoad", "mgpu_density_load"), ("GpuDensityReset", "mgpu_density_reset"))


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
    if name == "mgpu_density_configure":
        assert re.search(r"integer\(c_int\),\s*value\s*::\s*n_channels,\s*n_groups", body)
        assert re.search(r"integer\(c_int\),\s*intent\(in\)\s*::\s*n\(\*\),\s*types\(\*\),\s*group_of\(\*\)", body)
    elif name == "mgpu_density_accumulate_replicas":
        assert re.search(r"integer\(c_int\),\s*intent\(in\)\s*::\s*replicas\(\*\)", body)
    else:
        assert re.search(r"integer\(c_int\),\s*intent\(in\)\s*::\s*groups\(\*\)", body)
    if name in ("mgpu_density_read", "mgpu_density_load"):
        intent = "out" if name == "mgpu_density_read" else "in"
        assert re.search(r"integer\(c_long_long\),\s*intent\(" + intent + r"\)\s*::\s*hist\(\*\),\s*samples\(\*\)", body)


def test_fortran_wrappers_and_integration_rows():
    f90 = _read("maniac_mc_amd", "fortran", "maniac_gpu.f90")
    doc = _read("INTEGRATION.md")
    for wrapper, entry in WRAPPERS:
        assert re.search(r"subroutine\s+" + wrapper + r"\s*\(engine,", f90), wrapper
        assert wrapper in doc and f"`{entry}`" in doc, f"{entry} is named in INTEGRATION.md"
    # atom types are 1-based in the wrapper, as for GpuRdf*
    body = re.search(r"subroutine GpuDensityConfigure.*?end subroutine GpuDensityConfigure", f90, re.S).group(0)
    assert "types - 1" in body


def test_abi_version_is_unchanged_and_the_limit_has_one_name():
    from maniac_mc_amd import _lib, density
    header = _read("include", "maniac_gpu.h")
    assert "MGPU_ABI_VERSION 2" in " ".join(header.split())
    assert _lib.ABI_VERSION == 2
    assert "#define MGPU_DENSITY_MAX_BYTES (2ull << 30)" in header and density.MAX_BYTES == 2 << 30
    src = _read("maniac_mc_amd", "csrc", "mgpu_replicas.hip") + _read("maniac_mc_amd", "csrc", "mgpu_kernels_density.h")
    assert "MGPU_DENSITY_MAX_BYTES" in src and "2ull << 30" not in src, "the engine compares with the header's constant"


def test_the_library_exports_them_and_checks_its_arguments_before_any_device_work():
    from maniac_mc_amd import _lib
    L = _lib.lib()
    for name in SIGNATURES:
        assert hasattr(L, name)
    three = (C.c_int * 3)(4, 4, 4)
    one = (C.c_int * 1)(0)
    u = (C.c_ulonglong * 1)(0)
    null = C.c_void_p(None)
    for rc in (L.mgpu_density_configure(null, three, C.c_int(1), one, C.c_int(1), one),
               L.mgpu_density_accumulate_replicas(null, C.c_int(1), one, C.c_int(0)),
               L.mgpu_density_read(null, C.c_int(1), one, u, u),
               L.mgpu_density_load(null, C.c_int(1), one, u, u),
               L.mgpu_density_reset(null, C.c_int(1), one)):
        assert rc == 1, "MGPU_ERR_INVALID_ARG"
        assert b"null engine" in L.mgpu_last_error()


def test_the_kernel_header_is_a_dependency_of_the_build():
    from maniac_mc_amd import _lib
    assert "mgpu_kernels_density.h" in _lib.HEADERS
    assert os.path.isfile(os.path.join(_lib.CSRC, "mgpu_kernels_density.h"))
    kernel = _read("maniac_mc_amd", "csrc", "mgpu_kernels_density.h")
    assert "density_map_kernel" in kernel and "asm" not in kernel


def test_python_wrappers_exist_with_the_stated_defaults():
    import inspect
    from maniac_mc_amd import density
    from maniac_mc_amd.engine import Engine
    from maniac_mc_amd.fortran_host import FortranFarm
    from maniac_mc_amd.replicas import run_replicas
    p = inspect.signature(Engine.density_configure).parameters
    assert list(p)[1:] == ["grid", "types", "group_of", "n_groups"] and p["group_of"].default is None
    p = inspect.signature(Engine.density_accumulate).parameters
    assert p["replicas"].default is None and p["chunk"].default is None
    assert inspect.signature(Engine.density_read).parameters["groups"].default is None
    assert inspect.signature(Engine.density_reset).parameters["groups"].default is None
    p = inspect.signature(Engine.density_load).parameters
    assert list(p)[1:3] == ["hist", "samples"] and p["groups"].default is None
    p = inspect.signature(FortranFarm.density_sample).parameters
    assert p["replicas"].default is None and p["chunk"].default is None
    assert inspect.signature(run_replicas).parameters["density"].default is None
    for f in ("parse_spec", "parse_types", "check_spec", "identity_array", "number_density", "profiles", "write_counts",
              "write_profiles", "write_cube"):
        assert callable(getattr(density, f))
