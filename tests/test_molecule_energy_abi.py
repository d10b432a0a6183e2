"""The molecule-energy interface without a device: the C header declares the six mgpu_molecule_energ* entry points with the
argument lists the engine implements, the Python loader and the Fortran binding name them, the built library exports them, the
ABI version did not move (additions), the kernel header is a dependency of the build, and the Python wrappers exist with the
stated defaults."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURES = {
    "mgpu_molecule_energies_replicas": ["mgpu_engine *e", "int n", "const int *replicas", "int chunk", "int n_sel", "const int *types",
                                        "double *out", "int *counts"],
    "mgpu_molecule_energy_configure": ["mgpu_engine *e", "int n_bins", "double e_min", "double e_max", "int n_sel", "const int *types"],
    "mgpu_molecule_energy_accumulate_replicas": ["mgpu_engine *e", "int n", "const int *replicas", "int chunk"],
    "mgpu_molecule_energy_read": ["mgpu_engine *e", "int n", "const int *replicas", "unsigned long long *hist",
                                  "unsigned long long *samples"],
    "mgpu_molecule_energy_load": ["mgpu_engine *e", "int n", "const int *replicas", "const unsigned long long *hist",
                                  "const unsigned long long *samples"],
    "mgpu_molecule_energy_reset": ["mgpu_engine *e", "int n", "const int *replicas"],
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_declares_the_signatures():
    header = _read("include", "maniac_gpu.h")
    for name, sig in SIGNATURES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert m, f"{name} is not declared in include/maniac_gpu.h"
        assert [" ".join(a.split()) for a in m.group(1).split(",")] == sig, name


def test_loader_and_fortran_binding_name_them():
    import ctypes as C
    from maniac_mc_amd import _lib
    f90 = _read("maniac_mc_amd", "fortran", "maniac_gpu.f90")
    for name, sig in SIGNATURES.items():
        assert name in _lib.EXPORTS
        assert len(_lib.SIGNATURES[name]) == len(sig), "the loader states the argument list"
        m = re.search(r"function\s+" + name + r"\s*\(([^)]*)\)\s*&?\s*bind\(C,\s*name=\"" + name + r"\"\)(.*?)end function", f90, re.S)
        assert m, f"{name} has no interface in maniac_gpu.f90"
        assert [a.strip() for a in m.group(1).replace("&", " ").split(",")] == [a.split()[-1].lstrip("*") for a in sig], name
        assert re.search(r"type\(c_ptr\),\s*value\s*::\s*e\b", m.group(2))
    assert _lib.SIGNATURES["mgpu_molecule_energy_configure"][2:4] == [C.c_double, C.c_double]
    assert _lib.SIGNATURES["mgpu_molecule_energy_read"][3:] == [C.POINTER(C.c_ulonglong)] * 2


def test_fortran_wrapper_and_integration_row():
    f90 = _read("maniac_mc_amd", "fortran", "maniac_gpu.f90")
    doc = _read("INTEGRATION.md")
    assert re.search(r"subroutine\s+GpuMoleculeEnergies\s*\(engine,\s*n,\s*replicas,\s*n_sel,\s*types,\s*out,\s*counts,\s*stat\)", f90)
    assert re.search(r"int\(types - 1, c_int\)", f90), "residue types are 1-based in the wrapper"
    assert len([ln for ln in doc.splitlines() if "GpuMoleculeEnergies" in ln and "`mgpu_molecule_energies_replicas`" in ln]) == 1


def test_abi_version_is_unchanged():
    from maniac_mc_amd import _lib
    header = _read("include", "maniac_gpu.h")
    assert "MGPU_ABI_VERSION 2" in " ".join(header.split())
    assert _lib.ABI_VERSION == 2


def test_the_library_exports_them():
    from maniac_mc_amd import _lib
    for name in SIGNATURES:
        assert hasattr(_lib.lib(), name), name


def test_the_kernel_header_is_a_dependency_of_the_build():
    from maniac_mc_amd import _lib
    assert "mgpu_kernels_molen.h" in _lib.HEADERS
    assert os.path.isfile(os.path.join(_lib.CSRC, "mgpu_kernels_molen.h"))
    assert _lib.SOURCES == ["mgpu_engine.hip", "mgpu_launch.hip", "mgpu_lanes.hip", "mgpu_windows.hip", "mgpu_replicas.hip",
                            "mgpu_host_setup.cpp", "mgpu_comm.cpp"], "the build recipe did not change"
    assert '#include "mgpu_kernels_molen.h"' in _read("maniac_mc_amd", "csrc", "mgpu_replicas.hip")


def test_python_wrappers_exist_with_the_stated_defaults():
    import inspect
    from maniac_mc_amd import checkpoint, molecule_energy
    from maniac_mc_amd.engine import Engine
    from maniac_mc_amd.fortran_host import FortranFarm
    from maniac_mc_amd.replicas import run_replicas
    p = inspect.signature(Engine.molecule_energies_replicas).parameters
    assert list(p)[1:] == ["types", "replicas", "chunk"] and p["replicas"].default is None and p["chunk"].default is None
    assert list(inspect.signature(Engine.molecule_energy_configure).parameters)[1:] == ["n_bins", "e_min", "e_max", "types"]
    for f in (Engine.molecule_energy_accumulate, FortranFarm.molecule_energy_sample):
        p = inspect.signature(f).parameters
        assert list(p)[1:] == ["replicas", "chunk"] and p["replicas"].default is None and p["chunk"].default is None
    for f in ("molecule_energy_read", "molecule_energy_load", "molecule_energy_reset"):
        assert inspect.signature(getattr(Engine, f)).parameters["replicas"].default is None
    assert inspect.signature(run_replicas).parameters["molecule_energy"].default is None
    assert list(inspect.signature(run_replicas).parameters)[-1] == "molecule_energy"
    for f in ("parse_spec", "check_spec", "from_args", "identity_array", "slot_index", "pooled", "write_dat", "read_dat",
              "write_counts", "read_counts"):
        assert callable(getattr(molecule_energy, f))
    assert all(hasattr(molecule_energy.Sampler, f) for f in ("identity_array", "configure", "sample", "state", "load", "finish"))
    assert checkpoint.ANALYSES[-1] == "molecule_energy" and "--molecule-energy" in checkpoint._NAMES["molecule_energy"]
