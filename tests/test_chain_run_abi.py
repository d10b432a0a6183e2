"""Chain runs' interface without a device: the C header, the Fortran binding and the Python loader name the same entry
points with the same argument lists, and the command line takes --chain-run K[,DEPTH]."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mgpu_chain_run_capacity", "mgpu_chain_run_open", "mgpu_chain_run_push", "mgpu_chain_run_launch", "mgpu_chain_run_collect",
         "mgpu_chain_run_force", "mgpu_chain_run_close", "mgpu_chain_run_get_stats", "mgpu_chain_run_get_launches"]


def _c_args(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
    assert m, f"{name} is not declared in include/maniac_gpu.h"
    args = []
    for a in m.group(1).split(","):
        a = " ".join(a.split())
        ident = re.search(r"(\w+)\s*(\[\w*\])?$", a).group(1)
        ctype = "double" if "double" in a else ("long long" if "long long" in a else ("ptr" if "mgpu_engine" in a else "int"))
        args.append((ident, ctype, "*" in a or "[" in a))
    return args


def _f_args(f90, name):
    m = re.search(r"function\s+" + name + r"\s*\(([^)]*)\)\s*&?\s*bind\(C,\s*name=\"" + name + r"\"\)(.*?)end function", f90, re.S)
    assert m, f"{name} has no interface in maniac_gpu.f90"
    names = [a.strip() for a in m.group(1).replace("&", " ").split(",")]
    decl = {}
    for line in m.group(2).split("\n"):
        line = line.split("!")[0]
        if "::" not in line or "import" in line:
            continue
        left, right = line.split("::")
        ftype = "ptr" if "c_ptr" in left else ("double" if "c_double" in left else ("long long" if "c_long_long" in left else "int"))
        for v in re.split(r",(?![^()]*\))", right):
            v = v.strip()
            decl[re.match(r"\w+", v).group(0)] = (ftype, "value" not in left)
    return [(n, *decl[n]) for n in names]


@pytest.mark.parametrize("name", NAMES)
def test_header_binding_and_loader_agree(name):
    from maniac_mc_amd import _lib
    header = open(os.path.join(ROOT, "include", "maniac_gpu.h")).read()
    f90 = open(os.path.join(ROOT, "maniac_mc_amd", "fortran", "maniac_gpu.f90")).read()
    assert name in _lib.EXPORTS
    c, f = _c_args(header, name), _f_args(f90, name)
    assert len(c) == len(f), (c, f)
    for (cn, ct, cptr), (fn, ft, fref) in zip(c, f):
        # a C pointer is a Fortran argument by reference (or the engine's c_ptr by value); a C scalar is passed by value
        if ct == "ptr":
            assert ft == "ptr" and not fref, (cn, fn)
        else:
            assert ct == ft and cptr == fref, (name, cn, fn)
    assert 'MGPU_ABI_VERSION 2' in " ".join(header.split())


def test_the_library_exports_them():
    from maniac_mc_amd import _lib
    L = _lib.lib()
    for name in NAMES:
        assert hasattr(L, name)
    import ctypes as C
    H = C.CDLL(os.path.join(ROOT, "maniac_mc_amd", "libmaniac_host.so"))
    assert hasattr(H, "mchain_set_chain_run") and hasattr(H, "mchain_get_chain_run")


def test_the_command_line_flag_parses(capsys):
    from maniac_mc_amd import run
    assert run.parse_chain_run("4") == (4, 3) and run.parse_chain_run("8,2") == (8, 2)
    for bad in ("", "0", "4,0", "a", "4,3,2", "-1"):
        with pytest.raises(ValueError):
            run.parse_chain_run(bad)
    import inspect
    assert inspect.signature(run.run_simulation).parameters["chain_run"].default is None
    # the parser takes the flag (the run stops at the missing input file, after parsing) and refuses a malformed value
    assert run.main(["-i", "/nonexistent.maniac", "-d", "x", "-p", "y", "--chain-run", "4,3"]) == 1
    with pytest.raises(SystemExit):
        run.main(["-i", "x", "-d", "x", "-p", "y", "--chain-run", "four"])
    with pytest.raises(SystemExit):
        run.main(["-i", "x", "-d", "x", "-p", "y", "--chain-run", "4", "--replicas", "2"])
