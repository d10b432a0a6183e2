"""A farm of replicas that starts from DISTINCT configurations (FortranFarm(initial=...), mfarm_set_replica), restarts from
the files an earlier farm wrote (run_replicas(restart_from=...)) and checks itself (FortranFarm.audit, audit.dat).

Fixtures spce_nvt and co2_gcmc: their inputs do not recalibrate the step sizes, so the replicas of a farm do not couple."""
import ctypes as C
import os

import numpy as np
import pytest

from maniac_mc_amd import io_maniac
from maniac_mc_amd.engine import Engine
from maniac_mc_amd.fortran_host import FortranFarm
from maniac_mc_amd.replicas import run_replicas
from maniac_mc_amd.system import KB_KCALMOL, NB_MAX_MOLECULE
from tests.util import GOLDEN, farm_tol

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "runs")
E_KEYS = ("non_coulomb", "coulomb", "recip_coulomb", "ewald_self", "intra_coulomb", "total")
R, BLOCKS, STEPS = 3, 2, 40


def _inputs(case):
    d = os.path.join(RUNS, case, "inputs")
    return os.path.join(d, "system.maniac"), os.path.join(d, "system.data"), os.path.join(d, "system.inc")


def _records(path):
    return [ln.split() for ln in open(path) if ln.strip() and not ln.startswith("#")]


def _tree(path):
    out = {}
    for base, _, files in os.walk(path):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, path)] = open(p, "rb").read()
    return out


def _without_dir(data, root):
    return b"\n".join(ln for ln in data.split(b"\n") if str(root).encode() not in ln)


_first = {}


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    """case -> (directory, result) of the run the restarts start from, made once per case"""
    def get(case):
        if case not in _first:
            out = tmp_path_factory.mktemp(case) / "A"
            res = run_replicas(*_inputs(case), str(out), replicas=R, seed=5, nb_block=BLOCKS, nb_step=STEPS)
            _first[case] = (str(out), res)
        return _first[case]
    yield get
    _first.clear()


def _file_systems(case, root):
    maniac, _, inc = _inputs(case)
    return [io_maniac.load_system(maniac, os.path.join(root, f"replica_{r:04d}", "topology.data"), inc)[0] for r in range(R)]


@pytest.mark.parametrize("case", ["spce_nvt", "co2_gcmc"])
def test_restart_from_the_farms_own_files(case, first_run, tmp_path):
    a_dir, a_res = first_run(case)
    maniac, data, inc = _inputs(case)
    out = str(tmp_path / "B")
    b_res = run_replicas(maniac, data, inc, out, replicas=R, seed=5, nb_block=BLOCKS, nb_step=STEPS, restart_from=a_dir, audit=True)
    systems = _file_systems(case, a_dir)
    inp = io_maniac.load_system(maniac, data, inc)[1]
    if case == "co2_gcmc":
        assert len({tuple(int(n) for n in s.n_mol) for s in systems}) > 1, "the files' counts differ between the replicas"
    for r, s in enumerate(systems):
        d = os.path.join(out, f"replica_{r:04d}")
        eng = Engine.from_system(s, n_replicas=1)
        try:
            e = eng.system_energy(0)
        finally:
            eng.close()
        # block 0 of the restarted run: the energy of the file's configuration, to the printed digits (F16.6: half a unit
        # of the last one, and the rounding of a sum of five terms of this size)
        rec = _records(os.path.join(d, "energy.dat"))[0]
        assert int(rec[0]) == 0
        want = [e["total"], e["recip_coulomb"], e["non_coulomb"], e["coulomb"], e["ewald_self"], e["intra_coulomb"]]
        for printed, v in zip(rec[1:], want):
            print(f"{case} replica {r}: printed {printed}, engine {v * KB_KCALMOL:.9f}")
            assert abs(float(printed) - v * KB_KCALMOL) <= 0.5e-6 + 1e-12 * abs(v * KB_KCALMOL), (case, r, printed, v * KB_KCALMOL)
        for k, rr in enumerate(inp.residues):
            if rr.is_active == 1 and s.n_mol[k] > 0:
                rec = _records(os.path.join(d, f"number_{rr.name}.dat"))[0]
                assert [int(v) for v in rec] == [0, int(s.n_mol[k])]
    # the audit after the last block: every replica's running energy against its energy from scratch
    a = b_res["audit"]
    assert b_res["recomputed_energy"].shape == (R, 6) and a["running"].shape == (R, 5)
    assert np.array_equal(a["running"], b_res["energy"])
    for r in range(R):
        tol = farm_tol(a["recomputed"][r], BLOCKS * STEPS)
        print(f"{case} replica {r}: energy deviation {a['energy_deviation'][r]:.3e} K (tol {tol:.3e}), max |A - S| {a['a_deviation'][r]:.3e}")
        assert a["energy_deviation"][r] == np.max(np.abs(a["running"][r] - a["recomputed"][r, :5]))
        assert a["energy_deviation"][r] <= tol
    lines = [ln for ln in open(os.path.join(out, "audit.dat"))]
    assert lines[0].startswith("#") and len(lines) == R + 1
    for r, ln in enumerate(lines[1:]):
        f = ln.split()
        last = _records(os.path.join(out, f"replica_{r:04d}", "energy.dat"))[-1]
        assert int(f[0]) == r and len(f) == 5
        assert abs(float(f[1]) - float(last[1])) <= 1e-6 + 1e-12 * abs(float(last[1]))
        assert abs(float(f[2]) - float(last[1])) <= 1e-6 + a["energy_deviation"][r] * KB_KCALMOL * 5
    assert sorted(os.listdir(out)) == sorted(["audit.dat", "replicas.dat"] + [f"replica_{r:04d}" for r in range(R)])


def test_a_default_run_writes_what_it_wrote(first_run):
    a_dir, _ = first_run("co2_gcmc")
    parent = os.path.dirname(a_dir)
    out = os.path.join(parent, "Z")                      # (beside the first run: log.maniac names its directory)
    res = run_replicas(*_inputs("co2_gcmc"), out, replicas=R, seed=5, nb_block=BLOCKS, nb_step=STEPS)
    assert "audit" not in res and "recomputed_energy" not in res
    ta, tb = _tree(a_dir), _tree(out)
    assert sorted(ta) == sorted(tb) and "audit.dat" not in tb
    for name in ta:
        assert _without_dir(ta[name], parent) == _without_dir(tb[name], parent), name


def _farm(case, system, device_build, window, initial=None):
    maniac, data, inc = _inputs(case)
    inp = io_maniac.load_system(maniac, data, inc)[1]
    topo = system.topo
    cap = [NB_MAX_MOLECULE if topo.is_active[t] == 1 else max(1, int(system.n_mol[t])) for t in range(topo.n_res)]
    active = [t for t in range(topo.n_res) if topo.is_active[t] == 1]
    gcmc = dict(p_translation=inp.translation_proba, p_rotation=inp.rotation_proba,
                fugacity=np.array([inp.fugacity_per_A3()[t] for t in active]))
    extra = dict(initial=initial) if initial is not None else {}
    return FortranFarm(system, R, seed=9, translation_step=inp.translation_step, rotation_step=inp.rotation_step_angle,
                       p_translation=inp.translation_proba, mol_capacity=cap, gcmc=gcmc, device_build=device_build,
                       window=window, **extra)


def _replica_state(farm, r):
    out = dict(counters=farm.chain_counters()[r], counts=farm.counts()[r], energy=farm.energy(r))
    frames = []
    for ia, t in enumerate(farm.active):
        if farm.device_build:
            frames.append(farm.eng.get_frames(r, int(t)))
        else:
            frames.append([farm.molecule(r, ia, m) for m in range(int(out["counts"][ia]))])
    out["frames"] = frames
    return out


def _same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b)


@pytest.mark.parametrize("device_build,window", [(True, True), (False, False)], ids=["windows", "host_built"])
def test_a_replica_does_not_depend_on_its_neighbours_start(first_run, device_build, window):
    """Replica 1 of a farm whose replicas all start from configuration 1 (the old way: copies of replica 0) and of a farm whose
    replicas start from configurations 0, 1, 2: the same chain, step for step."""
    a_dir, _ = first_run("co2_gcmc")
    s = _file_systems("co2_gcmc", a_dir)
    assert len({tuple(int(n) for n in v.n_mol) for v in s}) > 1
    old = _farm("co2_gcmc", s[1], device_build, window)
    try:
        assert old.window == window
        old.run(60)
        want = _replica_state(old, 1)
    finally:
        old.close()
    farm = _farm("co2_gcmc", s[1], device_build, window, initial=s)
    try:
        assert farm.window == window and farm.device_build == device_build
        assert np.array_equal(farm.counts(), [[int(v.n_mol[t]) for t in farm.active] for v in s])
        farm.run(60)
        got = _replica_state(farm, 1)
        assert farm.accepted > 0
        for k in ("counters", "counts", "energy"):
            assert np.array_equal(got[k], want[k]), k
        assert _same(got["frames"], want["frames"])
        # the farm checks itself: running against from-scratch energies of ALL its chains, one batched call
        a = farm.audit()
        single = np.array([[farm.eng.system_energy(r)[k] for k in E_KEYS] for r in range(R)])
        assert np.array_equal(a["recomputed"], single)
        assert np.array_equal(a["running"], [farm.energy(r) for r in range(R)])
        for r in range(R):
            tol = farm_tol(a["recomputed"][r], 60)
            print(f"replica {r}: energy deviation {a['energy_deviation'][r]:.3e} K (tol {tol:.3e}), max |A - S| {a['a_deviation'][r]:.3e}")
            assert a["energy_deviation"][r] <= tol
        sub = farm.audit([2, 0])
        assert np.array_equal(sub["recomputed"], single[[2, 0]]) and np.array_equal(sub["a_deviation"], a["a_deviation"][[2, 0]])
        # a replica's start is the farm's to set only before its first run
        farm._select()
        n = np.array([int(s[0].n_mol[t]) for t in farm.active], dtype=np.int32)
        com, off, e5 = np.zeros((max(1, int(n.sum())), 3)), np.zeros((max(1, int(n.sum())), farm.max_n1, 3)), np.zeros(5)
        dp = C.POINTER(C.c_double)
        rc = farm.H.mfarm_set_replica(C.c_int(0), n.ctypes.data_as(C.POINTER(C.c_int)), com.ctypes.data_as(dp),
                                      off.ctypes.data_as(dp), e5.ctypes.data_as(dp))
        assert rc != 0
        assert np.array_equal(farm.energy(0), a["running"][0])
    finally:
        farm.close()


def test_initial_refusals(first_run):
    a_dir, _ = first_run("co2_gcmc")
    s = _file_systems("co2_gcmc", a_dir)
    slots = dict(FortranFarm._slots)
    with pytest.raises(ValueError, match="initial"):
        _farm("co2_gcmc", s[1], True, True, initial=s[:2])                   # a wrong length
    other = s[2].copy()
    other.box_matrix = other.box_matrix * (1.0 + 1e-12)
    with pytest.raises(ValueError, match="box"):
        _farm("co2_gcmc", s[1], True, True, initial=[s[0], s[1], other])
    t = int(np.argmax(s[0].topo.is_active))
    cap = [max(1, max(int(v.n_mol[k]) for v in s) - (1 if k == t else 0)) for k in range(s[1].topo.n_res)]
    with pytest.raises(ValueError, match="capacity"):
        FortranFarm(s[1], R, seed=9, mol_capacity=cap, initial=s)
    assert FortranFarm._slots == slots, "no farm slot is taken by a refused start"
