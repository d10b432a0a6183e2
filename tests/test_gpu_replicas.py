"""A MANIAC input as a farm of replicas (maniac_mc_amd.replicas, mfarm_write_block, mgpu_farm_snapshot_*): the snapshot
equals the per-replica getters bit for bit; the farm's modes write the same bytes; every replica's files are consistent
with its final state; replicas are independent and reproducible; fugacity groups give an isotherm."""
import os
import subprocess
import sys

import numpy as np
import pytest

from maniac_mc_amd import io_maniac
from maniac_mc_amd.engine import Engine
from maniac_mc_amd.fortran_host import FortranFarm
from maniac_mc_amd.replicas import run_replicas
from maniac_mc_amd.system import KB_KCALMOL
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "runs")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(case):
    d = os.path.join(RUNS, case, "inputs")
    rsv = os.path.join(d, "reservoir.data")
    return (os.path.join(d, "system.maniac"), os.path.join(d, "system.data"), os.path.join(d, "system.inc"),
            rsv if os.path.exists(rsv) else None)


def _tree(path):
    out = {}
    for base, _, files in os.walk(path):
        for f in files:
            p = os.path.join(base, f)
            out[os.path.relpath(p, path)] = open(p, "rb").read()
    return out


def _run(case, out, **kw):
    maniac, data, inc, rsv = _inputs(case)
    return run_replicas(maniac, data, inc, str(out), reservoir_path=rsv, **kw)


@pytest.mark.parametrize("window", [True, False])
def test_snapshot_equals_getters(window):
    maniac, data, inc, rsv = _inputs("dumbbell_gcmc_reservoir")
    system, inp = io_maniac.load_system(maniac, data, inc)
    t = next(k for k in range(system.topo.n_res) if system.topo.is_active[k])
    R = 70
    fug = np.geomspace(0.2, 5.0, R)[:, None] * inp.fugacity_per_A3()[t]
    cap = [max(8, 3 * int(n)) if system.topo.is_active[k] else max(1, int(n)) for k, n in enumerate(system.n_mol)]
    farm = FortranFarm(system, R, seed=11, mol_capacity=cap, n_lanes=3, device_build=True, window=window,
                       gcmc=dict(p_translation=0.3, p_rotation=0.2, fugacity=fug),
                       reservoir=io_maniac.reservoir_offsets(rsv, inp))
    try:
        assert farm.window == window
        farm.run(40)
        assert farm.accepted > 0
        counts = farm.counts()[:, 0]
        assert len(set(counts.tolist())) > 1                   # the replicas' counts differ
        eng = farm.eng
        eng.set_num_molecules(5, t, 0)                          # a replica whose type has been emptied
        for reps, chunk in ((list(range(R)), None), ([69, 3, 5, 40, 0], None), (list(range(0, R, 2)), 7)):
            n, com, off, res = eng.farm_snapshot(reps, chunk=chunk)
            for i, r in enumerate(reps):
                for k in range(system.topo.n_res):
                    assert n[i, k] == eng.num_molecules(r, k)
                    if k != t:
                        continue
                    c, o = eng.get_frames(r, k)
                    assert np.array_equal(com[i][k], c) and np.array_equal(off[i][k], o)
                    assert np.array_equal(res[i][k], eng.get_reservoir(r, k))
        n, com, off, _ = eng.farm_snapshot([5])
        assert n[0, t] == 0 and com[0][t].shape == (0, 3)
    finally:
        farm.close()


@pytest.mark.parametrize("case", ["spce_nvt", "co2_gcmc", "dumbbell_gcmc_reservoir", "framework_water_nvt"])
def test_modes_write_the_same_bytes(case, tmp_path):
    trees = {}
    for mode in ("auto", "device", "device_accept"):
        res = _run(case, tmp_path / mode, replicas=4, seed=7, mode=mode, nb_block=3, nb_step=40, frames=(0, 2))
        assert res["mode"] in ("windows", "device", "device_accept")
        trees[mode] = _tree(tmp_path / mode)
    assert sorted(trees["auto"]) == sorted(trees["device"]) == sorted(trees["device_accept"])
    for name in trees["auto"]:
        a = [_without_dir(trees[m][name], tmp_path) for m in trees]
        assert a[0] == a[1] == a[2], name


def _without_dir(data, tmp_path):
    """The file's bytes without the lines that name the output directory (log.maniac's closing box)."""
    return b"\n".join(ln for ln in data.split(b"\n") if str(tmp_path).encode() not in ln)


def _last_record(path):
    rows = [ln.split() for ln in open(path) if ln.strip() and not ln.startswith("#")]
    return rows[-1]


def _check_replica_files(case, out, res, from_scratch=True):
    maniac, data, inc, _ = _inputs(case)
    R = res["energy"].shape[0]
    moves = np.zeros(8, dtype=np.int64)
    for r in range(R):
        d = os.path.join(out, f"replica_{r:04d}")
        for f in ("energy.dat", "moves.dat", "log.maniac", "topology.data"):
            assert os.path.exists(os.path.join(d, f)), (r, f)
        system, inp = io_maniac.load_system(maniac, os.path.join(d, "topology.data"), inc)
        last_e = float(_last_record(os.path.join(d, "energy.dat"))[1])
        if from_scratch:
            eng = Engine.from_system(system, n_replicas=1)
            try:
                eng.init_structure_factor(0, True)
                e = eng.system_energy(0)
            finally:
                eng.close()
            # topology.data holds the positions to 1e-7 A (F12.7): the energy of the file's configuration differs from the
            # chain's by that rounding (5e-6 kcal/mol on 64 SPC/E), the running total by the printed 1e-6
            assert abs(e["total"] * KB_KCALMOL - last_e) <= 1e-4, r
        assert abs(res["energy"][r].sum() * KB_KCALMOL - last_e) <= 1e-6 + 1e-12 * abs(last_e), r
        for k, rr in enumerate(inp.residues):
            if rr.is_active == 1 and system.n_mol[k] > 0:
                assert int(_last_record(os.path.join(d, f"number_{rr.name}.dat"))[1]) == int(system.n_mol[k])
        m = [int(v) for v in _last_record(os.path.join(d, "moves.dat"))]
        # moves.dat: block, trial T, T, trial C, C, trial D, D, trial R, (D again)
        moves += np.array([m[1], m[2], m[7], res["chain_counters"][r][3], m[3], m[4], m[5], m[6]])
        assert np.array_equal(res["chain_counters"][r][[0, 1, 2, 4, 5, 6, 7]], [m[1], m[2], m[7], m[3], m[4], m[5], m[6]])
    c = res["counters"]
    assert moves.tolist() == [c["trial_translations"], c["translations"], c["trial_rotations"], c["rotations"],
                              c["trial_creations"], c["creations"], c["trial_deletions"], c["deletions"]]


def _wrap(pos, matrix):
    # WrapIntoBox for an orthorhombic box: [-L/2, L/2] per axis with Fortran nint (half away from zero)
    L = np.diag(matrix)
    x = pos / L
    return pos - L * np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


@pytest.mark.parametrize("case", ["co2_gcmc", "spce_nvt"])
def test_replica_files_are_self_consistent(case, tmp_path):
    res = _run(case, tmp_path, replicas=3, seed=5, nb_block=2, nb_step=60, frames=(0, 1, 2))
    assert res["chain_counters"].sum(axis=0).tolist() == list(res["counters"].values())
    _check_replica_files(case, str(tmp_path), res)
    maniac, data, inc, _ = _inputs(case)
    for r in range(3):
        d = os.path.join(str(tmp_path), f"replica_{r:04d}")
        system, inp, dat = io_maniac.load_system(maniac, os.path.join(d, "topology.data"), inc, with_data=True)
        lines = open(os.path.join(d, "trajectory.lammpstrj")).read().splitlines()
        start = max(i for i, ln in enumerate(lines) if ln.startswith("ITEM: ATOMS"))
        xyz = np.array([[float(v) for v in ln.split()[2:5]] for ln in lines[start + 1:]])
        expect = []
        for k, rr in enumerate(inp.residues):
            for m in range(int(system.n_mol[k])):
                com = _wrap(system.com[k][m], dat["matrix"]) if rr.is_active == 1 else system.com[k][m]
                for a in range(rr.nb_atoms):
                    p = com + system.offsets[k][m][a]
                    expect.append(p if rr.is_active == 1 else _wrap(p, dat["matrix"]))
        assert xyz.shape == (len(expect), 3)
        L = np.diag(dat["matrix"])
        d = xyz - np.array(expect)
        d -= L * np.round(d / L)                     # (the file's centres may be placed differently: same sites modulo the box)
        assert np.max(np.abs(d)) <= 1e-6             # F12.7 of the same positions


def test_replicas_are_independent_and_reproducible(tmp_path):
    a = _run("co2_gcmc", tmp_path / "a", replicas=3, seed=9, nb_block=2, nb_step=50, frames=(0, 1, 2))
    _run("co2_gcmc", tmp_path / "b", replicas=3, seed=9, nb_block=2, nb_step=50, frames=(0, 1, 2))
    ta, tb = _tree(tmp_path / "a"), _tree(tmp_path / "b")
    assert sorted(ta) == sorted(tb)
    for name in ta:
        assert _without_dir(ta[name], tmp_path) == _without_dir(tb[name], tmp_path), name
    trajs = [ta[f"replica_{r:04d}/trajectory.lammpstrj"] for r in range(3)]
    assert len(set(trajs)) == 3
    assert len({tuple(e) for e in a["energy"].round(6).tolist()}) == 3


def test_triclinic_input_runs_host_built(tmp_path):
    res = _run("spce_triclinic_nvt", tmp_path, replicas=2, seed=3, nb_block=2, nb_step=40)
    assert res["mode"] == "host"
    # (the from-scratch energy of a triclinic topology.data read back is not checked: the farm's running energy equals its
    # engine's resident state, but the file read back through io_maniac does not reproduce it yet -- see DESIGN.md §5)
    _check_replica_files("spce_triclinic_nvt", str(tmp_path), res, from_scratch=False)
    assert os.path.exists(tmp_path / "replica_0000" / "trajectory.lammpstrj")
    assert not os.path.exists(tmp_path / "replica_0001" / "trajectory.lammpstrj")


def test_isotherm_groups(tmp_path):
    fug = [5.0, 20.0, 80.0]
    R = 6
    res = _run("lj_gcmc", tmp_path, replicas=R, seed=4, fugacities=fug, nb_block=2, nb_step=80)
    name = "Ar"
    numbers = [np.array([[int(v) for v in ln.split()] for ln in open(tmp_path / f"replica_{r:04d}" / f"number_{name}.dat")
                         if not ln.startswith("#")]) for r in range(R)]
    rows = [ln.split() for ln in open(tmp_path / "replicas.dat") if not ln.startswith("#")]
    assert len(rows) == 3 * len(fug)
    for row in rows:
        block, g = int(row[0]), int(row[1])
        assert float(row[2]) == pytest.approx(fug[g])
        sel = [r for r in range(R) if r % len(fug) == g]
        assert int(row[3]) == len(sel)
        x = np.array([numbers[r][numbers[r][:, 0] == block][0, 1] for r in sel], dtype=np.float64)
        assert float(row[6]) == pytest.approx(x.mean(), abs=1e-6)
        assert float(row[7]) == pytest.approx(x.std(ddof=1) / np.sqrt(x.size), abs=1e-6)
    for r in range(R):
        log = open(tmp_path / f"replica_{r:04d}" / "log.maniac").read()
        assert f"{fug[r % len(fug)]}" in log or f"{fug[r % len(fug)]:g}" in log
    with pytest.raises(ValueError, match="grand-canonical"):
        _run("spce_nvt", tmp_path / "nvt", replicas=2, fugacities=[1.0])


def test_cli_runs_replicas(tmp_path):
    maniac, data, inc, _ = _inputs("co2_gcmc")
    out = str(tmp_path / "out")
    p = subprocess.run([sys.executable, "-m", "maniac_mc_amd.run", "-i", maniac, "-d", data, "-p", inc, "-o", out,
                        "--replicas", "4", "--frames", "0,2", "--seed", "3"], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(out)) == ["replica_0000", "replica_0001", "replica_0002", "replica_0003", "replicas.dat"]
    for r in range(4):
        files = set(os.listdir(os.path.join(out, f"replica_{r:04d}")))
        assert {"energy.dat", "number_CO2.dat", "moves.dat", "log.maniac", "topology.data"} <= files
        assert ("trajectory.lammpstrj" in files) == (r in (0, 2))
    p = subprocess.run([sys.executable, "-m", "maniac_mc_amd.run", "-i", maniac, "-d", data, "-p", inc, "-o", out,
                        "--replicas", "4", "--as-written"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--as-written" in p.stderr
