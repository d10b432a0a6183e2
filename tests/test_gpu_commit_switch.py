"""Commit by switching A(k) buffers: a batched trial's k sweep stores every candidate's A + delta into its replica's other
buffer, and the commit of that trial makes the buffer current instead of recomputing A + delta.  Every case runs twin engines,
one made with MGPU_COMMIT_PASS=1 (every commit recomputes A + delta, as before) and one without, through the same sequence,
and holds them equal bit for bit: energies, counts, coordinates, frames and A(k) read back."""
import os

import numpy as np
import pytest

from maniac_mc_amd import synth
from maniac_mc_amd.engine import Engine
from maniac_mc_amd.system import TOL_K

pytestmark = pytest.mark.gpu


def _with_env(env, make):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: v for k, v in env.items() if v is not None})
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
    try:
        return make()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _twin_farms(s, R, extra_env=None, **kw):
    from maniac_mc_amd.fortran_host import FortranFarm
    env = dict(extra_env or {})
    ref = _with_env({**env, "MGPU_COMMIT_PASS": "1"}, lambda: FortranFarm(s, R, **kw))
    new = _with_env({**env, "MGPU_COMMIT_PASS": None}, lambda: FortranFarm(s, R, **kw))
    return ref, new


def _same_engines(a, b, s, R, frames=True):
    for r in range(R):
        for t in range(s.topo.n_res):
            assert a.num_molecules(r, t) == b.num_molecules(r, t), (r, t)
            assert np.array_equal(a.get_molecules(r, t), b.get_molecules(r, t)), (r, t)
            if frames and s.topo.is_active[t]:
                ca, oa = a.get_frames(r, t)
                cb, ob = b.get_frames(r, t)
                assert np.array_equal(ca, cb) and np.array_equal(oa, ob), (r, t)
        assert np.array_equal(a.structure_factor(r), b.structure_factor(r)), r


def _same_farms(f1, f2, s, R):
    assert f1.trials == f2.trials and f1.accepted == f2.accepted
    assert np.array_equal(f1.counts(), f2.counts())
    for r in range(R):
        assert np.array_equal(f1.energy(r), f2.energy(r)), r
    _same_engines(f1.eng, f2.eng, s, R)


def test_spce_fortran_farm_three_lanes():
    s = synth.spce_box(6)
    R = 48
    f1, f2 = _twin_farms(s, R, seed=29, translation_step=0.3, rotation_step=0.3, n_threads=4, n_lanes=3, device_build=True)
    try:
        assert f1.run(40) == f2.run(40)
        _same_farms(f1, f2, s, R)
    finally:
        f1.close()
        f2.close()


def test_co2_gcmc_deletions_to_small_n():
    s = synth.co2_box(6, seed=13)
    R = 12
    kw = dict(seed=17, translation_step=1.0, rotation_step=0.6, n_threads=4, mol_capacity=[40],
              gcmc=dict(p_translation=0.2, p_rotation=0.2, fugacity=np.full(R, 3.0 / 50.0 ** 3)), device_build=True)
    f1, f2 = _twin_farms(s, R, **kw)
    try:
        assert f1.run(300) == f2.run(300)
        c = f2.counters()
        assert c["deletions"] > 0 and c["creations"] > 0
        assert f2.counts()[:, 0].min() <= 2
        _same_farms(f1, f2, s, R)
    finally:
        f1.close()
        f2.close()


def test_framework_water_farm():
    s = synth.framework_water_box()
    R = 6
    kw = dict(seed=23, translation_step=0.5, rotation_step=0.5, n_threads=4, mol_capacity=[1, 120],
              gcmc=dict(p_translation=0.25, p_rotation=0.25, fugacity=np.full(R, 50.0 / 34.0 ** 3)), device_build=True)
    f1, f2 = _twin_farms(s, R, **kw)
    try:
        assert f1.run(60) == f2.run(60)
        _same_farms(f1, f2, s, R)
    finally:
        f1.close()
        f2.close()


@pytest.mark.parametrize("env", [{}, {"MGPU_RECIP_NO_MFMA": "1"}, {"MGPU_RECIP_PER_K": "1"}], ids=["mfma", "vector", "per_k"])
def test_adsorbate24_and_per_k_forms(env):
    s = synth.rigid_adsorbate_box(n_mol=6, n_sites=24)
    R = 6
    kw = dict(seed=5, translation_step=0.5, rotation_step=0.4, n_threads=2, device_build=True)
    f1, f2 = _twin_farms(s, R, extra_env=env, **kw)
    try:
        assert f1.run(20) == f2.run(20)
        _same_farms(f1, f2, s, R)
    finally:
        f1.close()
        f2.close()


def _twin_engines(s, R, frames=True, cap=None):
    def make():
        e = Engine.from_system(s, n_replicas=R, mol_capacity=cap)
        e.load_system(s, 0)
        if frames:
            e.set_frames(0, 0, s.com[0], s.offsets[0])
        e.init_structure_factor(0, True)
        for r in range(1, R):
            e.replica_copy(r, 0)
        return e
    return _with_env({"MGPU_COMMIT_PASS": "1"}, make), _with_env({"MGPU_COMMIT_PASS": None}, make)


def _fresh_A_and_energy(engines, R):
    for r in range(R):
        ea, eb = engines[0].system_energy(r), engines[1].system_energy(r)
        assert ea == eb
        A = engines[1].structure_factor(r)
        engines[1].init_structure_factor(r, True)
        assert np.max(np.abs(A - engines[1].structure_factor(r))) < 1e-9
        assert abs(engines[1].system_energy(r)["recip_coulomb"] - eb["recip_coulomb"]) < TOL_K


def test_engine_sequences_device_built():
    """Batched steps on three lanes (one with every candidate rejected; two trials before the commit of the second), farm
    windows in between, replica_copy from replicas whose current A(k) may be the other buffer; then the static energy and
    A(k) against a fresh evaluation after many switched commits."""
    s = synth.spce_box(5, seed=4)
    R = 8
    engines = _twin_engines(s, R)
    rng = np.random.default_rng(3)
    n_mol = int(s.n_mol[0])
    rep = np.arange(R, dtype=np.int32)
    zeros = np.zeros(R, np.int32)

    def batched(lane, accept):
        m = rng.integers(0, n_mol, R).astype(np.int32)
        move = rng.integers(1, 3, R).astype(np.int32)
        u = rng.uniform(0, 1, (R, 5))
        out = []
        for e in engines:
            out.append(e.move_trial(rep, zeros, m, move, u, 0.3, 0.3, lane=lane))
            e.commit_lane(lane, rep, zeros, m, zeros, accept)
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])

    for step in range(60):
        batched(step % 3, rng.integers(0, 2, R).astype(np.int32))
    batched(1, np.zeros(R, np.int32))
    m1 = rng.integers(0, n_mol, R).astype(np.int32)
    u1 = rng.uniform(0, 1, (R, 5))
    for e in engines:
        e.move_trial(rep, zeros, m1, np.ones(R, np.int32), u1, 0.3, 0.3, lane=2)
    batched(2, np.ones(R, np.int32))
    _same_engines(*engines, s, R)
    if engines[0].farm_window_capacity()[0] >= R:
        for _ in range(5):
            m = rng.integers(0, n_mol, R).astype(np.int32)
            move = rng.integers(1, 3, R).astype(np.int32)
            u = rng.uniform(0, 1, (R, 5))
            au = rng.uniform(0, 1, R)
            res = []
            for e in engines:
                e.farm_window_submit(rep, zeros, m, move, u, 0.3, 0.3, au, np.ones(R), 300.0, lane=1)
                res.append(e.farm_window_wait(R, lane=1))
            for a, b in zip(res[0], res[1]):
                assert np.array_equal(a, b)
        for step in range(10):
            batched(step % 3, rng.integers(0, 2, R).astype(np.int32))
        _same_engines(*engines, s, R)
    for step in range(8):
        batched(step % 3, np.ones(R, np.int32))
    for e in engines:
        e.replica_copy(0, R - 1)
        e.replica_copy(1, R - 2)
    for step in range(4):
        batched(step % 3, rng.integers(0, 2, R).astype(np.int32))
    _same_engines(*engines, s, R)
    _fresh_A_and_energy(engines, R)
    for e in engines:
        e.close()


def test_engine_sequences_host_sites():
    """Host-built candidates (moves, insertions, deletions): commits from the lane's resident rows switch buffers; commits
    with explicit sites that are not the last trial's (mgpu_commit_candidates) recompute A + delta."""
    s = synth.spce_box(5, seed=4)
    R = 8
    engines = _twin_engines(s, R, frames=False, cap=[200])
    rng = np.random.default_rng(5)
    rep = np.arange(R, dtype=np.int32)
    zeros = np.zeros(R, np.int32)
    for step in range(40):
        counts = [engines[0].num_molecules(r, 0) for r in range(R)]
        kind = rng.integers(0, 3, R).astype(np.int32)
        m = np.array([rng.integers(0, counts[r]) for r in range(R)], np.int32)
        sites = np.empty((R, 3, 3))
        for r in range(R):
            base = engines[0].get_molecules(r, 0)[m[r]]
            sites[r] = base + rng.uniform(-0.3, 0.3, (1, 3)) if kind[r] != 1 else base + rng.uniform(-4.0, 4.0, (1, 3))
        accept = rng.integers(0, 2, R).astype(np.int32)
        out = []
        for e in engines:
            out.append(e.gcmc_trial(rep, zeros, m, kind, sites, lane=step % 2))
            if step % 5 == 4:
                other = sites + 0.01
                e.commit_candidates(rep, zeros, m, kind, other, accept)
            else:
                e.commit_lane(step % 2, rep, zeros, m, kind, accept)
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    _same_engines(*engines, s, R, frames=False)
    _fresh_A_and_energy(engines, R)
    for e in engines:
        e.close()
