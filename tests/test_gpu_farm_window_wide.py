"""Farm windows for rigid molecules of 6 to 63 sites (farm_window_kernel<..., WIDE>): capacity by the
rule in include/maniac_gpu.h, then energies, verdicts and committed state (coordinates, frames, counts, A(k)) held bit for
bit to the batched device-built path for these molecules -- mgpu_move_trial_submit, the host's rule, mgpu_commit_submit --
for NVT and by-count GCMC windows, mixed sizes, framework boxes, the undecided protocol and the Fortran driver's window mode;
the 24-site case also against the oracle.  Reference: src/monte_carlo.f90:40-86, src/monte_carlo_utils.f90:184-226, :275-395."""
import contextlib
import os

import numpy as np
import pytest

from maniac_mc_amd import _lib, synth
from maniac_mc_amd.engine import Engine
from maniac_mc_amd.synth import lorentz_berthelot
from maniac_mc_amd.system import System, Topology
from tests.util import tol_for

pytestmark = pytest.mark.gpu

V_REJ, V_ACC, V_UND, V_STALLED, V_IDLE = 0, 1, 2, 4, 5


@contextlib.contextmanager
def _env(**kv):
    """switches read at engine creation"""
    os.environ.update({k: v for k, v in kv.items() if v is not None})
    try:
        yield
    finally:
        for k, v in kv.items():
            if v is not None:
                os.environ.pop(k, None)


def _shell(n_sites, seed=23):
    """template, atom types, charges of synth.large_adsorbate_box's molecule (any site count)"""
    s = synth.large_adsorbate_box(n_sites=n_sites, n_mol=1, L=4.0 * n_sites + 100.0, seed=seed)
    return s.offsets[0][0].copy(), np.array(s.topo.atom_types[0][:n_sites], np.int32), np.array(s.topo.charges[0][:n_sites], np.float64)


def _water():
    t = np.array([[0.0, 0.0, 0.0], [0.8165, 0.5773, 0.0], [-0.8165, 0.5773, 0.0]])
    return t - t.mean(0), np.array([1, 2, 2], np.int32), np.array([-0.8476, 0.4238, 0.4238])


def _system(box, specs, active=None, rc=10.0, tol=1e-5, seed=5, gap=2.5, fixed=None):
    """specs: [(template, types, charges, n_mol)], molecules at random places and orientations, surfaces at least `gap` apart;
    fixed = {type: (com, offsets)} places that type as given (a framework)."""
    box = np.asarray(box, dtype=np.float64)
    rng = np.random.default_rng(seed)
    lo = -0.5 * box.sum(0)
    n_t = len(specs)
    max_atom = max(len(sp[1]) for sp in specs)
    types = np.zeros((n_t, max_atom), np.int32)
    charges = np.zeros((n_t, max_atom))
    eps_d, sig_d = [], []
    base = 0
    for i, (tmpl, ty, q, _) in enumerate(specs):
        types[i, :len(ty)] = ty + base
        charges[i, :len(q)] = q
        for k in range(int(ty.max())):
            eps_d.append(0.05 + 0.03 * ((base + k) % 4)); sig_d.append(2.6 + 0.2 * ((base + k) % 3))
        base += int(ty.max())
    eps, sig = lorentz_berthelot(eps_d, sig_d)
    topo = Topology(atoms_in_res=[len(sp[1]) for sp in specs], atom_types=types, charges=charges,
                    is_active=active or [1] * n_t, epsilon=eps, sigma=sig)
    placed, coms, offs = [], [], []
    inv = np.linalg.inv(box)
    for i, (tmpl, ty, q, n_mol) in enumerate(specs):
        if fixed and i in fixed:
            coms.append(fixed[i][0]); offs.append(fixed[i][1])
            continue
        rad = float(np.max(np.linalg.norm(tmpl, axis=1)))
        c_t = []
        while len(c_t) < n_mol:
            p = lo + rng.uniform(0.0, 1.0, 3) @ box
            ok = True
            for (pp, rr) in placed:
                d = (p - pp) @ inv
                d -= np.rint(d)
                if np.linalg.norm(d @ box) < rad + rr + gap:
                    ok = False
                    break
            if ok:
                placed.append((p, rad)); c_t.append(p)
        coms.append(np.array(c_t).reshape(-1, 3))
        offs.append(np.einsum("mij,aj->mai", synth._random_rotations(rng, n_mol), tmpl))
    return System(topo, box, lo, rc, tol, 300.0, coms, offs)


def _box(name):
    """(system, active types)"""
    if name in ("6", "12", "24", "48"):
        return synth.rigid_adsorbate_box(n_mol=6, n_sites=int(name), seed=17), [0]
    if name == "7":
        return synth.large_adsorbate_box(n_sites=7, n_mol=6, L=30.0, seed=38), [0]
    if name == "3+24":
        return _system(np.diag([36.0, 36.0, 36.0]), [(*_water(), 10), (*_shell(24, seed=21), 3)], seed=21), [0, 1]
    if name == "64":
        return synth.large_adsorbate_box(n_sites=64, n_mol=3, L=34.0, seed=95), [0]
    raise KeyError(name)


def _twin(s, R, cap=None, env=None):
    """The batched engine and the window engine: R copies of `s`, resident molecule frames."""
    out = []
    with _env(**(env or {})):
        for _ in range(2):
            e = Engine.from_system(s, n_replicas=R, mol_capacity=cap)
            e.load_system(s, 0)
            for t in range(s.topo.n_res):
                if s.topo.is_active[t]:
                    e.set_frames(0, t, s.com[t], s.offsets[t])
            e.init_structure_factor(0, True)
            for r in range(1, R):
                e.replica_copy(r, 0)
            out.append(e)
    return out


def _same_state(a, b, s, R):
    for r in range(R):
        for t in range(s.topo.n_res):
            assert a.num_molecules(r, t) == b.num_molecules(r, t), (r, t)
            assert np.array_equal(a.get_molecules(r, t), b.get_molecules(r, t)), (r, t)
            if s.topo.is_active[t] and a.num_molecules(r, t):
                ca, oa = a.get_frames(r, t)
                cb, ob = b.get_frames(r, t)
                assert np.array_equal(ca, cb) and np.array_equal(oa, ob), (r, t)
        assert np.array_equal(a.structure_factor(r), b.structure_factor(r)), r


def _batched_step(a, rep, tt, m, move, u, ts, rs, au, pref, T, margin=16 * np.finfo(float).eps):
    """mgpu_move_trial_submit + the host's rule + mgpu_commit_submit: (old, new, accepted, near), near = the draw lies within
    the window's default margin of the probability (the window would leave such a step to the host)."""
    o, w = a.move_trial(rep, tt, m, move, u, ts, rs)
    x = pref * np.exp(-(w.sum(1) - o.sum(1)) / T)
    yes = au <= np.minimum(1.0, x)
    kind = np.where(move <= 2, _lib.MGPU_MOVE, np.where(move == 3, _lib.MGPU_CREATION, _lib.MGPU_DELETION)).astype(np.int32)
    a.commit_lane(0, rep, tt, m, kind, yes.astype(np.int32))
    near = (x < 1.0 + margin) & (np.abs(au - x) <= margin * x)
    return o, w, yes, near


def test_capacity_follows_the_rule():
    """> 0 for 6, 7, 12 and 24 sites and a 3 + 24 mixture; 48 sites as the type's own form says (untiled matrix-unit or
    vector form: > 0, tiled: 0); 0 for the per-k form, a 64-site (site-major) type and a tiled matrix-unit type."""
    for name in ("6", "7", "12", "24", "3+24"):
        s, _ = _box(name)
        a, b = _twin(s, 2)
        assert b.farm_window_capacity()[0] == 2, name
        a.close(); b.close()
    s, _ = _box("48")
    e = Engine.from_system(s, n_replicas=2)
    form = e.recip_form(48)["form"]
    assert (e.farm_window_capacity()[0] > 0) == (form in ("wide-vector", "wide-mfma")), form
    e.close()
    with _env(MGPU_RECIP_PER_K="1"):
        e = Engine.from_system(_box("24")[0], n_replicas=2)
    assert e.recip_form(24)["form"] == "per-k" and e.farm_window_capacity()[0] == 0
    e.close()
    e = Engine.from_system(_box("64")[0], n_replicas=2)
    assert e.farm_window_capacity()[0] == 0
    e.close()
    # a plane-major type in a dense k-space: capacity > 0 exactly where its form is untiled
    s = synth.large_adsorbate_box(n_sites=60, n_mol=2, L=60.0, rc=8.0, seed=7)
    e = Engine.from_system(s, n_replicas=2)
    f = e.recip_form(60)["form"]
    assert (e.farm_window_capacity()[0] > 0) == (f in ("wide-vector", "wide-mfma")), f
    e.close()


CASES = [("6", 4), ("7", 4), ("24", 4), ("24", 70), ("3+24", 4), ("3+24", 70)]


@pytest.mark.parametrize("form", ["mfma", "vector"])
@pytest.mark.parametrize("name,R", CASES)
def test_nvt_window_is_the_batched_step(name, R, form):
    """NVT steps of R chains, two windows in flight: old and new energies array_equal to the batched device-built step,
    verdicts those of the host's rule wherever the window decides, coordinates, frames and A(k) array_equal after every
    step.  MGPU_RECIP_NO_MFMA=1 covers the vector wide form, without it the matrix-unit form."""
    s, act = _box(name)
    a, b = _twin(s, R, env={"MGPU_RECIP_NO_MFMA": "1" if form == "vector" else None})
    big = max(int(s.topo.atoms_in_res[t]) for t in act)
    f = b.recip_form(big)["form"]
    assert f in ("rows", "wide-vector", "wide-mfma") and (form == "mfma" or f != "wide-mfma"), f
    assert b.farm_window_capacity()[0] >= R
    rng = np.random.default_rng(5 + R)
    rep = np.arange(R, dtype=np.int32)
    T = float(s.temperature)
    n_acc = 0
    for step in range(3):
        recs = []
        for _ in range(2):
            tt = rng.choice(act, R).astype(np.int32)
            m = np.array([rng.integers(0, int(s.n_mol[t])) for t in tt], np.int32)
            move = rng.integers(1, 3, R).astype(np.int32)
            u = rng.uniform(0, 1, (R, 5)); au = rng.uniform(0, 1, R)
            recs.append((tt, m, move, u, au))
            b.farm_window_submit(rep, tt, m, move, u, 0.5, 0.5, au, np.ones(R), T)
        for tt, m, move, u, au in recs:
            o1, w1, yes, near = _batched_step(a, rep, tt, m, move, u, 0.5, 0.5, au, np.ones(R), T)
            o2, w2, v = b.farm_window_wait(R)
            assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (step, np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))
            assert not near.any() and np.all((v == V_ACC) | (v == V_REJ)) and np.array_equal(v == V_ACC, yes)
            n_acc += int(yes.sum())
        _same_state(a, b, s, R)                                # (both windows have run on the window engine)
    assert n_acc > 0
    a.close(); b.close()


@pytest.mark.parametrize("n_sites", [12, 24])
def test_gcmc_by_count_records_are_the_batched_path(n_sites):
    """By-count insertion / deletion / move records of a 12- and a 24-site type: insertion into a partly filled type,
    deletion down to one molecule and to none, and the full / empty no-ops (idle).  Energies (five components), verdicts,
    counts and state as the batched path run with the slot and prefactor the count gives."""
    s = synth.rigid_adsorbate_box(n_mol=3, n_sites=n_sites, seed=17)
    R, cap = 6, 5
    a, b = _twin(s, R, cap=[cap])
    rng = np.random.default_rng(n_sites)
    T = float(s.temperature)
    phiV = 3.0
    tt = np.zeros(R, np.int32)
    rep = np.arange(R, dtype=np.int32)
    seen = set()
    for rnd in range(14):
        move = rng.integers(1, 5, R).astype(np.int32)
        move[rng.random(R) < 0.6] = rng.choice([3, 4])
        u = rng.uniform(0, 1, (R, 5)); au = rng.uniform(0, 1, R) * 0.3; su = rng.uniform(0, 1, R)
        pv = np.where(move >= 3, phiV, 1.0)
        b.farm_window_submit(rep, tt, np.zeros(R, np.int32), move, u, 1.0, 0.6, au, pv, T, slot_u=su)
        o2, w2, v = b.farm_window_wait(R)
        n_now = np.array([a.num_molecules(r, 0) for r in range(R)])
        live = np.where(move == 3, n_now < cap, n_now > 0)
        m = np.minimum((su * n_now).astype(np.int32), np.maximum(n_now - 1, 0)).astype(np.int32)
        pref = np.ones(R)
        pref[move == 3] = phiV / (n_now[move == 3] + 1.0)
        pref[move == 4] = ((n_now[move == 4] - 1.0) + 1.0) / phiV
        assert np.all(v[~live] == V_IDLE) and not np.any(o2[~live]) and not np.any(w2[~live])
        if live.any():
            o1, w1, yes, near = _batched_step(a, rep[live], tt[live], m[live], move[live], u[live], 1.0, 0.6, au[live], pref[live], T)
            assert np.array_equal(o1, o2[live]) and np.array_equal(w1, w2[live]), rnd
            assert not near.any() and np.array_equal(v[live] == V_ACC, yes)
        seen.update((int(mv), int(vv), int(nn)) for mv, vv, nn in zip(move, v, n_now))
        _same_state(a, b, s, R)
    assert any(mv == 3 and vv == V_ACC and 0 < nn < cap for mv, vv, nn in seen)
    assert any(mv == 4 and vv == V_ACC and nn == 2 for mv, vv, nn in seen)
    assert any(vv == V_IDLE for _, vv, _ in seen)
    a.close(); b.close()


def test_24_sites_against_the_oracle(refcpu_mod):
    """A window of four 24-site chains in different configurations, every step forced to accept: old / new components
    against the oracle for exactly the move the device built, and A(k) after the commit."""
    base = synth.rigid_adsorbate_box(n_mol=6, n_sites=24, seed=17)
    R = 4
    rng = np.random.default_rng(3)
    eng = Engine.from_system(base, n_replicas=R)
    systems, oracles = [], []
    for r in range(R):
        s = base.copy()
        s.com[0] = s.com[0] + rng.uniform(-0.2, 0.2, s.com[0].shape) * (r > 0)
        eng.load_system(s, r)
        eng.set_frames(r, 0, s.com[0], s.offsets[0])
        eng.init_structure_factor(r, True)
        P = refcpu_mod.RefCPU(s)
        P.system_energy(); P.init_amplitude(True)
        systems.append(s); oracles.append(P)
    rep = np.arange(R, dtype=np.int32)
    m = rng.integers(0, int(base.n_mol[0]), R).astype(np.int32)
    move = np.array([1, 2, 2, 1], np.int32)
    u5 = rng.uniform(0, 1, (R, 5))
    eng.farm_window_submit(rep, np.zeros(R, np.int32), m, move, u5, 0.4, 0.4, np.full(R, 0.5), np.ones(R), float(base.temperature),
                           forced=np.ones(R, np.int32))
    old, new, v = eng.farm_window_wait(R)
    assert np.all(v == V_ACC)
    for r in range(R):
        t, mm = 0, int(m[r])
        cand = eng.get_molecules(r, 0)[mm]
        P = oracles[r]
        com, off = P.get_molecule(t, mm)
        P.save_fourier(t, mm)
        eo = P.old_energy(t, mm, 0)[:5]
        P.set_molecule(t, mm, cand[0], cand - cand[0][None, :])
        en = P.new_energy(t, mm, 0)[:5]
        A_after = P.amplitude()
        for got, ref, what in ((old[r], eo, "old"), (new[r], en, "new")):
            err = np.max(np.abs(np.asarray(got) - np.asarray(ref)))
            assert err <= tol_for(*ref, *got), (r, what, err)
        assert np.max(np.abs(eng.structure_factor(r) - A_after)) <= 1e-10, r
    eng.close()


def test_undecided_wide_step_stalls_until_the_host_decides():
    """Margin wide open on 24-site chains: every step undecided, a window in flight behind it stalled (verdict 4), the step
    sent again with the host's decision obeyed; the state is then the batched path's."""
    s = synth.rigid_adsorbate_box(n_mol=6, n_sites=24, seed=17)
    R = 5
    a, b = _twin(s, R)
    rng = np.random.default_rng(2)
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    T = float(s.temperature)
    b.chain_set_margin(1e9)
    recs = [(rng.integers(0, 6, R).astype(np.int32), rng.integers(1, 3, R).astype(np.int32), rng.uniform(0, 1, (R, 5)),
             rng.uniform(0, 1, R)) for _ in range(2)]
    for m, move, u, au in recs:
        b.farm_window_submit(rep, tt, m, move, u, 0.5, 0.5, au, np.ones(R), T)
    o, w, v = b.farm_window_wait(R)
    assert np.all(v == V_UND)
    _, _, v2 = b.farm_window_wait(R)
    assert np.all(v2 == V_STALLED)
    m, move, u, au = recs[0]
    o1, w1, yes, _ = _batched_step(a, rep, tt, m, move, u, 0.5, 0.5, au, np.ones(R), T)
    assert np.array_equal(o1, o) and np.array_equal(w1, w)
    b.farm_window_submit(rep, tt, m, move, u, 0.5, 0.5, au, np.ones(R), T, forced=np.where(yes, 1, 2).astype(np.int32))
    o3, w3, v3 = b.farm_window_wait(R)
    assert np.array_equal(o3, o1) and np.array_equal(w3, w1) and np.array_equal(v3 == V_ACC, yes)
    _same_state(a, b, s, R)
    a.close(); b.close()


def _framework_guest(n_sites=12, n_frame=120, L=26.0, seed=9):
    """A frozen, inactive framework residue (jittered lattice, net neutral) and a guest of n_sites sites."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(n_frame ** (1 / 3)))
    a = L / side
    grid = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)
    fpos = (grid[np.sort(rng.permutation(grid.shape[0])[:n_frame])] + 0.5) * a - L / 2
    fpos = fpos + rng.uniform(-0.3, 0.3, fpos.shape)
    fq = rng.uniform(-0.5, 0.5, n_frame)
    fq -= fq.mean()
    fty = rng.integers(1, 4, n_frame).astype(np.int32)
    fcom = fpos.mean(0)
    frame = (fpos - fcom, fty, fq, 1)
    # guests at lattice cells
    tmpl, ty, q = _shell(n_sites, seed=seed)
    com = (grid[:4] + 0.0) * a - L / 2 + rng.uniform(-0.2, 0.2, (4, 3))
    offs = np.einsum("mij,aj->mai", synth._random_rotations(rng, 4), tmpl)
    return _system(np.diag([L] * 3), [frame, (tmpl, ty, q, 4)], active=[0, 1], seed=seed,
                   fixed={0: (fcom[None, :], (fpos - fcom)[None]), 1: (com, offs)})


@pytest.mark.parametrize("no_frozen_batch", [True, False])
def test_framework_box_with_a_wide_guest(no_frozen_batch):
    """A frozen framework and a 12-site guest: for n1 > 5 the batched path sweeps with the generic kernel with or without
    MGPU_NO_FROZEN_BATCH, and the window agrees with it either way (NVT and GCMC records)."""
    s = _framework_guest()
    R = 4
    a, b = _twin(s, R, cap=[1, 8], env={"MGPU_NO_FROZEN_BATCH": "1" if no_frozen_batch else None})
    assert b.farm_window_capacity()[0] >= R
    rng = np.random.default_rng(11)
    rep = np.arange(R, dtype=np.int32)
    tt = np.ones(R, np.int32)
    T = float(s.temperature)
    V = float(np.linalg.det(s.box_matrix))
    for step in range(6):
        n_now = np.array([a.num_molecules(r, 1) for r in range(R)])
        move = rng.integers(1, 5, R).astype(np.int32)
        move[(n_now <= 1) & (move == 4)] = 1
        move[(n_now >= 8) & (move == 3)] = 2
        m = np.array([rng.integers(0, n_now[r]) for r in range(R)], np.int32)
        m[move == 3] = 0
        u = rng.uniform(0, 1, (R, 5)); au = rng.uniform(0, 1, R) * 0.2
        pref = np.ones(R)
        pref[move == 3] = 2.0 / (n_now[move == 3] + 1.0)
        pref[move == 4] = n_now[move == 4] / 2.0
        b.farm_window_submit(rep, tt, m, move, u, 0.5, 0.5, au, pref, T)
        o2, w2, v = b.farm_window_wait(R)
        o1, w1, yes, near = _batched_step(a, rep, tt, m, move, u, 0.5, 0.5, au, pref, T)
        assert np.array_equal(o1, o2) and np.array_equal(w1, w2), step
        assert not near.any() and np.array_equal(v == V_ACC, yes)
        _same_state(a, b, s, R)
    assert V > 0
    a.close(); b.close()


@pytest.mark.parametrize("case", ["adsorbate24_nvt", "adsorbate12_gcmc"])
def test_fortran_window_farm_is_the_batched_farm(case):
    """mc_farm.f90 turns window mode on from the capacity query: for the 24-site box and a 12-site GCMC farm it does, and its
    counters, counts, running energies, coordinates and A(k) are the batched farm's, bit for bit."""
    from maniac_mc_amd.fortran_host import FortranFarm
    kw = dict(seed=23, n_threads=2, n_lanes=2, device_build=True, translation_step=0.8, rotation_step=0.5)
    if case == "adsorbate24_nvt":
        s, R, steps = synth.rigid_adsorbate_box(n_mol=6, n_sites=24, seed=17), 8, 40
    else:
        s, R, steps = synth.rigid_adsorbate_box(n_mol=4, n_sites=12, seed=17), 6, 80
        kw.update(mol_capacity=[12], gcmc=dict(p_translation=0.3, p_rotation=0.3, fugacity=6.0 / 26.0 ** 3))
    farms = [FortranFarm(s, R, window=w, window_depth=3, **kw) for w in (False, True)]
    assert farms[1].window and not farms[0].window
    for f in farms:
        f.run(steps)
    a, b = farms
    assert a.trials == b.trials and a.accepted == b.accepted and a.accepted > 0
    assert a.counters() == b.counters()
    assert np.array_equal(a.counts(), b.counts())
    for r in range(R):
        assert np.array_equal(a.energy(r), b.energy(r)), r
        assert np.array_equal(a.eng.structure_factor(r), b.eng.structure_factor(r)), r
        for t in a.active:
            assert np.array_equal(a.eng.get_molecules(r, int(t)), b.eng.get_molecules(r, int(t)))
    for f in farms:
        f.close()
