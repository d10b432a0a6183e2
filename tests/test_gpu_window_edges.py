"""The one-launch window kernels held to the oracle (oracle/refcpu.c) at their variants and edges: every kernel instance of
farm_window_kernel (FLAT x FASTW) on molecules of 1-5 sites with natural decisions, windows of more chains than travel in the
kernel arguments, kFarmDepth windows in flight and two lanes, insertions / deletions (caller-picked and by count), the
triclinic chain_window_kernel and its creation / deletion rows -- and the defects found in that region: the fast fold
behind an accepted non-tight step still in flight, insertion into an emptied type, a stall flag that outlived a reload, a
refused submit that left replicas marked, and counters shared by lanes.

Every farm window is replayed on the oracle: each chain's candidate is rebuilt from the record's numbers (the
construction of src/translation.f90:93-112, src/monte_carlo_utils.f90:30-92, src/create_molecule.f90:166-207), its old / new
components are evaluated there (ComputeOldEnergy / ComputeNewEnergy, src/monte_carlo_utils.f90:275-395), and the oracle
follows the chain only where the device's verdict is 1 -- so every later window is checked against a reference that has
followed the chain, and a rejected step is checked as closely as an accepted one."""
import os
import threading

import numpy as np
import pytest

from maniac_mc_amd import synth
from maniac_mc_amd._lib import MGPU_CREATION, MGPU_DELETION, MGPU_MOVE, MgpuError
from maniac_mc_amd.engine import Engine
from maniac_mc_amd.system import System
from tests.test_gpu_parity import amp_close, close

pytestmark = pytest.mark.gpu

V_REJ, V_ACC, V_UND, V_STALLED, V_IDLE = 0, 1, 2, 4, 5
MGPU_ERR_STATE = 5


def _engine(s, R, env=None, cap=None):
    """An engine of R replicas holding `s` with resident frames; `env` selects the kernel instance at creation."""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine.from_system(s, n_replicas=R, mol_capacity=cap)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for r in range(R):
        _load(eng, r, s)
    return eng


def _load(eng, r, s):
    eng.load_system(s, r)
    for t in range(s.topo.n_res):
        if s.topo.is_active[t]:
            eng.set_frames(r, t, s.com[t], s.offsets[t])
    eng.init_structure_factor(r, True)


class Replay:
    """The oracle of one replica, advanced by the device's verdicts."""

    def __init__(self, refcpu_mod, s):
        self.s = s
        self.P = refcpu_mod.RefCPU(s, mol_capacity=int(np.max(s.n_mol)) + 16)
        self.P.system_energy()
        self.P.init_amplitude(True)
        self.P.all_fourier_terms()
        self.lo = np.asarray(s.bounds_lo, dtype=np.float64)
        self.L = np.diag(np.asarray(s.box_matrix, dtype=np.float64).reshape(3, 3)).copy()

    def _recip_now(self):
        """The reciprocal energy of the oracle's current A(k) (what the device's k role reports as the old state of an
        insertion / deletion): ComputeRecipEnergySingleMol of a molecule against its own saved tables adds exactly zero."""
        P = self.P
        for t in range(self.s.topo.n_res):
            if P.num_residues(t) > 0:
                P.save_fourier(t, 0)
                return P.recip_singlemol(t, 0, 0)
        return 0.0

    def candidate(self, t, m, move, u, t_step, r_step):
        """(com, off) of the trial the record describes (trial_build_kernel's construction)."""
        P = self.P
        n1 = int(self.s.topo.atoms_in_res[t])
        com, off = P.get_molecule(t, 0 if move == 3 else m)
        if move == 1:
            com = P.apply_pbc(com + (np.asarray(u[:3]) - 0.5) * t_step)
        elif move == 2 or (move == 3 and n1 > 1):
            axis = int(u[4] * 3.0) + 1
            theta = (u[3] - 0.5) * r_step if move == 2 else u[3] * 2.0 * np.pi
            off = off @ P.rotation_matrix(axis, theta).T
        if move == 3:
            com = self.lo + self.L * np.asarray(u[:3])
        return com, off

    def step(self, t, m, move, u, t_step, r_step, verdict, committed=None):
        """Expected (old[5], new[5]) of the step; the oracle keeps it where verdict == 1.  `committed`: the device's frames
        of the accepted molecule (com, off), which the oracle then takes over exactly."""
        P = self.P
        A0 = P.amplitude()
        n = P.num_residues(t)
        if move in (1, 2):
            com0, off0 = P.get_molecule(t, m)
            com, off = self.candidate(t, m, move, u, t_step, r_step)
            if committed is not None:
                assert np.max(np.abs(committed[0] - com)) < 1e-9 and np.max(np.abs(committed[1] - off)) < 1e-9
                com, off = committed
            P.fourier_singlemol(t, m)
            P.save_fourier(t, m)
            old = P.old_energy(t, m, 0)[:5]
            P.set_molecule(t, m, com, off)
            new = P.new_energy(t, m, 0)[:5]
            if verdict != V_ACC:
                P.set_molecule(t, m, com0, off0)
                P.restore_fourier(t, m)
                P.set_amplitude(A0)
        elif move == 3:
            com, off = self.candidate(t, m, move, u, t_step, r_step)
            if committed is not None:
                assert np.max(np.abs(committed[0] - com)) < 1e-9 and np.max(np.abs(committed[1] - off)) < 1e-9
                com, off = committed
            P.set_energy_recip(self._recip_now())
            old = P.old_energy(t, n, 1)[:5]
            P.set_num_residues(t, n + 1)
            P.save_fourier(t, n)
            P.set_molecule(t, n, com, off)
            new = P.new_energy(t, n, 1)[:5]
            if verdict != V_ACC:
                P.set_num_residues(t, n)
                P.set_amplitude(A0)
        else:
            P.set_energy_recip(self._recip_now())
            P.fourier_singlemol(t, m)
            old = P.old_energy(t, m, 2)[:5]
            P.save_fourier(t, m)
            new = np.zeros(5)
            new[2] = P.recip_singlemol(t, m, 2)             # A - S_mol (the batched path's deletion, tests/test_gpu_gcmc.py)
            if verdict == V_ACC:
                lcom, loff = P.get_molecule(t, n - 1)           # swap-with-last, delete_molecule.f90:107-114
                P.set_molecule(t, m, lcom, loff)
                P.replace_fourier(t, m, n - 1)
                P.set_num_residues(t, n - 1)
            else:
                P.set_amplitude(A0)
        return old, new


def _same_as_oracle(eng, reps, what):
    """every replica's counts and sites against the oracle that followed it"""
    for r, rp in enumerate(reps):
        for t in range(rp.s.topo.n_res):
            if not rp.s.topo.is_active[t]:
                continue
            n = rp.P.num_residues(t)
            assert eng.num_molecules(r, t) == n, (what, r, t)
            got = eng.get_molecules(r, t)
            for m in range(n):
                com, off = rp.P.get_molecule(t, m)
                assert np.max(np.abs(got[m] - (com[None, :] + off))) < 1e-9, (what, r, t, m)


def _by_count(n_now, cap_t, move, su, phiV):
    """(live, m, pref) of a by-count record as the launch completes it from the count n_now (mc_farm.f90 select_move)."""
    if move == 3:
        return n_now < cap_t, 0, phiV / (n_now + 1.0)
    if n_now <= 0:
        return False, 0, 1.0
    m = min(int(su * n_now), n_now - 1)
    return True, m, ((n_now - 1.0) + 1.0) / phiV if move == 4 else 1.0


def _check_window(eng, reps, recs, old, new, v, t_step, r_step, what, readback=True):
    """Replay one collected window on the oracles: recs[c] = (replica, t, m, move, u); returns the verdicts seen.
    readback: no later window of these replicas has run yet -- an accepted step's committed frames are read back and
    compared with the candidate rebuilt here."""
    for c, (r, t, m, move, u) in enumerate(recs):
        if move == 0:
            assert v[c] == V_IDLE and not np.any(old[c]) and not np.any(new[c]), (what, c)
            continue
        assert v[c] in (V_ACC, V_REJ), (what, c, v[c])
        committed = None
        if readback and v[c] == V_ACC and move != 4:
            n = eng.num_molecules(r, t)
            slot = n - 1 if move == 3 else m
            com, off = eng.get_frames(r, t)
            committed = (com[slot], off[slot])
            sites = eng.get_molecules(r, t)[slot]
            assert np.array_equal(sites, com[slot][None, :] + off[slot]), (what, c)
        eo, en = reps[r].step(t, m, move, u, t_step, r_step, v[c], committed)
        close(old[c], eo, f"{what} chain {c} (replica {r}, move {move}) old")
        close(new[c], en, f"{what} chain {c} (replica {r}, move {move}) new")
    return list(v)


def _configs(base, R, rng, jitter=0.2):
    out = []
    for r in range(R):
        s = base.copy()
        for t in range(s.topo.n_res):
            if s.topo.is_active[t] and r > 0:
                s.com[t] = _wrap(s, s.com[t] + rng.uniform(-jitter, jitter, s.com[t].shape))
        out.append(s)
    return out


def _wrap(s, com):
    """centres back into the cell (the frames of a tight type: every centre in the cell)"""
    lo = np.asarray(s.bounds_lo, dtype=np.float64)
    L = np.diag(np.asarray(s.box_matrix, dtype=np.float64).reshape(3, 3))
    return lo + np.mod(com - lo, L)


def _records(rng, s, R, t_act, n_now):
    m = np.array([rng.integers(0, n_now[r]) for r in range(R)], dtype=np.int32)
    move = rng.integers(1, 3, R).astype(np.int32)
    if int(s.topo.atoms_in_res[t_act]) == 1:
        move[:] = 1
    u = rng.uniform(0, 1, (R, 5))
    au = np.where(rng.random(R) < 0.5, 0.03, 0.999999)
    return m, move, u, au


VARIANTS = {"flat_fast": {"MGPU_PAIR_FLAT": "1"}, "flat_exact": {"MGPU_PAIR_FLAT": "1", "MGPU_PAIR_EXACT_FOLD": "1"},
            "plane_fast": {"MGPU_PAIR_FLAT": "0"}, "plane_exact": {"MGPU_PAIR_FLAT": "0", "MGPU_PAIR_EXACT_FOLD": "1"}}
BOXES = {"argon": (lambda: synth.argon_box(3), 0), "co2": (lambda: synth.co2_box(12, L=30.0, seed=2), 0),
         "spce": (lambda: synth.spce_box(4, seed=4), 0), "five_site": (lambda: synth.five_site_water_box(n_mol=12), 0),
         "mixture": (lambda: synth.mixture_box(n_a=8, n_b=6, seed=5), 1)}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("box", sorted(BOXES))
def test_farm_window_instances_track_the_oracle(box, variant, refcpu_mod):
    """Every instance of farm_window_kernel on molecules of 1 to 5 sites (kMaxFusedSitesWide): three chains holding
    different configurations, natural decisions, two windows in flight at a time; each window replayed on the oracle."""
    maker, t_act = BOXES[box]
    base = maker()
    R = 3
    rng = np.random.default_rng(17)
    systems = _configs(base, R, rng)
    eng = _engine(base, R, VARIANTS[variant])
    for r in range(1, R):
        _load(eng, r, systems[r])
    reps = [Replay(refcpu_mod, s) for s in systems]
    T = float(base.temperature)
    rep = np.arange(R, dtype=np.int32)
    tt = np.full(R, t_act, np.int32)
    n_now = [int(base.n_mol[t_act])] * R
    seen = []
    for rnd in range(3):
        batch = []
        for _ in range(2):
            m, move, u, au = _records(rng, base, R, t_act, n_now)
            eng.farm_window_submit(rep, tt, m, move, u, 0.8, 0.6, au, np.ones(R), T)
            batch.append([(r, t_act, int(m[r]), int(move[r]), u[r]) for r in range(R)])
        for i, recs in enumerate(batch):
            old, new, v = eng.farm_window_wait(R)
            seen += _check_window(eng, reps, recs, old, new, v, 0.8, 0.6, f"{box}/{variant} round {rnd}", i == len(batch) - 1)
    assert V_ACC in seen and V_REJ in seen, seen
    _same_as_oracle(eng, reps, f"{box}/{variant}")
    for r in range(R):
        amp_close(eng.structure_factor(r), reps[r].P.amplitude(), f"{box}/{variant} replica {r} A(k)")
    eng.close()


def test_farm_window_of_more_chains_than_the_inline_records(refcpu_mod):
    """45 chains (> kFarmInline = 32: the records are read from pinned host memory), different configurations, two windows
    in flight; every chain replayed on the oracle."""
    base = synth.spce_box(3, seed=8)
    R = 45
    rng = np.random.default_rng(23)
    systems = _configs(base, R, rng, jitter=0.3)
    eng = _engine(base, R)
    assert eng.farm_window_capacity()[0] >= R
    for r in range(1, R):
        _load(eng, r, systems[r])
    reps = [Replay(refcpu_mod, s) for s in systems]
    T = float(base.temperature)
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    n_now = [int(base.n_mol[0])] * R
    batch = []
    for _ in range(2):
        m, move, u, au = _records(rng, base, R, 0, n_now)
        eng.farm_window_submit(rep, tt, m, move, u, 0.8, 0.6, au, np.ones(R), T)
        batch.append([(r, 0, int(m[r]), int(move[r]), u[r]) for r in range(R)])
    seen = []
    for i, recs in enumerate(batch):
        old, new, v = eng.farm_window_wait(R)
        seen += _check_window(eng, reps, recs, old, new, v, 0.8, 0.6, f"window {i}", i == len(batch) - 1)
    assert V_ACC in seen and V_REJ in seen
    _same_as_oracle(eng, reps, "45 chains")
    for r in range(R):
        amp_close(eng.structure_factor(r), reps[r].P.amplitude(), f"replica {r} A(k)")
    eng.close()


def test_farm_windows_in_flight_and_two_lanes(refcpu_mod):
    """kFarmDepth windows queued on one lane before any is collected, each checked against the oracle advanced by the
    verdicts of the windows before it; then two lanes with disjoint replicas, two windows in flight on each.  A(k) of every
    replica after the last wait (read back through the drain that moves it into its primary buffer)."""
    base = synth.co2_box(10, L=28.0, seed=4)
    R = 4
    rng = np.random.default_rng(31)
    systems = _configs(base, R, rng)
    eng = _engine(base, R)
    depth = eng.farm_window_capacity()[1]
    assert depth == 4
    for r in range(1, R):
        _load(eng, r, systems[r])
    reps = [Replay(refcpu_mod, s) for s in systems]
    T = float(base.temperature)
    n_now = [int(base.n_mol[0])] * R
    seen = []
    rep = np.arange(R, dtype=np.int32)
    batch = []
    for _ in range(depth):
        m, move, u, au = _records(rng, base, R, 0, n_now)
        eng.farm_window_submit(rep, np.zeros(R, np.int32), m, move, u, 1.0, 0.8, au, np.ones(R), T)
        batch.append([(r, 0, int(m[r]), int(move[r]), u[r]) for r in range(R)])
    with pytest.raises(MgpuError):
        eng.farm_window_submit(rep, np.zeros(R, np.int32), np.zeros(R, np.int32), np.ones(R, np.int32), np.full((R, 5), 0.5),
                               1.0, 0.8, np.full(R, 0.5), np.ones(R), T)
    for i, recs in enumerate(batch):
        old, new, v = eng.farm_window_wait(R)
        seen += _check_window(eng, reps, recs, old, new, v, 1.0, 0.8, f"depth window {i}", i == len(batch) - 1)
    for r in range(R):
        amp_close(eng.structure_factor(r), reps[r].P.amplitude(), f"replica {r} A(k) after {depth} windows in flight")
    # two lanes, disjoint replicas
    lanes = {0: np.array([0, 2], np.int32), 1: np.array([1, 3], np.int32)}
    queued = {0: [], 1: []}
    for _ in range(2):
        for lane, reps_l in lanes.items():
            m, move, u, au = _records(rng, base, 2, 0, n_now)
            eng.farm_window_submit(reps_l, np.zeros(2, np.int32), m, move, u, 1.0, 0.8, au, np.ones(2), T, lane=lane)
            queued[lane].append([(int(reps_l[c]), 0, int(m[c]), int(move[c]), u[c]) for c in range(2)])
    for lane in (1, 0):
        for i, recs in enumerate(queued[lane]):
            old, new, v = eng.farm_window_wait(2, lane=lane)
            seen += _check_window(eng, reps, recs, old, new, v, 1.0, 0.8, f"lane {lane} window {i}", i == 1)
    assert V_ACC in seen and V_REJ in seen
    _same_as_oracle(eng, reps, "two lanes")
    for r in range(R):
        amp_close(eng.structure_factor(r), reps[r].P.amplitude(), f"replica {r} A(k) after two lanes")
    assert eng.farm_window_stats() == (depth + 4, 0)
    eng.close()


@pytest.mark.parametrize("by_count", [False, True])
def test_farm_window_insertions_and_deletions_track_the_oracle(by_count, refcpu_mod):
    """CO2 GCMC through farm windows: caller-picked molecules (each window collected before the next) or by-count records
    (two windows in flight, the slot and prefactor completed from the count the launch sees).  Energies, verdicts, counts and
    A(k) after the commits against the oracle."""
    base = synth.co2_box(4, L=24.0, seed=6)
    R, cap = 4, 8
    rng = np.random.default_rng(41)
    systems = _configs(base, R, rng)
    eng = _engine(base, R, cap=[cap])
    for r in range(1, R):
        _load(eng, r, systems[r])
    reps = [Replay(refcpu_mod, s) for s in systems]
    T = float(base.temperature)
    V = float(np.prod(np.diag(base.box_matrix)))
    phiV = 3.0
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    seen = set()
    per = 2 if by_count else 1
    for rnd in range(8):
        batch = []
        for _ in range(per):
            n_now = [reps[r].P.num_residues(0) for r in range(R)]
            move = rng.integers(1, 5, R).astype(np.int32)
            move[rng.random(R) < 0.6] = rng.choice([3, 4])
            u = rng.uniform(0, 1, (R, 5))
            au = rng.uniform(0, 1, R)
            su = rng.uniform(0, 1, R)
            if by_count:
                pv = np.where(move >= 3, phiV, 1.0)
                eng.farm_window_submit(rep, tt, np.zeros(R, np.int32), move, u, 1.0, 0.6, au, pv, T, slot_u=su)
            else:
                move[(np.array(n_now) <= 1) & (move != 3)] = 3
                move[(np.array(n_now) >= cap) & (move == 3)] = 4
                m = np.array([rng.integers(0, max(n_now[r], 1)) for r in range(R)], np.int32)
                pref = np.array([_by_count(n_now[r], cap, move[r], su[r], phiV)[2] if move[r] >= 3 else 1.0 for r in range(R)])
                m[move == 3] = 0
                eng.farm_window_submit(rep, tt, m, move, u, 1.0, 0.6, au, pref, T)
                su = np.where(move == 3, 0.0, (m + 0.5) / np.maximum(np.array(n_now), 1))
            batch.append((move, u, su))
        for i, (move, u, su) in enumerate(batch):
            old, new, v = eng.farm_window_wait(R)
            recs = []
            for r in range(R):
                n_r = reps[r].P.num_residues(0)
                live, m, _ = _by_count(n_r, cap, int(move[r]), su[r], phiV)
                recs.append((r, 0, m, int(move[r]) if live else 0, u[r]))
            _check_window(eng, reps, recs, old, new, v, 1.0, 0.6, f"round {rnd}", i == len(batch) - 1)
            for r in range(R):
                seen.add((int(recs[r][3]), int(v[r])))
        _same_as_oracle(eng, reps, f"round {rnd}")
    for r in range(R):
        amp_close(eng.structure_factor(r), reps[r].P.amplitude(), f"replica {r} A(k)")
    assert (3, V_ACC) in seen and (4, V_ACC) in seen, seen
    eng.close()


def _chain_rows(rng, P, t, kinds, n_now, lo, L, tmpl_t):
    """host-built rows of a chain window: moves of distinct molecules, creations, deletions"""
    rows, ms = [], []
    free = list(rng.permutation(n_now))
    for k in kinds:
        if k == MGPU_MOVE:
            m = int(free.pop())
            com, off = P.get_molecule(t, m)
            sites = P.apply_pbc(com + rng.uniform(-0.4, 0.4, 3))[None, :] + off @ P.rotation_matrix(int(rng.integers(1, 4)), 0.3).T
        elif k == MGPU_CREATION:
            m = -1
            sites = (lo + rng.uniform(0.05, 0.95, 3) * L)[None, :] + tmpl_t @ P.rotation_matrix(2, float(rng.uniform(0, 6))).T
        else:
            m = int(free.pop())
            sites = np.zeros((tmpl_t.shape[0], 3))
        rows.append(sites)
        ms.append(m)
    return np.array(ms, np.int32), np.array(rows)


def _chain_oracle(P, t, k, m, sites, n_now, recip_now):
    A0 = P.amplitude()
    if k == MGPU_MOVE:
        com, off = P.get_molecule(t, m)
        P.fourier_singlemol(t, m)
        P.save_fourier(t, m)
        old = P.old_energy(t, m, 0)[:5]
        P.set_molecule(t, m, sites[0], sites - sites[0][None, :])
        new = P.new_energy(t, m, 0)[:5]
        A1 = P.amplitude()
        P.set_molecule(t, m, com, off)
        P.restore_fourier(t, m)
    elif k == MGPU_CREATION:
        P.set_energy_recip(recip_now)
        old = P.old_energy(t, n_now, 1)[:5]
        P.set_num_residues(t, n_now + 1)
        P.save_fourier(t, n_now)
        P.set_molecule(t, n_now, sites[0], sites - sites[0][None, :])
        new = P.new_energy(t, n_now, 1)[:5]
        A1 = P.amplitude()
        P.set_num_residues(t, n_now)
    else:
        P.set_energy_recip(recip_now)
        P.fourier_singlemol(t, m)
        old = P.old_energy(t, m, 2)[:5]
        P.save_fourier(t, m)
        new = np.zeros(5)
        new[2] = P.recip_singlemol(t, m, 2)
        A1 = P.amplitude()
    P.set_amplitude(A0)
    return old, new, A1


@pytest.mark.parametrize("case", ["triclinic_moves", "triclinic_gcmc", "orthorhombic_gcmc", "framework_exact"])
def test_chain_window_variants_against_the_oracle(case, refcpu_mod):
    """chain_window_kernel beyond the orthorhombic move windows: the TRI instance (a tilted mixture box), windows with
    creation and deletion rows, and the framework box with the exact fold.  Every row's components against the oracle,
    A(k), the count and the committed molecule after the device's commit of the first accepted row."""
    env = {}
    if case.startswith("triclinic"):
        s, t = synth.mixture_box(seed=6, tilt=(1.5, -0.8, 0.6)), 0
    elif case == "orthorhombic_gcmc":
        s, t = synth.co2_box(10, L=26.0, seed=3), 0
    else:
        s, t = synth.framework_water_box(n_water=10, n_frame=260, L=23.0, seed=9), 1
        env = {"MGPU_PAIR_EXACT_FOLD": "1"}
    old_env = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine.from_system(s, n_replicas=1)
    finally:
        for k in env:
            os.environ.pop(k, None) if old_env[k] is None else os.environ.__setitem__(k, old_env[k])
    eng.init_structure_factor(0, True)
    rp = Replay(refcpu_mod, s)
    P = rp.P
    rng = np.random.default_rng(5)
    kinds = [MGPU_MOVE, MGPU_MOVE, MGPU_MOVE, MGPU_MOVE] if case in ("triclinic_moves", "framework_exact") else \
        [MGPU_MOVE, MGPU_CREATION, MGPU_DELETION, MGPU_MOVE, MGPU_CREATION]
    kinds = np.array(kinds, np.int32)
    n = len(kinds)
    assert eng.chain_window_capacity() >= n
    tmpl = s.offsets[t][0]
    lo = np.asarray(s.bounds_lo, dtype=np.float64)
    L = np.diag(np.asarray(s.box_matrix, dtype=np.float64).reshape(3, 3))
    n_first = 0
    for w in range(3):
        n_now = eng.num_molecules(0, t)
        assert n_now == P.num_residues(t)
        m, sites = _chain_rows(rng, P, t, kinds, n_now, lo, L, tmpl)
        recip_now = rp._recip_now()
        exp = [_chain_oracle(P, t, int(kinds[c]), int(m[c]), sites[c], n_now, recip_now) for c in range(n)]
        u = np.full(n, 0.999999)
        u[w % n + 1 if w % n + 1 < n else 0] = 1e-300              # this row is accepted unless its energy is absurd
        pref = np.ones(n)
        old, new, first, und = eng.chain_window(0, np.full(n, t, np.int32), m, kinds, sites, u, pref, float(s.temperature),
                                                recip_now)
        assert und == -1
        for c in range(n):
            close(old[c], exp[c][0], f"{case} window {w} row {c} old")
            close(new[c], exp[c][1], f"{case} window {w} row {c} new")
        if first < 0:                                           # (nothing accepted: nothing committed)
            amp_close(eng.structure_factor(0), P.amplitude(), f"{case} window {w} A unchanged")
            continue
        n_first += 1
        k, mf = int(kinds[first]), int(m[first])
        amp_close(eng.structure_factor(0), exp[first][2], f"{case} window {w} A after the commit")
        # the oracle follows the commit
        if k == MGPU_MOVE:
            P.fourier_singlemol(t, mf); P.save_fourier(t, mf)
            P.set_molecule(t, mf, sites[first][0], sites[first] - sites[first][0][None, :])
            P.new_energy(t, mf, 0)
            assert np.array_equal(eng.get_molecules(0, t)[mf], sites[first])
        elif k == MGPU_CREATION:
            P.set_num_residues(t, n_now + 1); P.save_fourier(t, n_now)
            P.set_molecule(t, n_now, sites[first][0], sites[first] - sites[first][0][None, :])
            P.new_energy(t, n_now, 1)
            assert np.array_equal(eng.get_molecules(0, t)[n_now], sites[first])
        else:
            P.fourier_singlemol(t, mf); P.save_fourier(t, mf); P.recip_singlemol(t, mf, 2)
            lcom, lo_ff = P.get_molecule(t, n_now - 1)
            P.set_molecule(t, mf, lcom, lo_ff); P.replace_fourier(t, mf, n_now - 1); P.set_num_residues(t, n_now - 1)
        assert eng.num_molecules(0, t) == P.num_residues(t)
        amp_close(eng.structure_factor(0), P.amplitude(), f"{case} window {w} A followed")
    assert n_first >= 1
    eng.close()


# ---- edges of the ADVICE findings -----------------------------------------------------------------------------------------

def _rod_system():
    """A mixture box (18 x 21 x 24 A) where residue type 1 (diatomic) holds one long rigid rod along z: its offset of
    21 A exceeds 0.24 of the shortest edge (the frames of type 1 are not tight), but every site starts within 0.745 L of
    the cell centre.  Type 0 stays tight.  The other molecules sit away from the column the test uses."""
    s = synth.mixture_box(n_a=4, n_b=2, seed=3)
    lo = np.asarray(s.bounds_lo, dtype=np.float64)
    L = np.diag(np.asarray(s.box_matrix, dtype=np.float64).reshape(3, 3))
    ctr = lo + 0.5 * L
    col = np.array([ctr[0] - 4.0, ctr[1] - 5.0])                    # the (x, y) column of the rod and of the mover
    com0 = [np.array(s.com[0], dtype=np.float64), np.array(s.com[1], dtype=np.float64)]
    off0 = [np.array(s.offsets[0], dtype=np.float64), np.array(s.offsets[1], dtype=np.float64)]
    # type 0: molecule 0 is the mover (starts 5 A beside the column at z = ctr - 9.5), the others on the far side in x / y
    spots = [(col[0] + 5.0, col[1], ctr[2] - 9.5), (ctr[0] + 5.0, ctr[1] + 6.0, ctr[2]), (ctr[0] + 5.0, ctr[1] - 2.0, ctr[2] + 6.0),
             (ctr[0] - 6.0, ctr[1] + 6.0, ctr[2] + 2.0)]
    for i, p in enumerate(spots):
        com0[0][i] = p
    # type 1: molecule 0 is the rod (site 0 at z = ctr - 3.3, site 1 21 A above it); molecule 1 an ordinary diatomic
    com0[1][0] = (col[0], col[1], ctr[2] - 3.3)
    off0[1][0] = 0.0
    off0[1][0][1] = (0.0, 0.0, 21.0)
    com0[1][1] = (ctr[0] + 6.0, ctr[1] - 7.0, ctr[2] - 8.0)
    s2 = System(s.topo, s.box_matrix, s.bounds_lo, s.real_space_cutoff, s.ewald_tolerance, s.temperature, com0, off0)
    return s2, ctr, L


def test_fast_fold_after_an_accepted_non_tight_step_in_flight(refcpu_mod):
    """ADVICE (mgpu_windows.hip:394): window i translates the rod (type 1, frames not tight) with `forced` = accept so that
    its far site ends 32 A (1.33 L) above the cell centre on z; window i + 1, queued before window i is collected, moves a
    type-0 molecule of the same replica 3 A along x, to 2 A beside the rod's column at 9.5 A below the centre: 41.5 A
    (1.73 L) from that site on z, whose nearest image is 6.8 A away (< rc = 8 A) -- a two-instruction fold folds once and
    loses it.  Window i + 1 against the oracle and against an engine with the exact fold."""
    s, ctr, L = _rod_system()
    res = {}
    for name, env in (("default", {}), ("exact", {"MGPU_PAIR_EXACT_FOLD": "1"})):
        eng = _engine(s, 1, env)
        rp = Replay(refcpu_mod, s)
        T = float(s.temperature)
        # window i: the rod up by +14.3 A along z (its centre stays in the cell: ctr + 11.0)
        t_step = 30.0
        u_rod = np.array([[0.5, 0.5, 0.5 + 14.3 / t_step, 0.1, 0.1]])
        eng.farm_window_submit([0], [1], [0], [1], u_rod, t_step, 0.5, [0.5], [1.0], T, forced=[1])
        # window i + 1: the type-0 molecule 0 by -3 A along x
        t_step2 = 10.0
        u_a = np.array([[0.5 - 3.0 / t_step2, 0.5, 0.5, 0.1, 0.1]])
        eng.farm_window_submit([0], [0], [0], [1], u_a, t_step2, 0.5, [0.5], [1.0], T)
        o1, n1, v1 = eng.farm_window_wait(1)
        assert v1[0] == V_ACC
        com, off = eng.get_frames(0, 1)
        assert abs(com[0][2] + off[0][1][2] - (ctr[2] + 32.0)) < 1e-9          # the far site: 0.83 L above the centre
        _check_window(eng, [rp], [(0, 1, 0, 1, u_rod[0])], o1, n1, v1, t_step, 0.5, "window i (rod)", False)
        o2, n2, v2 = eng.farm_window_wait(1)
        res[name] = (o2[0].copy(), n2[0].copy())
        _check_window(eng, [rp], [(0, 0, 0, 1, u_a[0])], o2, n2, v2, t_step2, 0.5, f"window i + 1 ({name} fold)")
        eng.close()
    assert np.array_equal(res["default"][0], res["exact"][0]) and np.array_equal(res["default"][1], res["exact"][1])


@pytest.mark.parametrize("path", ["farm_picked", "farm_by_count", "batched"])
def test_insertion_into_an_emptied_type(path, refcpu_mod):
    """ADVICE (mgpu_kernels_windows.h:535): a type deleted down to zero, then an insertion.  Without a reservoir the
    reference copies molecule 1's offsets whatever the count (create_molecule.f90:196-200) -- the last molecule the type held,
    which its deletion left in slot 0.  Every device-built path does the same, checked against the oracle (geometry,
    energies, A(k)); a type that has never held a molecule on the replica is refused with MGPU_ERR_STATE on every path."""
    s = synth.co2_box(2, L=22.0, seed=9)
    cap = 4
    eng = _engine(s, 2, cap=[cap])
    rp = Replay(refcpu_mod, s)
    T = float(s.temperature)
    phiV = 5.0

    def run(move, m, u, au, pref, su=None):
        if path == "batched":
            o, w, acc = eng.move_trial_decide([0], [0], [m], [move], u[None], 1.0, 0.6, [au], [pref], T)
            eng.synchronize()
            return o, w, np.array([V_ACC if acc[0] else V_REJ])
        eng.farm_window_submit([0], [0], [m], [move], u[None], 1.0, 0.6, [au], [phiV if su is not None else pref], T,
                               forced=None, slot_u=None if su is None else [su])
        return eng.farm_window_wait(1)

    # delete both molecules (forced by a zero draw against a huge prefactor)
    for _ in range(2):
        n = rp.P.num_residues(0)
        u = np.full(5, 0.5)
        su = 0.0 if path == "farm_by_count" else None
        o, w, v = run(4, n - 1 if su is None else 0, u, 0.0, 1e300, su)
        assert v[0] == V_ACC
        _check_window(eng, [rp], [(0, 0, n - 1 if su is None else 0, 4, u)], o, w, v, 1.0, 0.6, "deletion")
    assert eng.num_molecules(0, 0) == 0 and rp.P.num_residues(0) == 0
    # insertion into the emptied type: molecule 1's offsets (slot 0's frame), rotated
    u = np.array([0.3, 0.6, 0.2, 0.37, 0.8])
    o, w, v = run(3, 0, u, 0.0, 1e300, 0.5 if path == "farm_by_count" else None)
    assert v[0] == V_ACC and np.all(np.isfinite(o)) and np.all(np.isfinite(w))
    _check_window(eng, [rp], [(0, 0, 0, 3, u)], o, w, v, 1.0, 0.6, "insertion into the emptied type")
    assert eng.num_molecules(0, 0) == 1
    amp_close(eng.structure_factor(0), rp.P.amplitude(), "A(k) after the insertion")
    # a type that never held a molecule on replica 1: refused, on every path
    eng.set_frames(1, 0, np.zeros((0, 3)), np.zeros((0, 3, 3)))
    eng.init_structure_factor(1, True)
    with pytest.raises(MgpuError) as ei:
        if path == "batched":
            eng.move_trial_decide([1], [0], [0], [3], u[None], 1.0, 0.6, [0.5], [1.0], T)
        else:
            eng.farm_window_submit([1], [0], [0], [3], u[None], 1.0, 0.6, [0.5], [1.0], T,
                                   slot_u=[0.5] if path == "farm_by_count" else None)
    assert ei.value.code == MGPU_ERR_STATE
    eng.close()


@pytest.mark.parametrize("reload", ["set_frames", "load_system", "replica_copy"])
def test_a_reload_clears_the_stall_flag(reload, refcpu_mod):
    """ADVICE (mgpu_kernels_windows.h:438): a replica stalled by an undecided step that is never sent again, then
    reloaded; with the margin back the next window is evaluated (not verdict 4) and matches the oracle."""
    s = synth.spce_box(4, seed=6)
    eng = _engine(s, 2)
    T = float(s.temperature)
    rng = np.random.default_rng(3)
    u = rng.uniform(0, 1, (1, 5))
    eng.chain_set_margin(1e9)
    eng.farm_window_submit([0], [0], [3], [1], u, 0.6, 0.5, [0.5], [1.0], T)
    _, _, v = eng.farm_window_wait(1)
    assert v[0] == V_UND
    eng.chain_set_margin(16.0 * np.finfo(np.float64).eps)
    if reload == "set_frames":
        eng.set_frames(0, 0, s.com[0], s.offsets[0])
    elif reload == "load_system":
        _load(eng, 0, s)
    else:
        eng.replica_copy(0, 1)
    eng.init_structure_factor(0, True)
    rp = Replay(refcpu_mod, s)
    u2 = rng.uniform(0, 1, (1, 5))
    eng.farm_window_submit([0], [0], [5], [2], u2, 0.6, 0.5, [0.4], [1.0], T)
    o, w, v = eng.farm_window_wait(1)
    assert v[0] in (V_ACC, V_REJ), f"after {reload}: verdict {v[0]}"
    _check_window(eng, [rp], [(0, 0, 5, 2, u2[0])], o, w, v, 0.6, 0.5, f"after {reload}")
    eng.close()


def test_a_refused_submit_leaves_no_replica_marked(refcpu_mod):
    """ADVICE (mgpu_windows.hip:366-367): a submit refused for an unknown move code, and one for a replica out of range,
    both after valid records of other replicas; a following valid submit for those same replicas succeeds and matches the
    oracle."""
    s = synth.spce_box(4, seed=7)
    R = 3
    eng = _engine(s, R)
    reps = [Replay(refcpu_mod, s) for _ in range(R)]
    T = float(s.temperature)
    rng = np.random.default_rng(9)
    u = rng.uniform(0, 1, (R, 5))
    with pytest.raises(MgpuError):
        eng.farm_window_submit([0, 1, 2], [0, 0, 0], [1, 2, 3], [1, 2, 7], u, 0.6, 0.5, np.full(R, 0.5), np.ones(R), T)
    with pytest.raises(MgpuError):
        eng.farm_window_submit([0, 1, 5], [0, 0, 0], [1, 2, 3], [1, 2, 1], u, 0.6, 0.5, np.full(R, 0.5), np.ones(R), T)
    au = np.array([0.03, 0.97, 0.5])
    eng.farm_window_submit([0, 1, 2], [0, 0, 0], [1, 2, 3], [1, 2, 1], u, 0.6, 0.5, au, np.ones(R), T)
    o, w, v = eng.farm_window_wait(R)
    _check_window(eng, reps, [(r, 0, r + 1, [1, 2, 1][r], u[r]) for r in range(R)], o, w, v, 0.6, 0.5, "after the refusals")
    assert eng.farm_window_stats() == (1, 0)
    eng.close()


def test_window_counters_of_lanes_driven_by_threads():
    """ADVICE (mgpu_windows.hip:430, 440, 478): three lanes driven from three host threads (ctypes releases the GIL) for a
    few hundred windows; the engine's counts equal what was submitted, exactly.  A regression guard: without atomic
    counters this can still pass by luck."""
    s = synth.spce_box(3, seed=2)
    R, n_lanes, per_lane = 6, 3, 120
    eng = _engine(s, R)
    T = float(s.temperature)
    errors = []

    def drive(lane):
        try:
            rng = np.random.default_rng(100 + lane)
            reps = np.array([2 * lane, 2 * lane + 1], np.int32)
            n_und = 0
            for _ in range(per_lane):
                m = rng.integers(0, int(s.n_mol[0]), 2).astype(np.int32)
                eng.farm_window_submit(reps, np.zeros(2, np.int32), m, np.ones(2, np.int32), rng.uniform(0, 1, (2, 5)), 0.3, 0.3,
                                       rng.uniform(0, 1, 2), np.ones(2), T, lane=lane, forced=np.full(2, 2, np.int32))
                _, _, v = eng.farm_window_wait(2, lane=lane)
                n_und += int(np.sum(v == V_UND))
                assert np.all(v == V_REJ)
        except Exception as exc:           # reported by the main thread
            errors.append(exc)

    threads = [threading.Thread(target=drive, args=(lane,)) for lane in range(n_lanes)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert eng.farm_window_stats() == (n_lanes * per_lane, 0)
    eng.close()
