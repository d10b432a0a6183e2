"""Device-built moves and farm windows in TRICLINIC cells (mgpu_set_triclinic_moves): the trial geometry bit for bit against
the oracle's ApplyPBC (tests/test_triclinic_wrap_oracle.py pins that to the compiled reference on these inputs), the energies
against the host-row path and the oracle, the windows against the batched device-built path bit for bit and against the
oracle directly, the Fortran farm's modes against one another, and replica runs.  Two cells (tests/triclinic_cases.py): a
mild tilt, and the largest tilt LAMMPS allows, where the distance search's eight-image certificate fails.
Reference: src/geometry_utils.f90:167-220 (ApplyPBC), :397-411 (ComputeDistance), src/create_molecule.f90:180-184."""
import os

import numpy as np
import pytest

from maniac_mc_amd import _lib
from maniac_mc_amd._lib import MGPU_CREATION, MGPU_DELETION, MGPU_MOVE
from maniac_mc_amd.engine import Engine
from tests import triclinic_cases as tc
from tests.test_gpu_parity import amp_close, close
from tests.util import farm_tol

pytestmark = pytest.mark.gpu

V_REJ, V_ACC, V_UND, V_STALLED, V_IDLE = 0, 1, 2, 4, 5
CELL_R = [("mild", 4), ("mild", 70), ("sheared", 4), ("sheared", 70)]


def _caps(s, extra=3):
    return [int(n) + extra for n in s.n_mol]


def _engine(s, R, cap=None, on=True):
    e = Engine.from_system(s, n_replicas=R, mol_capacity=cap or _caps(s), triclinic_moves=on)
    for t in range(s.topo.n_res):
        e.set_frames(0, t, s.com[t], s.offsets[t])
    e.init_structure_factor(0, True)
    for r in range(1, R):
        e.replica_copy(r, 0)
    return e


def _twin(s, R, cap=None):
    return _engine(s, R, cap), _engine(s, R, cap)


def _same_state(a, b, s, R):
    for r in range(R):
        for t in range(s.topo.n_res):
            assert a.num_molecules(r, t) == b.num_molecules(r, t), (r, t)
            assert np.array_equal(a.get_molecules(r, t), b.get_molecules(r, t)), (r, t)
            ca, oa = a.get_frames(r, t)
            cb, ob = b.get_frames(r, t)
            assert np.array_equal(ca, cb) and np.array_equal(oa, ob), (r, t)
            assert np.array_equal(a.get_reservoir(r, t), b.get_reservoir(r, t)), (r, t)
        assert np.array_equal(a.structure_factor(r), b.structure_factor(r)), r


def _kinds(move):
    return np.where(move <= 2, MGPU_MOVE, np.where(move == 3, MGPU_CREATION, MGPU_DELETION)).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------------
# 7. defaults
@pytest.mark.parametrize("name", tc.CELLS)
def test_without_the_switch_a_triclinic_engine_refuses_as_before(name):
    s = tc.cell(name)
    e = _engine(s, 2, on=False)
    assert e.farm_window_capacity()[0] == 0
    u = np.full((2, 5), 0.5)
    with pytest.raises(_lib.MgpuError) as ei:
        e.move_trial([0, 1], [0, 0], [1, 2], [1, 2], u, 0.4, 0.4)
    assert ei.value.code == 5 and "orthorhombic boxes only" in str(ei.value)          # MGPU_ERR_STATE
    with pytest.raises(_lib.MgpuError) as ei:
        e.move_trial_decide([0, 1], [0, 0], [1, 2], [1, 2], u, 0.4, 0.4, [0.5, 0.5], [1.0, 1.0], 300.0)
    assert ei.value.code == 5
    with pytest.raises(_lib.MgpuError):
        e.farm_window_submit([0, 1], [0, 0], [1, 2], [1, 2], u, 0.4, 0.4, [0.5, 0.5], [1.0, 1.0], 300.0)
    e.set_triclinic_moves(True)
    assert e.farm_window_capacity()[0] == 2
    e.move_trial([0, 1], [0, 0], [1, 2], [1, 2], u, 0.4, 0.4)
    e.set_triclinic_moves(False)
    assert e.farm_window_capacity()[0] == 0
    e.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. geometry
def _geometry_case(s, rng):
    """One candidate per replica: (t, m, move, u[5], com0) with centres that start outside the cell -- edge points of both
    families -- translations that leave them where they are (u = 1/2: f within 1e-16 of 0 and of 1), ordinary draws, and
    insertions at fractional coordinates on and next to the cell's faces."""
    recs = []
    edge = np.vstack([tc.edge_points(s, 12, 41, True), tc.edge_points(s, 6, 42)])
    far = rng.uniform(-200.0, 200.0, (6, 3))
    ins = np.array([0.0, 1e-17, 1e-16, 0.5, 1.0 - 1e-16, 0.25])
    k = 0
    for t in (0, 1):
        n = int(s.n_mol[t])
        for p in edge:                                   # translation by nothing of a centre on the wrap's edges
            u = rng.random(5); u[:3] = 0.5
            recs.append((t, k % n, 1, u, p)); k += 1
        for p in np.vstack([edge[:6], far]):             # translation by a draw, from outside the cell
            recs.append((t, k % n, 1, rng.random(5), p)); k += 1
        for i in range(6):                               # from inside the cell
            recs.append((t, k % n, 1, rng.random(5), None)); k += 1
        for i in range(6):                               # rotation about every axis, centre inside and outside
            u = rng.random(5); u[4] = (0.05, 0.4, 0.7, 0.99, 0.5, 0.2)[i]
            recs.append((t, k % n, 2, u, far[i] if i % 2 else None)); k += 1
        for i in range(8):                               # insertion
            u = rng.random(5); u[:3] = ins[rng.integers(0, len(ins), 3)] if i < 6 else rng.random(3)
            recs.append((t, 0, 3, u, None)); k += 1
    return recs


@pytest.mark.parametrize("name", tc.CELLS)
def test_device_built_geometry_is_the_oracles_bit_for_bit(name, refcpu_mod):
    """Translations, rotations and insertions built on the device, force-accepted and read back (get_frames): every centre
    equals refcpu.apply_pbc(com0 + (u - 1/2) step) EXACTLY, an insertion's equals lo + M u in the stated order, a rotation
    keeps its centre bit for bit; offsets as tests/test_gpu_topology_edges.py checks them (RotationMatrix to 1e-12 A), and
    the stored sites are the rounded sums com + off."""
    s = tc.cell(name)
    P = refcpu_mod.RefCPU(s, mol_capacity=max(_caps(s)))
    rng = np.random.default_rng(17)
    recs = _geometry_case(s, rng)
    n = len(recs)
    eng = Engine.from_system(s, n_replicas=n, mol_capacity=_caps(s), triclinic_moves=True)
    com0 = []
    for r, (t, m, mv, u, p) in enumerate(recs):
        if r:
            eng.replica_copy(r, 0)
        for tt in (0, 1):
            com = s.com[tt].copy()
            if tt == t and p is not None:
                com[m] = p
            eng.set_frames(r, tt, com, s.offsets[tt])
            if tt == t:
                com0.append(com[m].copy())
        eng.init_structure_factor(r, True)
    t = np.array([rc[0] for rc in recs], np.int32)
    m = np.array([rc[1] for rc in recs], np.int32)
    move = np.array([rc[2] for rc in recs], np.int32)
    u = np.array([rc[3] for rc in recs])
    rep = np.arange(n, dtype=np.int32)
    t_step, r_step = 6.0, 0.6
    eng.move_trial(rep, t, m, move, u, t_step, r_step)
    eng.commit_lane(0, rep, t, m, _kinds(move), np.ones(n, np.int32))
    seen_outside = 0
    for c in range(n):
        tt, mm = int(t[c]), int(m[c])
        off0 = s.offsets[tt][mm]
        slot = mm
        if move[c] == 1:
            target = com0[c] + (u[c, :3] - 0.5) * t_step
            com_e, off_e = P.apply_pbc(target), off0
            seen_outside += int(np.max(np.abs(target)) > 60.0)
        elif move[c] == 2:
            com_e, off_e = com0[c], off0 @ P.rotation_matrix(int(u[c, 4] * 3.0) + 1, (u[c, 3] - 0.5) * r_step).T
        else:
            slot = int(s.n_mol[tt])
            com_e = tc.cart(s, u[c, :3])
            off_e = s.offsets[tt][0] @ P.rotation_matrix(int(u[c, 4] * 3.0) + 1, u[c, 3] * 2 * np.pi).T
        com_d, off_d = eng.get_frames(c, tt)
        assert np.array_equal(com_d[slot], com_e), (name, c, int(move[c]), com_d[slot] - com_e)
        if move[c] == 1:
            assert np.array_equal(off_d[slot], off_e), (c, move[c])
        else:
            assert np.max(np.abs(off_d[slot] - off_e)) <= 1e-12, (c, move[c])
        assert np.array_equal(eng.get_molecules(c, tt)[slot], com_d[slot][None, :] + off_d[slot])
        assert eng.num_molecules(c, tt) == s.n_mol[tt] + (move[c] == 3)
    assert seen_outside >= 10
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. energies
@pytest.mark.parametrize("name", tc.CELLS)
def test_device_built_energies_are_the_host_row_paths_and_the_oracles(name, refcpu_mod):
    """The candidates the device builds, read back after a forced commit on one engine, are fed to gcmc_trial as host rows on
    an untouched twin: the five components of both states must be equal BIT FOR BIT; moves and insertions are also held to
    the oracle's ComputeOldEnergy / ComputeNewEnergy within tests/util.py's tol_for."""
    s = tc.cell(name)
    cap = _caps(s)
    rng = np.random.default_rng(23)
    move = np.array([1, 2, 3, 4] * 6, np.int32)
    n = len(move)
    t = np.array(([0] * 4 + [1] * 4) * 3, np.int32)
    a, b = _twin(s, n, cap)
    m = np.array([0 if mv == 3 else int(rng.integers(0, s.n_mol[tt])) for mv, tt in zip(move, t)], np.int32)
    u = rng.random((n, 5))
    rep = np.arange(n, dtype=np.int32)
    kinds = _kinds(move)
    old, new = a.move_trial(rep, t, m, move, u, 0.8, 0.6)
    a.commit_lane(0, rep, t, m, kinds, (move != 4).astype(np.int32))
    W = int(s.topo.atoms_in_res.max())
    rows = np.zeros((n, W, 3))
    for c in range(n):
        n1 = int(s.topo.atoms_in_res[t[c]])
        slot = int(s.n_mol[t[c]]) if move[c] == 3 else int(m[c])
        rows[c, :n1] = a.get_molecules(c, int(t[c]))[slot]
    mh = np.where(move == 3, -1, m).astype(np.int32)
    oh, nh = b.gcmc_trial(rep, t, mh, kinds, rows)
    assert np.array_equal(old, oh), np.max(np.abs(old - oh))
    assert np.array_equal(new, nh), np.max(np.abs(new - nh))
    P = refcpu_mod.RefCPU(s, mol_capacity=max(cap))
    e_sys = P.system_energy()
    P.init_amplitude(True)
    P.set_energy_recip(e_sys["recip_coulomb"])
    for c in range(n):
        tt, mm = int(t[c]), int(m[c])
        n1 = int(s.topo.atoms_in_res[tt])
        sites = rows[c, :n1]
        A0 = P.amplitude()
        if move[c] <= 2:
            com0, off0 = P.get_molecule(tt, mm)
            com_d, off_d = a.get_frames(c, tt)
            P.save_fourier(tt, mm)
            eo = P.old_energy(tt, mm, 0)[:5]
            P.set_molecule(tt, mm, com_d[mm], off_d[mm])
            en = P.new_energy(tt, mm, 0)[:5]
            P.set_molecule(tt, mm, com0, off0)
            P.restore_fourier(tt, mm)
        elif move[c] == 3:
            nn = int(s.n_mol[tt])
            com_d, off_d = a.get_frames(c, tt)
            eo = P.old_energy(tt, nn, 1)[:5]
            P.set_num_residues(tt, nn + 1)
            P.save_fourier(tt, nn)
            P.set_molecule(tt, nn, com_d[nn], off_d[nn])
            en = P.new_energy(tt, nn, 1)[:5]
            P.set_num_residues(tt, nn)
            P.set_amplitude(A0)
        else:
            continue
        close(old[c], eo, f"{name} candidate {c} (move {move[c]}) old")
        close(new[c], en, f"{name} candidate {c} (move {move[c]}) new")
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. windows == the batched device-built path, bit for bit
def _nvt_records(rng, s, R):
    tt = (np.arange(R) % 2).astype(np.int32)
    m = np.array([rng.integers(0, s.n_mol[t]) for t in tt], np.int32)
    move = rng.integers(1, 3, R).astype(np.int32)
    return tt, m, move, rng.uniform(0, 1, (R, 5)), rng.uniform(0, 1, R)


@pytest.mark.parametrize("name,R", CELL_R)
def test_nvt_windows_are_the_batched_device_built_steps(name, R):
    """both residue types, translations and rotations, every second window in flight behind the one before it"""
    s = tc.cell(name)
    a, b = _twin(s, R)
    cap, depth = b.farm_window_capacity()
    assert cap >= R and depth >= 2
    rng = np.random.default_rng(5)
    rep = np.arange(R, dtype=np.int32)
    T = float(s.temperature)
    n_acc = 0
    for step in range(3):
        recs = [_nvt_records(rng, s, R) for _ in range(2)]
        for tt, m, move, u, au in recs:
            b.farm_window_submit(rep, tt, m, move, u, 0.5, 0.5, au, np.ones(R), T)
        for tt, m, move, u, au in recs:
            o1, w1, acc = a.move_trial_decide(rep, tt, m, move, u, 0.5, 0.5, au, np.ones(R), T)
            a.synchronize()
            o2, w2, v = b.farm_window_wait(R)
            assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (step, np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))
            assert np.all((v == V_ACC) | (v == V_REJ)) and np.array_equal(v == V_ACC, acc != 0)
            n_acc += int(acc.sum())
        _same_state(a, b, s, R)
    assert 0 < n_acc <= 6 * R
    assert b.farm_window_stats() == (6, 0)
    a.close(); b.close()


def _by_count_round(a, b, s, R, cap, rng, T, phiV, seen, reservoir_t=None):
    """two by-count windows queued on b, then collected against a's batched decide path run step by step"""
    rep = np.arange(R, dtype=np.int32)
    recs = []
    for _ in range(2):
        tt = rng.integers(0, 2, R).astype(np.int32)
        move = rng.integers(1, 5, R).astype(np.int32)
        move[rng.random(R) < 0.5] = rng.choice([3, 4])
        u = rng.uniform(0, 1, (R, 5)); au = rng.uniform(0, 1, R); su = rng.uniform(0, 1, R)
        pv = np.where(move >= 3, phiV, 1.0)
        recs.append((tt, move, u, au, su, pv))
        b.farm_window_submit(rep, tt, np.zeros(R, np.int32), move, u, 0.8, 0.6, au, pv, T, slot_u=su)
    for tt, move, u, au, su, pv in recs:
        o2, w2, v = b.farm_window_wait(R)
        n_now = np.array([a.num_molecules(r, int(tt[r])) for r in range(R)])
        capt = np.array([cap[t] for t in tt])
        live = np.where(move == 3, n_now < capt, n_now > 0)
        if reservoir_t is not None:          # an insertion from an empty reservoir does nothing
            empty = np.array([a.get_reservoir(r, reservoir_t).shape[0] == 0 for r in range(R)])
            live &= ~((move == 3) & (tt == reservoir_t) & empty)
        m = np.minimum((su * n_now).astype(np.int32), np.maximum(n_now - 1, 0)).astype(np.int32)
        pref = np.ones(R)
        pref[move == 3] = phiV / (n_now[move == 3] + 1.0)
        pref[move == 4] = ((n_now[move == 4] - 1.0) + 1.0) / phiV
        assert np.all(v[~live] == V_IDLE) and not np.any(o2[~live]) and not np.any(w2[~live])
        if live.any():
            o1, w1, acc = a.move_trial_decide(rep[live], tt[live], m[live], move[live], u[live], 0.8, 0.6, au[live], pref[live], T)
            a.synchronize()
            assert np.array_equal(o1, o2[live]) and np.array_equal(w1, w2[live])
            assert np.array_equal(v[live] == V_ACC, acc != 0) and np.all((v[live] == V_ACC) | (v[live] == V_REJ))
        seen.update((int(mv), int(vv)) for mv, vv in zip(move, v))
    _same_state(a, b, s, R)


@pytest.mark.parametrize("name,R", CELL_R)
def test_by_count_insertion_and_deletion_windows_are_the_batched_steps(name, R):
    """insertions, deletions and moves of both types by count, two windows in flight: energies (five components), verdicts,
    counts, coordinates, frames and A(k)"""
    s = tc.cell(name)
    cap = _caps(s, 2)
    a, b = _twin(s, R, cap)
    rng = np.random.default_rng(21)
    seen = set()
    for rnd in range(4 if R > 8 else 10):
        _by_count_round(a, b, s, R, cap, rng, float(s.temperature), 6.0, seen)
    assert {(3, V_ACC), (4, V_ACC)} <= seen and any(mv <= 2 and vv == V_ACC for mv, vv in seen)
    a.close(); b.close()


@pytest.mark.parametrize("name,R", CELL_R)
def test_reservoir_windows_are_the_batched_steps(name, R):
    """type 1 holds a reservoir on every replica: insertions copy reservoir molecules unrotated at lo + M u, deletions feed
    it; box + reservoir count is conserved, and the reservoirs themselves are compared"""
    from maniac_mc_amd import synth
    s = tc.cell(name)
    cap = _caps(s, 2)
    a, b = _twin(s, R, cap)
    rng = np.random.default_rng(31)
    res = np.stack([s.offsets[1][0] @ synth._random_rotations(rng, 1)[0].T for _ in range(3)])
    for e in (a, b):
        for r in range(R):
            e.set_reservoir(r, 1, res)
    total = int(s.n_mol[1]) + 3
    seen = set()
    for rnd in range(3 if R > 8 else 8):
        _by_count_round(a, b, s, R, cap, rng, float(s.temperature), 6.0, seen, reservoir_t=1)
        for r in range(R):
            assert b.num_molecules(r, 1) + b.get_reservoir(r, 1).shape[0] == total, r
    assert (3, V_ACC) in seen and (4, V_ACC) in seen
    a.close(); b.close()


@pytest.mark.parametrize("name,R", CELL_R)
def test_forced_windows_are_the_batched_steps_with_the_same_decisions(name, R):
    """every step sent with the driver's decision: accepted ones are committed as the batched path commits them"""
    s = tc.cell(name)
    cap = _caps(s)
    a, b = _twin(s, R, cap)
    rng = np.random.default_rng(9)
    rep = np.arange(R, dtype=np.int32)
    T = float(s.temperature)
    for step in range(3):
        tt = rng.integers(0, 2, R).astype(np.int32)
        n_now = np.array([a.num_molecules(r, int(tt[r])) for r in range(R)])
        move = rng.integers(1, 5, R).astype(np.int32)
        move[(move == 3) & (n_now >= np.array([cap[t] for t in tt]))] = 1
        move[(move == 4) & (n_now <= 2)] = 2
        m = np.array([0 if mv == 3 else int(rng.integers(0, nn)) for mv, nn in zip(move, n_now)], np.int32)
        u = rng.uniform(0, 1, (R, 5))
        forced = rng.integers(1, 3, R).astype(np.int32)
        b.farm_window_submit(rep, tt, m, move, u, 0.8, 0.6, rng.uniform(0, 1, R), np.ones(R), T, forced=forced)
        o2, w2, v = b.farm_window_wait(R)
        assert np.array_equal(v == V_ACC, forced == 1) and np.all((v == V_ACC) | (v == V_REJ))
        o1, w1 = a.move_trial(rep, tt, m, move, u, 0.8, 0.6)
        assert np.array_equal(o1, o2) and np.array_equal(w1, w2), step
        a.commit_lane(0, rep, tt, m, _kinds(move), (forced == 1).astype(np.int32))
        _same_state(a, b, s, R)
    a.close(); b.close()


@pytest.mark.parametrize("name,R", CELL_R)
def test_undecided_windows_stall_until_the_host_decides(name, R):
    """the margin wide open: every step UNDECIDED, the window behind it stalled, the forced resend obeyed -- state as the
    batched path's for the same decisions"""
    s = tc.cell(name)
    a, b = _twin(s, R)
    rng = np.random.default_rng(2)
    rep = np.arange(R, dtype=np.int32)
    T = float(s.temperature)
    b.chain_set_margin(1e9)
    def records():
        """steps the wide margin leaves undecided: the margin is RELATIVE (undecided: x < 1 + margin and |u - x| <= margin x, x
        = the rule's exp term), so a step whose x underflows (a move into an overlap) or exceeds the margin (a move out of one
        -- the sheared start has some) is decided however wide it is; such draws are made again (energies from the twin)"""
        tt, m, move, u, au = _nvt_records(rng, s, R)
        for _ in range(50):
            o, w = a.move_trial(rep, tt, m, move, u, 0.5, 0.5)
            with np.errstate(over="ignore"):
                x = np.exp(-(w.sum(1) - o.sum(1)) / T)
            zero = ~((x > 1e-6) & (x < 1e6))
            if not zero.any():
                return tt, m, move, u, au
            _, m_new, move_new, u_new, _ = _nvt_records(rng, s, R)       # (another molecule too: one wedged against a neighbour
            m[zero], move[zero], u[zero] = m_new[zero], move_new[zero], u_new[zero]   #  in the sheared start has no such step)
        raise AssertionError("no step inside the margin found")
    tt, m, move, u, au = records()
    tt2, m2, move2, u2, au2 = records()
    move[R - 1] = 0
    move2[R - 1] = 0
    b.farm_window_submit(rep, tt, m, move, u, 0.5, 0.5, au, np.ones(R), T)
    b.farm_window_submit(rep, tt2, m2, move2, u2, 0.5, 0.5, au2, np.ones(R), T)
    o, w, v = b.farm_window_wait(R)
    assert np.all(v[:R - 1] == V_UND) and v[R - 1] == V_IDLE
    _, _, v2 = b.farm_window_wait(R)
    assert np.all(v2[:R - 1] == V_STALLED) and v2[R - 1] == V_IDLE
    live = move != 0
    o1, w1 = a.move_trial(rep[live], tt[live], m[live], move[live], u[live], 0.5, 0.5)
    assert np.array_equal(o1, o[live]) and np.array_equal(w1, w[live])
    yes = au[live] <= np.minimum(1.0, np.exp(-(w1.sum(1) - o1.sum(1)) / T))
    a.commit_lane(0, rep[live], tt[live], m[live], np.zeros(int(live.sum()), np.int32), yes.astype(np.int32))
    forced = np.zeros(R, np.int32)
    forced[live] = np.where(yes, 1, 2)
    b.farm_window_submit(rep, tt, m, move, u, 0.5, 0.5, au, np.ones(R), T, forced=forced)
    o3, w3, v3 = b.farm_window_wait(R)
    assert np.array_equal(o3[live], o1) and np.array_equal(w3[live], w1)
    assert np.array_equal(v3[live] == V_ACC, yes)
    _same_state(a, b, s, R)
    assert b.farm_window_stats()[1] == R - 1
    b.chain_set_margin(16 * np.finfo(float).eps)
    b.farm_window_submit(rep, tt2, m2, move2, u2, 0.5, 0.5, au2, np.ones(R), T)
    _, _, v5 = b.farm_window_wait(R)
    assert np.all((v5[:R - 1] == V_ACC) | (v5[:R - 1] == V_REJ)) and v5[R - 1] == V_IDLE
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. windows held to the oracle directly (mild cell)
def test_triclinic_farm_window_energies_against_the_oracle(refcpu_mod):
    """one window over four chains holding different configurations and both residue types, every step forced `accept`: old
    and new components against the oracle evaluated for the candidate the device built, A(k) after the commit, and the
    committed centre against the oracle's ApplyPBC bit for bit"""
    base = tc.cell("mild")
    R = 4
    rng = np.random.default_rng(3)
    eng = Engine.from_system(base, n_replicas=R, triclinic_moves=True)
    systems, oracles = [], []
    for r in range(R):
        s = base.copy()
        for t in (0, 1):
            s.com[t] = s.com[t] + rng.uniform(-0.2, 0.2, s.com[t].shape) * (r > 0)
        eng.load_system(s, r)
        for t in (0, 1):
            eng.set_frames(r, t, s.com[t], s.offsets[t])
        eng.init_structure_factor(r, True)
        P = refcpu_mod.RefCPU(s)
        P.system_energy(); P.init_amplitude(True)
        systems.append(s); oracles.append(P)
    rep = np.arange(R, dtype=np.int32)
    tt = np.array([0, 1, 0, 1], np.int32)
    m = np.array([rng.integers(0, base.n_mol[t]) for t in tt], np.int32)
    move = np.array([1, 2, 2, 1], np.int32)
    u5 = rng.uniform(0, 1, (R, 5))
    eng.farm_window_submit(rep, tt, m, move, u5, 0.5, 0.5, np.full(R, 0.5), np.ones(R), float(base.temperature),
                           forced=np.ones(R, np.int32))
    old, new, v = eng.farm_window_wait(R)
    assert np.all(v == V_ACC)
    for r in range(R):
        t, mm = int(tt[r]), int(m[r])
        P = oracles[r]
        com0, off0 = P.get_molecule(t, mm)
        com_d, off_d = eng.get_frames(r, t)
        if move[r] == 1:
            assert np.array_equal(com_d[mm], P.apply_pbc(systems[r].com[t][mm] + (u5[r, :3] - 0.5) * 0.5))
        P.save_fourier(t, mm)
        eo = P.old_energy(t, mm, 0)[:5]
        P.set_molecule(t, mm, com_d[mm], off_d[mm])
        en = P.new_energy(t, mm, 0)[:5]
        A_after = P.amplitude()
        P.set_molecule(t, mm, com0, off0)
        P.restore_fourier(t, mm)
        close(old[r], eo, f"chain {r} old")
        close(new[r], en, f"chain {r} new")
        amp_close(eng.structure_factor(r), A_after, f"chain {r} A after the commit")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the Fortran farm
def _farm(s, R, steps, **kw):
    from maniac_mc_amd.fortran_host import FortranFarm
    farm = FortranFarm(s, R, seed=11, translation_step=0.4, rotation_step=0.4, n_threads=2, triclinic_moves=True, **kw)
    acc = farm.run(steps)
    assert farm.trials + farm.skipped == R * steps and 0 < acc <= farm.trials and acc == farm.accepted
    return farm


def _farm_invariants(farm, R, steps):
    """test_fortran_farm_consistency's: running energies against a from-scratch evaluation, A(k) against a fresh S(k), the
    farm's molecules against the device's"""
    eng = farm.eng
    for r in range(R):
        e = eng.system_energy(r)
        run = farm.energy(r)
        ref = np.array([e[k] for k in ("non_coulomb", "coulomb", "recip_coulomb", "ewald_self", "intra_coulomb")])
        assert np.max(np.abs(run - ref)) < farm_tol(ref, steps), (r, run - ref)
        A = eng.structure_factor(r)
        eng.init_structure_factor(r, True)
        assert np.max(np.abs(A - eng.structure_factor(r))) < 1e-9
    for ia, t in enumerate(farm.active):
        dev = eng.get_molecules(R - 1, int(t))
        for slot in (0, dev.shape[0] - 1):
            com, off = farm.molecule(R - 1, ia, slot)
            assert np.array_equal(dev[slot], com[None, :] + off[:dev.shape[1]])


def _farm_state(farm, R):
    eng = farm.eng
    return ([farm.energy(r).copy() for r in range(R)],
            [[eng.get_molecules(r, int(t)).copy() for t in farm.active] for r in range(R)],
            [eng.structure_factor(r).copy() for r in range(R)])


@pytest.mark.parametrize("name", tc.CELLS)
@pytest.mark.parametrize("gcmc", [False, True], ids=["nvt", "gcmc"])
def test_fortran_farm_modes_in_a_triclinic_box(name, gcmc):
    """host, device, device_accept and window modes from one seed: with the switch the farm really is device-built (no host
    mirror: molecule() reads the frames back), every mode keeps the farm's invariants and tries the same number of moves;
    device mode equals window mode BIT FOR BIT.  Host-built against device-built: the same trial counts; whether the two
    constructions give the same last bits is printed (LABNOTES.md has the finding) -- the device-built one is the one held
    to the oracle bit for bit above."""
    s = tc.cell(name, seed=4)
    R, steps = 6, 60
    kw = {}
    if gcmc:
        V = abs(float(np.linalg.det(s.box_matrix)))
        kw = dict(mol_capacity=_caps(s, 6), gcmc=dict(p_translation=0.25, p_rotation=0.25, fugacity=np.array([14.0, 10.0]) / V))
    states, trials = {}, {}
    for mode, mk in (("host", dict(device_build=False)), ("device", dict(device_build=True)),
                     ("device_accept", dict(device_build=True, device_accept=True)), ("window", dict(device_build=True, window=True))):
        farm = _farm(s, R, steps, **mk, **kw)
        assert farm.device_build == (mode != "host")
        assert farm.window == (mode == "window")
        assert farm.device_accept == (mode == "device_accept")
        _farm_invariants(farm, R, steps)
        states[mode] = _farm_state(farm, R)
        trials[mode] = (farm.trials, farm.skipped, farm.accepted, farm.counts().copy())
        farm.close()
    assert trials["device"][:3] == trials["window"][:3] and np.array_equal(trials["device"][3], trials["window"][3])
    (e_d, x_d, A_d), (e_w, x_w, A_w) = states["device"], states["window"]
    for r in range(R):
        assert np.array_equal(e_d[r], e_w[r]) and np.array_equal(A_d[r], A_w[r]), r
        assert all(np.array_equal(p, q) for p, q in zip(x_d[r], x_w[r])), r
    for mode in ("host", "device_accept"):
        assert trials[mode][0] + trials[mode][1] == trials["device"][0] + trials["device"][1]
    same = trials["host"][:3] == trials["device"][:3] and all(
        np.array_equal(p, q) for r in range(R) for p, q in zip(states["host"][1][r], states["device"][1][r]))
    worst = max((float(np.max(np.abs(p - q))) for r in range(R) for p, q in zip(states["host"][1][r], states["device"][1][r])
                 if p.shape == q.shape), default=0.0)
    print(f"[triclinic farm {name} {'gcmc' if gcmc else 'nvt'}] host-built == device-built bit for bit: {same}; "
          f"max |dx| = {worst:.3e} A; accepted host {trials['host'][2]} device {trials['device'][2]}")


# ---------------------------------------------------------------------------------------------------------------------
# 6. replicas
@pytest.mark.parametrize("mode", ["windows", "device"])
def test_replica_runs_of_a_triclinic_input_in_the_device_modes(mode, tmp_path):
    from tests.test_gpu_replicas import _check_replica_files, _run
    res = _run("spce_triclinic_nvt", tmp_path, replicas=2, seed=3, nb_block=2, nb_step=40, mode=mode)
    assert res["mode"] == mode
    _check_replica_files("spce_triclinic_nvt", str(tmp_path), res, from_scratch=False)
    assert os.path.exists(tmp_path / "replica_0000" / "trajectory.lammpstrj")
