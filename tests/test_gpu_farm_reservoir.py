"""Reservoirs of device-built steps (mgpu_replica_set_reservoir / _get_reservoir; include/maniac_gpu.h): an insertion copies
reservoir[min(int(u[3] n_r), n_r - 1)] unrotated and takes it out of the reservoir (swap with the last), an accepted deletion
puts the box's last molecule of the type into it, rejected steps leave it alone, an empty reservoir inserts nothing.  Held to
the oracle, to the batched path bit for bit (farm windows, narrow and WIDE, caller-picked and by count), and to the farm's
invariants.  Reference: src/create_molecule.f90:117-128, :185-193; src/delete_molecule.f90:146-166."""
import os
from fractions import Fraction

import numpy as np
import pytest

from maniac_mc_amd import io_maniac, synth
from maniac_mc_amd._lib import MGPU_CREATION, MGPU_DELETION, MgpuError
from maniac_mc_amd.engine import Engine
from tests.test_gpu_parity import amp_close, close

pytestmark = pytest.mark.gpu

V_REJ, V_ACC, V_IDLE = 0, 1, 5
FIXTURE = os.path.join(os.path.dirname(__file__), "golden", "runs", "dumbbell_gcmc_reservoir", "inputs")


def _rotations(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], 1)


def _bent(tmpl):
    """the same molecule with its last site turned about the first by 0.35 rad in the plane of the first three: another
    intra-Coulomb energy"""
    t = tmpl.copy()
    a, b = t[1] - t[0], t[-1] - t[0]
    nrm = np.cross(a, b)
    nrm = nrm / np.linalg.norm(nrm) if np.linalg.norm(nrm) > 0 else np.array([0.0, 0.0, 1.0])
    th = 0.35
    t[-1] = t[0] + b * np.cos(th) + np.cross(nrm, b) * np.sin(th) + nrm * np.dot(nrm, b) * (1 - np.cos(th))
    return t - t.mean(0)


def _reservoir(rng, conformers, n):
    """n random rotations of the conformers, taken in turn"""
    rot = _rotations(rng, n)
    return np.stack([conformers[i % len(conformers)] @ rot[i].T for i in range(n)])


def _engines(s, R, cap, n=1):
    out = []
    for _ in range(n):
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


def _fma(a, b, c):
    return float(Fraction(a) + Fraction(b) * Fraction(c))


def _centre_is(got, lo, L, u):
    """lo + L u as the device forms it (a product and a sum, or one fused multiply-add)"""
    return all(got[d] == lo[d] + L[d] * u[d] or got[d] == _fma(lo[d], L[d], u[d]) for d in range(3))


def _dists(off):
    i, j = np.triu_indices(off.shape[0], 1)
    return np.linalg.norm(off[i] - off[j], axis=1)


@pytest.mark.parametrize("case", ["spce", "cage24"])
def test_batched_reservoir_step_bookkeeping_and_oracle(refcpu_mod, case):
    """One insertion (replica 0) and one deletion (replica 1) through mgpu_move_trial_submit: energies against the oracle;
    committed from the resident rows: the inserted frame is lo + L u plus reservoir[pick] bit for bit, the reservoir shows the
    swap-with-last, the deletion appends the LAST slot's offsets; a trial left uncommitted changes nothing."""
    rng = np.random.default_rng(3)
    s = synth.spce_box(5, seed=4) if case == "spce" else synth.rigid_adsorbate_box(n_mol=6, n_sites=24, L=26.0)
    N = int(s.n_mol[0])
    md = 7 if case == "spce" else 2                               # the molecule the deletions remove
    eng, = _engines(s, 2, [N + 20])
    tmpl = s.offsets[0][0]
    res = _reservoir(rng, [tmpl, _bent(tmpl)], 6)
    eng.set_reservoir(0, 0, res)
    eng.set_reservoir(1, 0, res)
    assert np.array_equal(eng.get_reservoir(0, 0), res) and np.array_equal(eng.get_reservoir(1, 0), res)
    L, lo = np.diag(s.box_matrix), s.bounds_lo
    for trial in range(2):
        u = rng.uniform(0, 1, (2, 5))
        u[0, 3] = 0.2 if trial == 0 else 0.99          # picks 1 (swapped with the last) and 5 (the last itself)
        m = np.array([0, md], np.int32)
        move = np.array([3, 4], np.int32)
        rep = np.array([0, 1], np.int32)
        tt = np.zeros(2, np.int32)
        before = [eng.get_reservoir(r, 0) for r in range(2)]
        com_last, off_last = eng.get_frames(1, 0)
        n0, n1 = eng.num_molecules(0, 0), eng.num_molecules(1, 0)
        old, new = eng.move_trial(rep, tt, m, move, u, 0.4, 0.4)
        nr = before[0].shape[0]
        pick = min(int(u[0, 3] * nr), nr - 1)
        if trial == 0:
            # oracle: the inserted molecule is reservoir[pick] at lo + L u; the deletion of molecule 7 (replica 1 = replica 0)
            P = refcpu_mod.RefCPU(s, mol_capacity=N + 20)
            e_sys = P.system_energy()
            P.init_amplitude(True)
            P.set_energy_recip(e_sys["recip_coulomb"])
            A0 = P.amplitude()
            com_new = lo + L * u[0, :3]
            exp_old = P.old_energy(0, N, 1)[:5]
            P.set_num_residues(0, N + 1)
            P.save_fourier(0, N)
            P.set_molecule(0, N, com_new, before[0][pick])
            exp_new = P.new_energy(0, N, 1)[:5]
            P.set_num_residues(0, N)
            P.set_amplitude(A0)
            close(old[0], exp_old, "insertion old")
            close(new[0], exp_new, "insertion new")
            P.all_fourier_terms()
            exp_old = P.old_energy(0, md, 2)[:5]
            P.save_fourier(0, md)
            exp_new_d = P.recip_singlemol(0, md, 2)
            P.set_amplitude(A0)
            close(old[1], exp_old, "deletion old")
            close(new[1, 2], exp_new_d, "deletion new recip")
            P.close()
            # an uncommitted trial leaves the reservoirs alone
            assert all(np.array_equal(eng.get_reservoir(r, 0), before[r]) for r in range(2))
            old, new = eng.move_trial(rep, tt, m, move, u, 0.4, 0.4)
        eng.commit_lane(0, rep, tt, m, np.array([MGPU_CREATION, MGPU_DELETION], np.int32), np.ones(2, np.int32))
        com0, off0 = eng.get_frames(0, 0)
        assert eng.num_molecules(0, 0) == n0 + 1 and eng.num_molecules(1, 0) == n1 - 1
        assert _centre_is(com0[n0], lo, L, u[0]) and np.array_equal(off0[n0], before[0][pick])
        assert np.array_equal(eng.get_molecules(0, 0)[n0], com0[n0][None, :] + off0[n0])
        exp0 = before[0].copy()
        exp0[pick] = before[0][nr - 1]
        assert np.array_equal(eng.get_reservoir(0, 0), exp0[: nr - 1])
        assert np.array_equal(eng.get_reservoir(1, 0), np.concatenate([before[1], off_last[n1 - 1][None]]))
        for r in range(2):
            A = eng.structure_factor(r)
            eng.init_structure_factor(r, True)
            amp_close(A, eng.structure_factor(r), f"replica {r}")
    eng.close()


def _gcmc_case(kind):
    rng = np.random.default_rng(11)
    if kind == "narrow":
        s = synth.spce_box(4, seed=8, spacing=6.0)          # dilute: insertions and deletions both accepted
        conf = [s.offsets[0][0], _bent(s.offsets[0][0])]
    else:
        s = synth.rigid_adsorbate_box(n_mol=6, n_sites=24, L=26.0)
        t0 = s.offsets[0][0] @ _rotations(rng, 1)[0].T
        conf = [t0, _bent(t0)]
    return s, conf, rng


def _rule(o, w, pref, au, T):
    """mc_acceptance_probability as the drivers form it (components added in order)"""
    e_old = e_new = 0.0
    for k in range(5):
        e_old = e_old + float(o[k])
        e_new = e_new + float(w[k])
    x = pref * np.exp(-(e_new - e_old) / T)
    return 1 if au <= min(1.0, x) else 0


@pytest.mark.parametrize("kind", ["narrow", "wide"])
def test_windows_are_the_batched_path_with_reservoirs(kind):
    """GCMC windows with reservoirs -- caller-picked records, then by-count records -- against the batched device-built path
    (mgpu_move_trial_submit, the host's rule, mgpu_commit_submit from the resident rows) on a twin engine: energies, verdicts,
    committed state and reservoirs bit for bit, step after step."""
    s, conf, rng = _gcmc_case(kind)
    R = 6
    N = int(s.n_mol[0])
    a, b = _engines(s, R, [N + 30], n=2)
    assert b.farm_window_capacity()[0] >= R
    for r in range(R):
        res = _reservoir(rng, conf, 24)
        a.set_reservoir(r, 0, res)
        b.set_reservoir(r, 0, res)
    T = float(s.temperature)
    V = float(np.linalg.det(s.box_matrix))
    phiV = float(N)
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    seen = set()
    for step in range(16):
        by_count = step >= 8
        n_now = np.array([b.num_molecules(r, 0) for r in range(R)])
        move = rng.integers(1, 5, R).astype(np.int32)
        move[(n_now <= 1) & (move == 4)] = 3
        sel = rng.uniform(0, 1, R)
        m = np.minimum((sel * n_now).astype(np.int32), n_now - 1).astype(np.int32)
        u = rng.uniform(0, 1, (R, 5))
        au = rng.uniform(0, 1, R) ** 3
        pref = np.ones(R)
        pref[move == 3] = phiV / (n_now[move == 3] + 1.0)
        pref[move == 4] = n_now[move == 4] / phiV
        if by_count:
            bp = np.ones(R)
            bp[move >= 3] = phiV
            b.farm_window_submit(rep, tt, np.zeros(R, np.int32), move, u, 0.5, 0.5, au, bp, T, slot_u=sel)
        else:
            b.farm_window_submit(rep, tt, m, move, u, 0.5, 0.5, au, pref, T)
        o2, w2, v = b.farm_window_wait(R)
        o1, w1 = a.move_trial(rep, tt, m, move, u, 0.5, 0.5)
        acc = np.array([_rule(o1[c], w1[c], pref[c], au[c], T) for c in range(R)], np.int32)
        kinds = np.where(move <= 2, 0, np.where(move == 3, MGPU_CREATION, MGPU_DELETION)).astype(np.int32)
        a.commit_lane(0, rep, tt, m, kinds, acc)
        assert np.array_equal(o1, o2) and np.array_equal(w1, w2), step
        assert np.array_equal(v == V_ACC, acc != 0) and np.all((v == V_ACC) | (v == V_REJ)), (step, v, acc)
        seen.update((int(mv), int(vv)) for mv, vv in zip(move, v))
        for r in range(R):
            assert a.num_molecules(r, 0) == b.num_molecules(r, 0)
            assert np.array_equal(a.get_reservoir(r, 0), b.get_reservoir(r, 0)), (step, r)
            ca, oa = a.get_frames(r, 0)
            cb, ob = b.get_frames(r, 0)
            assert np.array_equal(ca, cb) and np.array_equal(oa, ob), (step, r)
            assert np.array_equal(a.get_molecules(r, 0), b.get_molecules(r, 0)), (step, r)
            assert np.array_equal(a.structure_factor(r), b.structure_factor(r)), (step, r)
            assert a.num_molecules(r, 0) + a.get_reservoir(r, 0).shape[0] == N + 24
    assert (3, V_ACC) in seen and (4, V_ACC) in seen
    a.close(); b.close()


def _fixture_system():
    sm, inp = io_maniac.load_system(os.path.join(FIXTURE, "system.maniac"), os.path.join(FIXTURE, "system.data"),
                                    os.path.join(FIXTURE, "system.inc"))
    res = io_maniac.reservoir_offsets(os.path.join(FIXTURE, "reservoir.data"), inp)
    return sm, res


@pytest.mark.parametrize("case", ["spce", "fixture"])
def test_window_farm_invariants_with_reservoirs(case):
    """A farm of by-count GCMC windows with reservoirs (SPC/E with two bent conformers; the dumbbell_gcmc_reservoir run
    fixture's system and reservoir file): the running energies are the from-scratch system energy, A(k) a fresh S(k), box
    count + reservoir count conserved, every box molecule one of the conformers it could have come from."""
    rng = np.random.default_rng(19)
    if case == "spce":
        s = synth.spce_box(4, seed=2, spacing=6.0)             # dilute: insertions and deletions both accepted
        R = 4
        res = {r: _reservoir(rng, [s.offsets[0][0], _bent(s.offsets[0][0])], 16) for r in range(R)}
    else:
        s, rf = _fixture_system()
        R = 4
        res = {r: rf[0] for r in range(R)}
    N = int(s.n_mol[0])
    eng, = _engines(s, R, [N + 60])
    for r in range(R):
        eng.set_reservoir(r, 0, res[r])
    total = {r: N + res[r].shape[0] for r in range(R)}
    known = [_dists(o) for r in range(R) for o in np.concatenate([s.offsets[0], res[r]])]
    run = [eng.system_energy(r)["total"] for r in range(R)]
    T = float(s.temperature)
    phiV = float(N)
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    seen = set()
    for step in range(40):
        move = rng.integers(1, 5, R).astype(np.int32)
        bp = np.where(move >= 3, phiV, 1.0)
        eng.farm_window_submit(rep, tt, np.zeros(R, np.int32), move, rng.uniform(0, 1, (R, 5)), 0.5, 0.5, rng.uniform(0, 1, R),
                               bp, T, slot_u=rng.uniform(0, 1, R))
        o, w, v = eng.farm_window_wait(R)
        assert np.all((v == V_ACC) | (v == V_REJ) | (v == V_IDLE))
        seen.update(int(mv) for mv, vv in zip(move, v) if vv == V_ACC)
        for r in range(R):
            if v[r] == V_ACC:
                run[r] += float(np.sum(w[r]) - np.sum(o[r]))
    assert {3, 4} <= seen, seen                              # the reservoir did take part
    for r in range(R):
        nb = eng.num_molecules(r, 0)
        rsv = eng.get_reservoir(r, 0)
        assert nb + rsv.shape[0] == total[r]
        e = eng.system_energy(r)["total"]
        assert abs(run[r] - e) <= 1e-9 * max(1.0, abs(e)), (r, run[r], e)
        A = eng.structure_factor(r)
        eng.init_structure_factor(r, True)
        amp_close(A, eng.structure_factor(r), f"replica {r}")
        _, off = eng.get_frames(r, 0)
        for o in list(off) + list(rsv):
            d = _dists(o)
            assert min(np.max(np.abs(d - k)) for k in known) <= 1e-10
    eng.close()


def test_reservoir_edges():
    """Empty reservoir: verdict 5 in a window, rejected by the device-decided path, N never above the total.  replica_copy
    copies reservoirs (and removes them where the source has none).  A type that never held a molecule takes insertions from
    its reservoir.  Refusals: a bad type, n > cap, windows of the replica in flight."""
    rng = np.random.default_rng(7)
    s = synth.spce_box(4, seed=5)
    N = int(s.n_mol[0])
    eng, = _engines(s, 3, [N + 10])
    T = float(s.temperature)
    res = _reservoir(rng, [s.offsets[0][0]], 2)
    with pytest.raises(MgpuError):
        eng.set_reservoir(0, 3, res)
    with pytest.raises(MgpuError):
        eng.set_reservoir(0, 0, res, cap=1)
    eng.set_reservoir(0, 0, res)
    eng.replica_copy(1, 0)
    assert np.array_equal(eng.get_reservoir(1, 0), res)
    # forced insertions on replica 0: two from the reservoir, then nothing
    verdicts = []
    for _ in range(4):
        eng.farm_window_submit([0], [0], [0], [3], rng.uniform(0, 1, (1, 5)), 0.5, 0.5, [0.5], [1.0], T, forced=[1])
        verdicts.append(int(eng.farm_window_wait(1)[2][0]))
    assert verdicts == [V_ACC, V_ACC, V_IDLE, V_IDLE]
    assert eng.num_molecules(0, 0) == N + 2 and eng.get_reservoir(0, 0).shape[0] == 0
    # the device-decided path: one insertion from replica 1's reservoir of two, then rejections
    accs = []
    for _ in range(3):
        _, _, acc = eng.move_trial_decide([1], [0], [0], [3], rng.uniform(0, 1, (1, 5)), 0.5, 0.5, [0.0], [1e300], T)
        eng.synchronize()
        accs.append(int(acc[0]))
    assert accs == [1, 1, 0] and eng.num_molecules(1, 0) == N + 2
    # copies: replica 2 (no reservoir) over replica 1 removes its reservoir; replica 1 over 2 gives it one
    eng.set_reservoir(1, 0, res[:1])
    eng.replica_copy(2, 1)
    assert np.array_equal(eng.get_reservoir(2, 0), res[:1])
    eng.set_reservoir(2, 0, np.zeros((0, 3, 3)))
    eng.replica_copy(1, 2)
    assert eng.get_reservoir(1, 0).shape[0] == 0
    # in flight: refused
    eng.farm_window_submit([2], [0], [1], [1], rng.uniform(0, 1, (1, 5)), 0.5, 0.5, [0.5], [1.0], T)
    with pytest.raises(MgpuError):
        eng.set_reservoir(2, 0, res)
    eng.farm_window_wait(1)
    eng.close()
    # a type that never held a molecule: refused without a reservoir, inserted from it with one
    e2 = Engine.from_system(s, n_replicas=1, mol_capacity=[N + 10])
    e2.set_frames(0, 0, np.zeros((0, 3)), np.zeros((0, 3, 3)))
    e2.init_structure_factor(0, True)
    with pytest.raises(MgpuError):
        e2.farm_window_submit([0], [0], [0], [3], rng.uniform(0, 1, (1, 5)), 0.5, 0.5, [0.5], [1.0], T, forced=[1])
    e2.set_reservoir(0, 0, res)
    u = rng.uniform(0, 1, (1, 5))
    e2.farm_window_submit([0], [0], [0], [3], u, 0.5, 0.5, [0.5], [1.0], T, forced=[1])
    assert int(e2.farm_window_wait(1)[2][0]) == V_ACC
    _, off = e2.get_frames(0, 0)
    assert off.shape[0] == 1 and np.array_equal(off[0], res[min(int(u[0, 3] * 2), 1)])
    e2.close()


def test_ideal_gas_limit_with_a_reservoir():
    """Uncharged, non-interacting molecules (every epsilon and charge zero): with a reservoir, by-count windows with
    prefactors phi V / (N + 1) and N / (phi V) sample <N> = phi V (the reservoir only supplies geometries)."""
    s = synth.spce_box(3, seed=1)
    s.topo.charges[:] = 0.0
    s.topo.epsilon[:] = 0.0
    R = 16
    phiV = 6.0
    eng, = _engines(s, R, [60])
    rng = np.random.default_rng(23)
    for r in range(R):
        eng.set_reservoir(r, 0, _reservoir(rng, [s.offsets[0][0]], 40))
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    samples = []
    for step in range(600):
        move = np.where(rng.uniform(0, 1, R) < 0.5, 3, 4).astype(np.int32)
        eng.farm_window_submit(rep, tt, np.zeros(R, np.int32), move, rng.uniform(0, 1, (R, 5)), 0.5, 0.5, rng.uniform(0, 1, R),
                               np.full(R, phiV), float(s.temperature), slot_u=rng.uniform(0, 1, R))
        eng.farm_window_wait(R)
        if step >= 200 and step % 4 == 0:
            samples.append([eng.num_molecules(r, 0) for r in range(R)])
    mean = float(np.mean(samples))
    assert abs(mean - phiV) < 0.6, mean
    for r in range(R):
        assert eng.num_molecules(r, 0) + eng.get_reservoir(r, 0).shape[0] == int(s.n_mol[0]) + 40
    eng.close()
