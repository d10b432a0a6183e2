"""Chain runs of grand-canonical blocks (mgpu_chain_run_set_gc / mgpu_chain_run_push_gc, chain_run_kernel<..., GC>): BY-COUNT
records -- residue type, move 0-4, the construction's numbers, the acceptance draw, the draw of PickRandomMoleculeIndex and
phi V -- which every launch completes from the molecule count it finds: slot = min(int(u N), N - 1), prefactor phi V / (N + 1)
of an insertion, N / (phi V) of a deletion, nothing to do (verdict 5) for a move or deletion of an empty type and an insertion
into a full one.  Every comparison is np.array_equal against a twin engine advanced one step at a time by the batched
device-built path (mgpu_move_trial_decide_submit under MGPU_NO_FROZEN_BATCH=1; tests/test_gpu_chain_run.py's twin) with the slot
and the prefactor computed HERE from the twin's counts: rows of all five components, verdicts, coordinates, frames, counts,
A(k).  One case goes to oracle.refcpu directly.
Reference: src/monte_carlo.f90:40-86, src/monte_carlo_utils.f90:184-226, :275-395, src/create_molecule.f90,
src/delete_molecule.f90:100-142."""
import numpy as np
import pytest

from maniac_mc_amd import _lib, synth
from maniac_mc_amd.engine import Engine
from tests.test_gpu_chain_run import (R_STEP, T_STEP, U_ALWAYS, U_NEVER, V_ACC, V_IDLE, V_REJ, V_UND, _collect, _records, _same_state,
                                      _twin_steps)
from tests.test_gpu_farm_window import _twin
from tests.util import tol_for

pytestmark = pytest.mark.gpu

BELOW_ONE = 1.0 - 2.0 ** -40            # a draw of PickRandomMoleculeIndex that picks the last molecule of any count here


def _box(name):
    """(system, active type)"""
    if name == "co2":
        return synth.co2_box(n_mol=20), 0                       # 3 charged sites: self and intra terms
    if name == "argon":
        return synth.argon_box(3, rho_star=0.3), 0              # 1 site
    return synth.framework_water_box(n_water=12, n_frame=300, L=24.0), 1   # the flat pair sweep


# phi V of the insertion and of the deletion records in units of the initial count N0: the bare prefactors are then
# PHI[name][0] N0 / (N + 1) and N / (PHI[name][1] N0).  Dilute CO2 (|dE| << T): both near 1/2, so that about half of each kind
# is accepted.  Argon at rho* = 0.3: insertions of dE / T = -3 .. 1e5, deletions of +2.4: the rule tilted twenty-fold their way.
# The framework box is packed: an insertion's dE / T is 20 or more but for one in ten (measured: 20, 24, 53, 58, 2e2 ... 1e10),
# so phi V is set to accept those of up to ~25 (e^27.6 = 1e12) -- a number chosen for the test's coverage, not for physics -- and
# the records' seed is the one that has such insertions (SEED; seed 5 has none below 34).
PHI = {"co2": (0.5, 2.0), "argon": (20.0, 0.05), "framework": (1e12, 0.05)}
SEED = {"co2": 5, "argon": 5, "framework": 6}


def _caps(s, t_act, cap):
    return [cap if t == t_act else max(1, int(n)) for t, n in enumerate(s.n_mol)]


def _gc_records(rng, s, t_act, n, phi_ins, phi_del, p_move=0.4):
    """n by-count records of the active type: (t, move, u5, accept_u, sel_u, phi_v)"""
    move = np.where(rng.random(n) < p_move, rng.integers(1, 3, n), rng.integers(3, 5, n)).astype(np.int32)
    if int(s.topo.atoms_in_res[t_act]) == 1:
        move[move == 2] = 1
    phi_v = np.where(move == 3, phi_ins, np.where(move == 4, phi_del, 1.0))
    return np.full(n, t_act, np.int32), move, rng.uniform(0, 1, (n, 5)), rng.uniform(0, 1, n), rng.uniform(0, 1, n), phi_v


def _complete(n_now, cap, move, sel_u, phi_v):
    """What a launch makes of a by-count record at count n_now: (live, slot, prefactor) -- mc_farm.f90 select_move's arithmetic"""
    live = move != 0 and (n_now < cap if move == 3 else n_now > 0)
    m = min(int(sel_u * n_now), max(n_now - 1, 0))
    pref = 1.0
    if move == 3:
        pref = phi_v / (n_now + 1.0)
    if move == 4:
        pref = ((n_now - 1.0) + 1.0) / phi_v
    return live, m, pref


def _twin_gc_steps(a, rep, t_act, cap, recs, T, first=0, last=None):
    """The twin, one step at a time, slot and prefactor from ITS count: (old, new, verdict, kinds accepted).  A draw of U_NEVER is
    a forced rejection (tests/test_gpu_chain_run.py _twin_steps): evaluated by the same batched path, nothing committed."""
    t, move, u, au, su, pv = recs
    last = len(move) if last is None else last
    old = np.zeros((last - first, 5)); new = np.zeros((last - first, 5)); v = np.full(last - first, V_IDLE, np.int32)
    for i in range(first, last):
        live, m, pref = _complete(a.num_molecules(rep, t_act), cap, int(move[i]), float(su[i]), float(pv[i]))
        if not live:
            continue
        if au[i] == U_NEVER:
            o, w = a.move_trial([rep], [t[i]], [m], [move[i]], u[i:i + 1], T_STEP, R_STEP)
            acc = [0]
        else:
            o, w, acc = a.move_trial_decide([rep], [t[i]], [m], [move[i]], u[i:i + 1], T_STEP, R_STEP, au[i:i + 1], [pref], T)
        a.synchronize()
        old[i - first], new[i - first], v[i - first] = o[0], w[0], V_ACC if acc[0] else V_REJ
    return old, new, v


def _run(b, rep, k, T, recs, launches=None):
    b.chain_run_open(rep, k, T_STEP, R_STEP, T)
    b.chain_run_push_gc(*recs)
    n = len(recs[1])
    left = n if launches is None else launches
    while left > 0:
        b.chain_run_launch(min(left, 8))
        left -= 8
    out = _collect(b, n)
    b.chain_run_close()
    return out


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("R,rep", [(1, 0), (3, 2)])
@pytest.mark.parametrize("name", ["co2", "argon", "framework"])
def test_a_gc_run_is_the_step_by_step_path(name, R, rep, k):
    """32 random by-count records of moves 0-4 (one idle), every launch queued before anything is collected; phi V of the
    insertions and of the deletions set so that several of each are accepted."""
    s, t_act = _box(name)
    N0 = int(s.n_mol[t_act])
    cap = N0 + 24
    a, b = _twin(s, R, cap=_caps(s, t_act, cap))
    b.chain_run_set_gc(True)
    T = float(s.temperature)
    recs = _gc_records(np.random.default_rng(SEED[name]), s, t_act, 32, phi_ins=PHI[name][0] * N0, phi_del=PHI[name][1] * N0)
    recs[1][7] = 0
    o2, w2, v2 = _run(b, rep, k, T, recs)
    o1, w1, v1 = _twin_gc_steps(a, rep, t_act, cap, recs, T)
    move = recs[1]
    n_ins, n_del = int(((v1 == V_ACC) & (move == 3)).sum()), int(((v1 == V_ACC) & (move == 4)).sum())
    print(f"{name} R={R} k={k}: accepted {int((v1 == V_ACC).sum())} of 32 ({n_ins} insertions of {int((move == 3).sum())}, "
          f"{n_del} deletions of {int((move == 4).sum())}), launches {b.chain_run_launches()}")
    assert np.array_equal(v1, v2), (v1, v2)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))
    assert v2[7] == V_IDLE and not np.any(o2[7]) and not np.any(w2[7])
    assert n_ins >= 2 and n_del >= 2 and int((v2 == V_REJ).sum()) >= 1
    # an insertion carries the self and intra terms in its new row, a deletion in its old row (charged molecules)
    if name != "argon":
        assert np.all(w2[(move == 3) & (v2 != V_IDLE)][:, 3] != 0.0) and np.all(o2[(move == 4) & (v2 != V_IDLE)][:, 3] != 0.0)
        assert not np.any(o2[move == 3][:, [0, 1, 3, 4]]) and not np.any(w2[move == 4][:, [0, 1, 3, 4]])
    _same_state(a, b, s, R)
    assert b.num_molecules(rep, t_act) == N0 + n_ins - n_del
    launches, steps, void, und = b.chain_run_stats()
    assert (launches, steps, und) == (32, 32, 0)
    if k == 4:
        assert max(c for _, c in b.chain_run_launches()) > 1
    a.close(); b.close()


def test_an_insertion_and_a_deletion_against_the_oracle(refcpu_mod):
    """The rows of an accepted insertion and of a deletion of another molecule from the state it leaves, against oracle.refcpu
    (ComputeOldEnergy / ComputeNewEnergy, monte_carlo_utils.f90:275-395) within tol_for; the inserted sites are read back."""
    s = synth.co2_box(n_mol=20)
    N = 20
    (b,) = _twin(s, 1, cap=[N + 8])[:1]
    b.chain_run_set_gc(True)
    T = float(s.temperature)
    rng = np.random.default_rng(9)
    t = np.zeros(2, np.int32); move = np.array([3, 4], np.int32)
    recs = (t, move, rng.uniform(0, 1, (2, 5)), np.array([U_ALWAYS, U_NEVER]), np.array([0.0, 0.3]), np.full(2, 20.0))
    o2, w2, v2 = _run(b, 0, 4, T, recs)
    assert list(v2) == [V_ACC, V_REJ] and b.num_molecules(0, 0) == N + 1
    sites = b.get_molecules(0, 0)[N]
    md = min(int(0.3 * (N + 1)), N)
    P = refcpu_mod.RefCPU(s, mol_capacity=N + 8)
    e_sys = P.system_energy()
    P.init_amplitude(True)
    P.set_energy_recip(e_sys["recip_coulomb"])
    exp_old = np.zeros((2, 5)); exp_new = np.zeros((2, 5))
    exp_old[0] = P.old_energy(0, N, 1)[:5]
    P.set_num_residues(0, N + 1)
    P.save_fourier(0, N)
    P.set_molecule(0, N, sites[0], sites - sites[0][None, :])
    exp_new[0] = P.new_energy(0, N, 1)[:5]
    # the insertion stands: the deletion is a trial of that state
    e_sys = P.system_energy()
    P.init_amplitude(True)
    P.set_energy_recip(e_sys["recip_coulomb"])
    P.all_fourier_terms()
    exp_old[1] = P.old_energy(0, md, 2)[:5]
    P.save_fourier(0, md)
    exp_new[1, 2] = P.recip_singlemol(0, md, 2)                  # intended physics: A - S_mol
    for got, ref, what in ((o2, exp_old, "old"), (w2, exp_new, "new")):
        tol = tol_for(*np.ravel(ref), *np.ravel(got))
        err = float(np.max(np.abs(got - ref)))
        print(f"{what}: |run - oracle| = {err:.3e} K (tol {tol:.3e} K)")
        assert err <= tol, (what, got, ref)
    b.close()


def test_the_count_follows_the_cursor():
    """An accepted insertion ends its launch; the NEXT launch completes a by-count deletion with sel_u just below 1 from the new
    count: it removes slot N, the molecule just inserted, with prefactor (N + 1) / (phi V)."""
    s, t_act = _box("co2")
    N = int(s.n_mol[0])
    a, b = _twin(s, 1, cap=[N + 8])
    b.chain_run_set_gc(True)
    T = float(s.temperature)
    phi_v = 7.0
    rng = np.random.default_rng(3)
    t = np.zeros(3, np.int32); move = np.array([3, 4, 1], np.int32)
    recs = (t, move, rng.uniform(0, 1, (3, 5)), np.array([U_ALWAYS, U_ALWAYS, U_NEVER]), np.array([0.4, BELOW_ONE, 0.4]),
            np.full(3, phi_v))
    before = b.get_molecules(0, 0).copy()
    o2, w2, v2 = _run(b, 0, 4, T, recs, launches=3)
    assert b.chain_run_launches() == [(0, 1), (1, 1), (2, 1)] and list(v2) == [V_ACC, V_ACC, V_REJ]
    # the twin, with the slot and the prefactor written out
    o, w, acc = a.move_trial_decide([0], [0], [0], [3], recs[2][0:1], T_STEP, R_STEP, [U_ALWAYS], [phi_v / (N + 1.0)], T)
    assert acc[0] == 1 and np.array_equal(o[0], o2[0]) and np.array_equal(w[0], w2[0]) and a.num_molecules(0, 0) == N + 1
    inserted = a.get_molecules(0, 0)[N].copy()
    o, w, acc = a.move_trial_decide([0], [0], [N], [4], recs[2][1:2], T_STEP, R_STEP, [U_ALWAYS], [(N + 1.0) / phi_v], T)
    assert acc[0] == 1 and np.array_equal(o[0], o2[1]) and np.array_equal(w[0], w2[1])
    o, w = a.move_trial([0], [0], [int(0.4 * N)], [1], recs[2][2:3], T_STEP, R_STEP)
    assert np.array_equal(o[0], o2[2]) and np.array_equal(w[0], w2[2])
    _same_state(a, b, s, 1)
    assert b.num_molecules(0, 0) == N and np.array_equal(b.get_molecules(0, 0), before) and not np.any(np.all(before == inserted, axis=(1, 2)))
    a.close(); b.close()


@pytest.mark.parametrize("sel_u", [0.0, 0.5, BELOW_ONE])
def test_a_deletion_swaps_with_the_last_molecule(sel_u):
    """m == last (nothing moves) and m != last (the last molecule's coordinates and frame go into slot m)."""
    s, t_act = _box("co2")
    N = int(s.n_mol[0])
    a, b = _twin(s, 1, cap=[N + 8])
    b.chain_run_set_gc(True)
    T = float(s.temperature)
    rng = np.random.default_rng(4)
    recs = (np.zeros(2, np.int32), np.array([4, 2], np.int32), rng.uniform(0, 1, (2, 5)), np.array([U_ALWAYS, U_ALWAYS]),
            np.array([sel_u, sel_u]), np.full(2, 1.0))
    before = b.get_molecules(0, 0).copy()
    o2, w2, v2 = _run(b, 0, 4, T, recs)
    m = min(int(sel_u * N), N - 1)
    assert (m == N - 1) == (sel_u == BELOW_ONE)
    o1, w1, v1 = _twin_gc_steps(a, 0, 0, N + 8, recs, T)
    assert list(v2) == [V_ACC, V_ACC] and np.array_equal(v1, v2) and np.array_equal(o1, o2) and np.array_equal(w1, w2)
    _same_state(a, b, s, 1)
    after = b.get_molecules(0, 0)
    assert after.shape[0] == N - 1
    if m != N - 1:
        keep = np.arange(N - 1) != min(int(sel_u * (N - 1)), N - 2)   # (the rotation that follows moved one molecule)
        expect = before[:N - 1].copy(); expect[m] = before[N - 1]
        assert np.array_equal(after[keep], expect[keep])
    a.close(); b.close()


def test_the_edges_of_the_count():
    """A type brought down to 0: by-count moves and deletions do nothing (verdict 5, state unchanged); an insertion into the
    empty type is the farm window's for the same record, bit for bit; a type at capacity: an insertion does nothing."""
    s = synth.co2_box(n_mol=2)
    cap = 3
    a, b = _twin(s, 1, cap=[cap])
    b.chain_run_set_gc(True)
    T = float(s.temperature)
    rng = np.random.default_rng(6)
    #        N: 2  1  0  0  0  0->1 1->2 2->3  3   3
    move = np.array([4, 4, 1, 2, 4, 3, 3, 3, 3, 1], np.int32)
    au = np.array([U_ALWAYS, U_ALWAYS, U_ALWAYS, U_ALWAYS, U_ALWAYS, U_ALWAYS, U_ALWAYS, U_ALWAYS, U_ALWAYS, U_NEVER])
    n = len(move)
    recs = (np.zeros(n, np.int32), move, rng.uniform(0, 1, (n, 5)), au, rng.uniform(0, 1, n), np.full(n, 3.0))
    head = tuple(x[:5] for x in recs)
    tail = tuple(x[5:] for x in recs)
    b.chain_run_open(0, 4, T_STEP, R_STEP, T)
    b.chain_run_push_gc(*head)
    b.chain_run_launch(3)
    # the farm window of the same records on the twin, one step at a time, by count
    rows = []
    counts = []
    for i in range(n):
        counts.append(a.num_molecules(0, 0))
        a.farm_window_submit([0], [0], [0], [move[i]], recs[2][i:i + 1], T_STEP, R_STEP, au[i:i + 1], recs[5][i:i + 1], T,
                             slot_u=recs[4][i:i + 1])
        rows.append(a.farm_window_wait(1))
        if i == 4:
            a.farm_window_flush()
            empty = a.structure_factor(0).copy()
    a.farm_window_flush()
    o1, w1, v1 = (np.concatenate(x) for x in zip(*rows))
    assert counts == [2, 1, 0, 0, 0, 0, 1, 2, 3, 3]
    assert list(v1) == [V_ACC, V_ACC, V_IDLE, V_IDLE, V_IDLE, V_ACC, V_ACC, V_ACC, V_IDLE, V_REJ]
    o2, w2, v2 = _collect(b, 5)
    assert b.chain_run_launches() == [(0, 1), (1, 1), (2, 3)]
    # the empty type: count 0, and the moves and the deletion behind it changed nothing
    assert b.num_molecules(0, 0) == 0 and b.get_molecules(0, 0).shape[0] == 0 and np.array_equal(b.structure_factor(0), empty)
    b.chain_run_push_gc(*tail)
    b.chain_run_launch(n - 5)
    o3, w3, v3 = _collect(b, n - 5)
    b.chain_run_close()
    o2, w2, v2 = np.concatenate([o2, o3]), np.concatenate([w2, w3]), np.concatenate([v2, v3])
    assert np.array_equal(v1, v2), (v1, v2)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2)
    assert not np.any(o2[v2 == V_IDLE]) and not np.any(w2[v2 == V_IDLE])
    _same_state(a, b, s, 1)
    assert b.num_molecules(0, 0) == cap
    a.close(); b.close()


@pytest.mark.parametrize("accept", [True, False])
@pytest.mark.parametrize("kind", [3, 4])
def test_an_undecided_insertion_or_deletion_stalls_the_run_until_it_is_forced(kind, accept):
    """tests/test_gpu_chain_run.py's construction for an insertion and a deletion: phi V puts the step's probability at 0.5
    (from the twin's energies of the initial state), its draw ON the probability, the margin opened to 1e-2.  The step comes
    back undecided, the launches queued behind it are void, nothing is committed; force accept / reject both end in the
    twin's state."""
    s, t_act = _box("co2")
    N = int(s.n_mol[0])
    cap = N + 8
    a, b = _twin(s, 1, cap=[cap])
    b.chain_run_set_gc(True)
    T = float(s.temperature)
    rng = np.random.default_rng(17)
    n, st = 6, 2
    t = np.zeros(n, np.int32)
    move = np.array([1, 2, kind, 1, 3, 4], np.int32)
    u = rng.uniform(0, 1, (n, 5)); su = rng.uniform(0, 1, n)
    au = np.full(n, U_NEVER)
    # steps 0 .. st are trials of the initial state (the ones before st are rejected): the twin's batched path gives st's energies
    m_st = min(int(su[st] * N), N - 1)
    o, w = a.move_trial([0], [0], [m_st], [kind], u[st:st + 1], T_STEP, R_STEP)
    d_e = float(w[0].sum() - o[0].sum())
    assert np.isfinite(d_e) and abs(d_e / T) < 500.0
    bare = (1.0 / (N + 1.0)) if kind == 3 else float(N)
    phi_v = np.ones(n)
    phi_v[st] = 0.5 * np.exp(d_e / T) / bare if kind == 3 else bare * np.exp(-d_e / T) / 0.5
    phi_v[4] = 20.0 * N; phi_v[5] = N / 20.0
    pref = phi_v[st] / (N + 1.0) if kind == 3 else ((N - 1.0) + 1.0) / phi_v[st]
    x = pref * np.exp(-d_e / T)
    assert 0.49 < x < 0.51
    au[st] = x
    au[st + 1] = U_ALWAYS
    au[4:] = rng.uniform(0, 1, 2)
    recs = (t, move, u, au, su, phi_v)
    b.chain_set_margin(1e-2)
    b.chain_run_open(0, 4, T_STEP, R_STEP, T)
    b.chain_run_push_gc(*recs)
    b.chain_run_launch(5)
    rows = []
    while True:
        o2, w2, v2, stalled_at = b.chain_run_collect(n, wait=True)
        rows.append((o2, w2, v2))
        if stalled_at >= 0:
            break
    o2, w2, v2 = (np.concatenate(x_) for x_ in zip(*rows))
    assert stalled_at == st and list(v2) == [V_REJ, V_REJ, V_UND]
    assert np.array_equal(o2[st], o[0]) and np.array_equal(w2[st], w[0])
    b.synchronize()
    tags = b.chain_run_launches()
    assert tags[0] == (0, st) and tags[1:] == [(st, 0)] * 4      # the launches queued behind it: void
    assert b.chain_run_collect(n, wait=False)[3] == st
    _same_state(a, b, s, 1)                                     # nothing committed
    with pytest.raises(_lib.MgpuError):
        b.chain_run_close()
    b.chain_run_force(st, accept)
    b.chain_run_launch(n)
    o3, w3, v3 = _collect(b, n - st)
    b.chain_run_close()
    au1 = au.copy()
    au1[st] = U_ALWAYS if accept else U_NEVER
    o1, w1, v1 = _twin_gc_steps(a, 0, 0, cap, (t, move, u, au1, su, phi_v), T, first=st)
    assert v3[0] == (V_ACC if accept else V_REJ) and v3[1] == V_ACC
    assert np.array_equal(v1, v3) and np.array_equal(o1, o3) and np.array_equal(w1, w3)
    assert np.array_equal(o3[0], o[0]) and np.array_equal(w3[0], w[0])
    _same_state(a, b, s, 1)
    assert b.num_molecules(0, 0) == a.num_molecules(0, 0)
    a.close(); b.close()


def _refused(code):
    with pytest.raises(_lib.MgpuError) as ei:
        code()
    return str(ei.value)


def test_the_switch():
    """Off by default: push_gc is refused and push refuses moves 3 / 4 with the text it always had -- switch on or off.  set_gc is
    refused for a triclinic box, with a reservoir and while a run is open; the run stays usable.  With the switch on an NVT run
    through plain push is the run with the switch off."""
    s, t_act = _box("co2")
    N = int(s.n_mol[0])
    T = float(s.temperature)
    a, b = _twin(s, 1, cap=[N + 8])
    c, = _twin(s, 1, cap=[N + 8])[:1]
    rng = np.random.default_rng(31)
    gc = _gc_records(rng, s, 0, 4, 20.0 * N, N / 20.0)
    nvt = _records(np.random.default_rng(32), s, 0, 12)
    text = "chain_run_push: insertions and deletions do not ride in a run (moves only)"
    for on in (False, True):
        if on:
            b.chain_run_set_gc(True)
        b.chain_run_open(0, 4, T_STEP, R_STEP, T)
        if not on:
            assert "chain_run_push_gc" in _refused(lambda: b.chain_run_push_gc(*gc))
        for mv in (3, 4):
            t, m, move, u, au = _records(rng, s, 0, 3)
            move[1] = mv
            assert text in _refused(lambda: b.chain_run_push(t, m, move, u, au))
        assert "a run is open" in _refused(lambda: b.chain_run_set_gc(not on))
        if on:
            bad = list(gc); bad[4] = np.array([0.1, 1.0, 0.2, 0.3])          # sel_u outside [0, 1)
            _refused(lambda: b.chain_run_push_gc(*bad))
            bad = list(gc); bad[1] = np.array([1, 5, 3, 4], np.int32)
            _refused(lambda: b.chain_run_push_gc(*bad))
        # none of them left anything behind
        b.chain_run_push(*nvt)
        b.chain_run_launch(12)
        o2, w2, v2 = _collect(b, 12)
        b.chain_run_close()
        if not on:
            first = (o2, w2, v2)
            o1, w1, v1 = _twin_steps(a, 0, nvt, T)
            assert np.array_equal(v1, v2) and np.array_equal(o1, o2) and np.array_equal(w1, w2) and (v2 == V_ACC).sum() > 0
            _same_state(a, b, s, 1)
    # the same NVT records, switch on from the start (engine c), against the switch-off run of engine b's first block
    c.chain_run_set_gc(True)
    c.chain_run_open(0, 4, T_STEP, R_STEP, T)
    c.chain_run_push(*nvt)
    c.chain_run_launch(12)
    o3, w3, v3 = _collect(c, 12)
    c.chain_run_close()
    assert np.array_equal(first[2], v3) and np.array_equal(first[0], o3) and np.array_equal(first[1], w3)
    c.chain_run_set_gc(False)
    c.chain_run_open(0, 4, T_STEP, R_STEP, T)
    assert "chain_run_push_gc" in _refused(lambda: c.chain_run_push_gc(*gc))
    c.chain_run_close()
    for e in (a, b, c):
        e.close()
    # a reservoir
    e = Engine.from_system(s, n_replicas=1, mol_capacity=[N + 8])
    e.set_frames(0, 0, s.com[0], s.offsets[0])
    e.set_reservoir(0, 0, s.offsets[0][:4])
    assert "reservoir" in _refused(lambda: e.chain_run_set_gc(True))
    e.close()
    # triclinic boxes, with and without device-built moves
    from tests import triclinic_cases as tc
    tri = tc.cell("mild")
    caps = [int(n) + 3 for n in tri.n_mol]
    for moves in (False, True):
        e = Engine.from_system(tri, n_replicas=1, mol_capacity=caps, triclinic_moves=moves)
        assert "triclinic" in _refused(lambda: e.chain_run_set_gc(True))
        e.close()
