"""Chain runs of grand-canonical blocks in TRICLINIC cells (mgpu_chain_run_set_gc on an engine whose triclinic runs are on,
chain_run_kernel<false, false, true, true>): by-count records -- residue type, move 0-4, the construction's numbers, the
acceptance draw, the draw of PickRandomMoleculeIndex and phi V -- which every launch completes from the count it finds, built
with the triclinic form of the centre (an insertion at lo + box%matrix u, a translation through ApplyPBC) and swept with
ComputeDistance's image search.  Every comparison is np.array_equal against a twin engine advanced one step at a time by the
batched device-built path (move_trial_decide, move_trial for the forced rejections), which tests/test_gpu_triclinic_moves.py
holds to the oracle, insertions and deletions included, with the slot and the prefactor computed HERE from the twin's counts:
old and new rows of all five components, verdicts, coordinates, frames, counts, A(k).  One case goes to oracle.refcpu directly.
The cells are tests/triclinic_cases.py's: two-type mixtures of a 3-site molecule (one site uncharged) and a 2-site one; the
capacities are count + 24.
Reference: src/monte_carlo.f90:40-86, src/monte_carlo_utils.f90:184-226, :275-395, src/create_molecule.f90:180-200,
src/delete_molecule.f90:100-142, src/geometry_utils.f90:167-220, :397-411."""
import numpy as np
import pytest

from maniac_mc_amd import _lib
from maniac_mc_amd.engine import Engine
from tests import triclinic_cases as tc
from tests.test_gpu_chain_run import R_STEP, T_STEP, U_ALWAYS, U_NEVER, V_ACC, V_IDLE, V_REJ, V_UND, _collect
from tests.test_gpu_chain_run_gcmc import BELOW_ONE, _complete, _run
from tests.test_gpu_chain_run_triclinic import _records as _nvt_records
from tests.test_gpu_triclinic_moves import _engine, _same_state
from tests.util import tol_for

pytestmark = pytest.mark.gpu

MGPU_ERR_STATE = 5
# phi V of the insertion and of the deletion records in units of the record's type's initial count N0: the bare prefactors are
# then PHI[0] N0 / (N + 1) and N / (PHI[1] N0), both near 1/2 -- the cells are dilute (|dE| << T away from an overlap), so about
# half of each kind is accepted.
PHI = (0.5, 2.0)
# Seeds of the record sets, chosen on the CPU by stepping the same records with oracle.refcpu (each step's dE as the difference
# of ComputeSystemEnergy's totals after and before the change, the rule x = prefactor exp(-dE / T), u <= min(1, x), the slot and
# the prefactor from the stepped counts, a launch of k = 4 ending behind its first accepted step); every test asserts on the
# twin what its seed was chosen for.
#   SEED_RUN    of the 32 records: at least 2 accepted insertions, 2 accepted deletions, a rejection, a launch of more than one
#               step at k = 4, and no draw within 1e-3 (relative) of its probability -- the device's margin is 16 ulp
#   SEED_EDGE   the numbers beside the fractions of the inserted centres (angle, axis; the rotation's) with which no insertion,
#               rotation or deletion accepted by fiat costs more than 8 T (a step accepted by fiat whose probability underflows
#               to 0 is undecided)
#   SEED_STALL  step 2's insertion / deletion of the initial state has |dE / T| < 500, and steps 4 and 5 are not within the
#               opened margin
SEED_RUN = {"mild": 1, "sheared": 1}
SEED_EDGE = 1
SEED_STALL = 17


def _caps(s):
    return [int(n) + 24 for n in s.n_mol]


def _twin(s, R):
    """(a, b): two engines holding R copies of `s` with resident frames and device-built triclinic moves; b takes triclinic
    runs and grand-canonical ones."""
    a, b = _engine(s, R, _caps(s)), _engine(s, R, _caps(s))
    b.chain_run_set_triclinic(True)
    b.chain_run_set_gc(True)
    return a, b


def _gc_records(rng, s, n, phi_ins=PHI[0], phi_del=PHI[1], p_move=0.4):
    """n by-count records over both residue types: (t, move, u5, accept_u, sel_u, phi_v)"""
    t = rng.integers(0, s.topo.n_res, n).astype(np.int32)
    move = np.where(rng.random(n) < p_move, rng.integers(1, 3, n), rng.integers(3, 5, n)).astype(np.int32)
    n0 = np.asarray(s.n_mol, dtype=np.float64)[t]
    phi_v = np.where(move == 3, phi_ins * n0, np.where(move == 4, phi_del * n0, 1.0))
    return t, move, rng.uniform(0, 1, (n, 5)), rng.uniform(0, 1, n), rng.uniform(0, 1, n), phi_v


def _twin_steps(a, rep, caps, recs, T, first=0, last=None):
    """The twin, one step at a time, slot and prefactor from ITS count of the record's type: (old, new, verdict).  A draw of
    U_NEVER is a forced rejection (tests/test_gpu_chain_run.py _twin_steps): the same batched path, nothing committed."""
    t, move, u, au, su, pv = recs
    last = len(move) if last is None else last
    old = np.zeros((last - first, 5)); new = np.zeros((last - first, 5)); v = np.full(last - first, V_IDLE, np.int32)
    for i in range(first, last):
        tt = int(t[i])
        live, m, pref = _complete(a.num_molecules(rep, tt), caps[tt], int(move[i]), float(su[i]), float(pv[i]))
        if not live:
            continue
        if au[i] == U_NEVER:
            o, w = a.move_trial([rep], [tt], [m], [move[i]], u[i:i + 1], T_STEP, R_STEP)
            acc = [0]
        else:
            o, w, acc = a.move_trial_decide([rep], [tt], [m], [move[i]], u[i:i + 1], T_STEP, R_STEP, au[i:i + 1], [pref], T)
        a.synchronize()
        old[i - first], new[i - first], v[i - first] = o[0], w[0], V_ACC if acc[0] else V_REJ
    return old, new, v


def _same_rows(one, two):
    (o1, w1, v1), (o2, w2, v2) = one, two
    assert np.array_equal(v1, v2), (v1, v2)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))


# ---------------------------------------------------------------------------------------------------------------------
# 1. a run is the step-by-step path
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("R,rep", [(1, 0), (3, 2)])
@pytest.mark.parametrize("name", tc.CELLS)
def test_a_gc_run_is_the_step_by_step_path(name, R, rep, k):
    """32 by-count records over both types, moves 0-4, step 7 idle; every launch queued before anything is collected."""
    s = tc.cell(name)
    caps = _caps(s)
    a, b = _twin(s, R)
    T = float(s.temperature)
    recs = _gc_records(np.random.default_rng(SEED_RUN[name]), s, 32)
    recs[1][7] = 0
    run = _run(b, rep, k, T, recs)
    twin = _twin_steps(a, rep, caps, recs, T)
    t, move = recs[0], recs[1]
    v1 = twin[2]
    n_ins, n_del = int(((v1 == V_ACC) & (move == 3)).sum()), int(((v1 == V_ACC) & (move == 4)).sum())
    print(f"{name} R={R} k={k}: accepted {int((v1 == V_ACC).sum())} of 32 ({n_ins} insertions of {int((move == 3).sum())}, "
          f"{n_del} deletions of {int((move == 4).sum())}), rejected {int((v1 == V_REJ).sum())}, launches {b.chain_run_launches()}")
    assert n_ins >= 2 and n_del >= 2 and int((v1 == V_REJ).sum()) >= 1          # (the preconditions, on the twin alone)
    _same_rows(twin, run)
    o2, w2, v2 = run
    assert v2[7] == V_IDLE and not np.any(o2[7]) and not np.any(w2[7])
    # an insertion carries the self and intra terms in its new row, a deletion in its old row; the absent state is zero
    assert np.all(w2[(move == 3) & (v2 != V_IDLE)][:, 3] != 0.0) and np.all(o2[(move == 4) & (v2 != V_IDLE)][:, 3] != 0.0)
    assert not np.any(o2[move == 3][:, [0, 1, 3, 4]]) and not np.any(w2[move == 4][:, [0, 1, 3, 4]])
    _same_state(a, b, s, R)
    for tt in range(s.topo.n_res):
        d = int(((v2 == V_ACC) & (move == 3) & (t == tt)).sum()) - int(((v2 == V_ACC) & (move == 4) & (t == tt)).sum())
        assert b.num_molecules(rep, tt) == int(s.n_mol[tt]) + d
    launches, steps, void, und = b.chain_run_stats()
    assert (launches, steps, und) == (32, 32, 0)
    if k == 4:
        assert max(c for _, c in b.chain_run_launches()) > 1
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the oracle directly
def test_an_insertion_and_a_deletion_against_the_oracle(refcpu_mod):
    """The sheared cell: the rows of an accepted insertion of the 3-site type and of a deletion of another molecule from the
    state it leaves, against oracle.refcpu (ComputeOldEnergy / ComputeNewEnergy) within tol_for, all five components; the
    inserted frame is read back."""
    s = tc.cell("sheared")
    N = int(s.n_mol[0])
    caps = _caps(s)
    b = _twin(s, 1)[1]
    T = float(s.temperature)
    rng = np.random.default_rng(9)
    t = np.zeros(2, np.int32); move = np.array([3, 4], np.int32)
    recs = (t, move, rng.uniform(0, 1, (2, 5)), np.array([U_ALWAYS, U_NEVER]), np.array([0.0, 0.3]), np.full(2, 20.0))
    o2, w2, v2 = _run(b, 0, 4, T, recs)
    assert list(v2) == [V_ACC, V_REJ] and b.num_molecules(0, 0) == N + 1
    com_d, off_d = b.get_frames(0, 0)
    assert np.array_equal(com_d[N], tc.cart(s, recs[2][0, :3]))
    md = min(int(0.3 * (N + 1)), N)
    P = refcpu_mod.RefCPU(s, mol_capacity=max(caps))
    e_sys = P.system_energy()
    P.init_amplitude(True)
    P.set_energy_recip(e_sys["recip_coulomb"])
    exp_old = np.zeros((2, 5)); exp_new = np.zeros((2, 5))
    exp_old[0] = P.old_energy(0, N, 1)[:5]
    P.set_num_residues(0, N + 1)
    P.save_fourier(0, N)
    P.set_molecule(0, N, com_d[N], off_d[N])
    exp_new[0] = P.new_energy(0, N, 1)[:5]
    # the insertion stands: the deletion is a trial of that state
    e_sys = P.system_energy()
    P.init_amplitude(True)
    P.set_energy_recip(e_sys["recip_coulomb"])
    P.all_fourier_terms()
    exp_old[1] = P.old_energy(0, md, 2)[:5]
    P.save_fourier(0, md)
    exp_new[1, 2] = P.recip_singlemol(0, md, 2)                  # intended physics: A - S_mol
    assert np.all(exp_new[0, 2:] != 0.0) and np.all(exp_old[1, 2:] != 0.0)          # (charged: every Coulomb term is there)
    for got, ref, what in ((o2, exp_old, "old"), (w2, exp_new, "new")):
        tol = tol_for(*np.ravel(ref), *np.ravel(got))
        err = float(np.max(np.abs(got - ref)))
        print(f"{what}: |run - oracle| = {err:.3e} K (tol {tol:.3e} K)")
        assert err <= tol, (what, got, ref)
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the inserted centre
@pytest.mark.parametrize("name", tc.CELLS)
def test_the_inserted_centre_is_lo_plus_matrix_u(name):
    """Seven insertions accepted whatever they cost (U_ALWAYS) whose first three construction numbers take every value of
    triclinic_cases.EDGE_FRAC on every axis (axis d of insertion j takes EDGE_FRAC[(j + 2 d) % 7]): the committed centre is
    triclinic_cases.cart(s, u) bit for bit (create_molecule.f90:181-182: no wrap, whichever side of a face it falls on).  The
    next launch builds on that centre: a translation of the LAST molecule of the type -- the one just inserted -- evaluated and
    rejected by fiat (in the sheared cell ApplyPBC takes such a centre to the far corner, where the 27-image search sees other
    neighbours: its cost is not the test's to bound), then a rotation accepted by fiat, which keeps the centre bit for bit.  A
    deletion of that molecule, accepted by fiat, restores the counts: six of the seven values are 0 or 1 to within 1e-16, so
    the insertions would otherwise land on one another."""
    s = tc.cell(name)
    caps = _caps(s)
    a, b = _twin(s, 1)
    T = float(s.temperature)
    rng = np.random.default_rng(SEED_EDGE)
    E = np.asarray(tc.EDGE_FRAC)
    n = 28
    t = np.repeat(np.arange(7) % 2, 4).astype(np.int32)
    move = np.tile(np.array([3, 1, 2, 4], np.int32), 7)
    u = rng.uniform(0, 1, (n, 5))
    for j in range(7):
        u[4 * j, :3] = [E[(j + 2 * d) % 7] for d in range(3)]
    for d in range(3):
        assert sorted(u[0::4, d]) == sorted(E)
    au = np.tile(np.array([U_ALWAYS, U_NEVER, U_ALWAYS, U_ALWAYS]), 7)
    recs = (t, move, u, au, np.full(n, BELOW_ONE), np.full(n, 50.0))
    b.chain_run_open(0, 4, T_STEP, R_STEP, T)
    b.chain_run_push_gc(*recs)
    rows = []
    for j in range(7):
        tt = int(t[4 * j])
        n_was = b.num_molecules(0, tt)
        want = tc.cart(s, u[4 * j, :3])
        b.chain_run_launch(1)
        rows.append(_collect(b, 1))
        assert rows[-1][2][0] == V_ACC and b.num_molecules(0, tt) == n_was + 1
        centre, off = (x[n_was].copy() for x in b.get_frames(0, tt))
        assert np.array_equal(centre, want), (j, centre - want)
        b.chain_run_launch(1)                                    # the translation (rejected) and the rotation (accepted)
        rows.append(_collect(b, 2))
        assert list(rows[-1][2]) == [V_REJ, V_ACC] and np.any(rows[-1][0][0]) and np.any(rows[-1][0][1])
        centre2, off2 = (x[n_was] for x in b.get_frames(0, tt))
        assert np.array_equal(centre2, want) and not np.array_equal(off2, off)
        b.chain_run_launch(1)
        rows.append(_collect(b, 1))
        assert rows[-1][2][0] == V_ACC and b.num_molecules(0, tt) == n_was
    b.chain_run_close()
    run = tuple(np.concatenate(x) for x in zip(*rows))
    twin = _twin_steps(a, 0, caps, recs, T)
    # (a probability that underflows to 0 would leave a U_ALWAYS step to the margin rule: not these records)
    with np.errstate(over="ignore"):
        assert np.all(np.exp(-(twin[1].sum(1) - twin[0].sum(1)) / T)[au == U_ALWAYS] > 0.0)
    _same_rows(twin, run)
    assert b.chain_run_launches() == [(4 * j + f, c) for j in range(7) for f, c in ((0, 1), (1, 2), (3, 1))]
    _same_state(a, b, s, 1)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the edges of the count
def _quiet_insertion(a, tt, rng, T):
    """construction numbers of an insertion of type tt into the twin's state that lands in no deep overlap (the twin's own
    energies of the trial; nothing is committed)"""
    for _ in range(64):
        u = rng.uniform(0, 1, (1, 5))
        o, w = a.move_trial([0], [tt], [0], [3], u, T_STEP, R_STEP)
        a.synchronize()
        if abs(float(w[0].sum() - o[0].sum())) / T < 50.0:
            return u[0]
    raise AssertionError("no insertion without an overlap in 64 draws")


def test_the_edges_of_the_count():
    """The sheared cell's 2-site type (8 molecules, capacity 32).  Deleted down to one molecule, then that one: moves and a
    deletion of the emptied type do nothing (verdict 5, state unchanged); an insertion into the empty type; then insertions up
    to the capacity, and one more, which does nothing.  Every step is accepted by fiat; the insertions' numbers are drawn
    against the twin until they land in no overlap.  Rows, verdicts and the state are the twin's."""
    s = tc.cell("sheared")
    caps = _caps(s)
    tt, N0, cap = 1, int(s.n_mol[1]), caps[1]
    a, b = _twin(s, 1)
    T = float(s.temperature)
    rng = np.random.default_rng(6)
    move = np.array([4] * N0 + [1, 2, 4] + [3] * (cap + 1) + [1], np.int32)
    n = len(move)
    u = rng.uniform(0, 1, (n, 5)); su = rng.uniform(0, 1, n)
    au = np.full(n, U_ALWAYS); au[-1] = U_NEVER
    pv = np.where(move == 3, 1e3, 1e-3)
    t = np.full(n, tt, np.int32)
    recs = (t, move, u, au, su, pv)
    # the twin first: an insertion's numbers are chosen against the state it meets
    rows, counts = [], []
    for i in range(n):
        counts.append(a.num_molecules(0, tt))
        if move[i] == 3 and counts[-1] < cap:
            u[i] = _quiet_insertion(a, tt, rng, T)
        rows.append(_twin_steps(a, 0, caps, recs, T, i, i + 1))
        if i == N0 + 2:
            empty = a.structure_factor(0).copy()
    twin = tuple(np.concatenate(x) for x in zip(*rows))
    assert counts == list(range(N0, 0, -1)) + [0, 0, 0] + list(range(0, cap + 1)) + [cap]
    assert list(twin[2]) == [V_ACC] * N0 + [V_IDLE] * 3 + [V_ACC] * cap + [V_IDLE, V_REJ]
    b.chain_run_open(0, 4, T_STEP, R_STEP, T)
    head = N0 + 3
    b.chain_run_push_gc(*(x[:head] for x in recs))
    b.chain_run_launch(head)
    first = _collect(b, head)
    # the emptied type: count 0, and the moves and the deletion behind it changed nothing
    assert b.num_molecules(0, tt) == 0 and b.get_molecules(0, tt).shape[0] == 0 and np.array_equal(b.structure_factor(0), empty)
    assert (N0, 3) in b.chain_run_launches()                     # one launch took the three steps that do nothing
    got = [first]
    for lo in range(head, n, 16):                                # (the rest in pieces the ring takes whatever its size)
        hi = min(lo + 16, n)
        b.chain_run_push_gc(*(x[lo:hi] for x in recs))
        b.chain_run_launch(hi - lo)
        got.append(_collect(b, hi - lo))
    b.chain_run_close()
    run = tuple(np.concatenate(x) for x in zip(*got))
    _same_rows(twin, run)
    assert not np.any(run[0][run[2] == V_IDLE]) and not np.any(run[1][run[2] == V_IDLE])
    _same_state(a, b, s, 1)
    assert b.num_molecules(0, tt) == cap
    a.close(); b.close()


@pytest.mark.parametrize("sel_u", [0.0, 0.5, BELOW_ONE])
def test_a_deletion_swaps_with_the_last_molecule(sel_u):
    """The sheared cell's 3-site type: m == last (nothing moves) and m != last (the last molecule's coordinates and frame go
    into slot m); a rotation by count follows from the new count."""
    s = tc.cell("sheared")
    caps = _caps(s)
    N = int(s.n_mol[0])
    a, b = _twin(s, 1)
    T = float(s.temperature)
    rng = np.random.default_rng(4)
    recs = (np.zeros(2, np.int32), np.array([4, 2], np.int32), rng.uniform(0, 1, (2, 5)), np.array([U_ALWAYS, U_ALWAYS]),
            np.array([sel_u, sel_u]), np.full(2, 1.0))
    before = b.get_molecules(0, 0).copy()
    frames_before = b.get_frames(0, 0)[0].copy()
    run = _run(b, 0, 4, T, recs)
    m = min(int(sel_u * N), N - 1)
    assert (m == N - 1) == (sel_u == BELOW_ONE)
    twin = _twin_steps(a, 0, caps, recs, T)
    assert list(run[2]) == [V_ACC, V_ACC]
    _same_rows(twin, run)
    _same_state(a, b, s, 1)
    after = b.get_molecules(0, 0)
    assert after.shape[0] == N - 1
    if m != N - 1:
        keep = np.arange(N - 1) != min(int(sel_u * (N - 1)), N - 2)   # (the rotation that follows moved one molecule)
        expect = before[:N - 1].copy(); expect[m] = before[N - 1]
        assert np.array_equal(after[keep], expect[keep])
        assert np.array_equal(b.get_frames(0, 0)[0][m], frames_before[N - 1])      # (a rotation keeps its centre)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. an undecided insertion and an undecided deletion
@pytest.mark.parametrize("accept", [True, False])
@pytest.mark.parametrize("kind", [3, 4])
def test_an_undecided_insertion_or_deletion_stalls_the_run_until_it_is_forced(kind, accept):
    """tests/test_gpu_chain_run_gcmc.py's construction in the sheared cell: phi V puts the step's probability at 0.5 (from the
    twin's energies of the initial state), its draw ON the probability, the margin opened to 1e-2.  The step comes back
    undecided, the launches queued behind it are void, nothing is committed; force accept / reject both end in the twin's
    state."""
    s = tc.cell("sheared")
    caps = _caps(s)
    N = int(s.n_mol[0])
    a, b = _twin(s, 1)
    T = float(s.temperature)
    rng = np.random.default_rng(SEED_STALL)
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
    run = _collect(b, n - st)
    b.chain_run_close()
    au1 = au.copy()
    au1[st] = U_ALWAYS if accept else U_NEVER
    twin = _twin_steps(a, 0, caps, (t, move, u, au1, su, phi_v), T, first=st)
    assert run[2][0] == (V_ACC if accept else V_REJ) and run[2][1] == V_ACC
    _same_rows(twin, run)
    assert np.array_equal(run[0][0], o[0]) and np.array_equal(run[1][0], w[0])
    _same_state(a, b, s, 1)
    assert b.num_molecules(0, 0) == a.num_molecules(0, 0)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. the switch
def _refused(call):
    with pytest.raises(_lib.MgpuError) as ei:
        call()
    assert ei.value.code == MGPU_ERR_STATE
    return str(ei.value)


def test_the_switch():
    """set_gc on a triclinic box: refused, naming the triclinic-run switch, while triclinic runs are off -- with device-built
    moves on and with them off, and with a reservoir besides; admitted once they are on; still refused with a reservoir and
    while a run is open, in the words those refusals always had.  Triclinic runs cannot be switched off under it.  With the
    switch on, NVT records through the plain push give the rows of the NVT triclinic run with it off, bit for bit, and the
    capacity does not depend on it."""
    s = tc.cell("mild")
    caps = _caps(s)
    T = float(s.temperature)
    # triclinic runs off
    for moves in (False, True):
        e = Engine.from_system(s, n_replicas=1, mol_capacity=caps, triclinic_moves=moves)
        text = _refused(lambda: e.chain_run_set_gc(True))
        assert "triclinic" in text and "mgpu_chain_run_set_triclinic" in text
        e.close()
    e = _engine(s, 1, caps)
    e.set_reservoir(0, 1, s.offsets[1][:2].copy())
    assert "triclinic" in _refused(lambda: e.chain_run_set_gc(True))
    e.chain_run_set_triclinic(True)
    assert "reservoir" in _refused(lambda: e.chain_run_set_gc(True))              # (on: the reservoir's own refusal)
    e.close()
    # admitted once triclinic runs are on; the capacity is the switch-off one
    b, c = _engine(s, 1, caps), _engine(s, 1, caps)
    assert "triclinic" in _refused(lambda: b.chain_run_set_gc(True))
    for e in (b, c):
        e.chain_run_set_triclinic(True)
    cap = b.chain_run_capacity()
    assert cap[0] >= 4
    b.chain_run_set_gc(True)
    assert b.chain_run_capacity() == cap == c.chain_run_capacity()
    # triclinic runs stay on under it
    _refused(lambda: b.chain_run_set_triclinic(False))
    assert b.chain_run_capacity() == cap
    b.chain_run_set_triclinic(True)                              # (on again is no change)
    # a run open: neither switch moves; NVT records through the plain push, against engine c's run with the switch off
    nvt = _nvt_records(np.random.default_rng(32), s, 12)
    out = []
    for e in (b, c):
        e.chain_run_open(0, 4, T_STEP, R_STEP, T)
        if e is b:
            assert "a run is open" in _refused(lambda: b.chain_run_set_gc(False))
            assert "a run is open" in _refused(lambda: b.chain_run_set_gc(True))
            for mv in (3, 4):                                    # the plain push still refuses them, in its own words
                t, m, move, u, au = _nvt_records(np.random.default_rng(33), s, 3)
                move[1] = mv
                with pytest.raises(_lib.MgpuError) as ei:
                    b.chain_run_push(t, m, move, u, au)
                assert "chain_run_push: insertions and deletions do not ride in a run (moves only)" in str(ei.value)
        else:
            with pytest.raises(_lib.MgpuError) as ei:
                c.chain_run_push_gc(*_gc_records(np.random.default_rng(34), s, 4))
            assert "chain_run_push_gc" in str(ei.value)
        e.chain_run_push(*nvt)
        e.chain_run_launch(12)
        out.append(_collect(e, 12))
        e.chain_run_close()
    _same_rows(out[1], out[0])
    assert 0 < int((out[0][2] == V_ACC).sum())
    _same_state(c, b, s, 1)
    # off again, and triclinic runs may then go
    b.chain_run_set_gc(False)
    b.chain_run_set_triclinic(False)
    assert b.chain_run_capacity() == (0, 0, 0)
    assert "triclinic" in _refused(lambda: b.chain_run_set_gc(True))
    b.close(); c.close()
