"""Chain runs in TRICLINIC cells (mgpu_chain_run_set_triclinic, chain_run_kernel<false, false, true>): launches of one
chain queued back to back, each building its steps from the resident frames with ApplyPBC's triclinic form and sweeping
with ComputeDistance's image search.  Every comparison is np.array_equal against a twin engine advanced one step at a time
by the batched device-built path (move_trial_decide, move_trial for the forced rejections), which
tests/test_gpu_triclinic_moves.py holds to the oracle: per-step old / new rows, verdicts, coordinates, frames, counts, A(k).
The cells are tests/triclinic_cases.py's: a mild tilt, and the largest tilt LAMMPS allows.
Reference: src/monte_carlo.f90:40-86, src/geometry_utils.f90:167-220 (ApplyPBC), :397-411 (ComputeDistance)."""
import numpy as np
import pytest

from maniac_mc_amd import _lib, synth
from maniac_mc_amd.engine import Engine
from tests import triclinic_cases as tc
from tests.test_gpu_chain_run import U_ALWAYS, U_NEVER, V_ACC, V_IDLE, V_REJ, V_UND, _collect, _twin_steps
from tests.test_gpu_triclinic_moves import _caps, _engine, _same_state
from tests.util import TOL_K

pytestmark = pytest.mark.gpu

T_STEP, R_STEP = 0.4, 0.4
# Seeds of the record sets below, chosen by stepping the same records with the CPU oracle (oracle.refcpu); each test asserts
# on the twin what its seed was chosen for.
#   SEED_RUN    rejections among the 24 steps (mild 20 of 23 accepted, sheared 13), a rejected step ahead of another inside a
#               window of four
#   SEED_WRAP   none of the six steps accepted by fiat lands in an overlap deep enough for exp() to underflow
#   SEED_STALL  step 3 is the first with 1e-6 < x < 0.99 in the initial state
#   SEED_ORACLE the first non-idle step is a translation out of no overlap (energies of ~7e3 K: 16 ulp are far below TOL_K)
SEED_RUN = {"mild": 3, "sheared": 6}
SEED_WRAP = {"mild": 30, "sheared": 35}
SEED_STALL = 24
SEED_ORACLE = 7


def _twin(s, R):
    """(a, b): two engines holding R copies of `s` with resident frames and device-built triclinic moves; b takes runs."""
    a, b = _engine(s, R), _engine(s, R)
    b.chain_run_set_triclinic(True)
    return a, b


def _records(rng, s, n, idle=()):
    """n NVT records over both residue types: (t, m, move, u5, accept_u); steps in `idle` carry move 0."""
    t = rng.integers(0, s.topo.n_res, n).astype(np.int32)
    m = np.array([rng.integers(0, s.n_mol[tt]) for tt in t], np.int32)
    move = rng.integers(1, 3, n).astype(np.int32)
    for i in idle:
        move[i] = 0
    return t, m, move, rng.uniform(0, 1, (n, 5)), rng.uniform(0, 1, n)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("R,rep", [(1, 0), (3, 2)])
@pytest.mark.parametrize("name", tc.CELLS)
def test_a_run_is_the_step_by_step_path(name, R, rep, k):
    """24 random NVT records of both types (one of them idle), every launch queued -- three at a time -- before anything is
    collected."""
    s = tc.cell(name)
    a, b = _twin(s, R)
    max_k, depth, ring = b.chain_run_capacity()
    assert max_k >= 4 and depth >= 24 and ring >= 24
    T = float(s.temperature)
    recs = _records(np.random.default_rng(SEED_RUN[name]), s, 24, idle=(7,))
    b.chain_run_open(rep, k, T_STEP, R_STEP, T)
    b.chain_run_push(*recs)
    for _ in range(8):                                          # 24 launches: enough whatever is accepted
        b.chain_run_launch(3)
    o2, w2, v2 = _collect(b, 24)
    b.chain_run_close()
    o1, w1, v1 = _twin_steps(a, rep, recs, T, T_STEP, R_STEP)
    print(f"{name} R={R} k={k}: accepted {int((v1 == V_ACC).sum())} of 24, launches {b.chain_run_launches()}")
    assert 0 < int((v1 == V_ACC).sum()) < 24                    # (the precondition, on the twin alone)
    assert np.array_equal(v1, v2), (v1, v2)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))
    assert v2[7] == V_IDLE and not np.any(o2[7]) and not np.any(w2[7])
    _same_state(a, b, s, R)
    launches, steps, void, und = b.chain_run_stats()
    assert (launches, steps, und) == (24, 24, 0) and void == 24 - len([c for _, c in b.chain_run_launches() if c])
    if k == 4:
        assert max(c for _, c in b.chain_run_launches()) > 1
    a.close(); b.close()


@pytest.mark.parametrize("name", tc.CELLS)
def test_steps_that_cross_a_cell_face(name, refcpu_mod):
    """A translation step of half the shortest cell edge.  Steps 2-7 push ONE molecule along +x by 0.45 steps each and are
    accepted whatever they cost (U_ALWAYS): six of them cover 1.35 edges, so the molecule leaves through a face, and -- k = 4,
    one launch per accepted step -- the wrapped centre one launch commits is the resident frame the next builds on.
    Every committed centre is the oracle's ApplyPBC of (old centre + displacement), bit for bit.  That map goes through
    f = box%reciprocal v and back through box%matrix f, and box%reciprocal is the inverse of the matrix's TRANSPOSE
    (tests/triclinic_cases.py): it is no pure lattice translation of the Cartesian position (a centre inside the cell moves
    too), so "wrapped by a lattice vector" is asserted where it holds: the committed centre against lo + M f with f NOT
    reduced differs by M n, n = floor(f) a non-zero integer vector, for at least one step."""
    s = tc.cell(name)
    M, lo = np.asarray(s.box_matrix, dtype=np.float64), np.asarray(s.bounds_lo, dtype=np.float64)
    t_step = 0.5 * float(np.min(np.linalg.norm(M, axis=1)))
    T = float(s.temperature)
    P = refcpu_mod.RefCPU(s)
    rcp = P.box()[2]
    a, b = _twin(s, 1)
    t, m, move, u, au = _records(np.random.default_rng(SEED_WRAP[name]), s, 12)
    push = slice(2, 8)
    t[push], m[push], move[push], au[push] = t[2], m[2], 1, U_ALWAYS
    u[push, 0], u[push, 1], u[push, 2] = 0.95, 0.5, 0.5
    recs = (t, m, move, u, au)
    b.chain_run_open(0, 4, t_step, R_STEP, T)
    b.chain_run_push(*recs)
    b.chain_run_launch(12)
    o2, w2, v2 = _collect(b, 12)
    b.chain_run_close()
    # the twin, step by step, with the moved molecule's centre before and after every accepted translation
    rows, wrapped = [], 0
    for i in range(12):
        before = a.get_frames(0, int(t[i]))[0][int(m[i])].copy()
        rows.append(_twin_steps(a, 0, recs, T, t_step, R_STEP, i, i + 1))
        if move[i] == 1 and rows[-1][2][0] == V_ACC:
            after = a.get_frames(0, int(t[i]))[0][int(m[i])]
            target = before + (u[i, :3] - 0.5) * t_step
            assert np.array_equal(after, P.apply_pbc(target)), (i, after - P.apply_pbc(target))
            f = rcp @ (target - lo)
            n = np.floor(f)
            if np.any(n != 0):
                assert np.max(np.abs((after - (lo + M @ f)) + M @ n)) < 1e-9, (i, f)
                wrapped += 1
    o1, w1, v1 = (np.concatenate(x) for x in zip(*rows))
    # (an acceptance probability that underflows to 0 would leave a U_ALWAYS step to the margin rule: not these records)
    with np.errstate(over="ignore"):
        x = np.exp(-(w1.sum(1) - o1.sum(1)) / T)
    assert np.all(x[push] > 0.0) and np.all(v1[push] == V_ACC)
    assert wrapped >= 1
    print(f"{name}: t_step {t_step:.3f}, {wrapped} committed centres wrapped, launches {b.chain_run_launches()}")
    assert np.array_equal(v1, v2), (v1, v2)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))
    assert not np.array_equal(o2[3], o2[2])                     # (step 3's old row is of the molecule where step 2 put it)
    _same_state(a, b, s, 1)
    assert b.chain_run_stats()[3] == 0
    a.close(); b.close()


@pytest.mark.parametrize("accept", [True, False])
def test_an_undecided_step_stalls_the_run_until_it_is_forced(accept):
    """The sheared cell; one step's draw is put ON its acceptance probability (taken from the twin's energies, 1e-6 < x < 1)
    and the margin opened to 1e-2: the step comes back undecided, the launches queued behind it do nothing and nothing is
    committed; close is refused; after force the run ends in the twin's state, for either decision."""
    s = tc.cell("sheared")
    T = float(s.temperature)
    a, b = _twin(s, 1)
    t, m, move, u, au = _records(np.random.default_rng(SEED_STALL), s, 10)
    au[:] = U_NEVER
    # the steps up to the chosen one are rejected: each is a trial of the initial state, whose energies the twin gives
    o, w = a.move_trial(np.zeros(10, np.int32), t, m, move, u, T_STEP, R_STEP)
    with np.errstate(over="ignore"):
        x = np.exp(-(w.sum(1) - o.sum(1)) / T)
    ok = np.nonzero((x > 1e-6) & (x < 0.99))[0]
    assert ok.size > 0 and ok[0] < 8
    st = int(ok[0])
    au[st] = x[st]
    au[st + 1] = U_ALWAYS
    recs = (t, m, move, u, au)
    b.chain_set_margin(1e-2)
    b.chain_run_open(0, 4, T_STEP, R_STEP, T)
    b.chain_run_push(*recs)
    b.chain_run_launch(6)
    rows = []
    while True:
        o2, w2, v2, stalled_at = b.chain_run_collect(10, wait=True)
        rows.append((o2, w2, v2))
        if stalled_at >= 0:
            break
    o2, w2, v2 = (np.concatenate(x_) for x_ in zip(*rows))
    assert stalled_at == st and len(v2) == st + 1 and v2[st] == V_UND and np.all(v2[:st] == V_REJ)   # the row is published
    assert np.array_equal(o2, o[:st + 1]) and np.array_equal(w2, w[:st + 1])
    b.synchronize()
    tags = b.chain_run_launches()
    assert sum(c for _, c in tags) == st and all(c == 0 for f, c in tags if f == st) and tags[-1] == (st, 0)   # queued launches: void
    assert b.chain_run_collect(10, wait=False)[3] == st          # nothing more before the decision
    _same_state(a, b, s, 1)                                     # nothing committed at or behind the step
    with pytest.raises(_lib.MgpuError):
        b.chain_run_close()
    with pytest.raises(_lib.MgpuError):
        b.chain_run_set_triclinic(False)                        # not while the run is open
    assert b.chain_run_stats()[3] >= 1
    b.chain_run_force(st, accept)
    b.chain_run_launch(6)
    o3, w3, v3 = _collect(b, 10 - st)
    b.chain_run_close()
    au1 = au.copy()
    au1[st] = U_ALWAYS if accept else U_NEVER
    o1, w1, v1 = _twin_steps(a, 0, (t, m, move, u, au1), T, T_STEP, R_STEP, first=st)
    assert v3[0] == (V_ACC if accept else V_REJ) and v3[1] == V_ACC
    assert np.array_equal(v1, v3) and np.array_equal(o1, o3) and np.array_equal(w1, w3)
    _same_state(a, b, s, 1)
    a.close(); b.close()


def test_the_first_step_against_the_oracle(refcpu_mod):
    """The sheared cell's first non-idle step, accepted whatever it costs: its old and new rows against the oracle evaluated
    for the candidate the device built and committed (ComputeOldEnergy / ComputeNewEnergy), within TOL_K; a translation's
    committed centre against the oracle's ApplyPBC bit for bit."""
    s = tc.cell("sheared")
    T = float(s.temperature)
    b = _engine(s, 1)
    b.chain_run_set_triclinic(True)
    t, m, move, u, au = _records(np.random.default_rng(SEED_ORACLE), s, 4, idle=(0,))
    au[:] = U_NEVER
    au[1] = U_ALWAYS
    b.chain_run_open(0, 4, T_STEP, R_STEP, T)
    b.chain_run_push(t, m, move, u, au)
    b.chain_run_launch(1)
    old, new, v = _collect(b, 2)
    b.chain_run_close()
    assert v[0] == V_IDLE and v[1] == V_ACC
    tt, mm = int(t[1]), int(m[1])
    P = refcpu_mod.RefCPU(s, mol_capacity=max(_caps(s)))
    P.system_energy()
    P.init_amplitude(True)
    com_d, off_d = b.get_frames(0, tt)
    if move[1] == 1:
        assert np.array_equal(com_d[mm], P.apply_pbc(s.com[tt][mm] + (u[1, :3] - 0.5) * T_STEP))
    P.save_fourier(tt, mm)
    eo = P.old_energy(tt, mm, 0)[:5]
    P.set_molecule(tt, mm, com_d[mm], off_d[mm])
    en = P.new_energy(tt, mm, 0)[:5]
    err_o, err_n = float(np.max(np.abs(old[1] - eo))), float(np.max(np.abs(new[1] - en)))
    print(f"step 1 (move {move[1]}, type {tt}): |old - oracle| = {err_o:.3e} K, |new - oracle| = {err_n:.3e} K (TOL_K {TOL_K:.2e})")
    assert err_o <= TOL_K and err_n <= TOL_K
    b.close()


def _refused(call):
    with pytest.raises(_lib.MgpuError) as ei:
        call()
    return ei.value.code


def test_the_switch_and_its_refusals():
    MGPU_ERR_STATE = 5
    s = tc.cell("mild")
    T = float(s.temperature)
    # an orthorhombic engine: refused, and its capacity is what it was
    so = synth.spce_box(6, seed=3)
    eo = Engine.from_system(so, n_replicas=1)
    cap_o = eo.chain_run_capacity()
    assert cap_o[0] > 0
    for on in (True, False):
        assert _refused(lambda: eo.chain_run_set_triclinic(on)) == MGPU_ERR_STATE
    assert eo.chain_run_capacity() == cap_o
    eo.close()
    # a triclinic engine without device-built moves: refused, capacity 0 -- also once the moves are switched on (the run
    # switch is still off: the refused calls did not move it)
    e = Engine.from_system(s, n_replicas=1, mol_capacity=_caps(s))
    assert _refused(lambda: e.chain_run_set_triclinic(True)) == MGPU_ERR_STATE
    assert e.chain_run_capacity() == (0, 0, 0)
    e.set_triclinic_moves(True)
    assert e.chain_run_capacity() == (0, 0, 0)
    _refused(lambda: e.chain_run_open(0, 1, T_STEP, R_STEP, T))
    e.close()
    # the switch, on and off again; refused while a run is open, which leaves it on
    e = _engine(s, 1)
    assert e.chain_run_capacity() == (0, 0, 0)
    e.chain_run_set_triclinic(True)
    cap = e.chain_run_capacity()
    assert cap[0] >= 4 and cap[1] >= 24 and cap[2] >= 24
    e.chain_run_open(0, 2, T_STEP, R_STEP, T)
    for on in (False, True):
        assert _refused(lambda: e.chain_run_set_triclinic(on)) == MGPU_ERR_STATE
    rng = np.random.default_rng(31)
    for mv in (3, 4):                                            # insertions and deletions do not ride in a run
        t, m, move, u, au = _records(rng, s, 3)
        move[1] = mv
        _refused(lambda: e.chain_run_push(t, m, move, u, au))
    e.chain_run_close()
    assert e.chain_run_capacity() == cap
    # device-built moves off: capacity 0 whatever the run switch says, and the switch cannot be touched
    e.set_triclinic_moves(False)
    assert e.chain_run_capacity() == (0, 0, 0)
    assert _refused(lambda: e.chain_run_set_triclinic(False)) == MGPU_ERR_STATE
    e.set_triclinic_moves(True)
    assert e.chain_run_capacity() == cap
    e.chain_run_set_triclinic(False)
    assert e.chain_run_capacity() == (0, 0, 0)
    _refused(lambda: e.chain_run_open(0, 1, T_STEP, R_STEP, T))
    # a reservoir: capacity 0 with the switch on
    e.chain_run_set_triclinic(True)
    e.set_reservoir(0, 1, s.offsets[1][:2].copy())
    assert e.chain_run_capacity() == (0, 0, 0)
    _refused(lambda: e.chain_run_open(0, 1, T_STEP, R_STEP, T))
    e.close()
    # a 24-site active type in a triclinic box: capacity 0 with the switch on
    big = synth.rigid_adsorbate_box(n_mol=6, n_sites=24, seed=17).copy()
    big.box_matrix[1, 0], big.box_matrix[2, 0], big.box_matrix[2, 1] = 1.5, -0.8, 0.6
    assert big.is_triclinic()
    e = Engine.from_system(big, n_replicas=1, triclinic_moves=True)
    e.chain_run_set_triclinic(True)
    assert e.chain_run_capacity() == (0, 0, 0)
    _refused(lambda: e.chain_run_open(0, 1, T_STEP, R_STEP, 300.0))
    e.close()


def test_an_orthorhombic_run_is_untouched():
    """one k = 4 run of the SPC/E box (tests/test_gpu_chain_run.py's) still equals its twin"""
    from tests import test_gpu_chain_run as ortho
    s, t_act = ortho._box("spce")
    a, b = ortho._twin(s, 1)
    T = float(s.temperature)
    recs = ortho._records(np.random.default_rng(5), s, t_act, 24, idle=(7,))
    b.chain_run_open(0, 4, ortho.T_STEP, ortho.R_STEP, T)
    b.chain_run_push(*recs)
    for _ in range(8):
        b.chain_run_launch(3)
    o2, w2, v2 = _collect(b, 24)
    b.chain_run_close()
    o1, w1, v1 = _twin_steps(a, 0, recs, T)
    assert np.array_equal(v1, v2) and np.array_equal(o1, o2) and np.array_equal(w1, w2)
    assert 0 < int((v2 == V_ACC).sum()) < 24
    ortho._same_state(a, b, s, 1)
    assert b.chain_run_stats()[:2] == (24, 24) and max(c for _, c in b.chain_run_launches()) > 1
    a.close(); b.close()
