"""Chain runs of rigid molecules of 6 to 63 sites (mgpu_chain_run_set_wide, chain_run_kernel<FLAT, FASTW, false, GC, true>): the
WIDE instances put farm_window_kernel<..., WIDE>'s front end (rows rebuilt from the resident frames, the LDS-staged NS = 0 pair
sweep) and chain_window_kernel<..., WIDE>'s k role (the form of the row's own type, A + delta into the step's own buffer) behind
the run's cursor, ticket and resolver.  Off at creation: an engine with such an active type reports capacity 0 as it always did.
Every bit-for-bit comparison is np.array_equal against a twin engine advanced one record at a time by the batched device-built
path under MGPU_NO_FROZEN_BATCH=1 (tests/test_gpu_chain_run.py's and tests/test_gpu_chain_run_gcmc.py's twins, code of the commit
before this one), with the slot and prefactor of a by-count record computed here from the twin's counts: rows of five
components, verdicts, coordinates, frames, counts, A(k).  One move, one insertion and one deletion of 24 sites go to
oracle.refcpu directly.
The edges: 6 sites (the first WIDE size), 8, 24 (the matrix-unit form; the vector form under MGPU_RECIP_NO_MFMA=1), more than
kIntraThreadMax = 32 sites (the wave form of the intra term), and launches that mix narrow and WIDE steps (the 3 + 24 mixture).
Reference: src/monte_carlo.f90:40-86, src/monte_carlo_utils.f90:184-226, :275-395, src/create_molecule.f90,
src/delete_molecule.f90:100-142."""
import numpy as np
import pytest

from maniac_mc_amd import _lib, synth
from maniac_mc_amd.engine import Engine
from tests.test_gpu_chain_run import (R_STEP, T_STEP, U_ALWAYS, U_NEVER, V_ACC, V_IDLE, V_REJ, V_UND, _collect, _records, _same_state,
                                      _twin_steps)
from tests.test_gpu_chain_run_gcmc import BELOW_ONE, _complete, _gc_records, _twin_gc_steps
from tests.test_gpu_farm_window_wide import _batched_step, _env, _framework_guest, _shell, _system, _twin, _water

pytestmark = pytest.mark.gpu

MGPU_ERR_STATE = 5
NFB = {"MGPU_NO_FROZEN_BATCH": "1"}


def _box(name):
    """(system, active types)"""
    if name in ("6", "8", "12", "24", "40"):
        return synth.rigid_adsorbate_box(n_mol=6, n_sites=int(name), L=26.0, seed=17), [0]
    if name == "3+24":
        return _system(np.diag([36.0, 36.0, 36.0]), [(*_water(), 10), (*_shell(24, seed=21), 3)], seed=21), [0, 1]
    raise KeyError(name)


def _pair(s, R, cap=None, env=None, wide=True):
    """the twin (batched path) and the run engine, WIDE runs on"""
    a, b = _twin(s, R, cap=cap, env=dict(NFB, **(env or {})))
    if wide:
        b.chain_run_set_wide(True)
    return a, b


def _mixed_records(rng, s, act, n, idle=(), never=0.4):
    """n NVT records over the active types: (t, m, move, u5, accept_u)"""
    t = rng.choice(act, n).astype(np.int32)
    m = np.array([rng.integers(0, int(s.n_mol[tt])) for tt in t], np.int32)
    move = rng.integers(1, 3, n).astype(np.int32)
    for i in idle:
        move[i] = 0
    u, au = rng.uniform(0, 1, (n, 5)), rng.uniform(0, 1, n)
    # (the boxes are dilute -- nearly every move is downhill or within T of it -- so a launch would rarely get past its first step:
    #  `never` of the draws are replaced by U_NEVER, a rejection whatever the energies, as tests/test_gpu_chain_run.py does)
    au[rng.random(n) < never] = U_NEVER
    return t, m, move, u, au


def _row_form(a, s):
    """every active type takes the row form of the reciprocal update: the deciding batched submit (mgpu_move_trial_decide_submit,
    _twin_steps' and _twin_gc_steps' call) takes the engine; it refuses the wide forms"""
    return all(a.recip_form(int(s.topo.atoms_in_res[t]))["form"] == "rows" for t in range(s.topo.n_res) if s.topo.is_active[t])


def _one_batched(a, rep, t, m, move, u, au, pref, T):
    """one record through mgpu_move_trial_submit, the host's rule and mgpu_commit_submit (tests/test_gpu_farm_window_wide.py
    _batched_step: the twin of the WIDE farm windows, for the types whose form the deciding submit refuses)"""
    o, w, yes, near = _batched_step(a, np.array([rep], np.int32), np.array([t], np.int32), np.array([m], np.int32),
                                    np.array([move], np.int32), u[None, :], T_STEP, R_STEP, np.array([au]), np.array([pref]), T)
    a.synchronize()
    assert au == U_NEVER or not near[0]                          # (the run would leave such a step to the host)
    return o[0], w[0], V_ACC if yes[0] else V_REJ


def _steps(a, s, rep, recs, T, first=0, last=None):
    """The twin, one NVT record at a time: _twin_steps where the deciding submit takes the engine, else _one_batched."""
    if _row_form(a, s):
        return _twin_steps(a, rep, recs, T, first=first, last=last)
    t, m, move, u, au = recs
    last = len(m) if last is None else last
    old = np.zeros((last - first, 5)); new = np.zeros((last - first, 5)); v = np.full(last - first, V_IDLE, np.int32)
    for i in range(first, last):
        if move[i] != 0:
            old[i - first], new[i - first], v[i - first] = _one_batched(a, rep, t[i], m[i], move[i], u[i], au[i], 1.0, T)
    return old, new, v


def _gc_steps(a, s, rep, t_act, cap, recs, T, first=0, last=None):
    """The twin, one by-count record at a time, slot and prefactor from ITS count (_complete): _twin_gc_steps or _one_batched."""
    if _row_form(a, s):
        return _twin_gc_steps(a, rep, t_act, cap, recs, T, first=first, last=last)
    t, move, u, au, su, pv = recs
    last = len(move) if last is None else last
    old = np.zeros((last - first, 5)); new = np.zeros((last - first, 5)); v = np.full(last - first, V_IDLE, np.int32)
    for i in range(first, last):
        live, m, pref = _complete(a.num_molecules(rep, t_act), cap, int(move[i]), float(su[i]), float(pv[i]))
        if live:
            old[i - first], new[i - first], v[i - first] = _one_batched(a, rep, t[i], m, move[i], u[i], au[i], pref, T)
    return old, new, v


def _refused(code):
    with pytest.raises(_lib.MgpuError) as ei:
        code()
    assert ei.value.code == MGPU_ERR_STATE
    return str(ei.value)


# ---------------------------------------------------------------------------------------------- capacity and the switch

@pytest.mark.parametrize("name", ["6", "8", "24", "3+24"])
def test_capacity_follows_the_switch(name):
    s, act = _box(name)
    T = float(s.temperature)
    a, b = _pair(s, 1, wide=False)
    assert b.chain_run_capacity()[0] == 0
    assert "chain_run_open: not available" in _refused(lambda: b.chain_run_open(0, 1, T_STEP, R_STEP, T))
    b.chain_run_set_wide(True)
    max_k, depth, ring = b.chain_run_capacity()
    assert max_k >= 4 and depth >= 32 and ring >= 32
    b.chain_run_set_wide(False)
    assert b.chain_run_capacity() == (0, 0, 0)
    assert "chain_run_open: not available" in _refused(lambda: b.chain_run_open(0, 1, T_STEP, R_STEP, T))
    # the switch while a run is open: refused either way, and the run stays usable
    b.chain_run_set_wide(True)
    b.chain_run_open(0, 4, T_STEP, R_STEP, T)
    for on in (False, True):
        assert "a run is open" in _refused(lambda: b.chain_run_set_wide(on))
    recs = _mixed_records(np.random.default_rng(2), s, act, 4)
    b.chain_run_push(*recs)
    b.chain_run_launch(4)
    o2, w2, v2 = _collect(b, 4)
    b.chain_run_close()
    o1, w1, v1 = _steps(a, s, 0, recs, T)
    assert np.array_equal(v1, v2) and np.array_equal(o1, o2) and np.array_equal(w1, w2)
    _same_state(a, b, s, 1)
    b.chain_run_set_wide(False)
    assert b.chain_run_capacity()[0] == 0
    a.close(); b.close()


def test_what_keeps_capacity_zero_or_is_refused_by_name():
    # a 300-site (site-major) type: the switch is taken, the capacity stays 0
    e = Engine.from_system(synth.large_adsorbate_box(), n_replicas=1)
    e.chain_run_set_wide(True)
    assert e.chain_run_capacity()[0] == 0
    e.close()
    # the per-k form of the reciprocal update
    with _env(MGPU_RECIP_PER_K="1"):
        e = Engine.from_system(_box("24")[0], n_replicas=1)
    assert e.recip_form(24)["form"] == "per-k"
    e.chain_run_set_wide(True)
    assert e.chain_run_capacity()[0] == 0
    e.close()
    # a tilted 24-site box with device-built triclinic moves and triclinic runs on: no WIDE sweep has the image search
    s = _box("24")[0]
    L = float(s.box_matrix[0, 0])
    s.box_matrix = np.array([[L, 0.0, 0.0], [1.5, L, 0.0], [-0.8, 0.6, L]])
    e = Engine.from_system(s, n_replicas=1, triclinic_moves=True)
    e.chain_run_set_triclinic(True)
    text = _refused(lambda: e.chain_run_set_wide(True))
    assert "triclinic" in text and "image search" in text
    assert e.chain_run_capacity()[0] == 0
    e.chain_run_set_wide(False)                                  # (off is no change)
    e.close()
    # an engine with a reservoir: no RSV instance of the run kernel
    s = _box("24")[0]
    e = Engine.from_system(s, n_replicas=1, mol_capacity=[10])
    e.set_frames(0, 0, s.com[0], s.offsets[0])
    e.set_reservoir(0, 0, s.offsets[0][:4])
    text = _refused(lambda: e.chain_run_set_wide(True))
    assert "reservoir" in text and "RSV" in text
    assert e.chain_run_capacity()[0] == 0
    e.close()


# ---------------------------------------------------------------------------------------------- NVT runs

# (box, R, replica, form).  The boxes are dilute and the steps 0.4 A / 0.4 rad: with draws in [0, 1) alone the twin accepts 30 or 31
# of the 31 live steps (measured, seeds 5-7), so 40 % of the draws are U_NEVER (_mixed_records) and the twin then accepts 15 to 21
# and rejects 10 to 16.  Seed 6 is the one of the three with a rejection that the energies decide, in the 6-, 8- and 24-site boxes.
NVT_CASES = [("6", 1, 0, None), ("8", 1, 0, None), ("24", 1, 0, None), ("24", 1, 0, "vector"), ("24", 3, 2, None), ("3+24", 1, 0, None),
             ("3+24", 3, 2, None)]
NVT_SEED = 6


def _nvt_run(b, rep, k, T, recs):
    n = len(recs[1])
    b.chain_run_open(rep, k, T_STEP, R_STEP, T)
    b.chain_run_push(*recs)
    for _ in range(n // 4):                                      # n launches: enough whatever is accepted; none collected yet
        b.chain_run_launch(4)
    out = _collect(b, n)
    b.chain_run_close()
    return out


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("name,R,rep,form", NVT_CASES)
def test_a_wide_run_is_the_step_by_step_path(name, R, rep, form, k):
    """32 random move records, one of them idle, every launch queued before anything is collected."""
    s, act = _box(name)
    a, b = _pair(s, R, env={"MGPU_RECIP_NO_MFMA": "1"} if form == "vector" else None)
    big = max(int(s.topo.atoms_in_res[t]) for t in act)
    f = b.recip_form(big)["form"]
    assert f in ("rows", "wide-vector", "wide-mfma") and (form != "vector" or f != "wide-mfma"), f
    if name == "24" and form is None:
        assert f == "wide-mfma"
    assert b.chain_run_capacity()[0] >= 4
    T = float(s.temperature)
    recs = _mixed_records(np.random.default_rng(NVT_SEED), s, act, 32, idle=(7,))
    o2, w2, v2 = _nvt_run(b, rep, k, T, recs)
    o1, w1, v1 = _steps(a, s, rep, recs, T)
    tags = b.chain_run_launches()
    print(f"{name} R={R} form={f} k={k}: twin accepted {int((v1 == V_ACC).sum())}, rejected {int((v1 == V_REJ).sum())} of 32, launches {tags}")
    assert int((v1 == V_ACC).sum()) >= 2 and int((v1 == V_REJ).sum()) >= 1
    assert np.array_equal(v1, v2), (v1, v2)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))
    assert v2[7] == V_IDLE and not np.any(o2[7]) and not np.any(w2[7])
    assert not np.any(o2[:, 3:]) and not np.any(w2[:, 3:])      # a move has no self or intra term
    _same_state(a, b, s, R)
    launches, steps, void, und = b.chain_run_stats()
    assert (launches, steps, und) == (32, 32, 0)
    if k == 4:
        assert max(c for _, c in tags) > 1
        if name == "3+24":
            # some launch consumed steps of both types: narrow and WIDE code in one launch
            n1 = np.array([int(s.topo.atoms_in_res[t]) for t in recs[0]])
            live = recs[2] != 0
            assert any(len({int(x) for x in n1[f0:f0 + c][live[f0:f0 + c]]}) == 2 for f0, c in tags if c > 1), tags
    a.close(); b.close()


def test_a_framework_box_with_a_wide_guest():
    """A frozen framework and a 12-site guest (the flat family, FLAT = true): the same comparison at k = 4."""
    s = _framework_guest()
    a, b = _pair(s, 1, cap=[1, 8])
    assert b.chain_run_capacity()[0] >= 4
    T = float(s.temperature)
    recs = _records(np.random.default_rng(11), s, 1, 16)
    o2, w2, v2 = _nvt_run(b, 0, 4, T, recs)
    o1, w1, v1 = _steps(a, s, 0, recs, T)
    print(f"framework + 12-site guest: twin accepted {int((v1 == V_ACC).sum())} of 16, launches {b.chain_run_launches()}")
    assert np.array_equal(v1, v2), (v1, v2)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))
    assert int((v1 == V_REJ).sum()) >= 1 and max(c for _, c in b.chain_run_launches()) > 1
    _same_state(a, b, s, 1)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- grand-canonical runs

# phi V of the insertion and of the deletion records in units of the initial count N0 = 6, as tests/test_gpu_chain_run_gcmc.py's PHI:
# the bare prefactors are PHI[0] N0 / (N + 1) and N / (PHI[1] N0).  The twin's dE / T of these records (measured with the twin
# alone, 32 records): an insertion that overlaps nothing is downhill by 0 to 20 (more with more sites: the rings attract), one
# that overlaps a molecule -- a third of them -- is uphill by 40 to 1e11 and rejected whatever the prefactor; a deletion is uphill
# by 0 to 3 at 12 sites, 0.3 to 5 at 24 and 1 to 20 at 40.  So: 12 sites, prefactors near 1/2 (seed 5: 5 insertions and 4 deletions
# accepted, 11 steps rejected); 24 sites, the deletions' prefactor raised four-fold (seed 6: 6 and 4, 10 rejected); 40 sites, forty-
# fold -- N / (0.05 N0) = 20 or more accepts the deletions of up to dE / T = 3, of which seed 6 has four.
PHI = {"12": (0.5, 2.0), "24": (2.0, 0.5), "40": (2.0, 0.05)}
GC_SEED = {"12": 5, "24": 6, "40": 6}
GC_N = {"12": 32, "24": 32, "40": 32}


def _gc_run(b, rep, k, T, recs):
    n = len(recs[1])
    b.chain_run_open(rep, k, T_STEP, R_STEP, T)
    b.chain_run_push_gc(*recs)
    for _ in range((n + 3) // 4):                                # at least n launches: enough whatever is accepted
        b.chain_run_launch(4)
    out = _collect(b, n)
    b.chain_run_close()
    return out


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("name", ["12", "24", "40"])
def test_a_wide_gc_run_is_the_step_by_step_path(name, k):
    """Random by-count records of moves 0-4 (one idle) on charged 12-, 24- and 40-site boxes."""
    s, _ = _box(name)
    N0 = int(s.n_mol[0])
    cap = N0 + 6
    a, b = _pair(s, 1, cap=[cap])
    b.chain_run_set_gc(True)
    assert b.chain_run_capacity()[0] >= 4
    T = float(s.temperature)
    n = GC_N[name]
    recs = _gc_records(np.random.default_rng(GC_SEED[name]), s, 0, n, phi_ins=PHI[name][0] * N0, phi_del=PHI[name][1] * N0)
    recs[1][7] = 0
    o2, w2, v2 = _gc_run(b, 0, k, T, recs)
    o1, w1, v1 = _gc_steps(a, s, 0, 0, cap, recs, T)
    move = recs[1]
    n_ins, n_del = int(((v1 == V_ACC) & (move == 3)).sum()), int(((v1 == V_ACC) & (move == 4)).sum())
    print(f"{name} k={k}: twin accepted {int((v1 == V_ACC).sum())} of {n} ({n_ins} insertions of {int((move == 3).sum())}, "
          f"{n_del} deletions of {int((move == 4).sum())}), rejected {int((v1 == V_REJ).sum())}, launches {b.chain_run_launches()}")
    assert n_ins >= 2 and n_del >= 2 and int((v1 == V_REJ).sum()) >= 1
    assert np.array_equal(v1, v2), (v1, v2)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))
    assert v2[7] == V_IDLE and not np.any(o2[7]) and not np.any(w2[7])
    # an insertion carries the self and intra terms in its new row, a deletion in its old row; what is never written reads as zero
    ins, dele = (move == 3) & (v2 != V_IDLE), (move == 4) & (v2 != V_IDLE)
    assert np.all(w2[ins][:, 3] != 0.0) and np.all(w2[ins][:, 4] != 0.0) and np.all(o2[dele][:, 3] != 0.0) and np.all(o2[dele][:, 4] != 0.0)
    assert not np.any(o2[move == 3][:, [0, 1, 3, 4]]) and not np.any(w2[move == 4][:, [0, 1, 3, 4]])
    assert not np.any(o2[move <= 2][:, 3:]) and not np.any(w2[move <= 2][:, 3:])
    _same_state(a, b, s, 1)
    assert b.num_molecules(0, 0) == N0 + n_ins - n_del
    launches, steps, void, und = b.chain_run_stats()
    assert (launches, steps, und) == (n, n, 0)
    if k == 4:
        assert max(c for _, c in b.chain_run_launches()) > 1
    a.close(); b.close()


@pytest.mark.parametrize("sel_u", [0.0, 0.5, BELOW_ONE])
def test_a_wide_deletion_swaps_with_the_last_molecule(sel_u):
    """m == last (nothing moves) and m != last (the last molecule's 24 sites and frame go into slot m)."""
    s, _ = _box("24")
    N = int(s.n_mol[0])
    a, b = _pair(s, 1, cap=[N + 2])
    b.chain_run_set_gc(True)
    T = float(s.temperature)
    rng = np.random.default_rng(4)
    recs = (np.zeros(2, np.int32), np.array([4, 2], np.int32), rng.uniform(0, 1, (2, 5)), np.array([U_ALWAYS, U_ALWAYS]),
            np.array([sel_u, sel_u]), np.full(2, 1.0))
    before = b.get_molecules(0, 0).copy()
    o2, w2, v2 = _gc_run(b, 0, 4, T, recs)
    m = min(int(sel_u * N), N - 1)
    assert (m == N - 1) == (sel_u == BELOW_ONE)
    o1, w1, v1 = _gc_steps(a, s, 0, 0, N + 2, recs, T)
    assert list(v2) == [V_ACC, V_ACC] and np.array_equal(v1, v2) and np.array_equal(o1, o2) and np.array_equal(w1, w2)
    _same_state(a, b, s, 1)
    after = b.get_molecules(0, 0)
    assert after.shape[0] == N - 1
    if m != N - 1:
        keep = np.arange(N - 1) != min(int(sel_u * (N - 1)), N - 2)   # (the rotation that follows moved one molecule)
        expect = before[:N - 1].copy(); expect[m] = before[N - 1]
        assert np.array_equal(after[keep], expect[keep])
    a.close(); b.close()


def test_the_edges_of_the_count_of_a_wide_type():
    """A 24-site type brought down to 0: by-count moves and deletions do nothing (verdict 5, state unchanged); an insertion into the
    empty type is the farm window's for the same record, bit for bit; refilled to the capacity: an insertion does nothing."""
    s = synth.rigid_adsorbate_box(n_mol=2, n_sites=24, L=26.0, seed=17)
    cap = 3
    a, b = _pair(s, 1, cap=[cap])
    b.chain_run_set_gc(True)
    T = float(s.temperature)
    rng = np.random.default_rng(6)
    #        N: 2  1  0  0  0  0->1 1->2 2->3  3   3
    move = np.array([4, 4, 1, 2, 4, 3, 3, 3, 3, 1], np.int32)
    au = np.array([U_ALWAYS] * 9 + [U_NEVER])
    n = len(move)
    recs = (np.zeros(n, np.int32), move, rng.uniform(0, 1, (n, 5)), au, rng.uniform(0, 1, n), np.full(n, 3.0))
    head = tuple(x[:5] for x in recs)
    tail = tuple(x[5:] for x in recs)
    b.chain_run_open(0, 4, T_STEP, R_STEP, T)
    b.chain_run_push_gc(*head)
    b.chain_run_launch(3)
    # the farm window (its WIDE instance) of the same records on the twin, one step at a time, by count
    rows, counts = [], []
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


def test_a_move_an_insertion_and_a_deletion_of_24_sites_against_the_oracle(refcpu_mod):
    """The rows of an accepted insertion, of an accepted move in the state it leaves and of a deletion from the state after both,
    against oracle.refcpu (ComputeOldEnergy / ComputeNewEnergy, monte_carlo_utils.f90:275-395) within tol_for; the sites the
    device built are read back."""
    from tests.util import tol_for
    s, _ = _box("24")
    N = int(s.n_mol[0])
    a, b = _pair(s, 1, cap=[N + 2])
    b.chain_run_set_gc(True)
    T = float(s.temperature)
    t = np.zeros(3, np.int32); move = np.array([3, 1, 4], np.int32)
    su = np.array([0.0, 0.4, 0.3])
    # (the first seed whose insertion overlaps nothing -- the twin's energies say so: a probability that underflows to 0 with a
    #  draw of 0 lies ON it, and the step would be left undecided)
    for seed in range(9, 30):
        u = np.random.default_rng(seed).uniform(0, 1, (3, 5))
        o, w = a.move_trial([0], [0], [0], [3], u[0:1], T_STEP, R_STEP)
        if abs(float(w[0].sum() - o[0].sum())) / T < 50.0:
            break
    a.close()
    recs = (t, move, u, np.array([U_ALWAYS, U_ALWAYS, U_NEVER]), su, np.full(3, 20.0))
    o2, w2, v2 = _gc_run(b, 0, 4, T, recs)
    assert list(v2) == [V_ACC, V_ACC, V_REJ] and b.num_molecules(0, 0) == N + 1
    mols = b.get_molecules(0, 0)
    mm, md = min(int(0.4 * (N + 1)), N), min(int(0.3 * (N + 1)), N)
    assert mm != N                                               # the move displaced a molecule other than the inserted one
    P = refcpu_mod.RefCPU(s, mol_capacity=N + 2)
    exp_old = np.zeros((3, 5)); exp_new = np.zeros((3, 5))

    def settle():
        e_sys = P.system_energy()
        P.init_amplitude(True)
        P.set_energy_recip(e_sys["recip_coulomb"])
        P.all_fourier_terms()

    e_sys = P.system_energy()
    P.init_amplitude(True)
    P.set_energy_recip(e_sys["recip_coulomb"])
    # the insertion at slot N, where the device appended it
    exp_old[0] = P.old_energy(0, N, 1)[:5]
    P.set_num_residues(0, N + 1)
    P.save_fourier(0, N)
    P.set_molecule(0, N, mols[N][0], mols[N] - mols[N][0][None, :])
    exp_new[0] = P.new_energy(0, N, 1)[:5]
    settle()
    # the move of molecule mm, a trial of that state, to where the device put it
    P.save_fourier(0, mm)
    exp_old[1] = P.old_energy(0, mm, 0)[:5]
    P.set_molecule(0, mm, mols[mm][0], mols[mm] - mols[mm][0][None, :])
    exp_new[1] = P.new_energy(0, mm, 0)[:5]
    settle()
    # the deletion of molecule md from the state after both
    exp_old[2] = P.old_energy(0, md, 2)[:5]
    P.save_fourier(0, md)
    exp_new[2, 2] = P.recip_singlemol(0, md, 2)                  # intended physics: A - S_mol
    for got, ref, what in ((o2, exp_old, "old"), (w2, exp_new, "new")):
        tol = tol_for(*np.ravel(ref), *np.ravel(got))
        err = float(np.max(np.abs(got - ref)))
        print(f"{what}: |run - oracle| = {err:.3e} K (tol {tol:.3e} K)")
        assert err <= tol, (what, got, ref)
    assert exp_new[0, 3] != 0.0 and exp_new[0, 4] != 0.0 and exp_old[2, 4] != 0.0
    b.close()


# ---------------------------------------------------------------------------------------------- undecided steps, neighbours

@pytest.mark.parametrize("accept", [True, False])
def test_an_undecided_wide_move_stalls_the_run_until_it_is_forced(accept):
    """tests/test_gpu_chain_run.py's construction on the 24-site box: one move's draw ON its probability (from the twin's energies),
    the margin opened to 1e-2; the steps behind the forced step go on."""
    s, act = _box("24")
    T = float(s.temperature)
    a, b = _pair(s, 1)
    t, m, move, u, au = _records(np.random.default_rng(17), s, 0, 10)
    au[:] = U_NEVER
    o, w = a.move_trial(np.zeros(10, np.int32), t, m, move, u, T_STEP, R_STEP)
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
    assert stalled_at == st and len(v2) == st + 1 and v2[st] == V_UND and np.all(v2[:st] == V_REJ)
    assert np.array_equal(o2, o[:st + 1]) and np.array_equal(w2, w[:st + 1])
    b.synchronize()
    tags = b.chain_run_launches()
    assert sum(c for _, c in tags) == st and all(c == 0 for f0, c in tags if f0 == st) and tags[-1] == (st, 0)
    _same_state(a, b, s, 1)                                     # nothing committed
    with pytest.raises(_lib.MgpuError):
        b.chain_run_close()
    b.chain_run_force(st, accept)
    b.chain_run_launch(6)
    o3, w3, v3 = _collect(b, 10 - st)
    b.chain_run_close()
    au1 = au.copy()
    au1[st] = U_ALWAYS if accept else U_NEVER
    o1, w1, v1 = _steps(a, s, 0, (t, m, move, u, au1), T, first=st)
    assert v3[0] == (V_ACC if accept else V_REJ) and v3[1] == V_ACC
    assert np.array_equal(v1, v3) and np.array_equal(o1, o3) and np.array_equal(w1, w3)
    _same_state(a, b, s, 1)
    a.close(); b.close()


@pytest.mark.parametrize("accept", [True, False])
def test_an_undecided_wide_insertion_stalls_the_run_until_it_is_forced(accept):
    """tests/test_gpu_chain_run_gcmc.py's construction for an insertion of 24 sites: phi V puts its probability at 0.5 (from the
    twin's energies of the initial state), its draw ON the probability, the margin opened to 1e-2."""
    s, _ = _box("24")
    N = int(s.n_mol[0])
    cap = N + 4
    a, b = _pair(s, 1, cap=[cap])
    b.chain_run_set_gc(True)
    T = float(s.temperature)
    n, st = 6, 2
    t = np.zeros(n, np.int32)
    move = np.array([1, 2, 3, 1, 3, 4], np.int32)
    # (the insertion's five numbers: the first seed whose candidate overlaps nothing, so that phi V stays a finite number)
    for seed in range(17, 40):
        rng = np.random.default_rng(seed)
        u = rng.uniform(0, 1, (n, 5)); su = rng.uniform(0, 1, n)
        o, w = a.move_trial([0], [0], [0], [3], u[st:st + 1], T_STEP, R_STEP)
        d_e = float(w[0].sum() - o[0].sum())
        if np.isfinite(d_e) and abs(d_e / T) < 50.0:
            break
    assert np.isfinite(d_e) and abs(d_e / T) < 50.0
    au = np.full(n, U_NEVER)
    phi_v = np.ones(n)
    phi_v[st] = 0.5 * np.exp(d_e / T) * (N + 1.0)
    phi_v[4] = 20.0 * N; phi_v[5] = N / 20.0
    x = phi_v[st] / (N + 1.0) * np.exp(-d_e / T)
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
    assert w2[st][3] != 0.0 and w2[st][4] != 0.0
    b.synchronize()
    tags = b.chain_run_launches()
    assert tags[0] == (0, st) and tags[1:] == [(st, 0)] * 4      # the launches queued behind it: void
    _same_state(a, b, s, 1)                                     # nothing committed
    with pytest.raises(_lib.MgpuError):
        b.chain_run_close()
    b.chain_run_force(st, accept)
    b.chain_run_launch(n)
    o3, w3, v3 = _collect(b, n - st)
    b.chain_run_close()
    au1 = au.copy()
    au1[st] = U_ALWAYS if accept else U_NEVER
    o1, w1, v1 = _gc_steps(a, s, 0, 0, cap, (t, move, u, au1, su, phi_v), T, first=st)
    assert v3[0] == (V_ACC if accept else V_REJ) and v3[1] == V_ACC
    assert np.array_equal(v1, v3) and np.array_equal(o1, o3) and np.array_equal(w1, w3)
    assert np.array_equal(o3[0], o[0]) and np.array_equal(w3[0], w[0])
    _same_state(a, b, s, 1)
    assert b.num_molecules(0, 0) == a.num_molecules(0, 0)
    a.close(); b.close()


def test_neighbours_of_an_open_wide_run():
    """During a run of the 3 + 24 mixture a synchronous call drains the launches queued so far and sees the committed state, and a
    lane-0 trial is ordered behind them; the results stay collectable (tests/test_gpu_chain_run.py test_blocks_and_neighbours)."""
    s, act = _box("3+24")
    T = float(s.temperature)
    a, b = _pair(s, 2)
    rng = np.random.default_rng(23)
    recs = _mixed_records(rng, s, act, 12)
    b.chain_run_open(1, 4, T_STEP, R_STEP, T)
    b.chain_run_push(*recs)
    b.chain_run_launch(2)
    sf = b.structure_factor(1)                                   # drains the two launches
    done = sum(c for _, c in b.chain_run_launches())
    assert 2 <= done <= 8
    o1, w1, v1 = _steps(a, s, 1, recs, T, first=0, last=done)
    assert np.array_equal(sf, a.structure_factor(1))
    for t in act:
        ca, oa = a.get_frames(1, t); cb, ob = b.get_frames(1, t)
        assert np.array_equal(ca, cb) and np.array_equal(oa, ob)
    probe = _mixed_records(rng, s, [1], 1)                       # a 24-site trial on lane 0 in between: commits nothing
    rep = np.ones(1, np.int32)
    ea = a.move_trial(rep, probe[0], probe[1], probe[2], probe[3], T_STEP, R_STEP)
    eb = b.move_trial(rep, probe[0], probe[1], probe[2], probe[3], T_STEP, R_STEP)
    assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1])
    b.chain_run_launch(12)
    o2, w2, v2 = _collect(b, 12)
    o1b, w1b, v1b = _steps(a, s, 1, recs, T, first=done, last=12)
    assert np.array_equal(np.concatenate([v1, v1b]), v2)
    assert np.array_equal(np.concatenate([o1, o1b]), o2) and np.array_equal(np.concatenate([w1, w1b]), w2)
    b.chain_run_close()
    _same_state(a, b, s, 2)
    assert (v2 == V_ACC).sum() > 0
    a.close(); b.close()
