"""Chain runs (mgpu_chain_run_*, chain_run_kernel): launches of ONE chain queued back to back, each of which reads the step
cursor from device memory, builds and decides the next up to k steps as trials of the state it finds, commits the first
accepted one and advances the cursor.  Every comparison is np.array_equal against a twin engine advanced one step at a time
by the batched device-built path (mgpu_move_trial_decide_submit under MGPU_NO_FROZEN_BATCH=1), itself held to the oracle by
tests/test_gpu_farm.py and tests/test_gpu_parity.py: per-step old / new rows, verdicts, coordinates, frames, counts, A(k).
Reference: src/monte_carlo.f90:40-86, src/monte_carlo_utils.f90:184-226, :275-395."""
import os

import numpy as np
import pytest

from maniac_mc_amd import _lib, synth
from maniac_mc_amd.engine import Engine

pytestmark = pytest.mark.gpu

V_REJ, V_ACC, V_UND, V_IDLE = 0, 1, 2, 5
U_NEVER, U_ALWAYS = 2.0, 0.0          # acceptance draws no probability in (0, 1] leaves open: rejected / accepted
T_STEP, R_STEP = 0.4, 0.4


def _box(name):
    if name == "spce":
        return synth.spce_box(6, seed=3), 0
    if name == "framework":
        return synth.framework_water_box(n_water=12, n_frame=300, L=24.0, seed=7), 1
    return synth.five_site_water_box(), 0


def _twin(s, R):
    """Two engines holding R copies of `s` with resident frames (tests/test_gpu_farm_window.py's twin)."""
    out = []
    os.environ["MGPU_NO_FROZEN_BATCH"] = "1"
    try:
        for _ in range(2):
            e = Engine.from_system(s, n_replicas=R)
            e.load_system(s, 0)
            for t in range(s.topo.n_res):
                if s.topo.is_active[t]:
                    e.set_frames(0, t, s.com[t], s.offsets[t])
            e.init_structure_factor(0, True)
            for r in range(1, R):
                e.replica_copy(r, 0)
            out.append(e)
    finally:
        os.environ.pop("MGPU_NO_FROZEN_BATCH", None)
    return out


def _same_state(a, b, s, R):
    for r in range(R):
        for t in range(s.topo.n_res):
            assert a.num_molecules(r, t) == b.num_molecules(r, t), (r, t)
            assert np.array_equal(a.get_molecules(r, t), b.get_molecules(r, t)), (r, t)
            if s.topo.is_active[t]:
                ca, oa = a.get_frames(r, t)
                cb, ob = b.get_frames(r, t)
                assert np.array_equal(ca, cb) and np.array_equal(oa, ob), (r, t)
        assert np.array_equal(a.structure_factor(r), b.structure_factor(r)), r


def _records(rng, s, t_act, n, idle=()):
    """n NVT records of the active type: (t, m, move, u5, accept_u); steps in `idle` carry move 0."""
    n_mol = int(s.n_mol[t_act])
    m = rng.integers(0, n_mol, n).astype(np.int32)
    move = rng.integers(1, 3, n).astype(np.int32)
    if int(s.topo.atoms_in_res[t_act]) == 1:
        move[:] = 1
    for i in idle:
        move[i] = 0
    return np.full(n, t_act, np.int32), m, move, rng.uniform(0, 1, (n, 5)), rng.uniform(0, 1, n)


def _twin_steps(a, rep, recs, T, t_step=T_STEP, r_step=R_STEP, first=0, last=None):
    """The twin, one step at a time: (old[n,5], new[n,5], verdict[n]) of steps [first, last).  A step whose draw is U_NEVER
    is a FORCED rejection: the batched rule (x >= 1 or u <= x) and the resolvers' (u <= min(1, x)) are the same rule for every
    draw in [0, 1) but not for this one -- a downhill step passes the first before its draw is looked at -- so the twin
    evaluates such a step with the same batched path and commits nothing."""
    t, m, move, u, au = recs
    last = len(m) if last is None else last
    old = np.zeros((last - first, 5)); new = np.zeros((last - first, 5)); v = np.full(last - first, V_IDLE, np.int32)
    for i in range(first, last):
        if move[i] == 0:
            continue
        if au[i] == U_NEVER:
            o, w = a.move_trial([rep], [t[i]], [m[i]], [move[i]], u[i:i + 1], t_step, r_step)
            acc = [0]
        else:
            o, w, acc = a.move_trial_decide([rep], [t[i]], [m[i]], [move[i]], u[i:i + 1], t_step, r_step, au[i:i + 1], [1.0], T)
        a.synchronize()
        old[i - first], new[i - first], v[i - first] = o[0], w[0], V_ACC if acc[0] else V_REJ
    return old, new, v


def _collect(b, n):
    """n steps in order (blocking), as (old, new, verdict)."""
    olds, news, vs = [], [], []
    got = 0
    while got < n:
        o, w, v, st = b.chain_run_collect(n - got, wait=True)
        assert st == -1 and len(v) > 0
        olds.append(o); news.append(w); vs.append(v)
        got += len(v)
    return np.concatenate(olds), np.concatenate(news), np.concatenate(vs)


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("R,rep", [(1, 0), (3, 2)])
@pytest.mark.parametrize("name", ["spce", "framework", "five_site"])
def test_a_run_is_the_step_by_step_path(name, R, rep, k):
    """24 random NVT records (one of them idle), every launch queued -- three at a time -- before anything is collected."""
    s, t_act = _box(name)
    a, b = _twin(s, R)
    max_k, depth, ring = b.chain_run_capacity()
    assert max_k >= 4 and depth >= 24 and ring >= 24
    T = float(s.temperature)
    recs = _records(np.random.default_rng(5), s, t_act, 24, idle=(7,))
    b.chain_run_open(rep, k, T_STEP, R_STEP, T)
    b.chain_run_push(*recs)
    for _ in range(8):                                          # 24 launches: enough whatever is accepted
        b.chain_run_launch(3)
    o2, w2, v2 = _collect(b, 24)
    b.chain_run_close()
    o1, w1, v1 = _twin_steps(a, rep, recs, T)
    print(f"{name} R={R} k={k}: accepted {int((v1 == V_ACC).sum())} of 24, launches {b.chain_run_launches()}")
    assert np.array_equal(v1, v2), (v1, v2)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))
    assert v2[7] == V_IDLE and not np.any(o2[7]) and not np.any(w2[7])
    assert 0 < int((v2 == V_ACC).sum()) < 24
    _same_state(a, b, s, R)
    launches, steps, void, und = b.chain_run_stats()
    assert (launches, steps, und) == (24, 24, 0) and void == 24 - len([c for _, c in b.chain_run_launches() if c])
    if k == 4:
        assert max(c for _, c in b.chain_run_launches()) > 1
    a.close(); b.close()


def test_the_cursor_and_surplus_launches():
    """k = 4, steps 0-7 with verdicts fixed by their draws: the launches' tags show where each started and what it consumed;
    a translation of the molecule the step before it moved sees the committed state; launches past `pushed` do nothing, and a
    later push continues from the same cursor."""
    s, t_act = _box("spce")
    T = float(s.temperature)
    for accept_at, tags in (((1, 5), [(0, 2), (2, 4), (6, 2)]), ((), [(0, 4), (4, 4)])):
        a, b = _twin(s, 1)
        t, m, move, u, au = _records(np.random.default_rng(11), s, t_act, 8)
        au[:] = U_NEVER
        au[list(accept_at)] = U_ALWAYS
        m[2] = m[1]; move[1] = move[2] = 1                       # two consecutive translations of one molecule
        recs = (t, m, move, u, au)
        b.chain_run_open(0, 4, T_STEP, R_STEP, T)
        b.chain_run_push(*recs)
        b.chain_run_launch(len(tags))
        o2, w2, v2 = _collect(b, 8)
        assert b.chain_run_launches() == tags
        o1, w1, v1 = _twin_steps(a, 0, recs, T)
        assert np.array_equal(v1, v2) and [i for i in range(8) if v2[i] == V_ACC] == list(accept_at)
        assert np.array_equal(o1, o2) and np.array_equal(w1, w2)
        if accept_at:
            assert not np.array_equal(o2[2], o2[1])              # (step 2's old row is of the molecule where step 1 put it)
        _same_state(a, b, s, 1)
        # ---- ten launches after the cursor has reached `pushed`
        before = b.chain_run_stats()
        b.chain_run_launch(10)
        b.synchronize()
        after = b.chain_run_stats()
        assert after[0] == before[0] + 10 and after[1] == before[1] and after[2] == before[2] + 10
        assert b.chain_run_launches()[-10:] == [(8, 0)] * 10
        assert b.chain_run_collect(4, wait=False)[2].size == 0
        _same_state(a, b, s, 1)
        # ---- a later push and launch go on from the same cursor
        more = _records(np.random.default_rng(12), s, t_act, 3)
        b.chain_run_push(*more)
        b.chain_run_launch(3)
        o2, w2, v2 = _collect(b, 3)
        o1, w1, v1 = _twin_steps(a, 0, more, T)
        assert np.array_equal(v1, v2) and np.array_equal(o1, o2) and np.array_equal(w1, w2)
        assert b.chain_run_launches()[-3][0] == 8
        b.chain_run_close()
        _same_state(a, b, s, 1)
        a.close(); b.close()


@pytest.mark.parametrize("accept", [True, False])
def test_an_undecided_step_stalls_the_run_until_it_is_forced(accept):
    """One step's draw is put ON its acceptance probability (taken from the twin's energies, 1e-6 < x < 1) and the margin opened
    to 1e-2: the step comes back undecided, the launches queued behind it do nothing and nothing is committed; close is
    refused; after force the run ends in the twin's state, for either decision."""
    s, t_act = _box("spce")
    T = float(s.temperature)
    a, b = _twin(s, 1)
    t, m, move, u, au = _records(np.random.default_rng(17), s, t_act, 10)
    au[:] = U_NEVER
    # the steps up to the chosen one are rejected: each is a trial of the initial state, whose energies the twin gives
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
    assert sum(c for _, c in tags) == st and all(c == 0 for f, c in tags if f == st) and tags[-1] == (st, 0)
    assert b.chain_run_collect(10, wait=False)[3] == st          # nothing more before the decision
    _same_state(a, b, s, 1)                                     # nothing committed
    with pytest.raises(_lib.MgpuError):
        b.chain_run_close()
    with pytest.raises(_lib.MgpuError):
        b.chain_run_force(st + 1, 1)                            # not the step the run waits for
    n_und = b.chain_run_stats()[3]
    assert n_und >= 1
    b.chain_run_force(st, accept)
    b.chain_run_launch(6)
    o3, w3, v3 = _collect(b, 10 - st)
    b.chain_run_close()
    au1 = au.copy()
    au1[st] = U_ALWAYS if accept else U_NEVER
    o1, w1, v1 = _twin_steps(a, 0, (t, m, move, u, au1), T, first=st)
    assert v3[0] == (V_ACC if accept else V_REJ) and v3[1] == V_ACC
    assert np.array_equal(v1, v3) and np.array_equal(o1, o3) and np.array_equal(w1, w3)
    _same_state(a, b, s, 1)
    a.close(); b.close()


def test_blocks_and_neighbours():
    """Close, reopen with other step sizes and run again; between and DURING runs a synchronous call drains the launches queued
    so far and sees the committed state, and a lane-0 trial is ordered behind them; results stay collectable."""
    s, t_act = _box("framework")
    T = float(s.temperature)
    a, b = _twin(s, 2)
    rng = np.random.default_rng(23)
    for block, (ts, rs) in enumerate(((0.4, 0.4), (0.7, 0.25))):
        recs = _records(rng, s, t_act, 12)
        b.chain_run_open(1, 4, ts, rs, T)
        b.chain_run_push(*recs)
        b.chain_run_launch(2)
        # during the run: the state after the two launches, whatever they consumed
        sf = b.structure_factor(1)
        done = sum(c for _, c in b.chain_run_launches())
        assert 2 <= done <= 8
        o1, w1, v1 = _twin_steps(a, 1, recs, T, ts, rs, 0, done)
        assert np.array_equal(sf, a.structure_factor(1))
        ca, oa = a.get_frames(1, t_act); cb, ob = b.get_frames(1, t_act)
        assert np.array_equal(ca, cb) and np.array_equal(oa, ob)
        # a trial on lane 0 in between: evaluated on that state, commits nothing
        probe = _records(rng, s, t_act, 1)
        rep = np.ones(1, np.int32)
        ea = a.move_trial(rep, probe[0], probe[1], probe[2], probe[3], ts, rs)
        eb = b.move_trial(rep, probe[0], probe[1], probe[2], probe[3], ts, rs)
        assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1])
        b.chain_run_launch(12)
        o2, w2, v2 = _collect(b, 12)
        o1b, w1b, v1b = _twin_steps(a, 1, recs, T, ts, rs, done, 12)
        assert np.array_equal(np.concatenate([v1, v1b]), v2)
        assert np.array_equal(np.concatenate([o1, o1b]), o2) and np.array_equal(np.concatenate([w1, w1b]), w2)
        b.chain_run_close()
        _same_state(a, b, s, 2)
        assert (v2 == V_ACC).sum() > 0, block
    with pytest.raises(_lib.MgpuError):
        b.chain_run_launch(1)                                   # no run is open
    a.close(); b.close()


def test_refusals_leave_the_run_usable():
    s, t_act = _box("spce")
    T = float(s.temperature)
    a, b = _twin(s, 1)
    rng = np.random.default_rng(31)
    k_max, depth, ring = b.chain_run_capacity()
    n_mol = int(s.n_mol[t_act])
    good = _records(rng, s, t_act, 6)

    def bad(code, **kw):
        with pytest.raises(_lib.MgpuError) as ei:
            code(**kw)
        return ei.value.code

    b.chain_run_open(0, 2, T_STEP, R_STEP, T)
    for mv in (3, 4):                                            # insertions and deletions do not ride in a run
        t, m, move, u, au = _records(rng, s, t_act, 3)
        move[1] = mv
        bad(lambda: b.chain_run_push(t, m, move, u, au))
    t, m, move, u, au = _records(rng, s, t_act, 3)
    m[2] = n_mol                                                 # a slot >= the count
    bad(lambda: b.chain_run_push(t, m, move, u, au))
    big = _records(rng, s, t_act, ring + 1)                      # beyond the ring
    bad(lambda: b.chain_run_push(*big))
    bad(lambda: b.chain_run_open(0, 2, T_STEP, R_STEP, T))       # a second open
    bad(lambda: b.chain_run_launch(depth + 1))                   # beyond max_in_flight
    # none of them left anything behind: a valid run follows
    b.chain_run_push(*good)
    b.chain_run_launch(6)
    o2, w2, v2 = _collect(b, 6)
    o1, w1, v1 = _twin_steps(a, 0, good, T)
    assert np.array_equal(v1, v2) and np.array_equal(o1, o2) and np.array_equal(w1, w2)
    b.chain_run_close()
    bad(lambda: b.chain_run_open(0, k_max + 1, T_STEP, R_STEP, T))
    bad(lambda: b.chain_run_open(1, 2, T_STEP, R_STEP, T))       # replica out of range
    bad(b.chain_run_close)                                       # nothing open
    good2 = _records(rng, s, t_act, 4)
    b.chain_run_open(0, 2, T_STEP, R_STEP, T)
    b.chain_run_push(*good2)
    b.chain_run_launch(4)
    o2, w2, v2 = _collect(b, 4)
    o1, w1, v1 = _twin_steps(a, 0, good2, T)
    assert np.array_equal(v1, v2) and np.array_equal(o1, o2) and np.array_equal(w1, w2)
    b.chain_run_close()
    _same_state(a, b, s, 1)
    a.close(); b.close()
    # open without frames
    e = Engine.from_system(s, n_replicas=1)
    e.load_system(s, 0)
    e.init_structure_factor(0, True)
    assert e.chain_run_capacity()[0] > 0
    bad(lambda: e.chain_run_open(0, 2, T_STEP, R_STEP, T))
    e.set_frames(0, t_act, s.com[t_act], s.offsets[t_act])
    e.chain_run_open(0, 2, T_STEP, R_STEP, T)
    e.chain_run_close()
    e.close()


def test_capacity_is_zero_where_no_instance_exists():
    """The per-k reciprocal form, a triclinic box (with or without device-built moves) and a 24-site molecule: capacity 0,
    open refused."""
    s, _ = _box("spce")
    os.environ["MGPU_RECIP_PER_K"] = "1"
    try:
        e = Engine.from_system(s, n_replicas=1)
    finally:
        os.environ.pop("MGPU_RECIP_PER_K", None)
    from tests import triclinic_cases as tc
    tri = tc.cell("mild")
    caps = [int(n) + 3 for n in tri.n_mol]
    engines = [e, Engine.from_system(tri, n_replicas=1, mol_capacity=caps),
               Engine.from_system(tri, n_replicas=1, mol_capacity=caps, triclinic_moves=True),
               Engine.from_system(synth.rigid_adsorbate_box(n_mol=6, n_sites=24, seed=17), n_replicas=1)]
    for e in engines:
        assert e.chain_run_capacity() == (0, 0, 0)
        with pytest.raises(_lib.MgpuError):
            e.chain_run_open(0, 1, 0.3, 0.3, 300.0)
        e.close()
