"""The whole resident state of many replicas per call (mgpu_state_export_submit / _wait, mgpu_state_import; Engine.state_export
/ state_import): engines of five replicas holding DIFFERENT configurations -- committed moves, insertions and deletions; counts
of 65, 64, 63, 1 and 0 with the emptied type's slot 0 still holding a frame; reservoirs; a triclinic cell -- export any list in
any order as one block whose every piece is bitwise what the per-replica getters return, the block goes into a SECOND engine
and comes out of it the same bytes, and the two engines then compute the same energies and verdicts.  Everything is compared
with np.array_equal or as bytes: a copy has no tolerance."""
import numpy as np
import pytest

from maniac_mc_amd import synth
from maniac_mc_amd._lib import MGPU_CREATION, MGPU_DELETION, MgpuError
from maniac_mc_amd.engine import STATE_FLAGS, Engine, state_unpack
from tests import triclinic_cases

pytestmark = pytest.mark.gpu

R = 5                       # replicas with their own configurations; replica R is a spare one (the slot order of A(k))
LIST = [3, 0, 4]
MGPU_ERR_INVALID_ARG, MGPU_ERR_CAPACITY, MGPU_ERR_STATE = 1, 3, 5


def _systems(name):
    if name == "spce216":
        return synth.spce_box(6, seed=4), 8
    if name == "co2":
        return synth.co2_box(65, L=40.0, seed=5), 8
    if name == "spce_reservoir":
        return synth.spce_box(4, seed=8, spacing=6.0), 30
    return triclinic_cases.cell("mild"), 6


def _engine(s, extra, tri):
    cap = [int(n) + (extra if s.topo.is_active[t] else 0) for t, n in enumerate(s.n_mol)]
    e = Engine.from_system(s, n_replicas=R + 1, mol_capacity=cap, triclinic_moves=tri)
    for t in range(s.topo.n_res):
        if s.topo.is_active[t]:
            e.set_frames(0, t, s.com[t], s.offsets[t])
    e.init_structure_factor(0, True)
    for r in range(1, R + 1):
        e.replica_copy(r, 0)
    return e


def _forced(eng, rep, move, m, rng):
    """one device-built step per listed replica of type 0, committed whatever its energy"""
    n = len(rep)
    rep = np.asarray(rep, np.int32); move = np.asarray(move, np.int32); m = np.asarray(m, np.int32)
    eng.move_trial(rep, np.zeros(n, np.int32), m, move, rng.uniform(0, 1, (n, 5)), 0.4, 0.4)
    kinds = np.where(move <= 2, 0, np.where(move == 3, MGPU_CREATION, MGPU_DELETION)).astype(np.int32)
    eng.commit_lane(0, rep, np.zeros(n, np.int32), m, kinds, np.ones(n, np.int32))


def _diverge(name, eng, s, rng):
    """replicas 0..4: a translation, a rotation, an insertion, a deletion, a translation; then (co2) deletions down to the
    counts 65, 64, 63, 1, 0.  Returns slot 0's frame of replica 4 as it stood before its last molecule went (co2), else None."""
    N = int(s.n_mol[0])
    if name == "spce_reservoir":
        tmpl = s.offsets[0][0]
        for r in range(R):
            rot = synth._random_rotations(rng, 4 + r)
            eng.set_reservoir(r, 0, np.stack([tmpl @ q.T for q in rot]))
    _forced(eng, [0, 1, 2, 3, 4], [1, 2, 3, 4, 1], [3, 5, 0, 2, 1], rng)
    if name != "co2":
        return None
    want = [65, 64, 63, 1, 0]
    stale = None
    while True:
        now = [eng.num_molecules(r, 0) for r in range(R)]
        todo = [r for r in range(R) if now[r] > want[r]]
        if not todo:
            return stale
        if now[4] == 1:
            com, off = eng.get_frames(4, 0)
            stale = (com[0].copy(), off[0].copy())
        _forced(eng, todo, [4] * len(todo), [0 if now[r] == 1 else 1 for r in todo], rng)


def _slot_of_k(eng):
    """slot of A(k) the engine keeps k-vector k in: read off an export of the spare replica holding A(k) = (k + 1) (1 - i)"""
    k1 = np.arange(1, eng.nk + 1, dtype=np.float64)
    eng.set_structure_factor(k1 - 1j * k1, R)
    A = state_unpack(eng.state_export([R]))[0]["A"]
    slot = np.full(eng.nk, -1)
    for j in np.nonzero(A[:, 0])[0]:
        assert A[j, 1] == -A[j, 0]
        slot[int(A[j, 0]) - 1] = j
    assert np.all(slot >= 0) and len(set(slot.tolist())) == eng.nk
    return slot


_cases = {}


def _case(name):
    """two engines of one system; the first diverged and described by its getters, once per system"""
    if name not in _cases:
        s, extra = _systems(name)
        tri = name == "triclinic"
        a, b = _engine(s, extra, tri), _engine(s, extra, tri)
        stale = _diverge(name, a, s, np.random.default_rng(sum(map(ord, name))))
        _cases[name] = (s, extra, a, b, stale, _slot_of_k(a))
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for c in _cases.values():
        c[2].close(); c[3].close()
    _cases.clear()


def _same_bytes(x, y, what):
    x = np.frombuffer(x, np.uint8); y = np.frombuffer(y, np.uint8)
    if x.shape == y.shape and np.array_equal(x, y):
        return
    k = min(len(x), len(y))
    diff = np.nonzero(x[:k] != y[:k])[0]
    first = int(diff[0]) if len(diff) else k
    raise AssertionError(f"{what}: {len(x)} and {len(y)} bytes, first difference at byte {first} (word {first // 8})")


NAMES = ["spce216", "co2", "spce_reservoir", "triclinic"]


@pytest.mark.parametrize("name", NAMES)
def test_export_is_the_getters_bit_for_bit(name):
    s, extra, a, b, stale, slot = _case(name)
    counts = [[a.num_molecules(r, t) for t in range(s.topo.n_res)] for r in range(R)]
    print(name, "counts", counts)
    assert len({tuple(c) for c in counts}) > 1, "the replicas hold different configurations"
    if name == "co2":
        assert [c[0] for c in counts] == [65, 64, 63, 1, 0]
    block = a.state_export(LIST)
    got = state_unpack(block)
    assert [g["replica"] for g in got] == LIST
    for g, r in zip(got, LIST):
        Ak = a.structure_factor(r)
        assert np.array_equal(g["A"][slot, 0], Ak.real) and np.array_equal(g["A"][slot, 1], Ak.imag), (name, r)
        for t in range(s.topo.n_res):
            n = counts[r][t]
            assert g["n"][t] == n
            assert np.array_equal(g["pos"][t], a.get_molecules(r, t)), (name, r, t)
            if s.topo.is_active[t]:
                com, off = a.get_frames(r, t)
                assert np.array_equal(g["com"][t][:n], com) and np.array_equal(g["off"][t][:n], off), (name, r, t)
                assert g["flags"][t] & STATE_FLAGS["frames_ok"]
            if name == "spce_reservoir" and t == 0:
                res = a.get_reservoir(r, t)
                assert res.shape[0] > 0 and np.array_equal(g["rsv"][t], res), (name, r, t)
                assert g["rsv_cap"][t] >= res.shape[0] + n
            else:
                assert g["rsv"][t] is None
    if name == "co2":
        # the emptied type: slot 0's frame, which a by-count insertion copies, travels although the count is 0
        g4 = got[LIST.index(4)]
        assert g4["n"][0] == 0 and g4["flags"][0] & STATE_FLAGS["frames_held"] and g4["off"][0].shape[0] == 1
        assert np.array_equal(g4["com"][0][0], stale[0]) and np.array_equal(g4["off"][0][0], stale[1])
    if name == "spce_reservoir":
        assert len({g["rsv"][0].shape[0] for g in got}) > 1, "reservoirs of different counts"


@pytest.mark.parametrize("name", NAMES)
def test_one_call_is_the_calls_of_one_replica(name):
    s, extra, a, b, stale, slot = _case(name)
    block = a.state_export(LIST)
    w = np.frombuffer(block, np.int64)
    reps_at = 8 + 12 + 2 * s.topo.n_res
    starts = [int(w[reps_at + 2 * i + 1]) for i in range(len(LIST))] + [int(w[5])]
    for i, r in enumerate(LIST):
        one = a.state_export([r])
        w1 = np.frombuffer(one, np.int64)
        _same_bytes(block[8 * starts[i]: 8 * starts[i + 1]], one[8 * int(w1[8 + 12 + 2 * s.topo.n_res + 1]):], f"{name}: replica {r}")


@pytest.mark.parametrize("name", NAMES)
def test_import_into_a_second_engine_and_out_again(name):
    s, extra, a, b, stale, slot = _case(name)
    N = int(s.n_mol[0])
    block = a.state_export(LIST)
    before = b.state_export([1, 2])
    b.state_import(LIST, block)
    _same_bytes(b.state_export(LIST), block, f"{name}: list {LIST}")
    _same_bytes(b.state_export([1, 2]), before, f"{name}: the replicas not listed")
    everything = a.state_export(list(range(R)))
    b.state_import(list(range(R)), everything)
    _same_bytes(b.state_export(list(range(R))), everything, f"{name}: all replicas")
    for r in range(R):
        assert [b.num_molecules(r, t) for t in range(s.topo.n_res)] == [a.num_molecules(r, t) for t in range(s.topo.n_res)]
    # identical records on both engines: one batched trial, then one farm window (decided and committed on the device)
    rng = np.random.default_rng(17)
    n_now = np.array([a.num_molecules(r, 0) for r in range(R)])
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    move = np.where(n_now == 0, 3, 1).astype(np.int32)
    m = np.where(n_now == 0, 0, np.minimum(1, n_now - 1)).astype(np.int32)
    u = rng.uniform(0, 1, (R, 5))
    ea, eb = a.move_trial(rep, tt, m, move, u, 0.4, 0.4), b.move_trial(rep, tt, m, move, u, 0.4, 0.4)
    assert np.array_equal(ea[0], eb[0]) and np.array_equal(ea[1], eb[1]), (name, ea, eb)
    move = np.array([1, 2, 4, 3, 3], np.int32)
    m = np.where(move == 3, 0, np.minimum(1, np.maximum(n_now - 1, 0))).astype(np.int32)
    u = rng.uniform(0, 1, (R, 5))
    au = rng.uniform(0, 1, R) ** 3
    pref = np.ones(R)
    pref[move == 3] = N / (n_now[move == 3] + 1.0)
    pref[move == 4] = n_now[move == 4] / float(N)
    out = []
    for e in (a, b):
        e.farm_window_submit(rep, tt, m, move, u, 0.5, 0.5, au, pref, float(s.temperature))
        out.append(e.farm_window_wait(R))
    print(name, "window verdicts", out[0][2], out[1][2])
    for x, y in zip(out[0], out[1]):
        assert np.array_equal(x, y), (name, out)
    _same_bytes(b.state_export(list(range(R))), a.state_export(list(range(R))), f"{name}: after the window")


def test_refusals():
    s, extra, a, b, stale, slot = _case("co2")
    block = a.state_export([2])
    keep = b.state_export(list(range(R)))
    with pytest.raises(MgpuError) as err:                        # a replica listed twice, either way
        a.state_export([1, 1])
    assert err.value.code == MGPU_ERR_INVALID_ARG
    with pytest.raises(MgpuError) as err:
        b.state_import([1, 1], a.state_export([1, 2]))
    assert err.value.code == MGPU_ERR_INVALID_ARG
    with pytest.raises(MgpuError) as err:                        # more replicas listed than the block holds
        b.state_import([1, 2], block)
    assert err.value.code == MGPU_ERR_INVALID_ARG
    with pytest.raises(MgpuError) as err:                        # a truncated block
        b.state_import([2], block[:-16])
    assert err.value.code == MGPU_ERR_INVALID_ARG
    # another capacity, another topology, another box
    c = _engine(s, extra + 1, False)
    with pytest.raises(MgpuError) as err:
        c.state_import([2], block)
    assert err.value.code == MGPU_ERR_CAPACITY
    c.close()
    s2, extra2, a2, b2, _, _ = _case("triclinic")
    with pytest.raises(MgpuError) as err:
        b2.state_import([2], block)
    assert err.value.code in (MGPU_ERR_INVALID_ARG, MGPU_ERR_CAPACITY)
    s3 = synth.co2_box(65, L=41.0, seed=5)
    c = _engine(s3, extra, False)
    with pytest.raises(MgpuError) as err:
        c.state_import([2], block)
    assert err.value.code == MGPU_ERR_INVALID_ARG
    c.close()
    # while a window of the replica is in flight
    one = np.zeros(1, np.int32)
    b.farm_window_submit(one + 3, one, one, one + 1, np.full((1, 5), 0.5), 0.3, 0.3, np.ones(1), np.ones(1), float(s.temperature))
    with pytest.raises(MgpuError) as err:
        b.state_import([3], block)
    assert err.value.code == MGPU_ERR_STATE
    b.state_import([2], block)                                   # another replica's import goes through beside it
    b.farm_window_wait(1)
    # nothing was written by any refused call (replica 2 was imported just now, replica 3 took the window's step)
    now = state_unpack(b.state_export(list(range(R))))
    was = state_unpack(keep)
    for r in (0, 1, 4):
        assert np.array_equal(now[r]["pos"][0], was[r]["pos"][0]) and np.array_equal(now[r]["A"], was[r]["A"])
    _same_bytes(b.state_export([2]), block, "the import beside the window")
