"""Farm windows for rigid molecules of 6 to 63 sites in a TRICLINIC box (farm_window_kernel<false, false, true, RSV, true>, DESIGN
section 4.4; mgpu_farm_set_wide_triclinic beside mgpu_set_triclinic_moves): capacity by the switches, then energies, verdicts and
committed state (coordinates, frames, counts, reservoirs, A(k)) held bit for bit to the batched device-built path for these
molecules in such a box -- mgpu_move_trial_submit, the host's rule, mgpu_commit_submit, which tests/test_gpu_wide_triclinic_twin.py
holds to the oracle -- for NVT windows, by-count insertion / deletion windows, reservoirs, the undecided protocol and a translation
across a face of the wrap cell; one move, one insertion and one deletion of 24 sites per cell, and insertions placed on a
neighbour's far image, against the oracle directly.  The cells and sizes are tests/test_gpu_chain_wide_triclinic.py's (the mild
tilt; the sheared cell, where the full 27-image search runs; 6, 24, 40 sites and the 3 + 24 mixture).  R = 4 chains, and R = 70:
beyond kFarmInline the records travel in pinned memory and pair workgroups serve several chains.
Energy comparisons are unconditional; a verdict comparison leaves out only steps the host's rule puts within the margin of the
draw, and the seeds below leave none (asserted).  No comparison draws again; draws repeated while inputs are built are counted and
printed (print_redraws).
Reference: src/monte_carlo.f90:40-86, src/monte_carlo_utils.f90:184-226, :275-395, src/create_molecule.f90:180-200,
src/delete_molecule.f90:100-142, src/energy_utils.f90:374-442, src/geometry_utils.f90:167-220, :359-415."""
import numpy as np
import pytest

from maniac_mc_amd import _lib, synth
from maniac_mc_amd.engine import Engine, box_prepare
from tests import triclinic_cases as tc
from tests.test_gpu_chain_run_wide_triclinic import _at_a_face_of_the_wrap_cell
from tests.test_gpu_chain_wide_triclinic import MILD, _images, print_redraws, redrawn, tri_box  # noqa: F401  (print_redraws: autouse)
from tests.test_gpu_farm_window_wide import V_ACC, V_IDLE, V_REJ, V_STALLED, V_UND, _batched_step, _box, _env
from tests.test_gpu_triclinic_moves import _kinds
from tests.test_gpu_wide_triclinic_twin import FAR_IMAGE_DIST, _far_image_insertions
from tests.util import tol_for

pytestmark = pytest.mark.gpu

CELLS = ("mild", "sheared")
T_STEP = R_STEP = 0.5


def _twin(s, R, cap, env=None):
    """The batched engine and the window engine: R copies of `s`, resident frames, device-built triclinic moves on both and the
    farm's switch on the second."""
    out = []
    with _env(**(env or {})):
        for _ in range(2):
            e = Engine.from_system(s, n_replicas=R, mol_capacity=cap, triclinic_moves=True)
            e.load_system(s, 0)
            for t in range(s.topo.n_res):
                e.set_frames(0, t, s.com[t], s.offsets[t])
            e.init_structure_factor(0, True)
            for r in range(1, R):
                e.replica_copy(r, 0)
            out.append(e)
    a, b = out
    b.farm_set_wide_triclinic(True)
    assert b.farm_window_capacity()[0] == R and a.farm_window_capacity()[0] == 0
    return a, b


def _same_state(a, b, s, R):
    for r in range(R):
        for t in range(s.topo.n_res):
            assert a.num_molecules(r, t) == b.num_molecules(r, t), (r, t)
            assert np.array_equal(a.get_molecules(r, t), b.get_molecules(r, t)), (r, t)
            if a.num_molecules(r, t):
                ca, oa = a.get_frames(r, t)
                cb, ob = b.get_frames(r, t)
                assert np.array_equal(ca, cb) and np.array_equal(oa, ob), (r, t)
            assert np.array_equal(a.get_reservoir(r, t), b.get_reservoir(r, t)), (r, t)
        assert np.array_equal(a.structure_factor(r), b.structure_factor(r)), r


def _forced_step(a, rep, tt, m, move, u, accept):
    """the twin's step with the decision given: (old, new)"""
    o, w = a.move_trial(rep, tt, m, move, u, T_STEP, R_STEP)
    a.commit_lane(0, rep, tt, m, _kinds(move), np.asarray(accept, np.int32))
    return o, w


def _refused(call):
    with pytest.raises(_lib.MgpuError) as ei:
        call()
    assert ei.value.code == 5, ei.value                          # MGPU_ERR_STATE
    return str(ei.value)


# ---------------------------------------------------------------------------------------------- 1. the switch matrix

def test_capacity_follows_the_switches():
    """0 with device-built moves alone (as it always was) and with the new switch alone, min(kFarmMaxChains, R) with both, 0 again
    when device-built moves go off; the single-chain switch gives the farm nothing and the farm's gives the single-chain paths
    nothing; a window in flight holds the switch on."""
    R = 3
    for name, cell in (("6", "mild"), ("24", "mild"), ("40", "sheared"), ("3+24", "mild"), ("3+24", "sheared")):
        s, act, cap = tri_box(name, cell)
        assert s.is_triclinic()
        e = Engine.from_system(s, n_replicas=R, mol_capacity=cap)
        wide_t = act[-1]
        u = np.full((R, 5), 0.5)
        submit = lambda: e.farm_window_submit(np.arange(R), [wide_t] * R, [0] * R, [1] * R, u, 0.4, 0.4, [0.5] * R, [1.0] * R, 300.0)
        assert e.farm_window_capacity()[0] == 0, (name, cell)
        e.farm_set_wide_triclinic(True)
        assert e.farm_window_capacity()[0] == 0, (name, cell)        # the new switch alone admits nothing
        assert "not available" in _refused(submit)
        e.farm_set_wide_triclinic(False)
        e.set_triclinic_moves(True)
        assert e.farm_window_capacity()[0] == 0, (name, cell)        # today's value
        assert "not available" in _refused(submit)
        e.farm_set_wide_triclinic(True)
        assert e.farm_window_capacity()[0] == R, (name, cell)          # min(kFarmMaxChains, R)
        assert e.recip_form(int(s.topo.atoms_in_res[wide_t]))["form"] in ("rows", "wide-vector", "wide-mfma")
        e.set_triclinic_moves(False)
        assert e.farm_window_capacity()[0] == 0, (name, cell)
        e.set_triclinic_moves(True)
        assert e.farm_window_capacity()[0] == R, (name, cell)
        # the two switches are each path's own
        e.farm_set_wide_triclinic(False)
        e.chain_set_wide_triclinic(True)
        e.chain_set_wide(True)
        assert e.farm_window_capacity()[0] == 0 and e.chain_window_capacity() >= 8, (name, cell)
        e.chain_set_wide_triclinic(False)
        e.farm_set_wide_triclinic(True)
        assert e.farm_window_capacity()[0] == R and e.chain_window_capacity() == 0, (name, cell)
        e.chain_run_set_triclinic(True)
        assert "mgpu_chain_set_wide_triclinic" in _refused(lambda: e.chain_run_set_wide(True))
        assert e.chain_run_capacity()[0] == 0, (name, cell)
        e.close()
    # an orthorhombic engine refuses the switch by name, either way, and keeps its WIDE farm windows
    e = Engine.from_system(_box("24")[0], n_replicas=2)
    assert e.farm_window_capacity()[0] == 2
    for on in (True, False):
        assert "farm_set_wide_triclinic: the box is orthorhombic" in _refused(lambda: e.farm_set_wide_triclinic(on))
    assert e.farm_window_capacity()[0] == 2
    e.close()
    # the per-k form and a site-major type keep 0 with every switch on
    big = synth.large_adsorbate_box()
    big.box_matrix[1, 0], big.box_matrix[2, 0], big.box_matrix[2, 1] = MILD
    with _env(MGPU_RECIP_PER_K="1"):
        per_k = Engine.from_system(tri_box("24", "mild")[0], n_replicas=2, triclinic_moves=True)
    assert per_k.recip_form(24)["form"] == "per-k"
    for e in (Engine.from_system(big, n_replicas=2, triclinic_moves=True), per_k):
        e.farm_set_wide_triclinic(True)
        e.chain_set_wide_triclinic(True)
        e.chain_set_wide(True)
        assert e.farm_window_capacity()[0] == 0
        e.close()
    # switching off is refused while a window is uncollected; switching on (again) is not
    s, act, cap = tri_box("24", "mild")
    a, b = _twin(s, R, cap)
    rep = np.arange(R, dtype=np.int32)
    u = np.random.default_rng(1).uniform(0, 1, (R, 5))
    b.farm_window_submit(rep, [0] * R, [1] * R, [1] * R, u, T_STEP, R_STEP, [0.5] * R, [1.0] * R, 300.0)
    assert "farm window is in flight" in _refused(lambda: b.farm_set_wide_triclinic(False))
    assert b.farm_window_capacity()[0] == R
    b.farm_set_wide_triclinic(True)
    o2, w2, v = b.farm_window_wait(R)
    o1, w1, yes, near = _batched_step(a, rep, np.zeros(R, np.int32), np.ones(R, np.int32), np.ones(R, np.int32), u, T_STEP, R_STEP,
                                      np.full(R, 0.5), np.ones(R), 300.0)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2) and not near.any() and np.array_equal(v == V_ACC, yes)
    b.farm_set_wide_triclinic(False)
    assert b.farm_window_capacity()[0] == 0
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 2. NVT windows

NVT_CASES = [("6", "mfma"), ("24", "mfma"), ("24", "vector"), ("40", "mfma"), ("3+24", "mfma")]


@pytest.mark.parametrize("R", [4, 70])
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name,form", NVT_CASES)
def test_nvt_windows_are_the_batched_steps(name, form, cell, R):
    """Two windows in flight, three rounds: old and new rows of five components array_equal to the batched device-built step,
    verdicts the host's rule, coordinates, frames and A(k) array_equal after every round.  MGPU_RECIP_NO_MFMA=1 covers the vector
    wide form, without it the matrix-unit form."""
    s, act, cap = tri_box(name, cell)
    a, b = _twin(s, R, cap, env={"MGPU_RECIP_NO_MFMA": "1" if form == "vector" else None})
    f = b.recip_form(max(int(s.topo.atoms_in_res[t]) for t in act))["form"]
    if name != "6":
        assert f == ("wide-vector" if form == "vector" else "wide-mfma"), f
    rng = np.random.default_rng(5 + R)
    rep = np.arange(R, dtype=np.int32)
    T = float(s.temperature)
    n_acc = n_near = 0
    sizes = set()
    for step in range(3):
        recs = []
        for _ in range(2):
            tt = rng.choice(act, R).astype(np.int32)
            m = np.array([rng.integers(0, int(s.n_mol[t])) for t in tt], np.int32)
            move = rng.integers(1, 3, R).astype(np.int32)
            u = rng.uniform(0, 1, (R, 5)); au = rng.uniform(0, 1, R)
            recs.append((tt, m, move, u, au))
            sizes.update(int(s.topo.atoms_in_res[t]) for t in tt)
            b.farm_window_submit(rep, tt, m, move, u, T_STEP, R_STEP, au, np.ones(R), T)
        for tt, m, move, u, au in recs:
            o1, w1, yes, near = _batched_step(a, rep, tt, m, move, u, T_STEP, R_STEP, au, np.ones(R), T)
            o2, w2, v = b.farm_window_wait(R)
            assert np.array_equal(o1, o2) and np.array_equal(w1, w2), (step, np.max(np.abs(o1 - o2)), np.max(np.abs(w1 - w2)))
            n_near += int(near.sum())
            assert np.all((v == V_ACC) | (v == V_REJ)) and np.array_equal((v == V_ACC)[~near], yes[~near])
            n_acc += int(yes.sum())
        _same_state(a, b, s, R)
    print(f"{name} {form} {cell} R {R}: accepted {n_acc} of {6 * R}, within the margin {n_near}")
    assert n_near == 0 and n_acc > 0
    assert len(sizes) == len(act)                                # (the mixture: narrow and WIDE rows in one launch)
    assert b.farm_window_stats() == (6, 0)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 3. by-count windows

# phi V of the insertion and of the deletion records in units of the initial count (tests/test_gpu_chain_run_wide_triclinic.py's
# for these molecules: the deletions' prefactor raised to meet their cost)
PHI = (2.0, 0.05)


def _by_count_round(a, b, s, R, t, cap, rng, T, seen, reservoir=False):
    """two by-count windows of type t queued on b, then collected against a's batched steps run one after the other with the slot
    and the prefactor a's counts give; -> steps within the margin"""
    rep = np.arange(R, dtype=np.int32)
    tt = np.full(R, t, np.int32)
    N0 = float(s.n_mol[t])
    recs, n_near = [], 0
    for _ in range(2):
        move = rng.integers(1, 5, R).astype(np.int32)
        move[rng.random(R) < 0.5] = rng.choice([3, 4])
        u = rng.uniform(0, 1, (R, 5)); au = rng.uniform(0, 1, R) ** 3; su = rng.uniform(0, 1, R)
        pv = np.where(move == 3, PHI[0] * N0, np.where(move == 4, PHI[1] * N0, 1.0))
        recs.append((move, u, au, su, pv))
        b.farm_window_submit(rep, tt, np.zeros(R, np.int32), move, u, T_STEP, R_STEP, au, pv, T, slot_u=su)
    for move, u, au, su, pv in recs:
        o2, w2, v = b.farm_window_wait(R)
        n_now = np.array([a.num_molecules(r, t) for r in range(R)])
        live = np.where(move == 3, n_now < cap, n_now > 0)
        if reservoir:                                            # an insertion from an empty reservoir does nothing
            live &= ~((move == 3) & np.array([a.get_reservoir(r, t).shape[0] == 0 for r in range(R)]))
        m = np.minimum((su * n_now).astype(np.int32), np.maximum(n_now - 1, 0)).astype(np.int32)
        pref = np.ones(R)
        pref[move == 3] = pv[move == 3] / (n_now[move == 3] + 1.0)
        pref[move == 4] = ((n_now[move == 4] - 1.0) + 1.0) / pv[move == 4]
        assert np.all(v[~live] == V_IDLE) and not np.any(o2[~live]) and not np.any(w2[~live])
        if live.any():
            with np.errstate(over="ignore"):                     # (an insertion wherever its draw lands: exp may overflow to inf)
                o1, w1, yes, near = _batched_step(a, rep[live], tt[live], m[live], move[live], u[live], T_STEP, R_STEP, au[live], pref[live], T)
            assert np.array_equal(o1, o2[live]) and np.array_equal(w1, w2[live]), (np.max(np.abs(o1 - o2[live])), np.max(np.abs(w1 - w2[live])))
            n_near += int(near.sum())
            vl = v[live]
            assert np.all((vl == V_ACC) | (vl == V_REJ)) and np.array_equal((vl == V_ACC)[~near], yes[~near])
        seen.update((int(mv), int(vv)) for mv, vv in zip(move, v))
    _same_state(a, b, s, R)
    return n_near


@pytest.mark.parametrize("R", [4, 70])
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", ["24", "40"])
def test_by_count_windows_are_the_batched_steps(name, cell, R):
    """Insertions, deletions and moves by count, two windows in flight: the slot and the prefactor follow from the count the
    launch finds, which is the twin's; energies (five components), verdicts, counts, coordinates, frames and A(k)."""
    s, _, cap = tri_box(name, cell)
    a, b = _twin(s, R, cap)
    rng = np.random.default_rng(21 + R)
    seen = set()
    n_near = 0
    for rnd in range(3 if R > 8 else 8):
        n_near += _by_count_round(a, b, s, R, 0, cap[0], rng, float(s.temperature), seen)
    print(f"{name} {cell} R {R}: (move, verdict) seen {sorted(seen)}, within the margin {n_near}")
    assert n_near == 0
    assert {(3, V_ACC), (4, V_ACC)} <= seen
    a.close(); b.close()


@pytest.mark.parametrize("R", [4, 70])
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", ["24", "40"])
def test_the_edges_of_the_count_the_slots_and_the_inserted_centre(name, cell, R):
    """By-count records with the decision given, so that every chain walks the same path: deletion of the last, the first and a
    middle slot (the swap with the last molecule); the type emptied -- a deletion and a move of the empty type do nothing, verdict 5
    -- then refilled to capacity at fractions on and next to the cell's faces -- the inserted centre is lo + box%matrix u in the
    oracle's order, bit for bit, and an insertion into the full type does nothing, verdict 5.  Rows and state are the twin's."""
    s, _, cap = tri_box(name, cell)
    cap0 = cap[0]
    a, b = _twin(s, R, cap)
    rng = np.random.default_rng(7)
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    T = float(s.temperature)
    N = int(s.n_mol[0])
    ones = np.ones(R, np.int32)

    def window(move, su, u=None):
        """one by-count window, every step accepted by fiat: the records that did something, against the twin"""
        move = np.full(R, move, np.int32)
        u = rng.uniform(0, 1, (R, 5)) if u is None else u
        n_now = np.array([a.num_molecules(r, 0) for r in range(R)])
        b.farm_window_submit(rep, tt, np.zeros(R, np.int32), move, u, T_STEP, R_STEP, np.full(R, 0.5), np.ones(R), T, forced=ones, slot_u=su)
        o2, w2, v = b.farm_window_wait(R)
        live = np.where(move == 3, n_now < cap0, n_now > 0)
        m = np.minimum((su * n_now).astype(np.int32), np.maximum(n_now - 1, 0)).astype(np.int32)
        assert np.all(v[~live] == V_IDLE) and not np.any(o2[~live]) and not np.any(w2[~live])
        assert np.all(v[live] == V_ACC)
        if live.any():
            o1, w1 = _forced_step(a, rep[live], tt[live], m[live], move[live], u[live], ones[live])
            assert np.array_equal(o1, o2[live]) and np.array_equal(w1, w2[live]), (np.max(np.abs(o1 - o2[live])), np.max(np.abs(w1 - w2[live])))
        _same_state(a, b, s, R)
        return m, v

    # the last, the first, a middle slot, by chain
    before = [b.get_molecules(r, 0).copy() for r in range(R)]
    want = np.array([(N - 1, 0, N // 2)[r % 3] for r in range(R)])
    m, _ = window(4, (want + 0.5) / N)
    assert np.array_equal(m, want)
    for r in range(R):
        now = b.get_molecules(r, 0)
        assert b.num_molecules(r, 0) == N - 1
        if want[r] != N - 1:
            assert np.array_equal(now[want[r]], before[r][N - 1]), r             # the swap with the last molecule
        keep = [k for k in range(N - 1) if k != want[r]]
        assert np.array_equal(now[keep], before[r][keep]), r
    # emptied
    for _ in range(N - 1):
        window(4, rng.uniform(0, 1, R))
    assert all(b.num_molecules(r, 0) == 0 for r in range(R))
    for move in (4, 1, 2):
        _, v = window(move, rng.uniform(0, 1, R))
        assert np.all(v == V_IDLE)
    # refilled to capacity: every centre at fractions on and next to the faces.  Per axis the fraction is one of three classes -- a
    # face (0, 1e-17, 1e-16 or 1 - 1e-16: one place of the periodic cell), 1/4, 1/2 -- and a chain's insertions take distinct triples
    # of classes, so that no two of its molecules are put on the same spot (coincident sites have no finite energy to compare)
    face = np.array([0.0, 1e-17, 1e-16, 1.0 - 1e-16])
    triples = np.array([[i, j, k] for i in range(3) for j in range(3) for k in range(3)])
    order = np.array([rng.permutation(len(triples)) for _ in range(R)])
    assert cap0 <= len(triples)
    for k in range(cap0):
        u = rng.uniform(0, 1, (R, 5))
        cls = triples[order[:, k]]
        u[:, :3] = np.where(cls == 0, face[rng.integers(0, len(face), (R, 3))], np.where(cls == 1, 0.25, 0.5))
        window(3, rng.uniform(0, 1, R), u)
        for r in range(R):
            com, _ = b.get_frames(r, 0)
            assert np.array_equal(com[k], tc.cart(s, u[r, :3])), (k, r, com[k] - tc.cart(s, u[r, :3]))
    assert all(b.num_molecules(r, 0) == cap0 for r in range(R))
    _, v = window(3, rng.uniform(0, 1, R))
    assert np.all(v == V_IDLE)
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 4. reservoirs

@pytest.mark.parametrize("R", [4, 70])
@pytest.mark.parametrize("cell", CELLS)
def test_reservoir_windows_are_the_batched_steps(cell, R):
    """The 24-site type holds a reservoir on every chain (the RSV instance): an insertion copies the picked reservoir molecule and
    takes it out, a deletion appends the box's last molecule, box count + reservoir count is conserved, an insertion from the empty
    reservoir does nothing (verdict 5); rows, verdicts, state and the reservoirs themselves are the batched steps'."""
    s, _, _ = tri_box("24", cell)
    N = int(s.n_mol[0])
    cap = [N + 5]
    a, b = _twin(s, R, cap)
    rng = np.random.default_rng(31 + R)
    res = np.stack([s.offsets[0][0] @ synth._random_rotations(rng, 1)[0].T for _ in range(3)])
    for e in (a, b):
        for r in range(R):
            e.set_reservoir(r, 0, res)
    assert b.farm_window_capacity()[0] == R
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    T = float(s.temperature)
    ones = np.ones(R, np.int32)
    zeros = np.zeros(R, np.int32)
    # the reservoir drawn empty by fiat, every pick read back
    for k in range(3):
        u = rng.uniform(0, 1, (R, 5))
        before = [b.get_reservoir(r, 0).copy() for r in range(R)]
        b.farm_window_submit(rep, tt, zeros, np.full(R, 3, np.int32), u, T_STEP, R_STEP, np.full(R, 0.5), np.ones(R), T, forced=ones,
                             slot_u=rng.uniform(0, 1, R))
        o2, w2, v = b.farm_window_wait(R)
        assert np.all(v == V_ACC)
        o1, w1 = _forced_step(a, rep, tt, zeros, np.full(R, 3, np.int32), u, ones)
        assert np.array_equal(o1, o2) and np.array_equal(w1, w2)
        _same_state(a, b, s, R)
        for r in range(R):
            com, off = b.get_frames(r, 0)
            pick = min(int(u[r, 3] * (3 - k)), 3 - k - 1)
            assert np.array_equal(off[N + k], before[r][pick]) and np.array_equal(com[N + k], tc.cart(s, u[r, :3])), (k, r)
            assert b.num_molecules(r, 0) + b.get_reservoir(r, 0).shape[0] == N + 3
    assert all(b.get_reservoir(r, 0).shape[0] == 0 and b.num_molecules(r, 0) == N + 3 < cap[0] for r in range(R))
    b.farm_window_submit(rep, tt, zeros, np.full(R, 3, np.int32), rng.uniform(0, 1, (R, 5)), T_STEP, R_STEP, np.full(R, 0.5), np.ones(R), T,
                         slot_u=rng.uniform(0, 1, R))
    o2, w2, v = b.farm_window_wait(R)
    assert np.all(v == V_IDLE) and not np.any(o2) and not np.any(w2)
    _same_state(a, b, s, R)
    # by the rule
    seen = set()
    n_near = 0
    for rnd in range(3 if R > 8 else 8):
        n_near += _by_count_round(a, b, s, R, 0, cap[0], rng, T, seen, reservoir=True)
        for r in range(R):
            assert b.num_molecules(r, 0) + b.get_reservoir(r, 0).shape[0] == N + 3, r
    print(f"24 {cell} R {R}: (move, verdict) seen {sorted(seen)}, within the margin {n_near}")
    assert n_near == 0
    assert {(3, V_ACC), (4, V_ACC)} <= seen
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 5. undecided and forced

def _free_fraction(rng, s, clearance=5.5):
    """fractions u of a point lo + M u at least `clearance` from every site of the start, over the 27 images"""
    M = np.asarray(s.box_matrix, dtype=np.float64)
    atoms = np.concatenate([(s.com[t][:, None, :] + s.offsets[t]).reshape(-1, 3) for t in range(s.topo.n_res)])
    shifts = _images(M)
    for _ in range(20000):
        f = rng.uniform(0.05, 0.95, 3)
        d = (atoms - tc.cart(s, f))[:, None, :] + shifts[None, :, :]
        if np.min(np.linalg.norm(d, axis=2)) > clearance:
            return f
        redrawn("free spot")
    raise AssertionError("no free spot")


@pytest.mark.parametrize("R", [4, 70])
@pytest.mark.parametrize("cell", CELLS)
def test_an_undecided_move_stalls_its_chain_until_the_host_decides(cell, R):
    """The margin raised to 1e-6 and every draw put 1e-7 (relative) above its probability of 0.3: every move comes back undecided
    (verdict 2) with its rows and nothing committed, the window queued behind it does nothing (verdict 4); the host's decision --
    accept on the even chains, reject on the odd ones -- is obeyed, and the next window, under the default margin, builds on the
    state the decisions left."""
    s, _, cap = tri_box("24", cell)
    a, b = _twin(s, R, cap)
    rng = np.random.default_rng(2)
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    T = float(s.temperature)
    N = int(s.n_mol[0])
    recs = [(rng.integers(0, N, R).astype(np.int32), rng.integers(1, 3, R).astype(np.int32), rng.uniform(0, 1, (R, 5))) for _ in range(2)]
    m, move, u = recs[0]
    # (the margin is relative, so a step whose Boltzmann factor underflows -- a move into an overlap: the sheared start has
    #  molecules wedged against a neighbour -- cannot be put at a probability of 0.3: such records are drawn again, from the twin's
    #  trial alone, which leaves its state as it is)
    for _ in range(50):
        o, w = a.move_trial(rep, tt, m, move, u, T_STEP, R_STEP)
        with np.errstate(over="ignore"):
            boltz = np.exp(-(w.sum(1) - o.sum(1)) / T)
        bad = ~((boltz > 1e-6) & (boltz < 1e6))
        if not bad.any():
            break
        redrawn("move into an overlap", int(bad.sum()))
        m[bad], move[bad], u[bad] = rng.integers(0, N, int(bad.sum())), rng.integers(1, 3, int(bad.sum())), rng.uniform(0, 1, (int(bad.sum()), 5))
    assert not bad.any(), "no move with a finite Boltzmann factor found"
    pref = 0.3 / boltz
    au = np.full(R, 0.3 * (1.0 + 1e-7))
    b.chain_set_margin(1e-6)
    b.farm_window_submit(rep, tt, m, move, u, T_STEP, R_STEP, au, pref, T)
    b.farm_window_submit(rep, tt, recs[1][0], recs[1][1], recs[1][2], T_STEP, R_STEP, np.full(R, 0.5), np.ones(R), T)
    o2, w2, v = b.farm_window_wait(R)
    assert np.all(v == V_UND) and np.array_equal(o2, o) and np.array_equal(w2, w)
    _, _, v = b.farm_window_wait(R)
    assert np.all(v == V_STALLED)
    _same_state(a, b, s, R)                                                   # nothing committed
    yes = (rep % 2 == 0).astype(np.int32)
    b.farm_window_submit(rep, tt, m, move, u, T_STEP, R_STEP, au, pref, T, forced=np.where(yes == 1, 1, 2).astype(np.int32))
    o3, w3, v = b.farm_window_wait(R)
    o1, w1 = _forced_step(a, rep, tt, m, move, u, yes)
    assert np.array_equal(o3, o1) and np.array_equal(w3, w1) and np.array_equal(v == V_ACC, yes == 1) and np.all((v == V_ACC) | (v == V_REJ))
    _same_state(a, b, s, R)
    assert b.farm_window_stats() == (3, R)
    b.chain_set_margin(16 * np.finfo(float).eps)
    m, move, u = recs[1]
    au = rng.uniform(0, 1, R)
    b.farm_window_submit(rep, tt, m, move, u, T_STEP, R_STEP, au, np.ones(R), T)
    o2, w2, v = b.farm_window_wait(R)
    o1, w1, ok, near = _batched_step(a, rep, tt, m, move, u, T_STEP, R_STEP, au, np.ones(R), T)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2)
    assert not near.any() and np.all((v == V_ACC) | (v == V_REJ)) and np.array_equal(v == V_ACC, ok)
    _same_state(a, b, s, R)
    a.close(); b.close()


@pytest.mark.parametrize("cell", CELLS)
def test_an_undecided_insertion_stalls_its_chain_until_the_host_decides(cell):
    """The same with a by-count insertion at a free spot of the cell: undecided under the raised margin, the by-count window behind
    it comes back 4 whatever its counts say, the decision sent both ways is obeyed (the even chains gain a molecule), and the next
    by-count window finds the counts the decisions left."""
    s, _, cap = tri_box("24", cell)
    R = 4
    a, b = _twin(s, R, cap)
    rng = np.random.default_rng(12)
    rep = np.arange(R, dtype=np.int32)
    tt = np.zeros(R, np.int32)
    zeros = np.zeros(R, np.int32)
    T = float(s.temperature)
    N = int(s.n_mol[0])
    move = np.full(R, 3, np.int32)
    u = rng.uniform(0, 1, (R, 5))
    u[:, :3] = np.array([_free_fraction(rng, s) for _ in range(R)])
    # (the same for an insertion whose Boltzmann factor leaves the doubles' range: another free spot, another orientation)
    for _ in range(50):
        o, w = a.move_trial(rep, tt, zeros, move, u, T_STEP, R_STEP)
        with np.errstate(over="ignore"):
            boltz = np.exp(-(w.sum(1) - o.sum(1)) / T)
        bad = ~((boltz > 1e-200) & (boltz < 1e200))
        if not bad.any():
            break
        redrawn("insertion out of range", int(bad.sum()))
        for c in np.flatnonzero(bad):
            u[c] = rng.uniform(0, 1, 5)
            u[c, :3] = _free_fraction(rng, s)
    assert not bad.any(), (o, w)
    phiV = 0.3 * (N + 1.0) / boltz                                            # the launch divides by N + 1: a probability of 0.3
    au = np.full(R, 0.3 * (1.0 + 1e-7))
    su = rng.uniform(0, 1, R)
    b.chain_set_margin(1e-6)
    b.farm_window_submit(rep, tt, zeros, move, u, T_STEP, R_STEP, au, phiV, T, slot_u=su)
    behind = (rng.integers(1, 5, R).astype(np.int32), rng.uniform(0, 1, (R, 5)), rng.uniform(0, 1, R), rng.uniform(0, 1, R))
    b.farm_window_submit(rep, tt, zeros, behind[0], behind[1], T_STEP, R_STEP, behind[2], np.full(R, 2.0 * N), T, slot_u=behind[3])
    o2, w2, v = b.farm_window_wait(R)
    assert np.all(v == V_UND) and np.array_equal(o2, o) and np.array_equal(w2, w)
    _, _, v = b.farm_window_wait(R)
    assert np.all(v == V_STALLED)
    _same_state(a, b, s, R)
    yes = (rep % 2 == 0).astype(np.int32)
    b.farm_window_submit(rep, tt, zeros, move, u, T_STEP, R_STEP, au, phiV, T, forced=np.where(yes == 1, 1, 2).astype(np.int32), slot_u=su)
    o3, w3, v = b.farm_window_wait(R)
    o1, w1 = _forced_step(a, rep, tt, zeros, move, u, yes)
    assert np.array_equal(o3, o1) and np.array_equal(w3, w1) and np.array_equal(v == V_ACC, yes == 1) and np.all((v == V_ACC) | (v == V_REJ))
    _same_state(a, b, s, R)
    assert [b.num_molecules(r, 0) for r in range(R)] == [N + 1, N, N + 1, N]
    b.chain_set_margin(16 * np.finfo(float).eps)
    seen = set()
    assert _by_count_round(a, b, s, R, 0, cap[0], rng, T, seen) == 0
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 6. the wrap

def test_a_translation_through_a_face_of_the_wrap_cell_in_the_sheared_box():
    """Molecule 0 of the sheared 24-site box stands a hair inside a face of the cell ApplyPBC wraps into, and every chain translates
    it by -0.19 A along x, across the face: accepted by fiat on the even chains, rejected on the odd ones.  Rows and state are the
    twin's; the accepted centre is the stated ApplyPBC of the unwrapped target, more than 10 A from it."""
    s, _ = _at_a_face_of_the_wrap_cell(tri_box("24", "sheared")[0])
    R = 4
    t_step = 0.4
    a, b = _twin(s, R, [int(s.n_mol[0]) + 2])
    rng = np.random.default_rng(8)
    rep = np.arange(R, dtype=np.int32)
    tt = zeros = np.zeros(R, np.int32)
    move = np.ones(R, np.int32)
    u = rng.uniform(0, 1, (R, 5))
    u[:, :3] = (0.025, 0.5, 0.5)
    yes = (rep % 2 == 0).astype(np.int32)
    com0 = s.com[0][0].copy()
    b.farm_window_submit(rep, tt, zeros, move, u, t_step, R_STEP, np.full(R, 0.5), np.ones(R), float(s.temperature),
                         forced=np.where(yes == 1, 1, 2).astype(np.int32))
    o2, w2, v = b.farm_window_wait(R)
    o1, w1 = a.move_trial(rep, tt, zeros, move, u, t_step, R_STEP)
    a.commit_lane(0, rep, tt, zeros, _kinds(move), yes)
    assert np.array_equal(o1, o2) and np.array_equal(w1, w2) and np.array_equal(v == V_ACC, yes == 1)
    _same_state(a, b, s, R)
    rcp = box_prepare(s.box_matrix)[2]
    target = com0 + (u[0, :3] - 0.5) * t_step
    f = np.asarray(rcp).reshape(3, 3) @ (target - s.bounds_lo)
    assert f[0] < 0.0 and np.all(f[1:] > 0.0) and np.all(f[1:] < 1.0), f
    for r in range(R):
        centre = b.get_frames(r, 0)[0][0]
        if yes[r]:
            assert np.array_equal(centre, tc.apply_pbc_stated(s, rcp, target)) and np.linalg.norm(centre - target) > 10.0, (r, centre, target)
        else:
            assert np.array_equal(centre, com0), r
    a.close(); b.close()


# ---------------------------------------------------------------------------------------------- 7. the oracle

@pytest.mark.parametrize("cell", CELLS)
def test_24_sites_against_the_oracle(cell, refcpu_mod):
    """One window over six chains of the same start: a translation, a rotation, an insertion wherever its draw lands, a deletion, and
    two insertions placed on a neighbour's FAR IMAGE (tests/test_gpu_wide_triclinic_twin.py's construction: the overlap exists only
    for a sweep that tries that image) -- old and new components against the oracle's ComputeOldEnergy / ComputeNewEnergy for the
    candidate the device built, within tests/util.tol_for.  The deletion is rejected by fiat, everything else accepted and read
    back."""
    s, _, _ = tri_box("24", cell)
    N = int(s.n_mol[0])
    cap = [N + 2]
    rng = np.random.default_rng(23)
    move = np.array([1, 2, 3, 4] + [3] * len(FAR_IMAGE_DIST), np.int32)
    n = len(move)
    a, b = _twin(s, n, cap)
    t = np.zeros(n, np.int32)
    m = np.array([0 if mv == 3 else int(rng.integers(0, N)) for mv in move], np.int32)
    u = rng.random((n, 5))                     # drawn once: whatever the insertion lands on goes to the oracle
    far = _far_image_insertions(s, FAR_IMAGE_DIST)
    u[-len(far):, :3] = far
    rep = np.arange(n, dtype=np.int32)
    b.farm_window_submit(rep, t, m, move, u, 0.8, 0.6, np.full(n, 0.5), np.ones(n), float(s.temperature),
                         forced=np.where(move != 4, 1, 2).astype(np.int32))
    old, new, v = b.farm_window_wait(n)
    assert np.array_equal(v == V_ACC, move != 4)
    P = refcpu_mod.RefCPU(s, mol_capacity=cap[0])
    e_sys = P.system_energy()
    P.init_amplitude(True)
    P.set_energy_recip(e_sys["recip_coulomb"])
    worst = 0.0
    for c in range(n):
        mm = int(m[c])
        A0 = P.amplitude()
        eo, en = np.zeros(5), np.zeros(5)
        if move[c] <= 2:
            com0, off0 = P.get_molecule(0, mm)
            com_d, off_d = b.get_frames(c, 0)
            P.save_fourier(0, mm)
            eo = P.old_energy(0, mm, 0)[:5]
            P.set_molecule(0, mm, com_d[mm], off_d[mm])
            en = P.new_energy(0, mm, 0)[:5]
            P.set_molecule(0, mm, com0, off0)
            P.restore_fourier(0, mm)
        elif move[c] == 3:
            com_d, off_d = b.get_frames(c, 0)
            assert np.array_equal(com_d[N], tc.cart(s, u[c, :3]))
            eo = P.old_energy(0, N, 1)[:5]
            P.set_num_residues(0, N + 1)
            P.save_fourier(0, N)
            P.set_molecule(0, N, com_d[N], off_d[N])
            en = P.new_energy(0, N, 1)[:5]
            P.set_num_residues(0, N)
            P.set_amplitude(A0)
        else:
            P.all_fourier_terms()
            eo = P.old_energy(0, mm, 2)[:5]
            P.save_fourier(0, mm)
            en[2] = P.recip_singlemol(0, mm, 2)
            P.set_amplitude(A0)
        for got, ref, what in ((old[c], eo, "old"), (new[c], en, "new")):
            err = float(np.max(np.abs(got - ref)))
            worst = max(worst, err)
            print(cell, c, int(move[c]), what, err, tol_for(*ref, *got))
            assert err <= tol_for(*ref, *got), (cell, c, int(move[c]), what, got, ref)
    # (the far-image insertions do overlap: their pair energy is not that of a molecule in free space)
    assert np.all(np.abs(new[-len(far):, 0]) + np.abs(new[-len(far):, 1]) > 1.0), new[-len(far):]
    print(f"{cell}: worst |window - oracle| = {worst:.3e} K")
    a.close(); b.close()
