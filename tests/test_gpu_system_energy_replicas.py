"""Whole-system energies and S(k) of many replicas per call (mgpu_system_energy_replicas,
mgpu_init_structure_factor_replicas): engines of five replicas holding DIFFERENT configurations -- perturbed, one with an
active type emptied, one at capacity, one with a molecule deleted -- give, through the batched calls, exactly what the
per-replica calls give (bit for bit, any order, any subset, any chunk), and what the oracle gives within the parity bar.

Tolerances: bit equality against the per-replica path (np.array_equal); tests/util.tol_for against the oracle, as every
static energy of the suite."""
import ctypes as C

import numpy as np
import pytest

from maniac_mc_amd import synth
from maniac_mc_amd.engine import Engine
from maniac_mc_amd.fortran_host import FortranFarm
from tests import triclinic_cases
from tests.util import golden_system, tol_for

pytestmark = pytest.mark.gpu

E_KEYS = ("non_coulomb", "coulomb", "recip_coulomb", "ewald_self", "intra_coulomb", "total")
MGPU_OK, MGPU_ERR_INVALID_ARG = 0, 1
R = 5                 # replicas with their own configurations; replica R is the spare one (S(k) of a copy)

SYSTEMS = {
    "spce216": lambda: golden_system("spce216")[1],
    "co2_20": lambda: golden_system("co2_20")[1],                       # with spare capacity: see _capacity
    "mixture": lambda: golden_system("mixture")[1],
    "framework_small": lambda: golden_system("framework_small")[1],      # an inactive framework: no intra items for it
    "triclinic_mild": lambda: triclinic_cases.cell("mild"),
    "triclinic_sheared": lambda: triclinic_cases.cell("sheared"),
    "adsorbate24": lambda: synth.rigid_adsorbate_box(),                  # wide row form
    "adsorbate64": lambda: synth.large_adsorbate_box(n_sites=64, n_mol=4, L=34.0, seed=95),   # wave intra kernel, site-major
}


def _first_active(s):
    return next(t for t in range(s.topo.n_res) if s.topo.is_active[t])


def _capacity(name, s):
    cap = [max(1, int(n)) for n in s.n_mol]
    if name == "co2_20":
        cap[_first_active(s)] += 3
    return cap


def _with(s, t, com, off):
    v = s.copy()
    v.com[t] = np.ascontiguousarray(com)
    v.offsets[t] = np.ascontiguousarray(off)
    return v


def _extra_molecules(s, t, n_extra, rng):
    """n_extra more molecules of type t (the geometry of molecule 0), every site at least 2.5 A from every site there is
    (separations folded per axis: the boxes this is used on are orthorhombic)"""
    L = np.diag(s.box_matrix)
    sites = np.concatenate([s.all_sites(k).reshape(-1, 3) for k in range(s.topo.n_res)])
    com, off = [c for c in s.com[t]], [o for o in s.offsets[t]]
    while n_extra > 0:
        c = s.bounds_lo + rng.uniform(0.0, 1.0, 3) * L
        new = c[None, :] + s.offsets[t][0]
        d = new[:, None, :] - sites[None, :, :]
        d -= L * np.round(d / L)
        if np.min(np.sum(d * d, axis=2)) < 2.5 ** 2:
            continue
        com.append(c); off.append(s.offsets[t][0].copy())
        sites = np.concatenate([sites, new])
        n_extra -= 1
    return np.array(com), np.array(off)


def _variants(name, s, cap):
    """The five configurations: as given | perturbed | first active type emptied | at capacity | one molecule deleted"""
    rng = np.random.default_rng(sum(ord(c) for c in name))
    t = _first_active(s)
    n = int(s.n_mol[t])
    v1 = _with(s, t, s.com[t] + rng.uniform(-0.15, 0.15, (n, 3)), s.offsets[t])
    v2 = _with(s, t, s.com[t][:0], s.offsets[t][:0])
    if cap[t] > n:
        v3 = _with(s, t, *_extra_molecules(s, t, cap[t] - n, rng))
    else:
        v3 = _with(s, t, s.com[t] + rng.uniform(-0.1, 0.1, (n, 3)), s.offsets[t])
    assert int(v3.n_mol[t]) == cap[t]
    keep = np.array([m for m in range(n) if m != 1])
    v4 = _with(s, t, s.com[t][keep] + rng.uniform(-0.1, 0.1, (n - 1, 3)), s.offsets[t][keep])
    return [s, v1, v2, v3, v4]


def _load(eng, variants, t):
    """replica r <- configuration r, through the existing setters (replica 2: loaded as given, then its type set to count 0)"""
    for r, v in enumerate(variants):
        if r == 2:
            eng.load_system(variants[0], r)
            eng.set_num_molecules(r, t, 0)
        else:
            eng.load_system(v, r)


_cases = {}


def _case(name):
    """The system, its variants, an engine loaded with them and the per-replica energies, built once per system."""
    if name not in _cases:
        s = SYSTEMS[name]()
        cap = _capacity(name, s)
        variants = _variants(name, s, cap)
        eng = Engine(s.topo, s.box_matrix, s.bounds_lo, s.real_space_cutoff, s.ewald_tolerance, R + 1, 0, cap)
        t = _first_active(s)
        _load(eng, variants, t)
        # A(k): initialised per replica, except replica 1 (zeroed: A != S there)
        for r in range(R):
            eng.init_structure_factor(r, full=(r != 1))
        single = np.array([[eng.system_energy(r)[k] for k in E_KEYS] for r in range(R)])
        _cases[name] = (s, cap, variants, eng, single)
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for c in _cases.values():
        c[3].close()
    _cases.clear()


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_batched_energies_are_the_per_replica_calls_bit_for_bit(name):
    s, cap, variants, eng, single = _case(name)
    t = _first_active(s)
    assert eng.num_molecules(2, t) == 0 and eng.num_molecules(3, t) == cap[t]
    assert len({tuple(row) for row in single.tolist()}) == R, "the replicas hold different configurations"
    for reps, chunk in ((None, None), ([4, 0, 2], None), (list(range(R)), 1), (list(range(R)), 2), ([3, 1, 4, 0], 2), ([2], None)):
        got = eng.system_energy_replicas(reps, chunk=chunk)
        if reps is None:                                       # every replica of the engine, the spare one last
            assert got.shape == (R + 1, 6)
            got = got[:R]
        want = single if reps is None else single[reps]
        assert got.shape == want.shape
        print(f"{name} reps {reps} chunk {chunk}: max |batched - single| = {np.max(np.abs(got - want)):.3e} K")
        assert np.array_equal(got, want), (name, reps, chunk)
    # the per-replica call still answers the same afterwards (the batched call changed nothing)
    again = np.array([[eng.system_energy(r)[k] for k in E_KEYS] for r in range(R)])
    assert np.array_equal(again, single)


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_batched_energies_against_the_oracle(name, refcpu_mod):
    s, cap, variants, eng, single = _case(name)
    got = eng.system_energy_replicas()[:R]
    for r, v in enumerate(variants):
        P = refcpu_mod.RefCPU(v, mol_capacity=max(8, max(cap) + 1))
        ref = P.system_energy()
        P.close()
        for i, k in enumerate(E_KEYS):
            tol = tol_for(ref[k], got[r, i])
            print(f"{name} replica {r} {k}: |dE| = {abs(got[r, i] - ref[k]):.3e} K (tol {tol:.3e})")
            assert abs(got[r, i] - ref[k]) <= tol, (name, r, k, got[r, i], ref[k])


def _numpy_deviation(eng, r):
    """max |A - S| of replica r: A as it is, S from a copy in the spare replica initialised there"""
    A = eng.structure_factor(r)
    eng.replica_copy(R, r)
    eng.init_structure_factor(R, True)
    S = eng.structure_factor(R)
    return max(float(np.max(np.abs(A.real - S.real))), float(np.max(np.abs(A.imag - S.imag))))


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_a_deviation(name):
    s, cap, variants, eng, single = _case(name)
    before = [eng.structure_factor(r) for r in range(R)]
    expect = np.array([_numpy_deviation(eng, r) for r in range(R)])
    out, dev = eng.system_energy_replicas(list(range(R)), a_deviation=True)
    assert np.array_equal(out, single)
    print(f"{name}: a_deviation {dev}, numpy {expect}")
    assert np.array_equal(dev, expect)
    assert dev[1] > 0.0, "replica 1's A(k) was zeroed: it is not its S(k)"
    assert all(dev[r] == 0.0 for r in (0, 2, 3, 4)), "A(k) just initialised is S(k) bit for bit"
    for reps, chunk in (([4, 1, 2], None), (list(range(R)), 2)):
        _, d = eng.system_energy_replicas(reps, chunk=chunk, a_deviation=True)
        assert np.array_equal(d, expect[reps])
    for r in range(R):
        assert np.array_equal(eng.structure_factor(r), before[r]), "A(k) is not changed by the call"
    # one k of replica 3 raised by 1e-3: that replica reports it, the others are as they were
    # (at the k whose real part is smallest: (A + 1e-3) - A then carries a rounding of at most 2^-53 |A + 1e-3|, far below
    # the 1e-15 the bound leaves)
    z = before[3].copy()
    k = int(np.argmin(np.abs(z.real)))
    assert abs(z[k].real) < 8.0
    z[k] += 1e-3
    eng.set_structure_factor(z, 3)
    try:
        _, d = eng.system_energy_replicas(list(range(R)), a_deviation=True)
        assert d[3] >= 1e-3 * (1.0 - 1e-12)
        assert np.array_equal(np.delete(d, 3), np.delete(expect, 3))
    finally:
        eng.set_structure_factor(before[3], 3)
    assert np.array_equal(eng.structure_factor(3), before[3])


@pytest.mark.parametrize("name", sorted(SYSTEMS))
@pytest.mark.parametrize("full", [True, False])
def test_batched_structure_factor_initialisation_equals_the_per_replica_one(name, full):
    s, cap, variants, eng, single = _case(name)
    twin = Engine(s.topo, s.box_matrix, s.bounds_lo, s.real_space_cutoff, s.ewald_tolerance, R + 1, 0, cap)
    try:
        _load(twin, variants, _first_active(s))
        kept = [eng.structure_factor(r) for r in range(R)]
        for r in range(R):                      # the twin starts from the same A(k): what is not listed must stay
            twin.set_structure_factor(kept[r], r)
        listed = [4, 0, 2, 1] if full else [1, 3, 4]
        twin.init_structure_factor_replicas(listed, full=full)
        try:
            for r in listed:
                eng.init_structure_factor(r, full)
            for r in range(R):
                assert np.array_equal(twin.structure_factor(r), eng.structure_factor(r)), (name, r, full)
            if not full:
                assert all(not np.any(twin.structure_factor(r)) for r in listed)
            assert np.array_equal(twin.structure_factor(0 if not full else 3), kept[0 if not full else 3])
        finally:
            for r in range(R):
                eng.set_structure_factor(kept[r], r)
    finally:
        twin.close()


def test_after_a_window_farm_run():
    """A farm of window launches leaves some replicas' current A(k) in the alternate buffer: the batched calls see each
    replica's current A(k) and rewrite it as the per-replica calls do."""
    _, s = golden_system("spce216")
    farm = FortranFarm(s, 6, seed=5, n_lanes=2, device_build=True, window=True)
    try:
        assert farm.window
        farm.run(12)
        assert farm.accepted > 0
        eng = farm.eng
        out, dev = eng.system_energy_replicas(a_deviation=True)          # the first synchronous call after the run
        A = [eng.structure_factor(r) for r in range(6)]
        for r in range(6):
            assert np.array_equal(out[r], [eng.system_energy(r)[k] for k in E_KEYS])
        eng.init_structure_factor_replicas([5, 1, 3])
        batched = {r: eng.structure_factor(r) for r in range(6)}
        for r in (0, 2, 4):
            assert np.array_equal(batched[r], A[r])
        for r in (5, 1, 3):
            expect = max(float(np.max(np.abs(A[r].real - batched[r].real))), float(np.max(np.abs(A[r].imag - batched[r].imag))))
            assert dev[r] == expect
            # a running A(k) differs from S(k) by the roundings of its updates only (the parity tests' bar for A(k))
            assert dev[r] < 1e-10
            eng.init_structure_factor(r, True)
            assert np.array_equal(eng.structure_factor(r), batched[r])
        assert max(dev[r] for r in (5, 1, 3)) > 0.0
        farm.run(12)                                                   # the farm goes on from the rewritten A(k)
        a = farm.audit()
        assert np.max(a["a_deviation"]) < 1e-10
    finally:
        farm.close()


def test_refusals_leave_everything_as_it_was():
    s, cap, variants, eng, single = _case("mixture")
    L, h = eng.L, eng.h
    ip, dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    A = [eng.structure_factor(r) for r in range(R)]

    def energy(reps, n=None, out=True):
        reps = np.asarray(reps, dtype=np.int32)
        buf = np.full((max(1, reps.size), 6), -7.0)
        rc = L.mgpu_system_energy_replicas(h, C.c_int(reps.size if n is None else n), reps.ctypes.data_as(ip), C.c_int(0),
                                           buf.ctypes.data_as(dp) if out else None, None)
        return rc, buf

    def init(reps, n=None):
        reps = np.asarray(reps, dtype=np.int32)
        return L.mgpu_init_structure_factor_replicas(h, C.c_int(reps.size if n is None else n), reps.ctypes.data_as(ip), C.c_int(0))

    for reps, n in (([0, 2, 0], None), ([1, R + 1], None), ([-1], None), ([0, 1], -1)):
        rc, buf = energy(reps, n)
        assert rc == MGPU_ERR_INVALID_ARG and np.all(buf == -7.0), (reps, n)
        assert init(reps, n) == MGPU_ERR_INVALID_ARG, (reps, n)
    assert energy([0, 1], out=False)[0] == MGPU_ERR_INVALID_ARG
    assert L.mgpu_system_energy_replicas(h, C.c_int(2), None, C.c_int(0), np.zeros(12).ctypes.data_as(dp), None) == MGPU_ERR_INVALID_ARG
    assert L.mgpu_init_structure_factor_replicas(h, C.c_int(2), None, C.c_int(1)) == MGPU_ERR_INVALID_ARG
    # nothing listed is nothing to do
    assert energy([], 0)[0] == MGPU_OK and init([], 0) == MGPU_OK
    assert L.mgpu_system_energy_replicas(h, C.c_int(0), None, C.c_int(0), None, None) == MGPU_OK
    assert eng.system_energy_replicas([]).shape == (0, 6)
    for r in range(R):
        assert np.array_equal(eng.structure_factor(r), A[r])
    assert np.array_equal(eng.system_energy_replicas(list(range(R))), single)
