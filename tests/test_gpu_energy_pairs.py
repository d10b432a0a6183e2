"""Energies by residue-type pair (mgpu_energy_pairs_replicas, Engine.energy_pairs_replicas) against the reference.

The pair-wise components are quadratic forms of the configuration, so the oracle's own ComputeSystemEnergy on sub-systems --
every other residue type's molecule count set to zero -- gives every entry: E[a][b] = E({a, b}) - E({a}) - E({b}) for a != b,
E[a][a] = E({a}).  The tolerance per component is the project's bar for ONE static total against the oracle (tests/util.py
tol_for) once per total that enters: tol_for(x_ab) + tol_for(x_a) + tol_for(x_b) + tol_for(device value) off the diagonal,
tol_for(x_a) + tol_for(device value) on it.  Nothing else is added.

Systems: a three-type box A3 / B2 / C1 (C1 uncharged, 70 molecules: its plane crosses a 64-lane unit) for the three
off-diagonal entries; spce216 (three full units and a tail); co2_20 with capacity + 3 (unoccupied slots at a plane's end);
framework_small (inactive frozen type + guest: layout 2); the 24-site adsorbate (the LDS slab); the 64-site one (site-major);
the mild and the sheared triclinic cell (both image searches).  Five replicas each -- as given, perturbed, first active type
emptied, at capacity, one molecule deleted -- and a sixth that is never loaded."""
import ctypes as C

import numpy as np
import pytest

from maniac_mc_amd import synth
from maniac_mc_amd._lib import MgpuError
from maniac_mc_amd.engine import Engine
from maniac_mc_amd.fortran_host import FortranFarm
from maniac_mc_amd.system import System, Topology
from tests import triclinic_cases
from tests.test_gpu_rdf import _capacity, _first_active, _load, _variants
from tests.util import golden_system, tol_for

pytestmark = pytest.mark.gpu

MGPU_ERR_INVALID_ARG = 1
R = 5                 # replicas with their own configurations; replica R is never loaded (no atoms)
NC, CO, RE, SE, IN = range(5)


def three_type_box(seed=11):
    """mixture_box's A3 and B2 plus an uncharged monatomic Lennard-Jones type C1: 12 / 9 / 70 molecules, centres at least
    3.2 A apart, as mixture_box places them"""
    rng = np.random.default_rng(seed)
    box = np.array([18.0, 21.0, 24.0])
    eps, sig = synth.lorentz_berthelot([0.12, 0.20, 0.0, 0.07, 0.15], [3.0, 3.4, 0.0, 2.7, 3.1])
    topo = Topology(atoms_in_res=[3, 2, 1], atom_types=[[1, 2, 3], [4, 2, 0], [5, 0, 0]],
                    charges=[[0.5, -0.5, 0.0], [0.3, -0.3, 0.0], [0.0, 0.0, 0.0]], is_active=[1, 1, 1],
                    epsilon=eps, sigma=sig, names=["A3", "B2", "C1"])
    n_a, n_b, n_c = 12, 9, 70
    frac = np.empty((0, 3))
    while frac.shape[0] < n_a + n_b + n_c:
        p = rng.uniform(0, 1, size=3)
        if frac.shape[0]:
            d = frac - p
            d -= np.rint(d)
            if np.min(np.einsum("ij,ij->i", d * box, d * box)) < 3.2 ** 2:
                continue
        frac = np.vstack([frac, p])
    lo = -box / 2
    com = lo[None, :] + frac * box[None, :]
    ta = np.array([[0.0, 0.0, 0.0], [1.1, 0.0, 0.0], [-0.4, 0.9, 0.0]])
    ta -= ta.mean(0)
    tb = np.array([[0.6, 0.0, 0.0], [-0.6, 0.0, 0.0]])
    off_a = np.einsum("mij,aj->mai", synth._random_rotations(rng, n_a), ta)
    off_b = np.einsum("mij,aj->mai", synth._random_rotations(rng, n_b), tb)
    return System(topo, np.diag(box), lo, 8.0, 1e-4, 250.0, [com[:n_a], com[n_a:n_a + n_b], com[n_a + n_b:]],
                  [off_a, off_b, np.zeros((n_c, 1, 3))], label="three_types")


SYSTEMS = {
    "three_types": three_type_box,
    "spce216": lambda: golden_system("spce216")[1],
    "co2_20": lambda: golden_system("co2_20")[1],
    "framework_small": lambda: golden_system("framework_small")[1],
    "adsorbate24": lambda: synth.rigid_adsorbate_box(),
    "adsorbate64": lambda: synth.large_adsorbate_box(n_sites=64, n_mol=4, L=34.0, seed=95),
    "triclinic_mild": lambda: triclinic_cases.cell("mild"),
    "triclinic_sheared": lambda: triclinic_cases.cell("sheared"),
}
NAMES = sorted(SYSTEMS)


def all_pairs(n_res):
    return [(a, b) for a in range(n_res) for b in range(a, n_res)]


def _five(d):
    return np.array([d["non_coulomb"], d["coulomb"], d["recip_coulomb"], d["ewald_self"], d["intra_coulomb"]])


def oracle_matrix(refcpu_mod, v):
    """{(a, b): (expected five components, the oracle's totals that entered)} from RefCPU.system_energy() on sub-systems"""
    n_res = v.topo.n_res
    counts = [int(n) for n in v.n_mol]
    P = refcpu_mod.RefCPU(v, mol_capacity=max(8, max(counts) + 1))

    def energy(types):
        for t in range(n_res):
            P.set_num_residues(t, counts[t] if t in types else 0)
        return _five(P.system_energy())

    single = {a: energy((a,)) for a in range(n_res)}
    out = {}
    for a, b in all_pairs(n_res):
        if a == b:
            out[(a, b)] = (single[a], [single[a]])
        else:
            both = energy((a, b))
            out[(a, b)] = (both - single[a] - single[b], [both, single[a], single[b]])
    P.close()
    return out


_cases = {}


def _case(name, refcpu_mod):
    """The system, its capacities, the five variants, an engine of R + 1 replicas loaded with them, the oracle's matrix of
    every variant and the device's full matrix: built once per system and shared, unchanged, by the tests."""
    if name not in _cases:
        s = SYSTEMS[name]()
        cap = _capacity(name, s)
        variants = _variants(name, s, cap)
        eng = Engine(s.topo, s.box_matrix, s.bounds_lo, s.real_space_cutoff, s.ewald_tolerance, R + 1, 0, cap)
        _load(eng, variants, _first_active(s))
        oracles = [oracle_matrix(refcpu_mod, v) for v in variants]
        full = eng.energy_pairs_replicas(all_pairs(s.topo.n_res))
        _cases[name] = (s, cap, variants, eng, oracles, full)
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for c in _cases.values():
        c[3].close()
    _cases.clear()


@pytest.mark.parametrize("name", NAMES)
def test_every_entry_against_the_oracle(name, refcpu_mod):
    s, cap, variants, eng, oracles, full = _case(name, refcpu_mod)
    pairs = all_pairs(s.topo.n_res)
    assert full.shape == (R + 1, len(pairs), 5) and full.dtype == np.float64
    worst = 0.0
    for r in range(R):
        for p, ab in enumerate(pairs):
            want, totals = oracles[r][ab]
            for c in range(5):
                tol = sum(tol_for(x[c]) for x in totals) + tol_for(full[r, p, c])
                ratio = abs(full[r, p, c] - want[c]) / tol
                worst = max(worst, ratio)
                assert ratio <= 1.0, (name, r, ab, c, full[r, p, c], want[c], tol)
    print(f"{name}: largest |difference| / tolerance = {worst:.3e}")
    assert np.any(full[0, :, NC] != 0.0)


@pytest.mark.parametrize("name", NAMES)
def test_the_entries_add_up_to_the_engines_totals(name, refcpu_mod):
    s, cap, variants, eng, oracles, full = _case(name, refcpu_mod)
    n_res = s.topo.n_res
    pairs = all_pairs(n_res)
    total = eng.system_energy_replicas()
    for r in range(R + 1):
        for c in (NC, CO, RE):
            tol = tol_for(total[r, c]) + sum(tol_for(full[r, p, c]) for p in range(len(pairs)))
            assert abs(full[r, :, c].sum() - total[r, c]) <= tol, (name, r, c)
        e_self = 0.0
        for t in range(n_res):
            e_self = e_self + full[r, pairs.index((t, t)), SE]
        assert e_self == total[r, SE], "the self terms in type order are the total's, bit for bit"
        e_in = 0.0
        for t in range(n_res):
            e_in = e_in + full[r, pairs.index((t, t)), IN]
        if int(np.sum(np.asarray(s.topo.is_active) == 1)) == 1:
            assert e_in == total[r, IN]
        else:
            assert abs(e_in - total[r, IN]) <= tol_for(total[r, IN])
        for t in range(n_res):
            if s.topo.is_active[t] != 1:
                assert full[r, pairs.index((t, t)), IN] == 0.0, "an inactive type has no intra term"


@pytest.mark.parametrize("name", NAMES)
def test_exact_zeros(name, refcpu_mod):
    s, cap, variants, eng, oracles, full = _case(name, refcpu_mod)
    pairs = all_pairs(s.topo.n_res)
    assert np.all(full[R] == 0.0), "the replica never loaded"
    t = _first_active(s)
    for p, (a, b) in enumerate(pairs):
        if t in (a, b):
            assert np.all(full[2, p] == 0.0), "a type without molecules"
        if a != b:
            assert np.all(full[:, p, SE] == 0.0) and np.all(full[:, p, IN] == 0.0)
        if name == "three_types" and 2 in (a, b):
            assert np.all(full[:, p, CO] == 0.0) and np.all(full[:, p, RE] == 0.0), "a type without a charged site"
            assert np.any(full[[0, 1, 3, 4], p, NC] != 0.0)


@pytest.mark.parametrize("name", NAMES)
def test_bit_for_bit_whatever_shares_the_call(name, refcpu_mod):
    s, cap, variants, eng, oracles, full = _case(name, refcpu_mod)
    pairs = all_pairs(s.topo.n_res)
    everyone = list(range(R + 1))
    for chunk in (1, 2, None):
        assert np.array_equal(eng.energy_pairs_replicas(pairs, chunk=chunk), full), chunk
    assert np.array_equal(eng.energy_pairs_replicas(pairs, everyone[::-1]), full[::-1])
    assert np.array_equal(eng.energy_pairs_replicas(pairs, [3, 0, 4], chunk=2), full[[3, 0, 4]])
    for r in everyone:
        assert np.array_equal(eng.energy_pairs_replicas(pairs, [r]), full[[r]])
    swapped = [(b, a) for a, b in pairs[::-1]]
    assert np.array_equal(eng.energy_pairs_replicas(swapped), full[:, ::-1])
    for p, ab in enumerate(pairs):
        assert np.array_equal(eng.energy_pairs_replicas([ab])[:, 0], full[:, p]), ab
    assert np.array_equal(eng.energy_pairs_replicas(pairs), full)


@pytest.mark.parametrize("name", NAMES)
def test_nothing_else_changes(name, refcpu_mod):
    s, cap, variants, eng, oracles, full = _case(name, refcpu_mod)
    n_res = s.topo.n_res
    eng.init_structure_factor_replicas()

    def state():
        return ([eng.structure_factor(r) for r in range(R + 1)],
                [eng.get_molecules(r, t) for r in range(R + 1) for t in range(n_res)], eng.system_energy_replicas())

    before = state()
    assert np.array_equal(eng.energy_pairs_replicas(all_pairs(n_res), chunk=2), full)
    after = state()
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(x, y)
    assert np.array_equal(before[2], after[2])


# ---- after real moves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["windows", "device"])
def test_after_a_farm_run_with_insertions_and_deletions(mode):
    s = three_type_box()
    Rf, n_steps = 4, 120
    pairs = all_pairs(3)
    farm = FortranFarm(s, Rf, seed=23, translation_step=1.0, rotation_step=0.6, n_threads=4, mol_capacity=[30, 30, 100],
                       gcmc=dict(p_translation=0.2, p_rotation=0.2, fugacity=np.full((Rf, 3), 12.0 / 50.0 ** 3)), device_build=True,
                       window=mode == "windows")
    try:
        assert farm.window == (mode == "windows")
        for block in range(2):
            farm.run(n_steps)
            got = farm.energy_pairs_sample(pairs)
            total = farm.audit()["recomputed"]
            c = farm.counters()
            print(mode, "block", block, "counts", farm.counts().tolist(), c)
            for r in range(Rf):
                for k in (NC, CO, RE):
                    tol = tol_for(total[r, k]) + sum(tol_for(got[r, p, k]) for p in range(len(pairs)))
                    assert abs(got[r, :, k].sum() - total[r, k]) <= tol, (mode, block, r, k)
                e_self = 0.0
                for t in range(3):
                    e_self = e_self + got[r, pairs.index((t, t)), SE]
                assert e_self == total[r, SE]
        assert c["creations"] + c["deletions"] > 0
        farm.run(20)                       # the farm goes on
    finally:
        farm.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _raw(eng, reps, ra, rb, n_sel=None, out=None):
    """the C call itself: (code, text, out) with out prefilled with a sentinel"""
    reps = np.ascontiguousarray(reps, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    a = None if ra is None else np.ascontiguousarray(ra, dtype=np.int32)
    b = None if rb is None else np.ascontiguousarray(rb, dtype=np.int32)
    n_sel = (0 if a is None else a.size) if n_sel is None else n_sel
    buf = np.full((reps.size, max(1, n_sel), 5), -7.25) if out is None else out
    rc = eng.L.mgpu_energy_pairs_replicas(eng.h, C.c_int(reps.size), reps.ctypes.data_as(ip), C.c_int(0), C.c_int(n_sel),
                                          None if a is None else a.ctypes.data_as(ip), None if b is None else b.ctypes.data_as(ip),
                                          buf.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, eng.L.mgpu_last_error().decode(), buf


def test_refusals_with_texts(refcpu_mod):
    s, cap, variants, eng, oracles, full = _case("three_types", refcpu_mod)
    n_res = s.topo.n_res
    for ra, rb, n_sel, text in (([0, 1, 1], [1, 1, 0], None, "pair 2 (1, 0) is a duplicate"),
                                ([2, 2], [2, 2], None, "pair 1 (2, 2) is a duplicate"),
                                ([0], [n_res], None, f"pair 0 (0, {n_res})"),
                                ([-1], [0], None, "pair 0 (-1, 0)"),
                                ([0], [0], 0, "n_sel 0 pairs"),
                                (list(range(37)), [0] * 37, 37, "n_sel 37 pairs"),
                                (None, [0], 1, "null pair list"),
                                ([0], None, 1, "null pair list")):
        rc, msg, buf = _raw(eng, [0, 1], ra, rb, n_sel)
        assert rc == MGPU_ERR_INVALID_ARG and text in msg, (rc, msg, text)
        assert np.all(buf == -7.25), "a refused call writes nothing"
    rc, msg, buf = _raw(eng, [0, 3, 0], [0], [0])
    assert rc == MGPU_ERR_INVALID_ARG and "replica 0 listed twice" in msg and np.all(buf == -7.25)
    with pytest.raises(MgpuError) as err:
        eng.energy_pairs_replicas([(0, 0), (0, 0)])
    assert err.value.code == MGPU_ERR_INVALID_ARG and "duplicate" in str(err.value)
    # nothing listed is nothing to do; the engine still answers
    assert eng.energy_pairs_replicas([(0, 1)], []).shape == (0, 1, 5)
    assert np.array_equal(eng.energy_pairs_replicas(all_pairs(n_res)), full)
