"""Density maps binned on the device (mgpu_density_*, Engine.density_*): the counts are held to the reference's ApplyPBC EXACTLY.
The expected maps come from the oracle's ApplyPBC (oracle.refcpu `apply_pbc`) of every occupied atom; the fractional coordinates
of the wrapped point are formed in NumPy (M f = w - bounds_lo, the cell vectors being the columns of box%matrix), then the floor
and the Euclidean mod; the device's hist and samples must equal them as integers.

The device forms s = box%reciprocal (r - bounds_lo) with fma and does not wrap first, so u = s n may differ from the oracle's in
the last bits (about 1e-13 at n = 1024).  Every comparison therefore first ASSERTS, from the oracle's numbers, that no counted
atom has a u_d within MARGIN = 1e-9 of an integer -- four orders above the possible difference.  Smallest margins of the five
variants of every system over the grids used here (checked on the CPU): MARGINS below.  A configuration that ever violated the
margin gets another fixed seed in this file, never a skip or a tolerance.  The voxel edges themselves are reached by the
exact-lattice tests at the end, whose cells, coordinates and grids are dyadic: every product and sum there is exact with or
without fma, and the expected voxel of every atom is written out by hand.

Systems, variants and engines' shapes are those of tests/test_gpu_rdf.py (spce216: 648 slots = two full blocks of 256 and a partial
one; co2_20 with capacity + 3; framework_small with guest-only channels -- the ballot exit --, a framework channel and eight
channels; the two triclinic cells; the 24-site adsorbate; the site-major 64-site one), plus a replica that is never loaded.

MARGINS (smallest |u - round(u)| over all counted atoms, axes and the grids of SHAPES):
    spce216 8.7e-05, co2_20 7.6e-04, mixture 6.5e-04, framework_small 3.9e-05, triclinic_mild 3.3e-04,
    triclinic_sheared 1.8e-05, adsorbate24 1.4e-04, adsorbate64 1.0e-04
"""
import numpy as np
import pytest

from maniac_mc_amd import rdf, synth
from maniac_mc_amd._lib import MgpuError
from maniac_mc_amd.engine import Engine, box_prepare
from maniac_mc_amd.system import System, Topology
from tests.test_gpu_rdf import SYSTEMS, _capacity, _first_active, _load, _variants

pytestmark = pytest.mark.gpu

MARGIN = 1.0e-9
MGPU_ERR_INVALID_ARG, MGPU_ERR_STATE = 1, 5
R = 5                 # replicas with their own configurations; replica R is never loaded (no atoms)

ONE = [0] * (R + 1)                       # all replicas in one map
IDENTITY = list(range(R + 1))             # one map per replica
UNEVEN = [0, 1, 1, -1, 0, 1]              # two maps of uneven size, replica 3 never counted

# name -> [(grid, channels (0-based atom types), group_of)]
SHAPES = {
    "spce216": [((16, 16, 16), [0], ONE), ((3, 5, 7), [1, 0], IDENTITY), ((1024, 1, 1), [0, 1], UNEVEN)],
    "co2_20": [((1, 1, 1), [0, 1], IDENTITY), ((64, 32, 8), [1], ONE), ((1, 1, 7), [0], UNEVEN)],
    "mixture": [((3, 5, 7), [0, 1, 2, 3], UNEVEN), ((16, 16, 16), [3], IDENTITY)],
    # atom types 0..6 are the framework's, 7..9 the guest's: guest only (whole waves leave by the ballot), a framework type
    # beside a guest type (every replica of a map adds into the same voxels), eight channels
    "framework_small": [((16, 16, 16), [7, 9], ONE), ((3, 5, 7), [2, 8], ONE), ((64, 32, 8), [7, 0, 8, 1, 9, 6, 3, 5], UNEVEN)],
    "triclinic_mild": [((3, 5, 7), [0, 1, 2, 3], IDENTITY), ((16, 16, 16), [1], ONE)],
    "triclinic_sheared": [((16, 16, 16), [0, 1, 2, 3], UNEVEN), ((1, 1, 7), [3, 1], IDENTITY), ((1024, 1, 1), [1], ONE)],
    "adsorbate24": [((3, 5, 7), [0, 1], IDENTITY), ((64, 32, 8), [1], UNEVEN)],
    "adsorbate64": [((16, 16, 16), [0, 1, 2], ONE), ((1, 1, 7), [2], IDENTITY)],
}


# ---- the oracle's side ------------------------------------------------------------------------------------------------------
def oracle_fractions(refcpu_mod, s, variants):
    """Per variant (atom type (n,), f (n, 3)): the fractional coordinates of the oracle's ApplyPBC of every occupied atom's
    position, f = M^-1 (w - bounds_lo) solved in NumPy from the wrapped point w."""
    P = refcpu_mod.RefCPU(s, mol_capacity=max(8, int(max(s.n_mol)) + 1))
    M, lo = np.asarray(s.box_matrix, dtype=np.float64), np.asarray(s.bounds_lo, dtype=np.float64)
    out = []
    try:
        for v in variants:
            ty, w = [], []
            for t in range(s.topo.n_res):
                sites = v.all_sites(t)
                for a in range(int(s.topo.atoms_in_res[t])):
                    for m in range(sites.shape[0]):
                        ty.append(int(s.topo.atom_types[t, a]) - 1)
                        w.append(P.apply_pbc(sites[m, a]))
            w = np.array(w, dtype=np.float64).reshape(-1, 3)
            f = np.linalg.solve(M, (w - lo[None, :]).T).T if len(ty) else np.zeros((0, 3))
            out.append((np.array(ty, dtype=np.int64), f))
    finally:
        P.close()
    return out


def expected_map(oracle, grid, types, what=""):
    """hist (n_channels, n2, n1, n0) of one configuration by the contract's rule from the oracle's fractional coordinates --
    after asserting that no counted atom has a u within MARGIN of an integer"""
    ty, f = oracle
    n = np.asarray(grid, dtype=np.int64)
    hist = np.zeros((len(types), grid[2], grid[1], grid[0]), dtype=np.uint64)
    for c, t in enumerate(types):
        u = f[ty == t] * n[None, :].astype(np.float64)
        if u.size == 0:
            continue
        margin = float(np.abs(u - np.round(u)).min())
        print(f"{what} type {t} grid {grid}: {u.shape[0]} atoms, smallest margin {margin:.2e}")
        assert margin > MARGIN, (what, t, grid, margin)
        v = np.mod(np.floor(u).astype(np.int64), n[None, :])
        np.add.at(hist[c], (v[:, 2], v[:, 1], v[:, 0]), np.uint64(1))
    return hist


def pooled(per_replica, group_of, listed=None):
    """(hist (n_groups, ...), samples (n_groups,)) from the per-replica maps (R + 1, ...) for the listed replicas (None: all)"""
    n_groups = max(group_of) + 1
    hist = np.zeros((n_groups,) + per_replica.shape[1:], dtype=np.uint64)
    samples = np.zeros(n_groups, dtype=np.uint64)
    for r in (range(len(group_of)) if listed is None else listed):
        if group_of[r] >= 0:
            hist[group_of[r]] += per_replica[r]
            samples[group_of[r]] += np.uint64(1)
    return hist, samples


_cases = {}


def _case(name, refcpu_mod):
    """The system, its capacities, the five variants, an engine of R + 1 replicas loaded with them, and the oracle's fractional
    coordinates of every variant: built once per system and shared, unchanged, by the tests."""
    if name not in _cases:
        s = SYSTEMS[name]()
        cap = _capacity(name, s)
        variants = _variants(name, s, cap)
        eng = Engine(s.topo, s.box_matrix, s.bounds_lo, s.real_space_cutoff, s.ewald_tolerance, R + 1, 0, cap)
        _load(eng, variants, _first_active(s))
        _cases[name] = (s, cap, variants, eng, oracle_fractions(refcpu_mod, s, variants))
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for c in _cases.values():
        c[3].close()
    _cases.clear()


def _per_replica(name, oracles, grid, types):
    maps = np.zeros((R + 1, len(types), grid[2], grid[1], grid[0]), dtype=np.uint64)
    for r in range(R):
        maps[r] = expected_map(oracles[r], grid, types, f"{name} replica {r}")
    return maps


def _atoms_of_type(topo, n_mol, t):
    """occupied atoms of atom type t from the molecule counts and the topology"""
    return sum(int(n_mol[k]) * int(np.sum(topo.atom_types[k, :int(topo.atoms_in_res[k])] == t + 1)) for k in range(topo.n_res))


@pytest.mark.parametrize("name,shape", [(n, k) for n in sorted(SHAPES) for k in range(len(SHAPES[n]))])
def test_counts_equal_the_oracles_exactly(name, shape, refcpu_mod):
    s, cap, variants, eng, oracles = _case(name, refcpu_mod)
    grid, types, group_of = SHAPES[name][shape]
    want_h, want_s = pooled(_per_replica(name, oracles, grid, types), group_of)
    eng.density_configure(grid, types, group_of)
    eng.density_accumulate()
    hist, samples = eng.density_read()
    assert hist.dtype == samples.dtype == np.uint64
    assert hist.shape == (max(group_of) + 1, len(types), grid[2], grid[1], grid[0]) and samples.shape == (max(group_of) + 1,)
    print(f"{name} grid {grid} types {types} groups {group_of}: counted {hist.sum(axis=(2, 3, 4)).tolist()}, samples {samples.tolist()}")
    assert np.array_equal(samples, want_s)
    assert np.array_equal(hist, want_h)
    assert want_h.sum() > 0
    # the sum over a map's voxels is the number of occupied atoms of the type over the group's samples
    for g in range(hist.shape[0]):
        for c, t in enumerate(types):
            atoms = sum(_atoms_of_type(s.topo, variants[r].n_mol, t) for r in range(R) if group_of[r] == g)
            assert int(hist[g, c].sum()) == atoms, (g, c, t)


@pytest.mark.parametrize("name", ["spce216", "co2_20", "framework_small", "triclinic_sheared", "adsorbate64"])
def test_any_order_subset_chunk_and_company(name, refcpu_mod):
    s, cap, variants, eng, oracles = _case(name, refcpu_mod)
    grid, types, _ = SHAPES[name][0]
    group_of = UNEVEN
    maps = _per_replica(name, oracles, grid, types)
    eng.density_configure(grid, types, group_of)                       # again: reallocated and zeroed
    assert not any(x.any() for x in eng.density_read())
    for reps, chunk in (([4, 0, 2], None), (list(range(R + 1)), 1), (list(range(R + 1)), 2), ([3, 1, 4, 0], 2), ([2], None),
                        ([5, 3], R + 1), ([3], None)):
        eng.density_reset()
        eng.density_accumulate(reps, chunk=chunk)
        hist, samples = eng.density_read()
        want_h, want_s = pooled(maps, group_of, reps)
        assert np.array_equal(samples, want_s), (reps, chunk)
        assert np.array_equal(hist, want_h), (reps, chunk)
        h2, s2 = eng.density_read([1, 0])                               # a read of a group list, in the caller's order
        assert np.array_equal(h2, hist[[1, 0]]) and np.array_equal(s2, samples[[1, 0]])
    # two accumulations are exactly twice one
    want_h, want_s = pooled(maps, group_of)
    eng.density_reset()
    eng.density_accumulate()
    eng.density_accumulate(list(range(R + 1))[::-1], chunk=2)
    hist, samples = eng.density_read()
    assert np.array_equal(hist, 2 * want_h) and np.array_equal(samples, 2 * want_s)
    # reset zeroes only the listed group
    eng.density_reset([1])
    h3, s3 = eng.density_read()
    assert not h3[1].any() and s3[1] == 0 and np.array_equal(h3[0], hist[0]) and s3[0] == samples[0]
    # read -> reset -> load is the identity; a load of other numbers is read back
    eng.density_reset()
    assert not any(x.any() for x in eng.density_read())
    eng.density_load(hist, samples)
    assert all(np.array_equal(x, y) for x, y in zip(eng.density_read(), (hist, samples)))
    eng.density_load(hist[[0]] + np.uint64(7), np.array([9], dtype=np.uint64), groups=[1])
    h4, s4 = eng.density_read()
    assert np.array_equal(h4[1], hist[0] + np.uint64(7)) and s4[1] == 9 and np.array_equal(h4[0], hist[0]) and s4[0] == samples[0]
    # a channel counts the same alone, beside the others, and in another position
    first = types[0]
    other = [t for t in range(s.topo.n_atom_types) if t != first][:2]
    for chans in ([first], other + [first]):
        eng.density_configure(grid, chans, group_of)
        eng.density_accumulate(chunk=2)
        h5, s5 = eng.density_read()
        assert np.array_equal(h5[:, chans.index(first)], want_h[:, 0]) and np.array_equal(s5, want_s), chans
    # the coordinates were not touched
    for r in (0, 3):
        t = _first_active(s)
        assert np.array_equal(eng.get_molecules(r, t), variants[r].all_sites(t))


def test_a_type_without_atoms_and_a_replica_without_molecules(refcpu_mod):
    s, cap, variants, eng, oracles = _case("co2_20", refcpu_mod)
    eng.density_configure((3, 5, 7), [1, 0], IDENTITY)
    eng.density_accumulate([2, R])                                      # replica 2: the type emptied; replica R: never loaded
    hist, samples = eng.density_read()
    assert not hist.any() and np.array_equal(samples, [0, 0, 1, 0, 0, 1])


# ---- side effects -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixture", "triclinic_mild"])
def test_nothing_else_changes(name, refcpu_mod):
    s, cap, variants, eng, oracles = _case(name, refcpu_mod)
    reps = list(range(R + 1))
    r_max = rdf.half_width(s.box_matrix)
    eng.rdf_configure(32, r_max, [(0, 1), (1, 1)])
    eng.rdf_accumulate()
    rdf_before = eng.rdf_read()
    state_before = eng.state_export(reps)
    energy_before = eng.system_energy_replicas()
    eng.density_configure((16, 16, 16), [0, 1], UNEVEN)
    eng.density_accumulate()
    eng.density_accumulate([4, 1], chunk=1)
    hist, samples = eng.density_read()
    assert hist.any() and np.array_equal(samples, [3, 4])
    assert np.array_equal(eng.state_export(reps), state_before), "the state blocks are bitwise unchanged"
    assert np.array_equal(eng.system_energy_replicas(), energy_before)
    assert all(np.array_equal(x, y) for x, y in zip(eng.rdf_read(), rdf_before)), "the rdf accumulators are independent"
    # ... and the other way round: an rdf sample, a replica copy and a setter leave the maps alone
    eng.rdf_accumulate()
    eng.replica_copy(R, 0)
    eng.set_num_molecules(R, _first_active(s), 0)
    assert all(np.array_equal(x, y) for x, y in zip(eng.density_read(), (hist, samples)))
    eng.rdf_configure(32, r_max, [])
    assert all(np.array_equal(x, y) for x, y in zip(eng.density_read(), (hist, samples)))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _refused(code, text, call, *args, **kw):
    with pytest.raises(MgpuError) as err:
        call(*args, **kw)
    assert err.value.code == code and text in str(err.value), (code, text, str(err.value))
    return str(err.value)


def test_refusals_with_texts(refcpu_mod):
    s, cap, variants, eng, oracles = _case("mixture", refcpu_mod)       # four atom types, R + 1 = 6 replicas
    eng.density_configure((4, 4, 4), [])                                 # frees
    for call, args in ((eng.density_accumulate, ([0],)), (eng.density_read, ([0],)), (eng.density_reset, ([0],)),
                       (eng.density_load, (np.zeros((1, 1, 4, 4, 4), np.uint64), np.zeros(1, np.uint64), [0]))):
        _refused(MGPU_ERR_STATE, "configure", call, *args)
    for grid in ((0, 4, 4), (4, 1025, 4), (4, 4, -1)):
        _refused(MGPU_ERR_INVALID_ARG, "outside [1, 1024]", eng.density_configure, grid, [0])
    msg = _refused(MGPU_ERR_INVALID_ARG, "exceeds the limit of 16777216", eng.density_configure, (1024, 1024, 32), [0])
    assert str(1024 * 1024 * 32) in msg
    eng.density_configure((1024, 1024, 16), [0])                         # 2^24 voxels: at the limit, 128 MiB
    eng.density_configure((4, 4, 4), [])
    _refused(MGPU_ERR_INVALID_ARG, "n_channels 9 is outside [1, 8]", eng.density_configure, (4, 4, 4), [0, 1, 2, 3, 0, 1, 2, 3, 0])
    # (no channel at all is the call that frees; the host's spec check refuses an empty selection by name)
    from maniac_mc_amd import density
    with pytest.raises(ValueError, match="no atom type is selected"):
        density.check_types([])
    for bad in ([4], [-1], [1, 16]):
        _refused(MGPU_ERR_INVALID_ARG, "atom type out of range [0, 3]", eng.density_configure, (4, 4, 4), bad)
    for dup in ([0, 0], [2, 1, 2]):
        _refused(MGPU_ERR_INVALID_ARG, "duplicate", eng.density_configure, (4, 4, 4), dup)
    _refused(MGPU_ERR_INVALID_ARG, "group 2 is outside [0, 1]", eng.density_configure, (4, 4, 4), [0], [0, 1, 2, 0, 0, 0], 2)
    _refused(MGPU_ERR_INVALID_ARG, "group -2", eng.density_configure, (4, 4, 4), [0], [0, 1, -2, 0, 0, 0], 2)
    for n_groups in (0, R + 2):
        _refused(MGPU_ERR_INVALID_ARG, "n_groups", eng.density_configure, (4, 4, 4), [0], [0] * (R + 1), n_groups)
    # the size: 6 maps x 8... here 4 channels x 2^24 voxels x 8 bytes x 6 groups = 3 GiB, above the 2 GiB limit
    msg = _refused(MGPU_ERR_INVALID_ARG, "the limit is 2147483648", eng.density_configure, (1024, 1024, 16), [0, 1, 2, 3], IDENTITY)
    assert str((6 * 4 * (1 << 24) + 6) * 8) in msg, "the text names the size asked for"
    _refused(MGPU_ERR_STATE, "configure", eng.density_accumulate, [0])   # every refusal left it unconfigured
    eng.density_configure((4, 4, 4), [0, 3], UNEVEN)
    # a refused configure leaves the earlier one standing
    _refused(MGPU_ERR_INVALID_ARG, "duplicate", eng.density_configure, (4, 4, 4), [1, 1])
    eng.density_accumulate([0])
    assert eng.density_read()[1].tolist() == [1, 0]
    eng.density_reset()
    _refused(MGPU_ERR_INVALID_ARG, "listed twice", eng.density_accumulate, [0, 2, 0])
    _refused(MGPU_ERR_INVALID_ARG, "out of range", eng.density_accumulate, [0, R + 1])
    _refused(MGPU_ERR_INVALID_ARG, "listed twice", eng.density_reset, [1, 1])
    _refused(MGPU_ERR_INVALID_ARG, "group out of range", eng.density_read, [2])
    assert not any(x.any() for x in eng.density_read()), "a refused call counted nothing"
    eng.density_accumulate([])                                           # nothing listed is nothing to do
    assert not eng.density_read()[1].any()


# ---- the voxel edges, exactly -----------------------------------------------------------------------------------------------
def _lattice_engine(box_matrix, lo, n_atoms):
    """An engine of two replicas for n_atoms single-site molecules of one type in the given cell"""
    topo = Topology(atoms_in_res=[1], atom_types=[[1]], charges=[[0.0]], is_active=[1], epsilon=[[100.0]], sigma=[[3.0]], names=["X"])
    return Engine(topo, np.asarray(box_matrix, dtype=np.float64), np.asarray(lo, dtype=np.float64), 6.0, 1e-4, 2, 0, [n_atoms + 1])


def _expect_voxels(eng, sites, voxels, grid):
    eng.set_molecules(0, 0, np.asarray(sites, dtype=np.float64).reshape(-1, 1, 3))
    eng.density_configure(grid, [0], [0, -1])
    eng.density_accumulate()
    hist, samples = eng.density_read()
    want = np.zeros((grid[2], grid[1], grid[0]), dtype=np.uint64)
    for v0, v1, v2 in voxels:
        want[v2, v1, v0] += np.uint64(1)
    got = [tuple(int(x) for x in idx[::-1]) for idx in np.argwhere(hist[0, 0]) for _ in range(int(hist[0, 0][tuple(idx)]))]
    assert samples.tolist() == [1] and np.array_equal(hist[0, 0], want), (sorted(got), sorted(voxels))


def test_voxel_edges_of_an_orthorhombic_cell_exactly():
    # lo = (-4, -4, -4), L = (16, 16, 16), grid (8, 4, 2): voxels of 2 x 4 x 8 A; 1 / L is a power of two, every step exact
    tiny = 2.0 ** -40
    atoms = [  # (x, y, z) -> (v0, v1, v2), by hand
        ((-4.0, -4.0, -4.0), (0, 0, 0)),            # at lo exactly
        ((12.0, 12.0, 12.0), (0, 0, 0)),            # at lo + L exactly: u = n folds to 0
        ((-0.0, -0.0, -0.0), (2, 1, 0)),            # minus zero: u = (2, 1, 0.5)
        ((2.0, 4.0, 4.0), (3, 2, 1)),               # on interior voxel faces: the upper voxel
        ((-6.0, -8.0, -12.0), (7, 3, 1)),           # one voxel below lo: the last voxel
        ((-4.0 - tiny, -4.0 - tiny, -4.0 - tiny), (7, 3, 1)),   # a hair below lo: the last voxel
        ((12.0 - 16 * tiny, 3.0, 3.0), (7, 1, 0)),  # a hair below lo + L
        ((3.0 + 48.0, 1.0 + 48.0, 5.0 + 48.0), (3, 1, 1)),      # three cells up: as (3, 1, 5)
        ((3.0 - 48.0, 1.0 - 48.0, 5.0 - 48.0), (3, 1, 1)),      # three cells down
        ((-4.0 + 48.0, -4.0 - 48.0, 4.0 + 48.0), (0, 0, 1)),    # on cell corners and a face, three cells away
        ((11.0, 11.0, 11.0), (7, 3, 1)),            # inside the last voxel
    ]
    eng = _lattice_engine(np.diag([16.0, 16.0, 16.0]), [-4.0, -4.0, -4.0], len(atoms))
    try:
        _expect_voxels(eng, [a[0] for a in atoms], [a[1] for a in atoms], (8, 4, 2))
    finally:
        eng.close()


def test_voxel_edges_of_a_sheared_cell_exactly():
    # box%matrix with rows (16, 0, 0), (8, 16, 0), (4, 8, 16), as the reader stores a tilted cell; det = 2^12, so box%reciprocal
    # (= the inverse of the transpose) is dyadic too:  rows (1/16, -1/32, 0), (0, 1/16, -1/32), (0, 0, 1/16).  A site is
    # r = lo + M^T s for a dyadic s written out below; every product and sum of s = reciprocal (r - lo) is then exact.
    M = np.array([[16.0, 0.0, 0.0], [8.0, 16.0, 0.0], [4.0, 8.0, 16.0]])
    lo = np.array([-4.0, 2.0, -8.0])
    rcp = box_prepare(M)[2].reshape(3, 3)
    assert np.array_equal(rcp, [[1 / 16, -1 / 32, 0.0], [0.0, 1 / 16, -1 / 32], [0.0, 0.0, 1 / 16]])
    tiny = 2.0 ** -30
    atoms = [  # s -> (v0, v1, v2) on the grid (8, 4, 2), by hand
        ((0.0, 0.0, 0.0), (0, 0, 0)),               # at lo
        ((1.0, 1.0, 1.0), (0, 0, 0)),               # the opposite corner
        ((0.375, 0.5, 0.5), (3, 2, 1)),             # on interior faces: u = (3, 2, 1)
        ((-0.125, -0.25, -0.5), (7, 3, 1)),         # one voxel below on every axis
        ((-tiny, -tiny, -tiny), (7, 3, 1)),         # a hair below
        ((1.0 - tiny, 0.25 - tiny, 0.5 - tiny), (7, 0, 0)),     # a hair below faces
        ((3.4375, -2.6875, 3.75), (3, 1, 1)),       # three cells away: as (0.4375, 0.3125, 0.75): u = (3.5, 1.25, 1.5)
        ((-3.0, 3.0, -3.0), (0, 0, 0)),             # on far corners
        ((0.9375, 0.9375, 0.9375), (7, 3, 1)),      # inside the last voxel
    ]
    s = np.array([a[0] for a in atoms])
    sites = lo[None, :] + s @ M                     # (M^T s)_i = sum_j M[j][i] s_j
    back = (sites - lo[None, :]) @ rcp.T
    assert np.array_equal(back, s), "the construction is exact"
    eng = _lattice_engine(M, lo, len(atoms))
    try:
        _expect_voxels(eng, sites, [a[1] for a in atoms], (8, 4, 2))
    finally:
        eng.close()
