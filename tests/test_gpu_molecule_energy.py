"""Per-molecule removal energies (mgpu_molecule_energies_replicas, Engine.molecule_energies_replicas) against the reference.

u[c](t, m) = E[c](X) - E[c](X without m).  The oracle is RefCPU.system_energy() with and without the molecule: the type's last
molecule is copied into slot m (set_molecule), the count lowered by one (set_num_residues), and both are restored.  For every
molecule of every selected type and every variant every component c holds
    |device - (E_with[c] - E_without[c])| <= tol_for(E_with[c]) + tol_for(E_without[c]) + tol_for(device),
the bar tests/test_gpu_energy_pairs.py uses for a difference of static totals; nothing else is added.  Besides, with no
cancellation in the oracle: non_coulomb and coulomb against RefCPU.pair_singlemol(t, m) within tol_for(oracle, device), self
against self_singlemol(t), intra against intra_singlemol(t, m).

Systems, variants and the sixth, never loaded replica are those of tests/test_gpu_energy_pairs.py: the three-type box (70
one-site molecules: a plane crosses a 64-lane unit; one type uncharged), spce216, co2_20 with capacity + 3, framework_small
(guest against a frozen inactive type), the 24-site adsorbate (the LDS slab), the 64-site one with 4 molecules (site-major, site
tiles in the reciprocal kernel: 64 sites x ktot rows exceed its LDS tile), the mild and the sheared triclinic cell.  (spce216's
oracle is 860 whole-system energies on the CPU, some 13 s: the issue's case, every molecule of every variant.)"""
import ctypes as C

import numpy as np
import pytest

from maniac_mc_amd import molecule_energy as me
from maniac_mc_amd._lib import MgpuError
from maniac_mc_amd.engine import Engine
from tests.test_gpu_energy_pairs import NAMES, SYSTEMS, _five
from tests.test_gpu_rdf import _capacity, _first_active, _load, _variants
from tests.util import tol_for

pytestmark = pytest.mark.gpu

MGPU_ERR_INVALID_ARG = 1
R = 5                 # replicas with their own configurations; replica R is never loaded (no atoms)
NC, CO, RE, SE, IN = range(5)

_cases = {}


def _active(s):
    return [t for t in range(s.topo.n_res) if s.topo.is_active[t] == 1]


def _row0(cap, types):
    """first row of every selected type"""
    return np.concatenate([[0], np.cumsum([cap[t] for t in types])[:-1]]).astype(int)


def _case(name):
    """The system, its capacities, the five variants, an engine of R + 1 replicas loaded with them, the active types and the
    device's energies and counts for all of them: built once per system and shared, unchanged, by the tests."""
    if name not in _cases:
        s = SYSTEMS[name]()
        cap = _capacity(name, s)
        variants = _variants(name, s, cap)
        eng = Engine(s.topo, s.box_matrix, s.bounds_lo, s.real_space_cutoff, s.ewald_tolerance, R + 1, 0, cap)
        _load(eng, variants, _first_active(s))
        types = _active(s)
        full, counts = eng.molecule_energies_replicas(types)
        _cases[name] = (s, cap, variants, eng, types, full, counts)
    return _cases[name]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for c in _cases.values():
        c[3].close()
    _cases.clear()


def _counts_of(variants, r, t, first):
    return 0 if r == 2 and t == first else int(variants[r].n_mol[t])


@pytest.mark.parametrize("name", NAMES)
def test_every_molecule_against_the_oracle(name, refcpu_mod):
    s, cap, variants, eng, types, full, counts = _case(name)
    first = _first_active(s)
    rows = sum(cap[t] for t in types)
    assert full.shape == (R + 1, rows, 5) and full.dtype == np.float64
    assert counts.shape == (R + 1, len(types)) and counts.dtype == np.int32
    row0 = _row0(cap, types)
    worst = worst_direct = 0.0
    n_checked = 0
    for r, v in enumerate(variants):
        n_of = [_counts_of(variants, r, t, first) for t in range(s.topo.n_res)]
        assert counts[r].tolist() == [n_of[t] for t in types]
        P = refcpu_mod.RefCPU(v, mol_capacity=max(8, int(max(v.n_mol)) + 1))
        for t in range(s.topo.n_res):
            P.set_num_residues(t, n_of[t])
        e_with = _five(P.system_energy())
        for k, t in enumerate(types):
            n = n_of[t]
            self_want = P.self_singlemol(t)
            for m in range(n):
                got = full[r, row0[k] + m]
                # ---- no cancellation in the oracle: the molecule's own pair, self and intra terms
                nc, co = P.pair_singlemol(t, m)
                for c, want in ((NC, nc), (CO, co), (SE, self_want), (IN, P.intra_singlemol(t, m))):
                    ratio = abs(got[c] - want) / tol_for(want, got[c])
                    worst_direct = max(worst_direct, ratio)
                    assert ratio <= 1.0, (name, r, t, m, c, got[c], want)
                # ---- the difference of two static totals
                keep = P.get_molecule(t, m)
                if m != n - 1:
                    P.set_molecule(t, m, *P.get_molecule(t, n - 1))
                P.set_num_residues(t, n - 1)
                e_without = _five(P.system_energy())
                P.set_num_residues(t, n)
                P.set_molecule(t, m, *keep)
                for c in range(5):
                    tol = tol_for(e_with[c]) + tol_for(e_without[c]) + tol_for(got[c])
                    ratio = abs(got[c] - (e_with[c] - e_without[c])) / tol
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (name, r, t, m, c, got[c], e_with[c] - e_without[c], tol)
                n_checked += 1
        assert np.array_equal(_five(P.system_energy()), e_with), "the oracle was restored"
        P.close()
    print(f"{name}: {n_checked} molecules; largest |difference| / tolerance = {worst:.3e} (totals), {worst_direct:.3e} (single-molecule terms)")
    assert n_checked > 0 and np.any(full[0, :, NC] != 0.0)


def test_the_pair_terms_add_up_to_twice_the_totals():
    name = "three_types"
    s, cap, variants, eng, types, full, counts = _case(name)
    assert types == [0, 1, 2], "all types are active and selected"
    total = eng.system_energy_replicas()
    for r in range(R + 1):
        for c in (NC, CO):
            live = np.concatenate([full[r, r0:r0 + n, c] for r0, n in zip(_row0(cap, types), counts[r])])
            tol = sum(tol_for(u) for u in live) + 2 * tol_for(total[r, c])
            assert abs(live.sum() - 2.0 * total[r, c]) <= tol, (r, c, live.sum(), 2.0 * total[r, c], tol)


@pytest.mark.parametrize("name", NAMES)
def test_bit_for_bit_whatever_shares_the_call(name):
    s, cap, variants, eng, types, full, counts = _case(name)
    everyone = list(range(R + 1))
    for chunk in (1, 2):
        e, n = eng.molecule_energies_replicas(types, chunk=chunk)
        assert np.array_equal(e, full) and np.array_equal(n, counts), chunk
    e, n = eng.molecule_energies_replicas(types, everyone[::-1])
    assert np.array_equal(e, full[::-1]) and np.array_equal(n, counts[::-1])
    e, n = eng.molecule_energies_replicas(types, [3, 0, 4], chunk=2)
    assert np.array_equal(e, full[[3, 0, 4]]) and np.array_equal(n, counts[[3, 0, 4]])
    # one type alone, and in a two-type selection in either order
    row0 = _row0(cap, types)
    for k, t in enumerate(types):
        mine = full[:, row0[k]:row0[k] + cap[t]]
        e, n = eng.molecule_energies_replicas([t])
        assert np.array_equal(e, mine) and np.array_equal(n[:, 0], counts[:, k]), t
        for j, u in enumerate(types):
            if u == t:
                continue
            other = full[:, row0[j]:row0[j] + cap[u]]
            e, n = eng.molecule_energies_replicas([t, u])
            assert np.array_equal(e, np.concatenate([mine, other], axis=1)) and n.tolist() == counts[:, [k, j]].tolist()
            e, n = eng.molecule_energies_replicas([u, t])
            assert np.array_equal(e, np.concatenate([other, mine], axis=1)) and n.tolist() == counts[:, [j, k]].tolist()
    e, n = eng.molecule_energies_replicas(types)
    assert np.array_equal(e, full) and np.array_equal(n, counts), "a repeated call"


@pytest.mark.parametrize("name", NAMES)
def test_edge_results_and_nothing_else_changes(name):
    s, cap, variants, eng, types, full, counts = _case(name)
    first = _first_active(s)
    row0 = _row0(cap, types)
    assert np.all(counts[R] == 0) and np.all(full[R] == 0.0), "the replica never loaded"
    k = types.index(first)
    assert counts[2, k] == 0 and np.all(full[2, row0[k]:row0[k] + cap[first]] == 0.0), "the emptied type"
    for r in range(R + 1):
        for j, t in enumerate(types):
            assert np.all(full[r, row0[j] + counts[r, j]:row0[j] + cap[t]] == 0.0), "rows beyond the count are exactly 0.0"
            live = full[r, row0[j]:row0[j] + counts[r, j]]
            if name == "three_types" and t == 2:
                assert np.all(live[:, [CO, RE, SE, IN]] == 0.0), "a type without a charged site"
                assert r in (R,) or np.any(live[:, NC] != 0.0)
            elif counts[r, j]:
                assert np.all(live[:, SE] == live[0, SE]), "one self term per type"
    assert counts[3, k] == cap[first], "the variant at capacity fills every row of its type"
    # A(k) of every replica is unchanged by the call, bit for bit, and so are the coordinates and the energies
    eng.init_structure_factor_replicas()

    def state():
        return ([eng.structure_factor(r) for r in range(R + 1)],
                [eng.get_molecules(r, t) for r in range(R + 1) for t in range(s.topo.n_res)], eng.system_energy_replicas())

    before = state()
    e, n = eng.molecule_energies_replicas(types, chunk=2)
    assert np.array_equal(e, full)
    after = state()
    for x, y in zip(before[0] + before[1], after[0] + after[1]):
        assert np.array_equal(x, y)
    assert np.array_equal(before[2], after[2])
    # the numpy restatement of the total is what the histograms will bin
    assert np.array_equal(me.total_energy(full), (((full[..., 0] + full[..., 1]) + full[..., 2]) + full[..., 3]) + full[..., 4])


def _raw(eng, reps, types, n_sel=None):
    """the C call itself: (code, text, out, counts) with the outputs prefilled with sentinels"""
    reps = np.ascontiguousarray(reps, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    ty = None if types is None else np.ascontiguousarray(types, dtype=np.int32)
    n_sel = (0 if ty is None else ty.size) if n_sel is None else n_sel
    out = np.full((reps.size, int(sum(eng.mol_capacity)), 5), -7.25)
    counts = np.full((reps.size, max(1, n_sel)), -3, dtype=np.int32)
    rc = eng.L.mgpu_molecule_energies_replicas(eng.h, C.c_int(reps.size), reps.ctypes.data_as(ip), C.c_int(0), C.c_int(n_sel),
                                               None if ty is None else ty.ctypes.data_as(ip),
                                               out.ctypes.data_as(C.POINTER(C.c_double)), counts.ctypes.data_as(ip))
    return rc, eng.L.mgpu_last_error().decode(), out, counts


def test_refusals_with_texts():
    s, cap, variants, eng, types, full, counts = _case("framework_small")
    assert s.topo.is_active[0] != 1 and types == [1]
    for ty, n_sel, text in (([0], None, "type 0 (residue type 0) is not an active type"),
                            ([1, 1], None, "type 1 (residue type 1) is a duplicate"),
                            ([2], None, "type 0 (residue type 2) is out of range [0, 1]"),
                            ([-1], None, "type 0 (residue type -1) is out of range"),
                            ([1], 0, "n_sel 0 types is outside [1, 8]"),
                            ([1] * 9, 9, "n_sel 9 types is outside [1, 8]"),
                            (None, 1, "null type list")):
        rc, msg, out, cnt = _raw(eng, [0, 1], ty, n_sel)
        assert rc == MGPU_ERR_INVALID_ARG and text in msg, (rc, msg, text)
        assert np.all(out == -7.25) and np.all(cnt == -3), "a refused call writes nothing"
    rc, msg, out, cnt = _raw(eng, [0, 3, 0], [1])
    assert rc == MGPU_ERR_INVALID_ARG and "replica 0 listed twice" in msg and np.all(out == -7.25) and np.all(cnt == -3)
    for bad in ([0], [1, 1], []):
        with pytest.raises(MgpuError) as err:
            eng.molecule_energies_replicas(bad)
        assert err.value.code == MGPU_ERR_INVALID_ARG
    with pytest.raises(MgpuError) as err:
        eng.molecule_energies_replicas([1], [2, 2])
    assert err.value.code == MGPU_ERR_INVALID_ARG and "listed twice" in str(err.value)
    # nothing listed is nothing to do; the engine still answers
    e, n = eng.molecule_energies_replicas([1], [])
    assert e.shape == (0, cap[1], 5) and n.shape == (0, 1)
    e, n = eng.molecule_energies_replicas(types)
    assert np.array_equal(e, full) and np.array_equal(n, counts)
