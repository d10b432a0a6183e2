"""The reciprocal-space update held to the oracle (oracle/refcpu.c) at the edges of its forms: every kernel launch_recip
(mgpu_launch.hip) can choose -- the narrow row form, the vector and matrix-unit wide row forms (one tile of site-states or
several), the per-k form with its site tiles -- on both sides of each LDS budget boundary, in k-space shapes that give row
tiles of few rows and rows of many kz (kmax_z 15 / 16 / 17, where the matrix-unit sweep's kz column tiles change), rows
whose only task is kz = 0, a sheared cell, single ions, uncharged and net-charged molecules and candidates outside the
cell.  Every case asserts the form it claims through Engine.recip_form (mgpu_recip_form), so that a change of a budget
constant cannot move a case to another form unnoticed, and compares with the oracle, never with another form:
energies to tol_for, A(k) after commits to 1e-10.

Mixed launches: the form of a molecule's update is that of its own residue type, whatever shares its launch (DESIGN
section 4.2), so a candidate's energies are bitwise those of a launch of its type alone, and a trial and its commit share
the sum order.  The intra-molecular sum is checked at the 32 / 33-site switch between intra_kernel and
intra_wave_kernel and at its 512-site LDS tiles."""
import contextlib
import os

import numpy as np
import pytest

from maniac_mc_amd import _lib, synth
from maniac_mc_amd._lib import MGPU_CREATION, MGPU_DELETION, MGPU_MOVE, MGPU_NONE
from maniac_mc_amd.engine import Engine, box_prepare, ewald_setup
from maniac_mc_amd.synth import lorentz_berthelot
from maniac_mc_amd.system import System, Topology
from tests.util import tol_for

MGPU_ERR_CAPACITY, MGPU_ERR_STATE = 3, 5

# k-space shapes (box diagonal or matrix, rc, tol) and the kmax mgpu_ewald_setup gives them (checked on the CPU)
SHAPES = {
    "kz15": (np.diag([24.0, 24.0, 57.0]), 10.0, 1e-5, (6, 6, 15)),
    "kz16": (np.diag([24.0, 24.0, 61.0]), 10.0, 1e-5, (6, 6, 16)),
    "kz17": (np.diag([24.0, 24.0, 64.0]), 10.0, 1e-5, (6, 6, 17)),
    "thin": (np.diag([7.0, 7.0, 180.0]), 3.0, 1e-2, (2, 2, 46)),
    "flat": (np.diag([120.0, 120.0, 4.5]), 3.0, 1e-2, (31, 31, 1)),
    "sheared": (np.array([[26.0, 0.0, 0.0], [11.0, 26.0, 0.0], [-9.0, 8.5, 26.0]]), 10.0, 1e-5, None),
}
# boxes of the budget-boundary cases: the switches sit at different n1 for different Nk and row counts
BUDGET_BOXES = {"cube26": np.diag([26.0, 26.0, 26.0]), "box22x34": np.diag([22.0, 22.0, 34.0])}
# the matrix-unit form's row records (n_rows int4) leave no room for four site-states: (51, 51, 1), 4138 rows
NO_ROOM_BOX = (np.diag([150.0, 150.0, 3.5]), 2.0, 1e-2, (51, 51, 1))


def kmax_of(box, rc, tol):
    _, _, _, met = box_prepare(box)
    return tuple(int(k) for k in ewald_setup(met, rc, tol)["kmax"])


# ---------------------------------------------------------------------------------------------------------------------
# systems
def shell(n_sites, seed=23, net_charge=0.0, charged=True):
    """template, atom types (1..3), charges of the synthetic shell of synth.large_adsorbate_box; net_charge spread over the
    charged sites, charged=False: every site uncharged."""
    s = synth.large_adsorbate_box(n_sites=n_sites, n_mol=1, L=4.0 * n_sites + 100.0, seed=seed)
    q = np.array(s.topo.charges[0][:n_sites], dtype=np.float64)
    if not charged:
        q[:] = 0.0
    elif net_charge:
        nz = q != 0.0 if np.any(q != 0.0) else np.ones(n_sites, bool)
        q[nz] += net_charge / np.count_nonzero(nz)
    return s.offsets[0][0].copy(), np.array(s.topo.atom_types[0][:n_sites], np.int32), q


def water():
    t = np.array([[0.0, 0.0, 0.0], [0.8165, 0.5773, 0.0], [-0.8165, 0.5773, 0.0]])
    return t - t.mean(0), np.array([1, 2, 2], np.int32), np.array([-0.8476, 0.4238, 0.4238])


def ion(q=1.0):
    return np.zeros((1, 3)), np.array([1], np.int32), np.array([q])


def make_system(box, specs, rc=10.0, tol=1e-5, seed=5, gap=2.5):
    """specs: [(template, types, charges, n_mol)]; molecules at random places and orientations, surfaces at least `gap`
    apart (minimum image, fractional coordinates: any cell)."""
    box = np.asarray(box, dtype=np.float64)
    rng = np.random.default_rng(seed)
    lo = -0.5 * box.sum(0)
    n_t = len(specs)
    max_atom = max(len(sp[1]) for sp in specs)
    types = np.zeros((n_t, max_atom), np.int32)
    charges = np.zeros((n_t, max_atom))
    eps_d, sig_d = [], []
    base = 0
    for i, (tmpl, ty, q, _) in enumerate(specs):
        types[i, :len(ty)] = ty + base
        charges[i, :len(q)] = q
        for k in range(int(ty.max())):
            eps_d.append(0.05 + 0.03 * ((base + k) % 4)); sig_d.append(2.6 + 0.2 * ((base + k) % 3))
        base += int(ty.max())
    eps, sig = lorentz_berthelot(eps_d, sig_d)
    topo = Topology(atoms_in_res=[len(sp[1]) for sp in specs], atom_types=types, charges=charges, is_active=[1] * n_t,
                    epsilon=eps, sigma=sig)
    placed, coms, offs = [], [], []
    inv = np.linalg.inv(box)
    for tmpl, ty, q, n_mol in specs:
        rad = float(np.max(np.linalg.norm(tmpl, axis=1)))
        c_t = []
        while len(c_t) < n_mol:
            f = rng.uniform(0.0, 1.0, 3)
            p = lo + f @ box
            ok = True
            for (pp, rr) in placed:
                d = (p - pp) @ inv
                d -= np.rint(d)
                if np.linalg.norm(d @ box) < rad + rr + gap:
                    ok = False
                    break
            if ok:
                placed.append((p, rad)); c_t.append(p)
        coms.append(np.array(c_t).reshape(-1, 3))
        offs.append(np.einsum("mij,aj->mai", synth._random_rotations(rng, n_mol), tmpl) if n_mol else np.zeros((0, len(ty), 3)))
    return System(topo, box, lo, rc, tol, 300.0, coms, offs)


@contextlib.contextmanager
def form_env(name):
    """MGPU_RECIP_NO_MFMA / MGPU_RECIP_PER_K are read at engine creation: set around Engine.from_system only."""
    var = {"vector": "MGPU_RECIP_NO_MFMA", "per-k": "MGPU_RECIP_PER_K"}.get(name)
    if var:
        os.environ[var] = "1"
    try:
        yield
    finally:
        if var:
            os.environ.pop(var, None)


def engine(s, env=None, n_replicas=1, cap=None):
    with form_env(env):
        eng = Engine.from_system(s, n_replicas=n_replicas, mol_capacity=cap)
    for r in range(n_replicas):
        eng.init_structure_factor(r, True)
    return eng


def assert_form(eng, n1, form, **shape):
    for commit in (False, True):
        got = eng.recip_form(n1, commit=commit)
        assert got["form"] == form, f"n1 = {n1}: the {'commit' if commit else 'trial'} takes {got}, not the {form} form"
        for k, v in shape.items():
            assert got[k] == v, f"n1 = {n1}: {got}, expected {k} = {v}"
    return eng.recip_form(n1)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
def close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    tol = tol_for(*np.ravel(b), *np.ravel(a))
    err = float(np.max(np.abs(a - b)))
    assert err <= tol, f"{what}: |diff| = {err:.3e} K > tol {tol:.3e} K\n got {a}\n ref {b}"


def amp_close(a, b, what):
    err = float(np.max(np.abs(np.asarray(a) - np.asarray(b))))
    assert err <= 1e-10, f"{what}: max |dA| = {err:.3e}"


def oracle(s, cap):
    from oracle import refcpu
    refcpu.build()
    P = refcpu.RefCPU(s, mol_capacity=cap)
    P.system_energy()
    sync(P)
    return P


def sync(P):
    """The oracle's A(k) and stored reciprocal energy from scratch for its current molecules."""
    P.all_fourier_terms()
    P.init_amplitude(True)
    P.set_energy_recip(P.recip_total())


def o_move(P, t, m, sites):
    A0 = P.amplitude()
    com, off = P.get_molecule(t, m)
    P.save_fourier(t, m)
    eo = P.old_energy(t, m, 0)[:3]
    P.set_molecule(t, m, sites[0], sites - sites[0][None, :])
    en = P.new_energy(t, m, 0)[:3]
    P.set_molecule(t, m, com, off)
    P.restore_fourier(t, m)
    P.set_amplitude(A0)
    return eo, en


def o_insert(P, t, sites):
    A0 = P.amplitude()
    n = P.num_residues(t)
    eo = P.old_energy(t, n, 1)[:5]
    P.set_num_residues(t, n + 1)
    P.save_fourier(t, n)
    P.set_molecule(t, n, sites[0], sites - sites[0][None, :])
    en = P.new_energy(t, n, 1)[:5]
    P.set_num_residues(t, n)
    P.set_amplitude(A0)
    return eo, en


def o_delete(P, t, m):
    A0 = P.amplitude()
    P.all_fourier_terms()
    eo = P.old_energy(t, m, 2)[:5]
    P.save_fourier(t, m)
    en = np.zeros(5)
    en[2] = P.recip_singlemol(t, m, 2)       # intended physics: A - S_mol (the engine's deletion)
    P.set_amplitude(A0)
    return eo, en


def o_intra(P, t, m, sites=None):
    if sites is None:
        return P.intra_singlemol(t, m)
    com, off = P.get_molecule(t, m)
    P.set_molecule(t, m, sites[0], sites - sites[0][None, :])
    u = P.intra_singlemol(t, m)
    P.set_molecule(t, m, com, off)
    return u


def moved(P, s, t, m, rng, step=0.4):
    com, off = P.get_molecule(t, m)
    ax = 1 + int(rng.integers(0, 3))
    return P.apply_pbc(com + rng.uniform(-step, step, 3))[None, :] + off @ P.rotation_matrix(ax, float(rng.uniform(-0.3, 0.3))).T


def free_spot(eng, s, t, rng, outside=0.0):
    """sites of a new molecule of type t (slot 0's template, rotated) at least a surface gap from every molecule; outside > 0:
    the same place one cell over, its centre up to `outside` beyond a face of the cell (the engine and the oracle fold it)."""
    box = np.asarray(s.box_matrix, float)
    inv = np.linalg.inv(box)
    tmpl = s.offsets[t][0]
    rad = float(np.max(np.linalg.norm(tmpl, axis=1)))
    allc = [(eng.get_molecules(0, tt)) for tt in range(s.topo.n_res)]
    face = int(rng.integers(0, 3))
    for _ in range(4000):
        f = rng.uniform(0.0, 1.0, 3)
        if outside:
            f[face] = rng.uniform(0.0, outside / np.linalg.norm(box[face]))
        p = s.bounds_lo + f @ box
        ok = True
        for tt, sites in enumerate(allc):
            if sites.shape[0] == 0:
                continue
            d = (sites.reshape(-1, 3) - p) @ inv
            d -= np.rint(d)
            if np.min(np.linalg.norm(d @ box, axis=1)) < rad + 2.5:
                ok = False
                break
        if ok:
            break
    else:
        raise AssertionError("no free spot for an insertion")
    if outside:
        p = p + box[face]
    return p[None, :] + tmpl @ synth._random_rotations(rng, 1)[0].T


# ---------------------------------------------------------------------------------------------------------------------
# one case: trial batch, new-only trial, insertion + deletion, committed move / insertion / deletion by swap-with-last
def exercise(eng, P, s, t, label, rng, n_batch=4, outside=0.0, commits=True):
    n1 = int(s.topo.atoms_in_res[t])
    n = eng.num_molecules(0, t)
    assert n >= 2 and P.num_residues(t) == n
    zeros = lambda k: np.zeros(k, np.int32)
    # --- a batch of trial moves (old + new in one pass)
    ms = np.arange(min(n, n_batch), dtype=np.int32)
    sites = np.stack([moved(P, s, t, int(m), rng) for m in ms])
    if outside:            # the first candidate one cell over: its centre beyond a face
        sites[0] += np.asarray(s.box_matrix, float)[int(rng.integers(0, 3))][None, :]
    exp = [o_move(P, t, int(m), sites[i]) for i, m in enumerate(ms)]
    old, new = eng.trial_energy_candidates(zeros(len(ms)), np.full(len(ms), t, np.int32), ms, sites)
    close(old, [e[0] for e in exp], f"{label}: batch old")
    close(new, [e[1] for e in exp], f"{label}: batch new")
    # --- a new-only trial (the insertion's k sweep alone) and an insertion + a deletion in one grand-canonical batch
    csite = free_spot(eng, s, t, rng, outside)
    ins_o, ins_n = o_insert(P, t, csite)
    u = eng.recip_energy_candidates([0], [t], [-1], [MGPU_CREATION], csite[None])
    close(u[0], ins_n[2], f"{label}: new-only recip")
    md = n - 1
    del_o, del_n = o_delete(P, t, md)
    rows = np.zeros((2, n1, 3)); rows[0] = csite
    o5, n5 = eng.gcmc_trial([0, 0], [t, t], [-1, md], [MGPU_CREATION, MGPU_DELETION], rows)
    close(o5[0], ins_o, f"{label}: insertion old")
    close(n5[0], ins_n, f"{label}: insertion new")
    close(o5[1], del_o, f"{label}: deletion old")
    close(n5[1], del_n, f"{label}: deletion new")
    if not commits:
        return
    # --- committed move
    m = int(ms[0])
    eng.commit_candidates([0], [t], [m], [MGPU_MOVE], sites[0:1], [1])
    P.set_molecule(t, m, sites[0, 0], sites[0] - sites[0, 0][None, :])
    sync(P)
    amp_close(eng.structure_factor(0), P.amplitude(), f"{label}: A after the committed move")
    assert np.array_equal(eng.get_molecules(0, t)[m], sites[0])
    # --- committed insertion
    eng.commit_candidates([0], [t], [-1], [MGPU_CREATION], csite[None], [1])
    P.set_num_residues(t, n + 1)
    P.set_molecule(t, n, csite[0], csite - csite[0][None, :])
    sync(P)
    assert eng.num_molecules(0, t) == n + 1
    assert np.array_equal(eng.get_molecules(0, t)[n], csite)
    amp_close(eng.structure_factor(0), P.amplitude(), f"{label}: A after the committed insertion")
    # --- committed deletion of molecule 0: the last one takes its slot
    last = eng.get_molecules(0, t)[n].copy()
    eng.commit_candidates([0], [t], [0], [MGPU_DELETION], None, [1])
    lcom, loff = P.get_molecule(t, n)
    P.set_molecule(t, 0, lcom, loff)
    P.set_num_residues(t, n)
    sync(P)
    assert eng.num_molecules(0, t) == n
    assert np.array_equal(eng.get_molecules(0, t)[0], last)
    amp_close(eng.structure_factor(0), P.amplitude(), f"{label}: A after the committed deletion")
    # the energies of the state the commits left, against the oracle's from scratch
    ms = np.arange(min(n, 2), dtype=np.int32)
    sites = np.stack([moved(P, s, t, int(m), rng) for m in ms])
    exp = [o_move(P, t, int(m), sites[i]) for i, m in enumerate(ms)]
    old, new = eng.trial_energy_candidates(zeros(len(ms)), np.full(len(ms), t, np.int32), ms, sites)
    close(old, [e[0] for e in exp], f"{label}: old after the commits")
    close(new, [e[1] for e in exp], f"{label}: new after the commits")


def switch_n1(eng, pred, lo=1, hi=2000):
    """the largest n1 in [lo, hi) for which pred(recip_form(n1)) holds, pred holding at lo and failing above the switch"""
    assert pred(eng.recip_form(lo))
    n1 = lo
    while n1 + 1 < hi and pred(eng.recip_form(n1 + 1)):
        n1 += 1
    assert n1 + 1 < hi, "no switch below the search bound"
    return n1


# ---------------------------------------------------------------------------------------------------------------------
# (a) budget boundaries
def _probe(box, env=None):
    s = make_system(box, [(*water(), 2)])
    with form_env(env):
        return Engine.from_system(s, n_replicas=1)


def _case_at(box, n1, env, label, seed, expect):
    rng = np.random.default_rng(seed)
    L = float(np.min(np.diag(box)))
    rad = float(np.sqrt(n1 * 1.2 ** 2 * 1.6 / (4 * np.pi)))
    n_mol = 3 if 2 * (2 * rad + 3.0) < L else 2
    s = make_system(box, [(*shell(n1, seed=seed), n_mol)], seed=seed, gap=2.0)
    eng = engine(s, env)
    got = assert_form(eng, n1, expect[0], **expect[1])
    P = oracle(s, n_mol + 8)
    exercise(eng, P, s, 0, f"{label} n1 = {n1} ({got})", rng, n_batch=n_mol)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("box", list(BUDGET_BOXES))
def test_rows_to_wide_boundary(refcpu_mod, box):
    b = BUDGET_BOXES[box]
    p = _probe(b)
    n1 = switch_n1(p, lambda f: f["form"] == "rows")
    wide = p.recip_form(n1 + 1)
    p.close()
    assert wide["form"] == "wide-mfma"
    _case_at(b, n1, None, f"{box} rows", 40 + n1, ("rows", {}))
    _case_at(b, n1 + 1, None, f"{box} wide", 41 + n1, ("wide-mfma", {"site_tiles": 1}))


@pytest.mark.gpu
@pytest.mark.parametrize("box", list(BUDGET_BOXES))
def test_mfma_one_to_two_site_tiles(refcpu_mod, box):
    b = BUDGET_BOXES[box]
    p = _probe(b)
    n1 = switch_n1(p, lambda f: f["form"] != "wide-mfma-tiled", lo=1)
    one, two = p.recip_form(n1), p.recip_form(n1 + 1)
    p.close()
    assert one["form"] == "wide-mfma" and one["site_tiles"] == 1
    assert two["form"] == "wide-mfma-tiled" and two["site_tiles"] == 2
    assert ((2 * (n1 + 1) + 3) & ~3) > one["site_states"], "n1* + 1 is the first whose padded site-states exceed a tile"
    cases = [n1, n1 + 1] + ([n1 + 2] if (n1 + 1) % 2 == 0 else [])      # an odd n1 among the tiled ones
    for c in cases:
        f = ("wide-mfma", {"site_tiles": 1}) if c == n1 else ("wide-mfma-tiled", {"site_tiles": 2})
        _case_at(b, c, None, f"{box} mfma", 50 + c, f)


@pytest.mark.gpu
@pytest.mark.parametrize("box", list(BUDGET_BOXES))
def test_per_k_one_to_two_site_tiles(refcpu_mod, box):
    b = BUDGET_BOXES[box]
    p = _probe(b, "per-k")
    n1 = switch_n1(p, lambda f: f["site_tiles"] == 1)
    assert p.recip_form(n1)["form"] == "per-k" and p.recip_form(n1 + 1)["site_tiles"] == 2
    p.close()
    _case_at(b, n1, "per-k", f"{box} per-k", 60 + n1, ("per-k", {"site_tiles": 1}))
    _case_at(b, n1 + 1, "per-k", f"{box} per-k", 61 + n1, ("per-k", {"site_tiles": 2}))


@pytest.mark.gpu
@pytest.mark.parametrize("box", list(BUDGET_BOXES))
def test_vector_wide_to_per_k_boundary(refcpu_mod, box):
    b = BUDGET_BOXES[box]
    p = _probe(b, "vector")
    lo = switch_n1(p, lambda f: f["form"] == "rows") + 1
    n1 = switch_n1(p, lambda f: f["form"] == "wide-vector", lo=lo)
    rpt = p.recip_form(n1)["rows_per_tile"]
    assert rpt >= 8 and p.recip_form(n1 + 1)["form"] == "per-k"
    p.close()
    _case_at(b, lo, "vector", f"{box} vector", 70 + lo, ("wide-vector", {}))
    _case_at(b, n1, "vector", f"{box} vector", 70 + n1, ("wide-vector", {"rows_per_tile": rpt}))
    _case_at(b, n1 + 1, "vector", f"{box} per-k", 71 + n1, ("per-k", {}))


@pytest.mark.gpu
def test_mfma_row_records_leave_no_room(refcpu_mod):
    """(51, 51, 1): 4138 rows of int4 records beside the tables leave no room for four site-states, so a molecule past the
    row form's budget takes the vector wide form or the per-k form, never the matrix-unit one."""
    box, rc, tol, _ = NO_ROOM_BOX
    s = make_system(box, [(*water(), 6), (*shell(8, seed=3), 3)], rc=rc, tol=tol, gap=1.0)
    eng = engine(s)
    kv = eng.kvectors()
    rows = len(set(zip(kv["kx"].tolist(), kv["ky"].tolist())))
    assert rows * 16 + 4 * ((int(eng.kmax.sum()) + 3) * 16 + 8) > 60 * 1024
    big = eng.recip_form(8)
    assert big["form"] in ("wide-vector", "per-k"), big
    P = oracle(s, 14)
    rng = np.random.default_rng(4)
    exercise(eng, P, s, 1, f"no-room {big['form']}", rng, n_batch=3)
    exercise(eng, P, s, 0, "no-room water", rng, n_batch=3)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# (b) k-space shapes, each in the narrow, matrix-unit and vector forms
# (the flat box's 2016 rows leave no room for the row form's XY table even at one site: there it is the per-k form)
SHAPE_CASES = [(sh, f) for sh in SHAPES for f in (["per-k"] if sh == "flat" else ["rows"]) + ["wide-mfma", "wide-vector"]]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,form", SHAPE_CASES)
def test_k_space_shapes(refcpu_mod, shape, form):
    box, rc, tol, _ = SHAPES[shape]
    thin = shape in ("thin", "flat")
    gap = 0.8 if thin else 2.5
    env = {"wide-vector": "vector", "per-k": "per-k"}.get(form)
    if form == "rows":
        spec = [(*water(), 8)]
        n1 = 3
    elif shape == "flat":       # a 4.5 A slab: a flat molecule (a ring of ten sites) lies in it
        n1 = 10
        ang = 2 * np.pi * np.arange(n1) / n1
        spec = [(np.stack([1.6 * np.cos(ang), 1.6 * np.sin(ang), np.zeros(n1)], 1), *shell(n1, seed=7)[1:], 4)]
    else:
        n1 = 22 if thin else 24      # (22 sites: past the row form's budget in the thin box's nine rows, within the vector form's)
        spec = [(*shell(n1, seed=7), 4 if thin else 3)]
    s = make_system(box, spec, rc=rc, tol=tol, gap=gap, seed=11)
    eng = engine(s, env)
    assert_form(eng, n1, form)
    P = oracle(s, 16)
    rng = np.random.default_rng(13)
    exercise(eng, P, s, 0, f"{shape} {form}", rng, n_batch=4)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# (c) charges and geometry
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["rows", "wide-mfma", "wide-vector", "per-k"])
def test_single_ion_uncharged_and_net_charged(refcpu_mod, form):
    env = {"wide-vector": "vector", "per-k": "per-k"}.get(form)
    big = 24
    s = make_system(np.diag([30.0, 30.0, 30.0]),
                    [(*ion(1.0), 4), (*shell(big, seed=9, charged=False), 3), (*shell(big, seed=10, net_charge=-1.0), 3)], seed=3)
    eng = engine(s, env)
    assert_form(eng, 1, "rows" if form in ("rows", "wide-mfma", "wide-vector") else "per-k")
    if form != "rows":
        assert_form(eng, big, form)
    assert s.topo.charges[2][:big].sum() == pytest.approx(-1.0)
    P = oracle(s, 12)
    rng = np.random.default_rng(17)
    exercise(eng, P, s, 0, f"ion ({form})", rng)
    if form != "rows":
        exercise(eng, P, s, 2, f"net-charged ({form})", rng, n_batch=3)
    # every site uncharged: delta = 0, so A(k) comes back bit for bit after a committed move / insertion / deletion
    A0 = eng.structure_factor(0)
    m = 1
    sites = moved(P, s, 1, m, rng)
    eng.commit_candidates([0], [1], [m], [MGPU_MOVE], sites[None], [1])
    assert np.array_equal(eng.structure_factor(0), A0), "an uncharged molecule's move changed A(k)"
    csite = free_spot(eng, s, 1, rng)
    eng.commit_candidates([0], [1], [-1], [MGPU_CREATION], csite[None], [1])
    eng.commit_candidates([0], [1], [0], [MGPU_DELETION], None, [1])
    assert np.array_equal(eng.structure_factor(0), A0), "an uncharged molecule's insertion / deletion changed A(k)"
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["rows", "wide-mfma", "per-k"])
def test_candidates_outside_the_cell(refcpu_mod, form):
    """Candidates whose centre lies up to a molecule radius beyond a face of the cell (no fold before the engine)."""
    n1 = 3 if form == "rows" else 24
    spec = [(*water(), 8)] if form == "rows" else [(*shell(n1, seed=12), 3)]
    s = make_system(np.diag([28.0, 28.0, 28.0]), spec, seed=8)
    eng = engine(s, "per-k" if form == "per-k" else None)
    assert_form(eng, n1, form)
    P = oracle(s, 14)
    rad = float(np.max(np.linalg.norm(s.offsets[0][0], axis=1)))
    exercise(eng, P, s, 0, f"outside ({form})", np.random.default_rng(19), outside=max(rad, 1.0))
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# (d) molecules of different sizes in one launch
def _mixed(big, seed=21):
    s = make_system(np.diag([36.0, 36.0, 36.0]), [(*water(), 10), (*shell(big, seed=seed), 3)], seed=seed)
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("big", [24, 128])
def test_mixed_sizes_in_one_launch(refcpu_mod, big):
    s = _mixed(big)
    eng = engine(s, n_replicas=6, cap=[20, 8])
    for r in range(1, 6):
        eng.replica_copy(r, 0)
    assert_form(eng, 3, "rows")
    f_big = assert_form(eng, big, "wide-mfma" if big == 24 else "wide-mfma-tiled")
    P = oracle(s, 20)
    rng = np.random.default_rng(big)
    # --- an interleaved batch against the oracle, and each candidate bitwise as in a batch of its own type alone
    t = np.array([0, 1, 0, 1, 0, 1], np.int32)
    m = np.array([0, 0, 1, 1, 2, 2], np.int32)
    rows = np.zeros((6, big, 3))
    exp_o, exp_n = [], []
    for c in range(6):
        rows[c, :s.topo.atoms_in_res[t[c]]] = moved(P, s, int(t[c]), int(m[c]), rng)
        eo, en = o_move(P, int(t[c]), int(m[c]), rows[c, :s.topo.atoms_in_res[t[c]]])
        exp_o.append(eo); exp_n.append(en)
    zeros = np.zeros(6, np.int32)
    old, new = eng.trial_energy_candidates(zeros, t, m, rows)
    close(old, exp_o, f"mixed {big}: old")
    close(new, exp_n, f"mixed {big}: new")
    # a decided trial (row form, one launch) on the lane whose last trial was split by form: its results in their own slots
    small = np.flatnonzero(t == 0)
    od, nd, acc = eng.gcmc_trial_decide(np.arange(3, dtype=np.int32), t[small], m[small], np.full(3, MGPU_MOVE, np.int32),
                                        rows[small][:, :3], np.full(3, 0.5), np.zeros(3), 300.0)
    assert not acc.any()
    close(od[:, :3], [exp_o[c] for c in small], f"mixed {big}: decided old after a split trial")
    close(nd[:, :3], [exp_n[c] for c in small], f"mixed {big}: decided new after a split trial")
    for ty in (0, 1):
        sel = np.flatnonzero(t == ty)
        o1, n1 = eng.trial_energy_candidates(zeros[sel], t[sel], m[sel], rows[sel][:, :s.topo.atoms_in_res[ty]])
        assert np.array_equal(o1, old[sel]) and np.array_equal(n1, new[sel]), \
            f"type {ty} in a mixed batch: {np.max(np.abs(n1 - new[sel]))} K from its own-type batch"
        u1 = eng.recip_energy_candidates(zeros[sel], t[sel], m[sel], np.full(len(sel), MGPU_MOVE), rows[sel][:, :s.topo.atoms_in_res[ty]])
        u = eng.recip_energy_candidates(zeros, t, m, np.full(6, MGPU_MOVE), rows)
        assert np.array_equal(u1, u[sel]) and np.array_equal(u1, new[sel, 2])
    # --- insertions / deletions of both types in one batch: oracle and own-type bitwise
    cs = free_spot(eng, s, 0, rng)
    cb = free_spot(eng, s, 1, rng)
    kinds = np.array([MGPU_CREATION, MGPU_CREATION, MGPU_DELETION, MGPU_DELETION], np.int32)
    tt = np.array([0, 1, 0, 1], np.int32)
    mm = np.array([-1, -1, 4, 2], np.int32)
    r4 = np.zeros((4, big, 3)); r4[0, :3] = cs; r4[1] = cb
    o5, n5 = eng.gcmc_trial(np.zeros(4, np.int32), tt, mm, kinds, r4)
    for c, (eo, en) in enumerate([o_insert(P, 0, cs), o_insert(P, 1, cb), o_delete(P, 0, 4), o_delete(P, 1, 2)]):
        close(o5[c], eo, f"mixed {big}: gcmc {c} old")
        close(n5[c], en, f"mixed {big}: gcmc {c} new")
    for ty in (0, 1):
        sel = np.flatnonzero(tt == ty)
        a5, b5 = eng.gcmc_trial(np.zeros(2, np.int32), tt[sel], mm[sel], kinds[sel], r4[sel][:, :s.topo.atoms_in_res[ty]])
        assert np.array_equal(a5, o5[sel]) and np.array_equal(b5, n5[sel])
    # --- trial / commit agreement: a mixed trial (small on replica 1, large on replica 2), only the small one committed
    A_before = eng.structure_factor(1)
    rep = np.array([1, 2], np.int32)
    rr = np.zeros((2, big, 3)); rr[0, :3] = rows[0, :3]; rr[1] = rows[1]
    o2, n2 = eng.gcmc_trial(rep, [0, 1], [0, 0], [MGPU_MOVE, MGPU_MOVE], rr, lane=1)
    eng.commit_lane(1, rep, [0, 1], [0, 0], [MGPU_MOVE, MGPU_MOVE], [1, 0])      # the lane's resident rows
    u_none = eng.recip_energy_candidates([1], [0], [0], [MGPU_NONE])
    assert u_none[0] == n2[0, 2], f"committed A(k) gives {u_none[0]!r}, the trial's new energy was {n2[0, 2]!r}"
    assert not np.array_equal(eng.structure_factor(1), A_before)
    assert np.array_equal(eng.structure_factor(2), eng.structure_factor(0)), "the rejected candidate's replica changed"
    # --- A(k) bitwise as a one-type launch commits it (replica 3, a copy of replica 1's state before)
    eng.commit_candidates([3], [0], [0], [MGPU_MOVE], rows[0:1, :3], [1])
    assert np.array_equal(eng.structure_factor(3), eng.structure_factor(1))
    P.set_molecule(0, 0, rows[0, 0], rows[0, :3] - rows[0, 0][None, :])
    sync(P)
    amp_close(eng.structure_factor(1), P.amplitude(), f"mixed {big}: A after the small candidate's commit")
    # --- a resident-rows commit of a mixed trial (both accepted) equals an explicit-sites commit
    rep = np.array([4, 5], np.int32)
    eng.replica_copy(4, 0); eng.replica_copy(5, 0)
    rb = np.zeros((2, big, 3)); rb[0, :3] = rows[2, :3]; rb[1] = rows[3]
    eng.gcmc_trial(rep, [0, 1], [1, 1], [MGPU_MOVE, MGPU_MOVE], rb, lane=0)
    eng.commit_lane(0, rep, [0, 1], [1, 1], [MGPU_MOVE, MGPU_MOVE], [1, 1])
    A4, A5 = eng.structure_factor(4), eng.structure_factor(5)
    eng.replica_copy(4, 0); eng.replica_copy(5, 0)
    eng.commit_candidates(rep, [0, 1], [1, 1], [MGPU_MOVE, MGPU_MOVE], rb, [1, 1])
    assert np.array_equal(eng.structure_factor(4), A4) and np.array_equal(eng.structure_factor(5), A5)
    assert np.array_equal(eng.get_molecules(5, 1)[1], rb[1])
    # --- the device-decided path refuses a mixed launch whose large type is not row-form, with a status code
    with pytest.raises(_lib.MgpuError) as ei:
        eng.gcmc_trial_decide([0, 1], [0, 1], [0, 0], [MGPU_MOVE, MGPU_MOVE], rb, [0.5, 0.5], [1.0, 1.0], 300.0)
    assert ei.value.code == MGPU_ERR_STATE
    o2b, n2b = eng.gcmc_trial([0], [0], [0], [MGPU_MOVE], rows[0:1, :3])     # the lane still works
    assert np.isfinite(n2b).all()
    assert f_big["form"] != "rows"
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# (e) the intra-molecular sum: thread / wave switch (32 / 33 sites), 512-site LDS tiles (512 / 513 / ~700)
@pytest.mark.gpu
@pytest.mark.parametrize("n1", [32, 33, 512, 513, 700])
def test_intra_sum_sizes(refcpu_mod, n1):
    rad = float(np.sqrt(n1 * 1.2 ** 2 * 1.6 / (4 * np.pi)))
    L = max(30.0, 2 * (2 * rad + 3.0) + 1.0)
    s = make_system(np.diag([L, L, L]), [(*shell(n1, seed=n1), 2)], seed=n1, rc=12.0)
    eng = engine(s, n_replicas=1, cap=[4])
    P = oracle(s, 4)
    rng = np.random.default_rng(n1)
    res = eng.intra_energy_candidates([0, 0], [0, 0], [0, 1])
    close(res, [o_intra(P, 0, 0), o_intra(P, 0, 1)], f"{n1}: resident intra")
    cand = moved(P, s, 0, 1, rng)
    u = eng.intra_energy_candidates([0], [0], [1], cand[None])
    close(u, [o_intra(P, 0, 1, cand)], f"{n1}: candidate intra")
    csite = free_spot(eng, s, 0, rng)
    eo, en = o_insert(P, 0, csite)
    o5, n5 = eng.gcmc_trial([0], [0], [-1], [MGPU_CREATION], csite[None])
    close(n5[0, 4], en[4], f"{n1}: insertion intra")
    if n1 == 513:
        assert eng.recip_form(n1)["site_tiles"] >= 2
        close(o5[0], eo, "513: insertion old")
        close(n5[0], en, "513: insertion new")
        exercise(eng, P, s, 0, "513 sites", rng, n_batch=2)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [(32, 33), (3, 513)])
def test_intra_mixed_thread_and_wave_items(refcpu_mod, sizes):
    """A launch holding a <= 32-site and a > 32-site type: intra_kernel and intra_wave_kernel both run, each skipping the
    other's items."""
    a, b = sizes
    rb = float(np.sqrt(b * 1.2 ** 2 * 1.6 / (4 * np.pi)))
    L = max(34.0, 2 * (2 * rb + 3.0) + 4.0)
    ta = water() if a == 3 else shell(a, seed=a)
    s = make_system(np.diag([L, L, L]), [(*ta, 3), (*shell(b, seed=b), 2)], seed=a + b, rc=12.0)
    eng = engine(s, cap=[6, 4])
    P = oracle(s, 6)
    rng = np.random.default_rng(a * b)
    t = [0, 1, 0, 1]
    m = [0, 0, 1, 1]
    close(eng.intra_energy_candidates([0] * 4, t, m), [o_intra(P, t[i], m[i]) for i in range(4)], f"{sizes}: resident")
    rows = np.zeros((4, b, 3))
    for i in range(4):
        rows[i, :s.topo.atoms_in_res[t[i]]] = moved(P, s, t[i], m[i], rng)
    close(eng.intra_energy_candidates([0] * 4, t, m, rows),
          [o_intra(P, t[i], m[i], rows[i, :s.topo.atoms_in_res[t[i]]]) for i in range(4)], f"{sizes}: candidates")
    ca, cb = free_spot(eng, s, 0, rng), free_spot(eng, s, 1, rng)
    r2 = np.zeros((2, b, 3)); r2[0, :a] = ca; r2[1] = cb
    o5, n5 = eng.gcmc_trial([0, 0], [0, 1], [-1, -1], [MGPU_CREATION, MGPU_CREATION], r2)
    close(n5[:, 4], [o_insert(P, 0, ca)[1][4], o_insert(P, 1, cb)[1][4]], f"{sizes}: insertion intra")
    o5, n5 = eng.gcmc_trial([0, 0], [0, 1], [2, 1], [MGPU_DELETION, MGPU_DELETION], np.zeros((2, b, 3)))
    close(o5[:, 4], [o_intra(P, 0, 2), o_intra(P, 1, 1)], f"{sizes}: deletion intra")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# (f) commit edges
@pytest.mark.gpu
@pytest.mark.parametrize("form", ["rows", "wide-mfma"])
def test_commit_edges(refcpu_mod, form):
    n1 = 3 if form == "rows" else 24
    t0 = water() if form == "rows" else shell(24, seed=31)
    s = make_system(np.diag([30.0, 30.0, 30.0]), [(*t0, 4), (*ion(-1.0), 1)], seed=31)
    cap = 5
    eng = engine(s, cap=[cap, 2])
    assert_form(eng, n1, form)
    P = oracle(s, cap)
    rng = np.random.default_rng(31)
    # insertion into the last free slot, then the capacity code
    csite = free_spot(eng, s, 0, rng)
    eng.commit_candidates([0], [0], [-1], [MGPU_CREATION], csite[None], [1])
    assert eng.num_molecules(0, 0) == cap
    P.set_num_residues(0, cap); P.set_molecule(0, cap - 1, csite[0], csite - csite[0][None, :]); sync(P)
    amp_close(eng.structure_factor(0), P.amplitude(), f"{form}: A after filling the last slot")
    with pytest.raises(_lib.MgpuError) as ei:
        eng.commit_candidates([0], [0], [-1], [MGPU_CREATION], free_spot(eng, s, 0, rng)[None], [1])
    assert ei.value.code == MGPU_ERR_CAPACITY
    assert eng.num_molecules(0, 0) == cap
    # deletion of the last molecule: no swap
    before = eng.get_molecules(0, 0).copy()
    eng.commit_candidates([0], [0], [cap - 1], [MGPU_DELETION], None, [1])
    assert eng.num_molecules(0, 0) == cap - 1
    assert np.array_equal(eng.get_molecules(0, 0), before[:cap - 1])
    P.set_num_residues(0, cap - 1); sync(P)
    amp_close(eng.structure_factor(0), P.amplitude(), f"{form}: A after deleting the last molecule")
    # deletion of the only molecule of a type: A(k) is S(k) of what remains
    eng.commit_candidates([0], [1], [0], [MGPU_DELETION], None, [1])
    assert eng.num_molecules(0, 1) == 0
    P.set_num_residues(1, 0); sync(P)
    A = eng.structure_factor(0)
    amp_close(A, P.amplitude(), f"{form}: A after emptying a type")
    eng.init_structure_factor(0, True)
    amp_close(A, eng.structure_factor(0), f"{form}: A after emptying a type vs init_structure_factor")
    eng.close()


@pytest.mark.gpu
def test_commit_by_accept_mask_word_edges(refcpu_mod):
    """70 candidates on 70 replicas, committed from the lane's resident rows by accept mask (row form), bits 0, 31, 32, 63
    and 64 set: the AcceptBits word edges."""
    s = make_system(np.diag([20.0, 20.0, 20.0]), [(*water(), 12)], seed=41)
    R = 70
    eng = engine(s, n_replicas=R)
    for r in range(1, R):
        eng.replica_copy(r, 0)
    assert_form(eng, 3, "rows")
    P = oracle(s, 20)
    rng = np.random.default_rng(41)
    m = (np.arange(R) % 12).astype(np.int32)
    rows = np.stack([moved(P, s, 0, int(m[c]), rng) for c in range(R)])
    exp = [o_move(P, 0, int(m[c]), rows[c]) for c in range(R)]
    rep = np.arange(R, dtype=np.int32)
    old, new = eng.gcmc_trial(rep, np.zeros(R, np.int32), m, np.full(R, MGPU_MOVE, np.int32), rows, lane=1)
    close(old[:, :3], [e[0] for e in exp], "70 candidates old")
    close(new[:, :3], [e[1] for e in exp], "70 candidates new")
    acc = np.zeros(R, np.int32)
    on = [0, 31, 32, 63, 64]
    acc[on] = 1
    A0 = eng.structure_factor(0)
    eng.commit_lane(1, rep, np.zeros(R, np.int32), m, np.full(R, MGPU_MOVE, np.int32), acc)
    for r in range(R):
        A = eng.structure_factor(r)
        if r in on:
            com, off = P.get_molecule(0, int(m[r]))
            P.set_molecule(0, int(m[r]), rows[r, 0], rows[r] - rows[r, 0][None, :]); sync(P)
            amp_close(A, P.amplitude(), f"replica {r}: A after its accepted move")
            assert np.array_equal(eng.get_molecules(r, 0)[m[r]], rows[r])
            assert eng.recip_energy_candidates([r], [0], [0], [MGPU_NONE])[0] == new[r, 2]
            P.set_molecule(0, int(m[r]), com, off); sync(P)
        else:
            assert np.array_equal(A, A0), f"replica {r} was not accepted but changed"
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# (g) CPU guard
def test_recip_edge_cases_are_what_they_claim():
    """The boxes give the kmax they claim through mgpu_ewald_setup; the shells have the site counts they claim."""
    for name, (box, rc, tol, kmax) in SHAPES.items():
        got = kmax_of(box, rc, tol)
        if kmax is not None:
            assert got == kmax, f"{name}: kmax {got}, claimed {kmax}"
    assert kmax_of(*NO_ROOM_BOX[:3]) == NO_ROOM_BOX[3]
    thin, flat = kmax_of(*SHAPES["thin"][:3]), kmax_of(*SHAPES["flat"][:3])
    assert max(thin[:2]) <= 2 and thin[2] >= 40 and min(flat[:2]) >= 30 and flat[2] == 1
    assert [kmax_of(*SHAPES[k][:3])[2] for k in ("kz15", "kz16", "kz17")] == [15, 16, 17]
    for n1 in (1, 8, 24, 32, 33, 77, 128, 512, 513, 700):
        tmpl, ty, q = shell(n1, seed=n1)
        assert tmpl.shape == (n1, 3) and ty.shape == (n1,) and q.shape == (n1,)
        assert abs(q.sum()) < 1e-12
    tmpl, ty, q = shell(24, seed=10, net_charge=-1.0)
    assert q.sum() == pytest.approx(-1.0)
    assert not np.any(shell(24, seed=9, charged=False)[2])
