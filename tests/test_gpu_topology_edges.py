"""The kernels held to the oracle (oracle/refcpu.c) at the limits of the topology: all kMaxRes = 8 residue types and all
kMaxTypes = 16 atom types in one box, and both sides of every switch the topology alone decides -- the frozen layout and
pair_flat_kernel's group (kMaxGrp = 32) and plane (kFlatMaxPlanes = 64) limits, a frozen framework of capacity > 1, the
63 / 64-site switch of an active type to the site-major layout, and when pair_frozen_kernel batches a framework.  Every GPU
case asserts where it sits through Engine.pair_layout (mgpu_pair_layout) and Engine.recip_form, so that a change of a limit
cannot move a case to the other side unnoticed; test_topologies_are_what_they_claim checks the same counts from the
topology on the CPU.

An index or stride slip in the per-(replica, type) state, the per-type segment and group offsets or the LDS pair table
shows only for residue types >= 2 or atom types above 10.  Here the framework is residue type 2, guests sit on both sides
of it, atom type 16 is a guest's, atom types are shared by residue types with different charges (charges belong to (t, a);
the frozen layout groups by atom type), one type starts empty, one sits at its capacity, and capacities 64 and 65 end on
either side of a tail unit.  On a box of four active types the device-built moves, reservoirs, farm windows (records naming
every type, caller-picked and by count, against the oracle replay and bit for bit against the batched path), chain windows
and the fast fold behind a non-tight step run on types 2 and 3; the Fortran farm runs on a framework box of three active
types in every mode.  Energies to tol_for, A(k) to 1e-10, counts and committed rows exactly."""
import os

import numpy as np
import pytest

from maniac_mc_amd import synth
from maniac_mc_amd._lib import MGPU_CREATION, MGPU_DELETION, MGPU_MOVE, MgpuError
from maniac_mc_amd.engine import Engine
from maniac_mc_amd.synth import lorentz_berthelot
from maniac_mc_amd.system import KB_KCALMOL, System, Topology
from tests.test_gpu_pair_edges import _check_items, _check_static, _close, _expect_new
from tests.test_gpu_recip_edges import amp_close, close, moved, o_delete, o_insert, oracle, sync
from tests.test_gpu_window_edges import (V_ACC, V_REJ, Replay, _by_count, _chain_oracle, _check_window, _rod_system,
                                         _same_as_oracle, _engine as window_engine)
from tests.util import farm_tol

MGPU_ERR_INVALID_ARG = 1
MAX_RES, MAX_TYPES, MAX_GRP, FLAT_MAX_PLANES = 8, 16, 32, 64      # mgpu_kernels_common.h
RC = 10.0

# like-pair (epsilon [kcal/mol], sigma [A]) of the sixteen atom types; 2, 5 and 10 carry no Lennard-Jones
ATOMS = [(0.1553, 3.166), (0.0, 0.0), (0.06, 3.0), (0.08, 3.3), (0.0, 0.0), (0.05, 2.8), (27.0 * KB_KCALMOL, 2.80),
         (79.0 * KB_KCALMOL, 3.05), (0.155, 3.1536), (0.0, 0.0), (0.10, 2.5), (0.10, 4.0), (0.09, 3.3), (0.06, 3.0),
         (0.07, 3.1), (0.11, 3.4)]


# ---------------------------------------------------------------------------------------------------------------------
# species and systems
def _ring(n, radius, z=0.0, phase=0.0):
    a = phase + 2 * np.pi * np.arange(n) / n
    return np.stack([radius * np.cos(a), radius * np.sin(a), np.full(n, z)], 1)


def _tip4p():
    r_oh, ang, r_om = 0.9572, np.deg2rad(104.52), 0.15
    t = np.array([[0.0, 0.0, 0.0], [r_oh * np.sin(ang / 2), r_oh * np.cos(ang / 2), 0.0],
                  [-r_oh * np.sin(ang / 2), r_oh * np.cos(ang / 2), 0.0], [0.0, r_om, 0.0]])
    return t - t.mean(0)


def _shell(n, seed):
    """a rigid shell of n sites >= 1.2 A apart (synth.large_adsorbate_box's template)"""
    return synth.large_adsorbate_box(n_sites=n, n_mol=1, L=4.0 * n + 100.0, seed=seed).offsets[0][0].copy()


def species(name):
    """(template, atom types, charges) of a guest"""
    if name == "cation":
        return np.zeros((1, 3)), [11], [1.0]
    if name == "anion":
        return np.zeros((1, 3)), [12], [-1.0]
    if name == "spce":                    # atom type 2 (no LJ) shared with tip4p at another charge
        return synth._spce_template(), [1, 2, 2], [-0.8476, 0.4238, 0.4238]
    if name == "co2":
        return np.array([[0.0, 0.0, 0.0], [1.16, 0.0, 0.0], [-1.16, 0.0, 0.0]]), [7, 8, 8], [0.70, -0.35, -0.35]
    if name == "tip4p":                   # the LJ site uncharged, the charge site without LJ
        return _tip4p(), [9, 2, 2, 10], [0.0, 0.52, 0.52, -1.04]
    if name == "five":
        return _shell(5, 31), [12, 5, 5, 7, 7], [0.0, 0.3, 0.3, -0.3, -0.3]
    if name == "ring12":                  # two uncharged sites
        return _ring(12, 2.4), [13, 14] * 6, [0.0, 0.0] + [0.25, -0.25] * 5
    if name == "shell24":                 # atom type 16: the last row of the LDS pair table
        return np.vstack([_ring(12, 2.4, 0.9), _ring(12, 2.4, -0.9, 0.26)]), [15, 16] * 12, [0.2, -0.2] * 12
    if name.startswith("shell"):          # shell63, shell64
        n = int(name[5:])
        q = np.resize([0.3, -0.3], n)
        q[-1] -= q.sum()
        return _shell(n, n), [int(a) for a in np.resize([13, 15, 16], n)], [float(x) for x in q]
    raise KeyError(name)


def frame(n, types, qpat):
    """(None, atom types, charges) of an inactive framework of n sites: types and charges cycled, then made neutral"""
    q = np.resize(np.asarray(qpat, dtype=np.float64), n)
    nz = q != 0.0
    q[nz] -= q.sum() / np.count_nonzero(nz)
    return None, [int(a) for a in np.resize(types, n)], [float(x) for x in q]


def build(specs, L=40.0, tilt=None, seed=5, gap=2.2):
    """specs: [(species or frame tuple, active, n_mol)] in residue-type order.  Framework sites are dealt from one jittered
    lattice over the cell; guests are placed whole, every site `gap` from every site placed before (minimum image)."""
    rng = np.random.default_rng(seed)
    box = np.diag([L, L, L])
    if tilt is not None:
        box[1, 0], box[2, 0], box[2, 1] = tilt
    inv = np.linalg.inv(box)
    lo = np.full(3, -L / 2)
    n_fr = sum(len(sp[0][1]) * sp[2] for sp in specs if sp[0][0] is None)
    fpos = np.zeros((0, 3))
    if n_fr:
        k = int(np.ceil(n_fr ** (1 / 3)))
        g = np.stack(np.meshgrid(*[np.arange(k)] * 3, indexing="ij"), -1).reshape(-1, 3)
        g = g[np.sort(rng.permutation(g.shape[0])[:n_fr])]
        fpos = lo + ((g + 0.5 + rng.uniform(-0.08, 0.08, g.shape)) / k) @ box
    placed = fpos.copy()
    coms, offs, at = [], [], 0
    for (tmpl, ty, q), active, n_mol in specs:
        if tmpl is None:
            c_t, o_t = [], []
            for _ in range(n_mol):
                sites = fpos[at:at + len(ty)]
                at += len(ty)
                c_t.append(sites.mean(0)); o_t.append(sites - sites.mean(0))
            coms.append(np.array(c_t).reshape(-1, 3)); offs.append(np.array(o_t).reshape(-1, len(ty), 3))
            continue
        c_t, o_t = [], []
        for _ in range(n_mol):
            for _try in range(20000):
                com = lo + rng.uniform(0.0, 1.0, 3) @ box
                off = tmpl @ synth._random_rotations(rng, 1)[0].T
                d = ((com + off)[:, None, :] - placed[None, :, :]) @ inv
                d -= np.rint(d)
                if placed.shape[0] == 0 or np.min(np.linalg.norm(d @ box, axis=2)) >= gap:
                    break
            else:
                raise AssertionError("no room for a molecule")
            placed = np.vstack([placed, com + off])
            c_t.append(com); o_t.append(off)
        coms.append(np.array(c_t).reshape(-1, 3)); offs.append(np.array(o_t).reshape(-1, len(ty), 3))
    w = max(len(sp[0][1]) for sp in specs)
    types = np.zeros((len(specs), w), np.int32)
    charges = np.zeros((len(specs), w))
    for t, ((_, ty, q), _, _) in enumerate(specs):
        types[t, :len(ty)] = ty
        charges[t, :len(q)] = q
    eps, sig = lorentz_berthelot([a[0] for a in ATOMS], [a[1] for a in ATOMS])
    topo = Topology([len(sp[0][1]) for sp in specs], types, charges, [sp[1] for sp in specs], eps, sig)
    return System(topo, box, lo, RC, 1e-5, 300.0, coms, offs)


# the main system: all eight residue types (the framework is type 2, the plane-major inactive anion type 5), all sixteen
# atom types; the framework shares atom type 1 with spce at another charge and has uncharged and LJ-free sites
MAIN_NAMES = ["cation", "spce", "frame", "co2", "tip4p", "anion", "ring12", "shell24"]
MAIN_N = [6, 64, 1, 0, 6, 6, 3, 2]
MAIN_CAPS = [65, 64, 1, 10, 12, 6, 6, 5]
MAIN_FRAME = frame(80, [1, 3, 4, 5, 6], [-0.4, 0.3, 0.0, 0.25, -0.15])
ACTIVE = [0, 1, 3, 4, 6, 7]
TILT = (2.0, -1.5, 1.0)


def main_system(tilt=None, seed=5):
    specs = [(MAIN_FRAME if nm == "frame" else species(nm), 0 if nm in ("frame", "anion") else 1, n)
             for nm, n in zip(MAIN_NAMES, MAIN_N)]
    return build(specs, tilt=tilt, seed=seed), list(MAIN_CAPS)


# relabelling: residue type i of the permuted system is type PERM[i] of the main one, atom type a becomes atom_perm(a)
PERM = [3, 6, 0, 7, 2, 5, 1, 4]


def atom_perm(a):
    return (7 * a) % 17                   # a permutation of 1..16


def relabelled(s, caps):
    topo = s.topo
    amap = np.array([0] + [atom_perm(a) for a in range(1, MAX_TYPES + 1)], np.int32)
    eps = np.zeros_like(topo.epsilon)
    sig = np.zeros_like(topo.sigma)
    for a in range(MAX_TYPES):
        for b in range(MAX_TYPES):
            eps[amap[a + 1] - 1, amap[b + 1] - 1] = topo.epsilon[a, b]
            sig[amap[a + 1] - 1, amap[b + 1] - 1] = topo.sigma[a, b]
    t2 = Topology(topo.atoms_in_res[PERM], amap[topo.atom_types[PERM]], topo.charges[PERM], topo.is_active[PERM], eps, sig)
    return (System(t2, s.box_matrix.copy(), s.bounds_lo.copy(), s.real_space_cutoff, s.ewald_tolerance, s.temperature,
                   [s.com[p].copy() for p in PERM], [s.offsets[p].copy() for p in PERM]), [caps[p] for p in PERM])


def flat_counts(topo, caps):
    """(groups, planes) of the frozen layout, as mgpu_engine_create judges pair_flat_kernel's eligibility"""
    groups = planes = 0
    for t in range(topo.n_res):
        n1 = int(topo.atoms_in_res[t])
        if n1 >= 64 and not topo.is_active[t]:
            g = len(set(topo.atom_types[t, :n1].tolist()))
            groups += g
            planes += caps[t] * g
        else:
            planes += n1
    return groups, planes


def expected_layout(s, caps, env, replicas_differ=False):
    """what Engine.pair_layout must report for s with `env` at creation"""
    topo = s.topo
    n1 = topo.atoms_in_res
    frozen = [t for t in range(topo.n_res) if n1[t] >= 64 and not topo.is_active[t]]
    groups, planes = flat_counts(topo, caps)
    want = bool(frozen) if "MGPU_PAIR_FLAT" not in env else env["MGPU_PAIR_FLAT"] != "0"
    ok = (not s.is_triclinic() and groups <= MAX_GRP and planes <= FLAT_MAX_PLANES
          and not any(n1[t] >= 64 and topo.is_active[t] for t in range(topo.n_res)))
    flat = want and ok
    codes = [(2 if flat and t in frozen else 1) if n1[t] >= 64 else 0 for t in range(topo.n_res)]
    fb = -1
    if flat and len(frozen) == 1 and "MGPU_NO_FROZEN_BATCH" not in env and not replicas_differ and s.n_mol[frozen[0]] >= 1:
        fb = frozen[0]
    return dict(flat=flat, groups=groups, planes=planes, frozen_batch=fb, site_major=codes)


# ---------------------------------------------------------------------------------------------------------------------
# the layout cases of part 4: name -> (specs, caps, replicas, what they claim)
FR16 = frame(64, list(range(1, 17)), [0.3, -0.3, 0.0, 0.2])
FR16_NEG = (None, FR16[1], [-q for q in FR16[2]])                  # the same atom types at the opposite charges
FR1 = frame(64, [3], [0.25, -0.25])
FR8 = frame(64, [1, 3, 4, 5, 6, 7, 8, 9], [-0.3, 0.3, 0.0, 0.2])
FR5 = frame(64, [1, 3, 4, 5, 6], [-0.4, 0.3, 0.0, 0.25, -0.15])
LAYOUT_CASES = ["groups_32", "groups_33", "planes_64", "planes_65", "frozen_cap4", "frozen_cap5", "active_63_64",
                "batch_on", "batch_frozen_diff", "batch_empty"]


def layout_case(name):
    sp = species
    if name == "groups_32":            # 16 + 16 groups, 36 planes: flat; two frozen types, so no batch
        specs = [(sp("spce"), 1, 4), (FR16, 0, 1), (FR16_NEG, 0, 1), (sp("cation"), 1, 3)]
        return specs, [12, 1, 1, 6], 1, dict(groups=32, planes=36, flat=True)
    if name == "groups_33":            # a third frozen residue brings the 33rd group: site-major
        specs = [(sp("spce"), 1, 4), (FR16, 0, 1), (FR16_NEG, 0, 1), (sp("cation"), 1, 3), (FR1, 0, 1)]
        return specs, [12, 1, 1, 6, 1], 1, dict(groups=33, planes=37, flat=False)
    if name in ("planes_64", "planes_65"):   # 16 framework planes + 24 + 12 + 5 + 4 + 3 (+ 1)
        specs = [(sp("shell24"), 1, 2), (FR16, 0, 1), (sp("ring12"), 1, 2), (sp("five"), 1, 3), (sp("tip4p"), 1, 3),
                 (sp("spce"), 1, 3)]
        caps = [4, 1, 4, 6, 6, 6]
        if name == "planes_65":
            specs.append((sp("cation"), 1, 3))
            caps.append(6)
        return specs, caps, 1, dict(groups=16, planes=64 if name == "planes_64" else 65, flat=name == "planes_64")
    if name in ("frozen_cap4", "frozen_cap5"):   # 8 groups x capacity 4 (5) + 3 + 5 + 24 planes
        cap = int(name[-1])
        specs = [(sp("spce"), 1, 3), (sp("five"), 1, 3), (FR8, 0, 1), (sp("shell24"), 1, 2)]
        return specs, [6, 6, cap, 4], 1, dict(groups=8, planes=8 * cap + 32, flat=cap == 4)
    if name == "active_63_64":         # two active shells either side of the site-major switch beside a plane-major type
        specs = [(sp("spce"), 1, 3), (sp("shell63"), 1, 2), (sp("shell64"), 1, 2)]
        return specs, [6, 4, 4], 1, dict(groups=0, planes=130, flat=False)
    if name in ("batch_on", "batch_frozen_diff", "batch_empty"):
        # one frozen type with a <= 5-site and a 12-site guest: the same in both replicas / its replicas differ / empty
        specs = [(sp("spce"), 1, 4), (sp("ring12"), 1, 2), (FR5, 0, 1)]
        return specs, [8, 4, 1], 1 if name == "batch_empty" else 2, dict(groups=5, planes=20, flat=True)
    raise KeyError(name)


def layout_system(name):
    specs, caps, R, claim = layout_case(name)
    s = build(specs, L=30.0, seed=9)
    if name == "batch_empty":
        s.com[2] = np.zeros((0, 3))
        s.offsets[2] = np.zeros((0, 64, 3))
    return s, caps, R, claim


# ---------------------------------------------------------------------------------------------------------------------
# CPU guards
def test_topologies_are_what_they_claim():
    """Every case sits where its test says: eight residue types and sixteen atom types in the main system (type 16 a
    guest's, atom types shared at different charges, LJ-free types, uncharged sites, an empty type, a full one,
    capacities 64 and 65), its flat layout within both limits, and the group and plane counts of each layout case on the
    side of the limit it claims -- computed here from the topology alone."""
    s, caps = main_system()
    topo = s.topo
    assert topo.n_res == MAX_RES and topo.n_atom_types == MAX_TYPES
    n1 = topo.atoms_in_res
    used = {int(topo.atom_types[t, a]) for t in range(topo.n_res) for a in range(n1[t])}
    assert used == set(range(1, MAX_TYPES + 1))
    assert any(topo.is_active[t] and MAX_TYPES in topo.atom_types[t, :n1[t]] for t in range(topo.n_res))
    assert [t for t in range(topo.n_res) if n1[t] >= 64 and not topo.is_active[t]] == [2]
    assert not topo.is_active[5] and n1[5] < 64
    assert [t for t in range(topo.n_res) if topo.is_active[t]] == ACTIVE
    assert flat_counts(topo, caps) == (5, 53)
    # atom types shared by residue types at different charges: 1 (framework, spce), 2 (spce, tip4p)
    for a in (1, 2):
        q = {float(topo.charges[t, i]) for t in range(topo.n_res) for i in range(n1[t]) if topo.atom_types[t, i] == a}
        res = {t for t in range(topo.n_res) for i in range(n1[t]) if topo.atom_types[t, i] == a}
        assert len(q) >= 2 and len(res) >= 2, a
    assert any(topo.epsilon[a - 1, a - 1] == 0.0 for a in used)
    assert any(topo.charges[t, i] == 0.0 for t in range(topo.n_res) for i in range(n1[t]))
    assert s.n_mol[3] == 0 and s.n_mol[1] == caps[1] and 64 in caps and 65 in caps
    assert all(s.n_mol[t] <= caps[t] for t in range(topo.n_res))
    lay = expected_layout(s, caps, {})
    assert lay["flat"] and lay["frozen_batch"] == 2 and lay["site_major"] == [0, 0, 2, 0, 0, 0, 0, 0]
    st, ct = main_system(tilt=TILT)
    assert st.is_triclinic() and not expected_layout(st, ct, {})["flat"]
    # the relabelled system: the same counts, the framework moved to another type
    s2, caps2 = relabelled(s, caps)
    assert sorted(atom_perm(a) for a in range(1, MAX_TYPES + 1)) == list(range(1, MAX_TYPES + 1))
    assert flat_counts(s2.topo, caps2) == (5, 53)
    assert expected_layout(s2, caps2, {})["frozen_batch"] == PERM.index(2) != 2
    # the layout cases: counts and the side of each limit
    counts = {}
    for name in LAYOUT_CASES:
        s, caps, R, claim = layout_system(name)
        counts[name] = flat_counts(s.topo, caps)
        assert counts[name] == (claim["groups"], claim["planes"]), name
        assert expected_layout(s, caps, {}, name == "batch_frozen_diff")["flat"] == claim["flat"], name
    assert counts["groups_32"][0] == MAX_GRP and counts["groups_33"][0] == MAX_GRP + 1
    assert max(counts["groups_32"][1], counts["groups_33"][1]) <= FLAT_MAX_PLANES
    assert counts["planes_64"][1] == FLAT_MAX_PLANES and counts["planes_65"][1] == FLAT_MAX_PLANES + 1
    assert max(counts["planes_64"][0], counts["planes_65"][0]) <= MAX_GRP
    assert sorted(layout_system("active_63_64")[0].topo.atoms_in_res.tolist()) == [3, 63, 64]


def _topo_limits(n_res, n_types, ty=1):
    eps, sig = lorentz_berthelot([0.1] * n_types, [3.0] * n_types)
    return Topology([2] * n_res, np.array([[1, ty]] * n_res, np.int32), np.zeros((n_res, 2)), [1] * n_res, eps, sig)


@pytest.mark.parametrize("case", ["n_res_9", "n_types_17", "atom_type_0", "atom_type_n_types_plus_1"])
def test_refusals(case):
    """mgpu_engine_create refuses what it cannot hold before it touches a device: nine residue types, seventeen atom
    types, an atom type id of 0 or n_types + 1 among a residue's sites"""
    topo = {"n_res_9": lambda: _topo_limits(MAX_RES + 1, 4), "n_types_17": lambda: _topo_limits(2, MAX_TYPES + 1),
            "atom_type_0": lambda: _topo_limits(2, 5, ty=0), "atom_type_n_types_plus_1": lambda: _topo_limits(2, 5, ty=6)}[case]()
    with pytest.raises(MgpuError) as ei:
        Engine(topo, np.diag([30.0] * 3), np.full(3, -15.0), RC, 1e-5, 1, 0, [4] * topo.n_res)
    assert ei.value.code == MGPU_ERR_INVALID_ARG, ei.value


# ---------------------------------------------------------------------------------------------------------------------
# GPU helpers
def _engine(s, env, caps, R=1):
    """an engine of R replicas holding s; `env` selects the layout and kernel instances at creation"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = Engine.from_system(s, n_replicas=R, mol_capacity=caps)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for r in range(R):
        eng.init_structure_factor(r, True)
    return eng


def assert_layout(eng, exp, what):
    got = eng.pair_layout()
    assert got == exp, f"{what}: pair_layout {got}, expected {exp}"


def o_move5(P, t, m, sites):
    """ComputeOldEnergy / ComputeNewEnergy of a move (five components); the oracle unchanged after"""
    A0 = P.amplitude()
    com, off = P.get_molecule(t, m)
    P.save_fourier(t, m)
    eo = P.old_energy(t, m, 0)[:5]
    P.set_molecule(t, m, sites[0], sites - sites[0][None, :])
    en = P.new_energy(t, m, 0)[:5]
    P.set_molecule(t, m, com, off)
    P.restore_fourier(t, m)
    P.set_amplitude(A0)
    return eo, en


def free_spot(s, eng, tmpl, rng, replica=0, gap=2.2):
    """sites of a new molecule (tmpl rotated) every site `gap` from every site the replica holds"""
    box = np.asarray(s.box_matrix, float)
    inv = np.linalg.inv(box)
    allsites = np.concatenate([eng.get_molecules(replica, t).reshape(-1, 3) for t in range(s.topo.n_res)])
    for _ in range(20000):
        com = s.bounds_lo + rng.uniform(0.0, 1.0, 3) @ box
        sites = com + tmpl @ synth._random_rotations(rng, 1)[0].T
        d = (sites[:, None, :] - allsites[None, :, :]) @ inv
        d -= np.rint(d)
        if np.min(np.linalg.norm(d @ box, axis=2)) >= gap:
            return sites
    raise AssertionError("no free spot")


def _template(t):
    return np.asarray(species(MAIN_NAMES[t])[0], dtype=np.float64)


def _form_key(f):
    """launches of one key share a kernel and its tile shape (same_recip_form): every row-form type together"""
    return f["form"] if f["form"] == "rows" else (f["form"], f["site_states"], f["rows_per_tile"])


# ---------------------------------------------------------------------------------------------------------------------
# part 2: the main system
MAIN_VARIANTS = {"flat_batch": {}, "flat_exact": {"MGPU_PAIR_EXACT_FOLD": "1"}, "flat_no_batch": {"MGPU_NO_FROZEN_BATCH": "1"},
                 "plane_fast": {"MGPU_PAIR_FLAT": "0"}, "plane_exact": {"MGPU_PAIR_FLAT": "0", "MGPU_PAIR_EXACT_FOLD": "1"},
                 "triclinic": {}}


def _main(variant):
    s, caps = main_system(tilt=TILT if variant == "triclinic" else None)
    env = MAIN_VARIANTS[variant]
    eng = _engine(s, env, caps)
    assert_layout(eng, expected_layout(s, caps, env), variant)
    return s, caps, eng


def _launch(s, caps, eng, P, rng):
    """(t, m, kind, rows, expected old[5], expected new[5]) of one launch: a move of every active type that holds a
    molecule, an insertion of every active type below its capacity, a deletion of every active type that holds one"""
    W = int(s.topo.atoms_in_res.max())
    items = []
    for ty in ACTIVE:
        n = P.num_residues(ty)
        if n:
            m = int(rng.integers(0, n))
            items.append((ty, m, MGPU_MOVE, moved(P, s, ty, m, rng)))
    for ty in ACTIVE:
        if P.num_residues(ty) < caps[ty]:
            items.append((ty, -1, MGPU_CREATION, free_spot(s, eng, _template(ty), rng)))
    for ty in ACTIVE:
        n = P.num_residues(ty)
        if n:
            items.append((ty, n - 1 if ty % 2 else 0, MGPU_DELETION, None))
    t = np.array([it[0] for it in items], np.int32)
    m = np.array([it[1] for it in items], np.int32)
    k = np.array([it[2] for it in items], np.int32)
    rows = np.zeros((len(items), W, 3))
    eo, en = np.zeros((len(items), 5)), np.zeros((len(items), 5))
    for c, (ty, mm, kk, x) in enumerate(items):
        if x is not None:
            rows[c, :x.shape[0]] = x
        if kk == MGPU_MOVE:
            eo[c], en[c] = o_move5(P, ty, mm, x)
        elif kk == MGPU_CREATION:
            eo[c], en[c] = o_insert(P, ty, x)
        else:
            eo[c], en[c] = o_delete(P, ty, mm)
    return t, m, k, rows, eo, en


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(MAIN_VARIANTS))
def test_eight_types_static(variant, refcpu_mod):
    """the static energy (all five components and the total), S(k) and every type's self energy; the guests' reciprocal
    updates take at least three launch forms"""
    s, caps, eng = _main(variant)
    P = oracle(s, max(caps))
    e, r = eng.system_energy(0), P.system_energy()
    for key in ("non_coulomb", "coulomb", "recip_coulomb", "ewald_self", "intra_coulomb", "total"):
        close(e[key], r[key], f"{variant}: system {key}")
    amp_close(eng.structure_factor(0), P.amplitude(), f"{variant}: S(k)")
    for t in range(s.topo.n_res):
        close(eng.self_energy(t), P.self_singlemol(t), f"{variant}: self energy of type {t}")
    forms = {t: eng.recip_form(int(s.topo.atoms_in_res[t])) for t in ACTIVE}
    assert len({_form_key(f) for f in forms.values()}) >= 3, forms
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(MAIN_VARIANTS))
def test_eight_types_one_launch(variant, refcpu_mod):
    """one launch of moves, insertions and deletions of every active type (six residue types) through every batched
    entry point, against the oracle -- and each trial bitwise as the same item launched with its own type alone (DESIGN
    section 4.2; pair_energy_candidates sweeps a launch at its common site count, so it is held to the oracle only);
    then the pair sweeps' own checks on the moves and insertions"""
    s, caps, eng = _main(variant)
    P = oracle(s, max(caps))
    rng = np.random.default_rng(7)
    t, m, k, rows, eo, en = _launch(s, caps, eng, P, rng)
    assert set(t.tolist()) == set(ACTIVE)
    n = len(t)
    rep = np.zeros(n, np.int32)
    old, new = eng.gcmc_trial(rep, t, m, k, rows)
    for c in range(n):
        close(old[c], eo[c], f"{variant}: item {c} (type {t[c]}, kind {k[c]}) old")
        close(new[c], en[c], f"{variant}: item {c} (type {t[c]}, kind {k[c]}) new")
    u = eng.recip_energy_candidates(rep, t, m, k, rows)
    close(u, en[:, 2], f"{variant}: recip_energy_candidates")
    nw = np.flatnonzero(k != MGPU_DELETION)
    a, b = eng.pair_energy_candidates(rep[nw], t[nw], m[nw], rows[nw])
    close(np.stack([a, b], 1), en[nw, :2], f"{variant}: pair_energy_candidates new")
    od = np.flatnonzero(k != MGPU_CREATION)
    a_o, b_o = eng.pair_energy_candidates(rep[od], t[od], m[od], None)
    close(np.stack([a_o, b_o], 1), eo[od, :2], f"{variant}: pair_energy_candidates resident")
    ins, dl = np.flatnonzero(k == MGPU_CREATION), np.flatnonzero(k == MGPU_DELETION)
    ui = eng.intra_energy_candidates(rep[ins], t[ins], m[ins], rows[ins])
    close(ui, en[ins, 4], f"{variant}: intra of the insertions")
    ud = eng.intra_energy_candidates(rep[dl], t[dl], m[dl], None)
    close(ud, eo[dl, 4], f"{variant}: intra of the deletions")
    mv = np.flatnonzero(k == MGPU_MOVE)
    to, tn = eng.trial_energy_candidates(rep[mv], t[mv], m[mv], rows[mv])
    close(to, eo[mv, :3], f"{variant}: trial_energy_candidates old")
    close(tn, en[mv, :3], f"{variant}: trial_energy_candidates new")
    # each type alone: the same bits
    for ty in ACTIVE:
        sel = np.flatnonzero(t == ty)
        o1, n1 = eng.gcmc_trial(rep[sel], t[sel], m[sel], k[sel], rows[sel])
        assert np.array_equal(o1, old[sel]) and np.array_equal(n1, new[sel]), f"{variant}: type {ty} alone differs"
        u1 = eng.recip_energy_candidates(rep[sel], t[sel], m[sel], k[sel], rows[sel])
        assert np.array_equal(u1, u[sel]), f"{variant}: type {ty} alone, reciprocal"
        s_mv = np.flatnonzero((t == ty) & (k == MGPU_MOVE))
        o2, n2 = eng.trial_energy_candidates(rep[s_mv], t[s_mv], m[s_mv], rows[s_mv])
        at = np.isin(mv, s_mv)
        assert np.array_equal(o2, to[at]) and np.array_equal(n2, tn[at]), f"{variant}: type {ty} alone, trial moves"
    _check_items(eng, P, t[nw], m[nw], rows[nw], f"{variant}: eight types")
    _check_static(eng, P, f"{variant}: eight types")
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["flat_batch", "plane_fast", "triclinic"])
def test_eight_types_markov_chain(variant, refcpu_mod):
    """40 scripted commits over every active type (moves, insertions, deletions; a quarter rejected): after each, the
    counts of every type, the committed rows exactly, every molecule of the type to 1e-12 A and A(k) to 1e-10 against
    the oracle; no drift of A(k) from a fresh S(k) at the end"""
    s, caps, eng = _main(variant)
    P = oracle(s, max(caps))
    rng = np.random.default_rng(40)
    W = int(s.topo.atoms_in_res.max())
    n_acc = 0
    for step in range(40):
        ty = ACTIVE[step % len(ACTIVE)]
        n = P.num_residues(ty)
        n1 = int(s.topo.atoms_in_res[ty])
        kinds = ([MGPU_MOVE, MGPU_DELETION] if n else []) + ([MGPU_CREATION] if n < caps[ty] else [])
        kind = int(rng.choice(kinds))
        x = None
        if kind == MGPU_MOVE:
            mm = int(rng.integers(0, n))
            x = moved(P, s, ty, mm, rng)
            eo, en = o_move5(P, ty, mm, x)
        elif kind == MGPU_CREATION:
            mm = -1
            x = free_spot(s, eng, _template(ty), rng)
            eo, en = o_insert(P, ty, x)
        else:
            mm = int(rng.integers(0, n))
            eo, en = o_delete(P, ty, mm)
        rows = np.zeros((1, W, 3))
        if x is not None:
            rows[0, :n1] = x
        old, new = eng.gcmc_trial([0], [ty], [mm], [kind], rows)
        close(old[0], eo, f"{variant} step {step}: old")
        close(new[0], en, f"{variant} step {step}: new")
        acc = int(rng.uniform() < 0.75)
        eng.commit_candidates([0], [ty], [mm], [kind], None if x is None else rows[:, :n1], [acc])
        if acc:
            n_acc += 1
            if kind == MGPU_MOVE:
                P.set_molecule(ty, mm, x[0], x - x[0][None, :])
            elif kind == MGPU_CREATION:
                P.set_num_residues(ty, n + 1)
                P.set_molecule(ty, n, x[0], x - x[0][None, :])
            else:
                lcom, loff = P.get_molecule(ty, n - 1)
                P.set_molecule(ty, mm, lcom, loff)
                P.set_num_residues(ty, n - 1)
            sync(P)
        for tt in range(s.topo.n_res):
            assert eng.num_molecules(0, tt) == P.num_residues(tt), (variant, step, tt)
        if acc and kind != MGPU_DELETION:
            assert np.array_equal(eng.get_molecules(0, ty)[mm if kind == MGPU_MOVE else n], x), (variant, step)
        got = eng.get_molecules(0, ty)
        for j in range(P.num_residues(ty)):
            com, off = P.get_molecule(ty, j)
            assert np.max(np.abs(got[j] - (com[None, :] + off))) <= 1e-12, (variant, step, ty, j)
        amp_close(eng.structure_factor(0), P.amplitude(), f"{variant} step {step}: A(k)")
    assert 15 <= n_acc <= 38
    A_chain = eng.structure_factor(0)
    eng.init_structure_factor(0, True)
    amp_close(A_chain, eng.structure_factor(0), f"{variant}: A(k) drift after the chain")
    _check_static(eng, P, f"{variant}: after the chain")
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# part 3: relabelling
@pytest.mark.gpu
def test_relabelling_changes_nothing(refcpu_mod):
    """the main system with its residue types permuted (the framework moves from type 2 to type 4) and its atom type ids
    permuted: every energy agrees with the unpermuted run, type by type"""
    s, caps = main_system()
    s2, caps2 = relabelled(s, caps)
    a = _engine(s, {}, caps)
    b = _engine(s2, {}, caps2)
    assert_layout(b, expected_layout(s2, caps2, {}), "relabelled")
    ea, eb = a.system_energy(0), b.system_energy(0)
    for key in ea:
        close(eb[key], ea[key], f"relabelled: system {key}")
    inv = [PERM.index(t) for t in range(MAX_RES)]
    for t in range(MAX_RES):
        close(b.self_energy(inv[t]), a.self_energy(t), f"relabelled: self energy of type {t}")
    P = oracle(s, max(caps))
    t, m, k, rows, eo, en = _launch(s, caps, a, P, np.random.default_rng(8))
    rep = np.zeros(len(t), np.int32)
    oa, na = a.gcmc_trial(rep, t, m, k, rows)
    t2 = np.array([inv[x] for x in t], np.int32)
    ob, nb = b.gcmc_trial(rep, t2, m, k, rows)
    for c in range(len(t)):
        close(ob[c], oa[c], f"relabelled: item {c} (type {t[c]} -> {t2[c]}) old")
        close(nb[c], na[c], f"relabelled: item {c} (type {t[c]} -> {t2[c]}) new")
        close(na[c], en[c], f"relabelled: item {c} new against the oracle")
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------------
# part 4: the layout switches on both sides
def _check_replica(eng, P, r, t, m, rows, what):
    """_check_items on replica r: the single-state sweep, the resident old state and the trial path, and the static total"""
    n = len(t)
    rep = np.full(n, r, np.int32)
    n1 = [int(P.sys.topo.atoms_in_res[tt]) for tt in t]
    exp_new = [_expect_new(P, int(t[c]), int(m[c]), rows[c, :n1[c]]) for c in range(n)]
    exp_old = [P.pair_singlemol(int(t[c]), int(m[c])) if m[c] >= 0 else (0.0, 0.0) for c in range(n)]
    a, b = eng.pair_energy_candidates(rep, t, m, rows)
    old, new = eng.gcmc_trial(rep, t, m, np.where(m >= 0, MGPU_MOVE, MGPU_CREATION).astype(np.int32), rows)
    for c in range(n):
        _close([a[c], b[c]], exp_new[c], f"{what}: candidate {c} single-state new")
        _close(old[c, :2], exp_old[c], f"{what}: candidate {c} trial old")
        _close(new[c, :2], exp_new[c], f"{what}: candidate {c} trial new")
    e, ref = eng.system_energy(r), P.system_energy()
    _close([e["non_coulomb"], e["coulomb"]], [ref["non_coulomb"], ref["coulomb"]], f"{what}: static total")


@pytest.mark.gpu
@pytest.mark.parametrize("name", LAYOUT_CASES)
def test_layout_switch(name, refcpu_mod):
    """each case's layout as claimed, then moves and insertions of every active type in one launch (single-state sweep,
    resident old state, trial path) and the static total against the oracle"""
    s, caps, R, claim = layout_system(name)
    diff = name == "batch_frozen_diff"
    for env in ([{}, {"MGPU_PAIR_FLAT": "1"}] if name == "active_63_64" else [{}]):
        eng = _engine(s, env, caps, R)
        if diff:                       # replica 1's framework 0.02 A off: frozen_diff
            s1 = s.copy()
            s1.com[2] = s.com[2] + np.array([0.01, -0.02, 0.015])
            eng.set_molecules(1, 2, s1.all_sites(2))
            eng.init_structure_factor(1, True)
        exp = expected_layout(s, caps, env, diff)
        assert exp["flat"] == claim["flat"] and (exp["groups"], exp["planes"]) == (claim["groups"], claim["planes"])
        assert_layout(eng, exp, f"{name} {env}")
        P = oracle(s, max(caps))
        rng = np.random.default_rng(len(name))
        W = int(s.topo.atoms_in_res.max())
        t, m, rows = [], [], []
        for ty in range(s.topo.n_res):
            if not s.topo.is_active[ty]:
                continue
            n1 = int(s.topo.atoms_in_res[ty])
            for mm in range(min(2, int(s.n_mol[ty]))):
                r = np.zeros((W, 3)); r[:n1] = moved(P, s, ty, mm, rng)
                t.append(ty); m.append(mm); rows.append(r)
            r = np.zeros((W, 3)); r[:n1] = free_spot(s, eng, s.offsets[ty][0], rng)
            t.append(ty); m.append(-1); rows.append(r)
        assert len(set(t)) >= 2
        _check_items(eng, P, np.array(t), np.array(m), np.array(rows), f"{name} {env}")
        _check_static(eng, P, f"{name} {env}")
        if diff:                       # the replica that differs, against an oracle of its own framework
            _check_replica(eng, oracle(s1, max(caps)), 1, np.array(t), np.array(m), np.array(rows), f"{name} replica 1")
        assert eng.pair_layout() == exp
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# part 5: device-built moves and reservoirs on types >= 2
def _four_types(extra64=False):
    specs = [(species("cation"), 1, 4), (species("spce"), 1, 6), (species("co2"), 1, 6), (species("tip4p"), 1, 6)]
    caps = [8, 10, 12, 12]
    if extra64:
        specs.append((species("shell64"), 1, 1))
        caps.append(2)
    return build(specs, L=30.0, seed=13), caps


@pytest.mark.gpu
def test_device_built_moves_and_reservoir_on_types_2_and_3(refcpu_mod):
    """four active plane-major types: farm windows take the box (and refuse it once a 64-site active type is added);
    translations, rotations and insertions built on the device for types 2 and 3, read back after their commit, are the
    oracle's ApplyPBC / RotationMatrix composition to 1e-12 A; reservoirs on types 2 and 3: box + reservoir count
    conserved per type"""
    s64, c64 = _four_types(True)
    e64 = _engine(s64, {}, c64)
    assert e64.farm_window_capacity()[0] == 0
    e64.close()
    s, caps = _four_types()
    P = oracle(s, max(caps))
    moves = [1, 2, 3] * 4
    n = len(moves)
    eng = _engine(s, {}, caps, R=n)
    assert eng.farm_window_capacity()[0] > 0
    for r in range(n):
        for t in range(4):
            eng.set_frames(r, t, s.com[t], s.offsets[t])
        eng.init_structure_factor(r, True)
    rng = np.random.default_rng(17)
    u = rng.random((n, 5))
    u[:, 4] = np.resize([0.05, 0.4, 0.7, 0.99], n)              # every rotation axis
    u[0, :3] = 0.02                                              # a translation out of the cell
    t = np.array([2, 2, 2, 3, 3, 3] * 2, np.int32)
    m = np.array([int(rng.integers(0, s.n_mol[tt])) for tt in t], np.int32)
    move = np.array(moves, np.int32)
    rep = np.arange(n, dtype=np.int32)
    t_step, r_step = 6.0, 0.6
    L = np.diag(s.box_matrix)
    lo = s.bounds_lo
    eng.move_trial(rep, t, m, move, u, t_step, r_step)
    kinds = np.where(move <= 2, MGPU_MOVE, MGPU_CREATION).astype(np.int32)
    eng.commit_lane(0, rep, t, m, kinds, np.ones(n, np.int32))
    for c in range(n):
        tt, mm = int(t[c]), int(m[c])
        com0, off0 = s.com[tt][mm], s.offsets[tt][mm]
        slot = mm
        if move[c] == 1:
            com_e, off_e = P.apply_pbc(com0 + (u[c, :3] - 0.5) * t_step), off0
        elif move[c] == 2:
            com_e, off_e = com0, off0 @ P.rotation_matrix(int(u[c, 4] * 3.0) + 1, (u[c, 3] - 0.5) * r_step).T
        else:
            slot = int(s.n_mol[tt])
            com_e = lo + L * u[c, :3]
            off_e = s.offsets[tt][0] @ P.rotation_matrix(int(u[c, 4] * 3.0) + 1, u[c, 3] * 2 * np.pi).T
        com_d, off_d = eng.get_frames(c, tt)
        assert np.max(np.abs(com_d[slot] - com_e)) <= 1e-12, (c, move[c])
        assert np.max(np.abs(off_d[slot] - off_e)) <= 1e-12, (c, move[c])
        assert np.array_equal(eng.get_molecules(c, tt)[slot], com_d[slot][None, :] + off_d[slot])
        for other in range(4):
            assert eng.num_molecules(c, other) == s.n_mol[other] + (other == tt and move[c] == 3), (c, other)
    # reservoirs on type 2 (replica 0) and type 3 (replica 3): an insertion takes a molecule out, a deletion puts one in;
    # per type, box + reservoir count is conserved and no other type's count or reservoir moves
    for r, ty in ((0, 2), (3, 3)):
        res = np.stack([s.offsets[ty][0] @ synth._random_rotations(rng, 1)[0].T for _ in range(5)])
        eng.set_reservoir(r, ty, res)
        total = eng.num_molecules(r, ty) + eng.get_reservoir(r, ty).shape[0]
        others = [o for o in range(4) if o != ty]
        before = [eng.num_molecules(r, o) for o in others]
        for mv in (3, 4, 3):
            eng.move_trial([r], [ty], [0], [mv], rng.random((1, 5)), t_step, r_step)
            eng.commit_lane(0, [r], [ty], [0], [MGPU_CREATION if mv == 3 else MGPU_DELETION], [1])
            assert eng.num_molecules(r, ty) + eng.get_reservoir(r, ty).shape[0] == total, (r, ty, mv)
            assert [eng.num_molecules(r, o) for o in others] == before, (r, ty, mv)
            assert all(eng.get_reservoir(r, o).shape[0] == 0 for o in others), (r, ty, mv)
        assert eng.num_molecules(r, ty) == s.n_mol[ty] + 1
        assert eng.get_reservoir(r, ty).shape[0] == total - s.n_mol[ty] - 1
        A = eng.structure_factor(r)
        eng.init_structure_factor(r, True)
        amp_close(A, eng.structure_factor(r), f"replica {r} A(k) after the reservoir steps of type {ty}")
    eng.close()


def _one_window(a, b, reps, caps, rng, rnd, by_count, t_step=0.8, r_step=0.6, phiV=3.0):
    """one farm window on engine a whose chains name all four types, against the oracle replay, and the same steps on the
    batched path of engine b (device-built trials, the window's verdicts committed): energies bit for bit"""
    R = len(reps)
    rep = np.arange(R, dtype=np.int32)
    tt = ((rep + rnd) % 4).astype(np.int32)
    n_now = np.array([reps[r].P.num_residues(int(tt[r])) for r in range(R)])
    move = rng.integers(1, 5, R).astype(np.int32)
    u = rng.uniform(0, 1, (R, 5))
    au = rng.uniform(0, 1, R)
    su = rng.uniform(0, 1, R)
    if by_count:
        pref = np.where(move >= 3, phiV, 1.0)
        a.farm_window_submit(rep, tt, np.zeros(R, np.int32), move, u, t_step, r_step, au, pref, 300.0, slot_u=su)
    else:
        move[(n_now <= 1) & (move == 4)] = 3
        move[n_now == 0] = 3
        move[(n_now >= np.array([caps[t] for t in tt])) & (move == 3)] = 1
        m = np.array([rng.integers(0, max(n_now[r], 1)) for r in range(R)], np.int32)
        m[move == 3] = 0
        pref = np.array([_by_count(int(n_now[r]), caps[tt[r]], int(move[r]), 0.0, phiV)[2] if move[r] >= 3 else 1.0
                         for r in range(R)])
        a.farm_window_submit(rep, tt, m, move, u, t_step, r_step, au, pref, 300.0)
        su = np.where(move == 3, 0.0, (m + 0.5) / np.maximum(n_now, 1))
    old, new, v = a.farm_window_wait(R)
    recs = []
    for r in range(R):
        live, mr, _ = _by_count(int(n_now[r]), caps[tt[r]], int(move[r]), su[r], phiV)
        recs.append((r, int(tt[r]), mr, int(move[r]) if live else 0, u[r]))
    live = np.array([rc[3] != 0 for rc in recs])
    lr = np.flatnonzero(live)
    mv = np.array([recs[r][3] for r in lr], np.int32)
    mm = np.array([recs[r][2] for r in lr], np.int32)
    ob, nb = b.move_trial(rep[lr], tt[lr], mm, mv, u[lr], t_step, r_step)
    assert np.array_equal(ob, old[lr]) and np.array_equal(nb, new[lr]), f"window {rnd}: the batched path differs"
    kinds = np.where(mv <= 2, MGPU_MOVE, np.where(mv == 3, MGPU_CREATION, MGPU_DELETION)).astype(np.int32)
    b.commit_lane(0, rep[lr], tt[lr], mm, kinds, (v[lr] == V_ACC).astype(np.int32))
    _check_window(a, reps, recs, old, new, v, t_step, r_step, f"window {rnd}")
    return [(rc[3], int(v[i])) for i, rc in enumerate(recs)]


@pytest.mark.gpu
@pytest.mark.parametrize("by_count", [False, True], ids=["caller_picked", "by_count"])
def test_farm_windows_over_four_types(by_count, refcpu_mod):
    """farm windows whose chains name all four active types in every launch -- translations, rotations, insertions and
    deletions, caller-picked or completed from the count: each window against the oracle replay and bit for bit against
    the batched device-built path given the same numbers and verdicts; counts, sites and A(k) of every replica after"""
    s, caps = _four_types()
    R = 4
    a = window_engine(s, R, cap=caps)
    b = window_engine(s, R, cap=caps)
    assert a.farm_window_capacity()[0] >= R
    reps = [Replay(refcpu_mod, s) for _ in range(R)]
    rng = np.random.default_rng(61 + by_count)
    seen = set()
    for rnd in range(12):
        seen.update(_one_window(a, b, reps, caps, rng, rnd, by_count))
    assert {(mv, V_ACC) for mv in (1, 3, 4)} <= seen and any(v == V_REJ for _, v in seen), seen
    _same_as_oracle(a, reps, "four-type windows")
    for r in range(R):
        amp_close(a.structure_factor(r), reps[r].P.amplitude(), f"replica {r} A(k)")
        assert np.array_equal(a.structure_factor(r), b.structure_factor(r)), r
        for t in range(4):
            assert np.array_equal(a.get_molecules(r, t), b.get_molecules(r, t)), (r, t)
    a.close()
    b.close()


@pytest.mark.gpu
def test_chain_windows_on_types_2_and_3(refcpu_mod):
    """chain_window_kernel with rows of types 2 (3 sites) and 3 (4 sites) in one window -- moves, an insertion, a
    deletion: every row against the oracle, and after the device's commit of the first accepted row A(k), the counts of
    every type and the committed molecule"""
    s, caps = _four_types()
    eng = _engine(s, {}, caps)
    rp = Replay(refcpu_mod, s)
    P = rp.P
    rng = np.random.default_rng(9)
    rows_t = np.array([2, 3, 2, 3, 3], np.int32)
    kinds = np.array([MGPU_MOVE, MGPU_MOVE, MGPU_CREATION, MGPU_DELETION, MGPU_MOVE], np.int32)
    n = len(kinds)
    assert eng.chain_window_capacity() >= n
    n_first = 0
    for w in range(4):
        n_now = {t: P.num_residues(t) for t in (2, 3)}
        free = {t: list(rng.permutation(n_now[t])) for t in (2, 3)}
        m = np.zeros(n, np.int32)
        sites = np.zeros((n, 4, 3))
        for c in range(n):
            t = int(rows_t[c])
            n1 = int(s.topo.atoms_in_res[t])
            if kinds[c] == MGPU_CREATION:
                m[c] = -1
                sites[c, :n1] = free_spot(s, eng, s.offsets[t][0], rng)
            else:
                m[c] = int(free[t].pop())
                if kinds[c] == MGPU_MOVE:
                    sites[c, :n1] = moved(P, s, t, int(m[c]), rng)
        recip_now = rp._recip_now()
        exp = [_chain_oracle(P, int(rows_t[c]), int(kinds[c]), int(m[c]), sites[c, :int(s.topo.atoms_in_res[rows_t[c]])],
                             n_now[int(rows_t[c])], recip_now) for c in range(n)]
        u = np.full(n, 0.999999)
        u[(w + 1) % n] = 1e-300
        old, new, first, und = eng.chain_window(0, rows_t, m, kinds, sites, u, np.ones(n), 300.0, recip_now)
        assert und == -1
        for c in range(n):
            close(old[c], exp[c][0], f"chain window {w} row {c} (type {rows_t[c]}) old")
            close(new[c], exp[c][1], f"chain window {w} row {c} (type {rows_t[c]}) new")
        if first < 0:
            amp_close(eng.structure_factor(0), P.amplitude(), f"chain window {w}: A unchanged")
            continue
        n_first += 1
        t, k, mf = int(rows_t[first]), int(kinds[first]), int(m[first])
        n1 = int(s.topo.atoms_in_res[t])
        x = sites[first, :n1]
        amp_close(eng.structure_factor(0), exp[first][2], f"chain window {w}: A after the commit")
        if k == MGPU_MOVE:
            P.set_molecule(t, mf, x[0], x - x[0][None, :])
            assert np.array_equal(eng.get_molecules(0, t)[mf], x)
        elif k == MGPU_CREATION:
            P.set_num_residues(t, n_now[t] + 1)
            P.set_molecule(t, n_now[t], x[0], x - x[0][None, :])
            assert np.array_equal(eng.get_molecules(0, t)[n_now[t]], x)
        else:
            lcom, loff = P.get_molecule(t, n_now[t] - 1)
            P.set_molecule(t, mf, lcom, loff)
            P.set_num_residues(t, n_now[t] - 1)
        sync(P)
        for tt in range(4):
            assert eng.num_molecules(0, tt) == P.num_residues(tt), (w, tt)
        amp_close(eng.structure_factor(0), P.amplitude(), f"chain window {w}: A followed")
    assert n_first >= 2
    eng.close()


def _rod_system_at_types_2_and_3():
    """test_gpu_window_edges' rod system with its two types moved to residue types 2 (tight) and 3 (the rod: not tight),
    behind two single-ion types placed away from the rod's column"""
    s, ctr, L = _rod_system()
    t0 = s.topo
    eps, sig = lorentz_berthelot([0.12, 0.20, 0.0, 0.07, 0.10, 0.10], [3.0, 3.4, 0.0, 2.7, 2.5, 4.0])
    types = np.zeros((4, t0.max_atom), np.int32)
    charges = np.zeros((4, t0.max_atom))
    types[0, 0], charges[0, 0], types[1, 0], charges[1, 0] = 5, 1.0, 6, -1.0
    types[2:], charges[2:] = t0.atom_types, t0.charges
    topo = Topology([1, 1] + list(t0.atoms_in_res), types, charges, [1, 1, 1, 1], eps, sig)
    col = np.array([ctr[0] - 4.0, ctr[1] - 5.0])
    allsites = np.concatenate([s.all_sites(t).reshape(-1, 3) for t in range(2)])
    lo = np.asarray(s.bounds_lo, dtype=np.float64)
    rng = np.random.default_rng(3)
    ions = []
    while len(ions) < 2:
        p = lo + rng.uniform(0.0, 1.0, 3) * L
        d = allsites - p
        d -= L * np.rint(d / L)
        dc = p[:2] - col
        dc -= L[:2] * np.rint(dc / L[:2])
        if np.min(np.linalg.norm(d, axis=1)) > 4.0 and np.linalg.norm(dc) > 7.0:
            ions.append(p)
            allsites = np.vstack([allsites, p])
    s2 = System(topo, s.box_matrix, s.bounds_lo, s.real_space_cutoff, s.ewald_tolerance, s.temperature,
                [ions[0][None], ions[1][None]] + [s.com[0], s.com[1]],
                [np.zeros((1, 1, 3)), np.zeros((1, 1, 3))] + [s.offsets[0], s.offsets[1]])
    return s2, ctr, L


@pytest.mark.gpu
def test_fast_fold_after_a_non_tight_step_on_types_2_and_3(refcpu_mod):
    """test_fast_fold_after_an_accepted_non_tight_step_in_flight with the two types at residue types 2 and 3: window i
    moves the rod (type 3, frames not tight) with forced acceptance, window i + 1, queued before i is collected, moves a
    type-2 molecule of the same replica next to the rod's far image; against the oracle and against the exact fold"""
    s, ctr, L = _rod_system_at_types_2_and_3()
    res = {}
    for name, env in (("default", {}), ("exact", {"MGPU_PAIR_EXACT_FOLD": "1"})):
        eng = window_engine(s, 1, env)
        rp = Replay(refcpu_mod, s)
        T = float(s.temperature)
        t_step = 30.0
        u_rod = np.array([[0.5, 0.5, 0.5 + 14.3 / t_step, 0.1, 0.1]])
        eng.farm_window_submit([0], [3], [0], [1], u_rod, t_step, 0.5, [0.5], [1.0], T, forced=[1])
        t_step2 = 10.0
        u_a = np.array([[0.5 - 3.0 / t_step2, 0.5, 0.5, 0.1, 0.1]])
        eng.farm_window_submit([0], [2], [0], [1], u_a, t_step2, 0.5, [0.5], [1.0], T)
        o1, n1, v1 = eng.farm_window_wait(1)
        assert v1[0] == V_ACC
        com, off = eng.get_frames(0, 3)
        assert abs(com[0][2] + off[0][1][2] - (ctr[2] + 32.0)) < 1e-9
        _check_window(eng, [rp], [(0, 3, 0, 1, u_rod[0])], o1, n1, v1, t_step, 0.5, "window i (rod, type 3)", False)
        o2, n2, v2 = eng.farm_window_wait(1)
        res[name] = (o2[0].copy(), n2[0].copy())
        _check_window(eng, [rp], [(0, 2, 0, 1, u_a[0])], o2, n2, v2, t_step2, 0.5, f"window i + 1 (type 2, {name} fold)")
        eng.close()
    assert np.array_equal(res["default"][0], res["exact"][0]) and np.array_equal(res["default"][1], res["exact"][1])


# ---------------------------------------------------------------------------------------------------------------------
# part 6: the Fortran farm on a framework box with three active types (types 0, 2 and 3; the framework is type 1)
FARM_MODES = {"host_built": dict(), "device_built": dict(device_build=True),
              "device_decided": dict(device_build=True, device_accept=True), "window": dict(device_build=True, window=True)}
FARM_KEYS = ("non_coulomb", "coulomb", "recip_coulomb", "ewald_self", "intra_coulomb")


def _farm(mode, R=6, env=None):
    from maniac_mc_amd.fortran_host import FortranFarm
    s = build([(species("spce"), 1, 5), (FR5, 0, 1), (species("co2"), 1, 5), (species("tip4p"), 1, 5)], L=24.0, seed=21)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        farm = FortranFarm(s, R, seed=19, translation_step=0.6, rotation_step=0.5, n_threads=2, mol_capacity=[24, 1, 24, 24],
                           gcmc=dict(p_translation=0.25, p_rotation=0.25, fugacity=6.0 / 24.0 ** 3), **FARM_MODES[mode])
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    return s, farm


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(FARM_MODES))
def test_fortran_farm_on_three_active_types(mode):
    """running energies equal a from-scratch evaluation within farm_tol, A(k) a fresh S(k), counts and host mirrors the
    device, for every active type.  The device-decided farm is the host-decided device-built farm bit for bit; so is the
    window farm, against a batched farm that sweeps the framework with pair_flat_kernel as the windows do (the frozen
    batch, pair_frozen_kernel, sums the framework in another order: the two then agree to rounding only)."""
    steps = 150
    env = {"MGPU_NO_FROZEN_BATCH": "1"} if mode == "window" else {}
    s, farm = _farm(mode, env=env)
    ref = _farm("device_built", env=env)[1] if mode in ("device_decided", "window") else None
    assert list(farm.active) == [0, 2, 3]
    assert farm.window == (mode == "window")
    assert farm.eng.pair_layout()["frozen_batch"] == (-1 if mode == "window" else 1)
    farm.run(steps)
    eng = farm.eng
    counts = farm.counts()
    c = farm.counters()
    assert c["creations"] > 0 and c["deletions"] > 0 and c["translations"] > 0, c
    if ref is not None:
        ref.run(steps)
        assert ref.trials == farm.trials and ref.accepted == farm.accepted and ref.skipped == farm.skipped
        assert ref.counters() == c and np.array_equal(ref.counts(), counts)
        for r in range(farm.R):
            assert np.array_equal(ref.energy(r), farm.energy(r)), r
            assert np.array_equal(ref.eng.structure_factor(r), eng.structure_factor(r)), r
            for t in farm.active:
                assert np.array_equal(ref.eng.get_molecules(r, int(t)), eng.get_molecules(r, int(t))), (r, t)
        ref.close()
    for r in range(farm.R):
        e = eng.system_energy(r)
        want = np.array([e[k] for k in FARM_KEYS])
        assert np.max(np.abs(farm.energy(r) - want)) < farm_tol(want, steps), (r, farm.energy(r) - want)
        A = eng.structure_factor(r)
        eng.init_structure_factor(r, True)
        assert np.max(np.abs(A - eng.structure_factor(r))) < 1e-9
        assert eng.num_molecules(r, 1) == 1
        for ia, t in enumerate(farm.active):
            dev = eng.get_molecules(r, int(t))
            assert dev.shape[0] == counts[r, ia], (r, t)
            for slot in range(counts[r, ia]):
                com, off = farm.molecule(r, ia, slot)
                assert np.array_equal(dev[slot], com[None, :] + off[: dev.shape[1]]), (r, t, slot)
    farm.close()
