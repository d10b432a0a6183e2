"""The two orthorhombic cells, the edge inputs and the reference arithmetic shared by tests/test_gpu_ortho_moves.py (the
device's trial geometry against the oracle's, bit for bit) and tests/test_gpu_gcmc.py.  Everything here is numpy or plain Python
and needs no GPU.  Reference: src/translation.f90:93-112, src/geometry_utils.f90:167-220 (ApplyPBC), src/monte_carlo_utils.f90:
30-92 (the rotation), src/create_molecule.f90:166-207, src/helper_utils.f90:39-77 (RotationMatrix)."""
import math
from fractions import Fraction

import numpy as np

CELLS = ("cubic", "ortho")
EDGES = {"cubic": (30.0, 30.0, 30.0), "ortho": (22.0, 26.5, 31.0)}
N_MOL = (8, 8, 4)                     # 1-site, 3-site, 6-site molecules: 20 per cell
EPS = 2.0 ** -52
U_LAST = 1.0 - 2.0 ** -53             # the largest double below 1
U_EDGE = (0.0, 2.0 ** -53, U_LAST)    # draws at the ends of [0, 1)
U_INSERT = (0.0, 2.0 ** -53, 1e-17, 0.5, U_LAST)
R_STEP = 0.6

# The bound on a ROTATED offset coordinate: |device - oracle| <= K_ROT * 2^-52 * (|x| + |y|), x and y the two components the
# rotation mixes.  The centre and every unmixed component are held bit for bit; only cos / sin (the device's sincos against
# libm's) and the order of the two-term sum differ.  Measured on an MI355X over the cases of tests/test_gpu_ortho_moves.py and
# of tests/test_gpu_gcmc.py::test_device_built_coordinates_are_the_references_moves (the batched build, the farm windows and the
# grand-canonical runs; 0.36 to 0.70 per test): the largest ratio is K_ROT_MEASURED; K_ROT is twice that, rounded up to an integer
# (LABNOTES.md).  For offsets of a few Angstrom that is about 1e-15 A, three orders below the 1e-12 A the suite asked before.
K_ROT_MEASURED = 0.702
K_ROT = 2


def _atom():
    """a neutral Lennard-Jones site"""
    return np.zeros((1, 3)), np.array([1], np.int32), np.array([0.0])


def cell(name, wide_active=True):
    """cubic: L = 30, bounds_lo = 0.  ortho: three different edges, bounds_lo = -L / 2 + 0.1 (no dyadic fraction: the sums
    lo + x round).  Both hold a 1-site type, a 3-site type and a rigid plane-major 6-site type, placed and oriented at random
    as tests/test_gpu_farm_window_wide.py places its types.  wide_active=False: the 6-site type is there but inactive (no
    path then takes the instances for 6 to 63 sites)."""
    from tests.test_gpu_farm_window_wide import _shell, _system, _water
    L = np.array(EDGES[name])
    specs = [(*_atom(), N_MOL[0]), (*_water(), N_MOL[1]), (*_shell(6, seed=21), N_MOL[2])]
    s = _system(np.diag(L), specs, active=[1, 1, 1 if wide_active else 0], rc=10.0, seed=31, gap=2.0)
    lo = np.zeros(3) if name == "cubic" else -0.5 * L + 0.1
    shift = lo - s.bounds_lo
    s.bounds_lo = lo.copy()
    s.com = [np.ascontiguousarray(c + shift) for c in s.com]
    for c in s.com:
        assert np.all(c >= lo) and np.all(c < lo + L)
    return s


def edges(s):
    return np.diag(s.box_matrix).copy()


def t_step(s):
    """2.5 max(L): a move from inside the cell leaves it by more than one period"""
    return 2.5 * float(np.max(edges(s)))


def face_values(s):
    """(6, 3): per axis lo, lo + L and the doubles next to each on both sides"""
    lo, L = s.bounds_lo, edges(s)
    rows = []
    for base in (lo, lo + L):
        rows += [base.copy(), np.nextafter(base, -np.inf), np.nextafter(base, np.inf)]
    return np.array(rows)


def axis_draws():
    """u[4] at 0, at 1/3 and 2/3 as doubles, at their neighbours on both sides and at the last double below 1"""
    a, b = 1.0 / 3.0, 2.0 / 3.0
    return [0.0, a, np.nextafter(a, 0.0), np.nextafter(a, 1.0), b, np.nextafter(b, 0.0), np.nextafter(b, 1.0), U_LAST]


def first_round(s, seed=7):
    """The edge cases, one candidate per replica: [(t, m, move, u[5], start centre or None)] -- None: the molecule starts where
    the cell holds it (inside)."""
    rng = np.random.default_rng(seed)
    lo, L = s.bounds_lo, edges(s)
    F = face_values(s)
    recs = []
    k = [0]

    def add(move, u, start=None, t=None):
        t_ = k[0] % 3 if t is None else t
        m = 0 if move == 3 else (k[0] // 3) % N_MOL[t_]
        recs.append((t_, m, move, np.array(u, dtype=np.float64), None if start is None else np.array(start, dtype=np.float64)))
        k[0] += 1

    def draws(**kw):
        u = rng.random(5)
        for i, v in kw.items():
            u[int(i[1:])] = v
        return u

    # ---- translations
    starts = [F[i] for i in range(6)]                                   # every axis on the same face value
    for i in range(6):                                                  # mixed: each axis on another one
        starts.append(np.array([F[(i + d * 2) % 6][d] for d in range(3)]))
    for p in starts:                                                    # a displacement of exactly zero: x == L must wrap to lo,
        add(1, draws(u0=0.5, u1=0.5, u2=0.5), p)                        # x just below zero comes back as lo + L
    for p in starts:
        add(1, rng.random(5), p)
    for _ in range(12):                                                 # up to 200 A outside: fmod takes a large quotient
        add(1, rng.random(5), rng.uniform(-200.0, 200.0, 3))
    for i in range(6):                                                  # the ends of [0, 1)
        add(1, draws(u0=U_EDGE[i % 3], u1=U_EDGE[(i + 1) % 3], u2=U_EDGE[(i + 2) % 3]))
    for _ in range(30):
        add(1, rng.random(5))
    # ---- rotations (3- and 6-site types)
    for t in (1, 2):
        for ua in axis_draws():
            add(2, draws(u4=ua), t=t)
        for ua in (0.1, 0.5, 0.9):                                      # the angle is zero: nothing may change in any bit
            add(2, draws(u3=0.5, u4=ua), t=t)
    # ---- insertions
    ax = axis_draws()
    for t in (0, 1, 2):
        for i in range(12):
            u = rng.random(5)
            if i < 6:
                u[:3] = np.array(U_INSERT)[rng.integers(0, len(U_INSERT), 3)]
            if i % 4 == 0:
                u[3] = 0.0                                              # cs = 1, sn = 0: molecule 1's offsets bit for bit
            if i >= 4:
                u[4] = ax[(i - 4) % len(ax)]
            add(3, u, t=t)
    return recs


# ---------------------------------------------------------------------------------------------------------------------
# the reference's arithmetic, elementwise in numpy (no product is fused into a sum)
def f_modulo(x, L):
    """Fortran's modulo(x, L), L > 0"""
    r = math.fmod(x, L)
    if r != 0.0 and r < 0.0:
        r = r + L
    return r


def wrap_stated(s, pos):
    """ApplyPBC of an orthorhombic cell in plain Python: lo + modulo(pos - lo, L)"""
    lo, L = s.bounds_lo, edges(s)
    return np.array([float(lo[d]) + f_modulo(float(pos[d]) - float(lo[d]), float(L[d])) for d in range(3)])


def translated(s, P, com0, u, step):
    """Translation: the displacement (u - 1/2) step is ROUNDED (translation.f90:104-105 stores it), added, then wrapped"""
    disp = (u[:3] - 0.5) * step
    return P.apply_pbc(com0 + disp)


def inserted(s, u):
    """CreateMolecule without a reservoir: lo + L u, the product rounded before lo is added (create_molecule.f90:181-182)"""
    prod = edges(s) * u[:3]
    return s.bounds_lo + prod


def axis_of(u4):
    return int(3.0 * u4) + 1


def rotated(P, off, axis, theta):
    """off (n1, 3) times RotationMatrix(axis, theta) as matmul forms it: every product rounded, summed left to right"""
    R = P.rotation_matrix(axis, theta)
    out = np.empty_like(off)
    for i in range(3):
        out[:, i] = (R[i, 0] * off[:, 0] + R[i, 1] * off[:, 1]) + R[i, 2] * off[:, 2]
    return out


def mixed_axes(axis):
    """the two Cartesian components RotationMatrix(axis) mixes"""
    return axis % 3, (axis + 1) % 3


def rotation_ratio(off_d, off_e, off0, axis):
    """Largest |device - oracle| / (2^-52 (|x| + |y|)) over the mixed components, and whether the third is unchanged"""
    p, q = mixed_axes(axis)
    r = 3 - p - q
    scale = EPS * (np.abs(off0[:, p]) + np.abs(off0[:, q]))
    worst = 0.0
    for i in (p, q):
        err = np.abs(off_d[:, i] - off_e[:, i])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0.0, 0.0, err / scale)
        worst = max(worst, float(np.max(ratio)))
    return worst, bool(np.array_equal(off_d[:, r], off0[:, r]))


def closest_approach(s, com, off, t, m, sites):
    """Smallest minimum-image distance between `sites` (a candidate for molecule (t, m); m = None: an insertion) and every site
    of every other molecule of the state (com[t] (n, 3), off[t] (n, n1, 3))"""
    L = edges(s)
    best = np.inf
    for tt in range(len(com)):
        keep = np.ones(com[tt].shape[0], bool)
        if tt == t and m is not None:
            keep[m] = False
        other = (com[tt][keep][:, None, :] + off[tt][keep]).reshape(-1, 3)
        if other.size == 0:
            continue
        d = sites[:, None, :] - other[None, :, :]
        d -= L * np.rint(d / L)
        best = min(best, float(np.sqrt(np.min(np.sum(d * d, axis=2)))))
    return best


# ---------------------------------------------------------------------------------------------------------------------
# what a fused multiply-add would give instead: exact rational arithmetic, rounded once
def fused(a, b, c):
    """round(a b + c)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def translated_fused(s, com0, u, step):
    lo, L = s.bounds_lo, edges(s)
    out = np.empty(3)
    for d in range(3):
        x = fused(u[d] - 0.5, step, com0[d]) - float(lo[d])
        out[d] = float(lo[d]) + f_modulo(x, float(L[d]))
    return out


def inserted_fused(s, u):
    lo, L = s.bounds_lo, edges(s)
    return np.array([fused(L[d], u[d], lo[d]) for d in range(3)])
