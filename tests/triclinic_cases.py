"""The two triclinic cells and the edge inputs shared by tests/test_triclinic_wrap_oracle.py (no GPU: the oracle's ApplyPBC
against the compiled reference's) and tests/test_gpu_triclinic_moves.py (the device's trial geometry against the oracle's)."""
import numpy as np

from maniac_mc_amd import synth

CELLS = ("mild", "sheared")
# fractional parts put within 1e-16 of 0 and of 1 (and exactly on them); integer cell offsets of up to three cells
EDGE_FRAC = (0.0, 1e-17, -1e-17, 1e-16, -1e-16, 0.5, 1.0 - 1e-16)


def cell(name, seed=6):
    """mild: the tilt of tests/test_oracle_pin.py's triclinic pin.  sheared: the largest tilt LAMMPS allows
    (tests/test_gpu_parity.py): the eight-image certificate of the distance search fails there and the full search runs."""
    if name == "mild":
        return synth.mixture_box(seed=seed, tilt=(1.5, -0.8, 0.6))
    return synth.mixture_box(box=(18.0, 21.0, 24.0), seed=seed, tilt=(8.9, -11.9, 10.4), n_a=10, n_b=8)


def cart(s, f, transpose=False):
    """lo + M f, each product rounded, summed left to right (create_molecule.f90:181-182): elementwise, so the same doubles
    on every host.  transpose: lo + M^T f"""
    f = np.asarray(f, dtype=np.float64)
    M, lo = np.asarray(s.box_matrix, dtype=np.float64), np.asarray(s.bounds_lo, dtype=np.float64)
    if transpose:
        M = M.T
    out = np.empty(f.shape)
    for i in range(3):
        out[..., i] = lo[i] + ((M[i, 0] * f[..., 0] + M[i, 1] * f[..., 1]) + M[i, 2] * f[..., 2])
    return out


def edge_points(s, n, seed, transpose=False):
    """n points lo + M f with f = an integer in [-3, 3] plus one of EDGE_FRAC, per axis.
    transpose: lo + M^T f.  ApplyPBC forms f = box%reciprocal (pos - lo), and box%reciprocal is the inverse of the TRANSPOSE
    of box%matrix (its rows are the reciprocal vectors of the cell vectors the reader stores as rows): these are the points
    whose fractional coordinates ApplyPBC finds within 1e-16 of 0 and of 1.  (lo + M f is the family the wrap was first
    checked on; a point of it lands anywhere in the cell.)"""
    rng = np.random.default_rng(seed)
    f = rng.integers(-3, 4, (n, 3)).astype(np.float64) + np.asarray(EDGE_FRAC)[rng.integers(0, len(EDGE_FRAC), (n, 3))]
    return cart(s, f, transpose)


def apply_pbc_stated(s, reciprocal, pos):
    """ApplyPBC of a triclinic cell as the engine's header states it, elementwise: v = pos - lo; f_i = rcp[i][0] v0 + rcp[i][1]
    v1 + rcp[i][2] v2 summed left to right; f <- modulo(f, 1) always; pos_i = lo_i + (m[i][0] f0 + m[i][1] f1 + m[i][2] f2)"""
    lo, rcp = np.asarray(s.bounds_lo, dtype=np.float64), np.asarray(reciprocal, dtype=np.float64).reshape(3, 3)
    v = np.asarray(pos, dtype=np.float64) - lo
    f = np.empty(v.shape)
    for i in range(3):
        f[..., i] = (rcp[i, 0] * v[..., 0] + rcp[i, 1] * v[..., 1]) + rcp[i, 2] * v[..., 2]
    r = np.fmod(f, 1.0)
    r = np.where((r != 0.0) & (r < 0.0), r + 1.0, r)
    return cart(s, r)


def wrap_inputs(s, n=20000, seed=101):
    """n uniform points of [-200, 200]^3 (centres many cells away), n edge points lo + M f and n edge points lo + M^T f"""
    rng = np.random.default_rng(seed)
    return np.vstack([rng.uniform(-200.0, 200.0, (n, 3)), edge_points(s, n, seed + 1), edge_points(s, n, seed + 2, True)])
