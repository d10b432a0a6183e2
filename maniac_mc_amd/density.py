"""Density maps of a replica farm: the host side of the engine's integer counts per voxel (mgpu_density_*,
include/maniac_gpu.h).  Nothing here needs the library or a device.

The engine counts; this module normalises:  rho_c(v) = H_c(v) / (samples V / (n0 n1 n2))  in sites per cubic Angstrom, H the
counts of a group pooled over its samples and replicas, `samples` the number of (replica, sample) configurations that went into
it.  Arrays are laid out as the engine's: hist[..., channel, v2, v1, v0], v_k the voxel along cell vector k (column k of
box%matrix).
"""
from __future__ import annotations

import os

import numpy as np

MAX_CHANNELS = 8
MAX_AXIS = 1024
MAX_VOXELS = 1 << 24
MAX_BYTES = 2 << 30            # include/maniac_gpu.h MGPU_DENSITY_MAX_BYTES: all accumulators of an engine together
BOHR = 0.529177210903          # Angstrom (CODATA 2018)

# standard atomic weights of the elements a framework or a guest usually holds; a mass within MASS_TOL of one names the element
MASS_TOL = 0.05
_MASSES = {1: 1.008, 2: 4.0026, 3: 6.94, 5: 10.81, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998, 10: 20.180, 11: 22.990, 12: 24.305,
           13: 26.982, 14: 28.085, 15: 30.974, 16: 32.06, 17: 35.45, 18: 39.948, 19: 39.098, 20: 40.078, 22: 47.867, 23: 50.942,
           24: 51.996, 25: 54.938, 26: 55.845, 27: 58.933, 28: 58.693, 29: 63.546, 30: 65.38, 35: 79.904, 36: 83.798, 40: 91.224,
           54: 131.29}


def atomic_number(mass):
    """The element whose standard atomic weight lies within MASS_TOL of `mass` (g/mol), 0 where there is none."""
    z = min(_MASSES, key=lambda k: abs(_MASSES[k] - float(mass)))
    return z if abs(_MASSES[z] - float(mass)) <= MASS_TOL else 0


def parse_spec(text):
    """--density N0,N1,N2[,EVERY] -> dict(grid=(n0, n1, n2), every); ValueError naming --density otherwise."""
    parts = [p.strip() for p in str(text).split(",")]
    if len(parts) not in (3, 4):
        raise ValueError(f"--density takes N0,N1,N2[,EVERY], not {text!r}")
    try:
        v = [int(p) for p in parts]
    except ValueError:
        raise ValueError(f"--density takes N0,N1,N2[,EVERY] (integers), not {text!r}") from None
    every = v[3] if len(v) == 4 else 1
    if every < 1:
        raise ValueError("--density: EVERY must be at least 1")
    try:
        return dict(grid=check_grid(v[:3]), every=every)
    except ValueError as err:
        raise ValueError("--" + str(err)) from None


def parse_types(text):
    """--density-types 3,4 (atom type ids as in the data file, 1-based) -> [t, ...] 0-based; ValueError otherwise."""
    items = [v.strip() for v in str(text).split(",")]
    if not all(v.isdigit() for v in items):
        raise ValueError(f"--density-types takes T,T,... (1-based atom type ids), not {text!r}")
    if any(int(v) < 1 for v in items):
        raise ValueError("--density-types: atom type ids start at 1")
    return check_types([int(v) - 1 for v in items])


def check_grid(grid):
    """The grid as a tuple of three ints; ValueError naming the limit it breaks."""
    grid = tuple(int(v) for v in grid)
    if len(grid) != 3:
        raise ValueError(f"density: the grid takes three voxel counts, not {len(grid)}")
    for k, v in enumerate(grid):
        if v < 1 or v > MAX_AXIS:
            raise ValueError(f"density: grid axis {k} has {v} voxels, outside [1, {MAX_AXIS}]")
    if grid[0] * grid[1] * grid[2] > MAX_VOXELS:
        raise ValueError(f"density: a grid of {grid[0] * grid[1] * grid[2]} voxels exceeds the limit of {MAX_VOXELS}")
    return grid


def check_types(types, n_atom_types=None):
    """The channels as a list of 0-based ints; ValueError for none, more than MAX_CHANNELS, a duplicate or a type out of range."""
    types = [int(t) for t in types]
    if not types:
        raise ValueError("density: no atom type is selected")
    if len(types) > MAX_CHANNELS:
        raise ValueError(f"density: {len(types)} atom types are selected, the limit is {MAX_CHANNELS}: name them with --density-types")
    for t in types:
        if t < 0 or (n_atom_types is not None and t >= n_atom_types):
            raise ValueError(f"density: atom type {t + 1} is outside the data file's types")
        if types.count(t) > 1:
            raise ValueError(f"density: atom type {t + 1} is given twice")
    return types


def check_size(grid, n_channels, n_groups):
    """The bytes the accumulators take; ValueError naming the limit and the size asked for beyond MAX_BYTES."""
    need = (int(n_groups) * int(n_channels) * grid[0] * grid[1] * grid[2] + int(n_groups)) * 8
    if need > MAX_BYTES:
        raise ValueError(f"density: the accumulators would take {need} bytes, the limit is {MAX_BYTES} "
                         f"({n_groups} groups x {n_channels} types x {grid[0]} x {grid[1]} x {grid[2]} voxels)")
    return need


def default_types(topo):
    """The atom types that occur in the ACTIVE residue types, 0-based, ascending."""
    return sorted({int(topo.atom_types[t, a]) - 1 for t in range(topo.n_res) if topo.is_active[t] == 1
                   for a in range(int(topo.atoms_in_res[t]))})


def check_spec(spec, topo):
    """run_replicas' ``density`` dict -> dict(grid, types, every, per_replica), checked; ValueError naming what is wrong."""
    unknown = set(spec) - {"grid", "types", "every", "per_replica"}
    if unknown or "grid" not in spec:
        raise ValueError(f"density: needs grid, and takes types, every and per_replica besides ({sorted(unknown)} unknown)")
    types = spec.get("types")
    out = dict(grid=check_grid(spec["grid"]), types=check_types(default_types(topo) if types is None else types, topo.n_atom_types),
               every=int(spec.get("every", 1)), per_replica=bool(spec.get("per_replica", False)))
    if out["every"] < 1:
        raise ValueError("density: every must be at least 1")
    return out


def from_args(ap, a):
    """--density, --density-types, --density-per-replica of the parsed command line `a` -> run_replicas' ``density`` dict,
    None without --density; ap.error for a sub-option without --density or an argument that does not parse."""
    if a.density is None and (a.density_types is not None or a.density_per_replica):
        ap.error("--density-types and --density-per-replica need --density N0,N1,N2[,EVERY]")
    if a.density is None:
        return None
    try:
        spec = parse_spec(a.density)
        spec["types"] = parse_types(a.density_types) if a.density_types is not None else None
        spec["per_replica"] = bool(a.density_per_replica)
    except ValueError as err:
        ap.error(str(err))
    return spec


def identity_array(spec):
    """What a resumed run's --density must share with the checkpointed one's, as one int64 array"""
    return np.asarray(list(spec["grid"]) + [int(spec["every"]), 1 if spec["per_replica"] else 0] + list(spec["types"]), dtype=np.int64)


def volume(box_matrix):
    return abs(float(np.linalg.det(np.asarray(box_matrix, dtype=np.float64).reshape(3, 3))))


def number_density(hist, samples, box_matrix):
    """rho = hist / (samples V / (n0 n1 n2)) in sites per cubic Angstrom for hist (..., n2, n1, n0) and samples broadcastable
    to hist's leading axes (for hist (G, C, n2, n1, n0): samples (G,)); zero where there are no samples."""
    hist = np.asarray(hist, dtype=np.float64)
    n_vox = hist.shape[-1] * hist.shape[-2] * hist.shape[-3]
    s = np.asarray(samples, dtype=np.float64)
    s = s.reshape(s.shape + (1,) * (hist.ndim - s.ndim))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(s > 0, hist / (s * (volume(box_matrix) / n_vox)), 0.0)


def profiles(hist):
    """The 1-D sums of hist (..., n2, n1, n0) along each cell axis: (along axis 0 (..., n0), axis 1 (..., n1), axis 2 (..., n2)),
    each entry the raw count of a slab, as integers."""
    hist = np.asarray(hist, dtype=np.uint64)
    return hist.sum(axis=(-3, -2)), hist.sum(axis=(-3, -1)), hist.sum(axis=(-2, -1))


# ---- the run's files ------------------------------------------------------------------------------------------------------
HEADER = "#  group  channel  type  axis  voxel         s_mid           x_mid     density(1/A^3)            count\n"


def write_profiles(path, hist, samples, types, box_matrix):
    """<out>/density_profiles.dat: per group, channel and cell axis the slabs' midpoints in fractional units and in Angstrom
    along the cell vector (s_mid |a_k|), the slab's mean number density and its raw count; atom types 1-based."""
    hist = np.asarray(hist, dtype=np.uint64)
    m = np.asarray(box_matrix, dtype=np.float64).reshape(3, 3)
    vol = volume(m)
    prof = profiles(hist)
    with open(path, "w") as f:
        f.write(HEADER)
        for g in range(hist.shape[0]):
            for c, t in enumerate(types):
                for k in range(3):
                    n = prof[k].shape[-1]
                    length = float(np.linalg.norm(m[:, k]))
                    for v in range(n):
                        count = int(prof[k][g, c, v])
                        s_mid = (v + 0.5) / n
                        rho = count / (float(samples[g]) * vol / n) if samples[g] else 0.0
                        f.write(f"{g:8d} {c:8d} {t + 1:5d} {k:5d} {v:6d} {s_mid:13.8f} {s_mid * length:15.8f} {rho:18.10e} {count:16d}\n")


def read_profiles(path):
    """density_profiles.dat back: dict (group, channel, axis) -> dict(type (1-based), s_mid, x_mid, density, count)"""
    out = {}
    with open(path) as f:
        if f.readline() != HEADER:
            raise ValueError(f"{path}: not a density_profiles.dat file")
        for line in f:
            w = line.split()
            d = out.setdefault((int(w[0]), int(w[1]), int(w[3])), dict(type=int(w[2]), s_mid=[], x_mid=[], density=[], count=[]))
            d["s_mid"].append(float(w[5])); d["x_mid"].append(float(w[6])); d["density"].append(float(w[7])); d["count"].append(int(w[8]))
    for d in out.values():
        for k in ("s_mid", "x_mid", "density"):
            d[k] = np.array(d[k])
        d["count"] = np.array(d["count"], dtype=np.uint64)
    return out


def write_counts(path, hist, samples, group_of, replica_group, types, grid, every, per_replica):
    """<out>/density_counts.npz: the raw accumulators per map, the spec, the map every replica added into (group_of) and every
    replica's fugacity group"""
    arrays = dict(hist=np.asarray(hist, dtype=np.uint64), samples=np.asarray(samples, dtype=np.uint64),
                  group_of=np.asarray(group_of, dtype=np.int64), group=np.asarray(replica_group, dtype=np.int64),
                  types=np.asarray(types, dtype=np.int64), grid=np.asarray(grid, dtype=np.int64), every=np.int64(every),
                  per_replica=np.int64(1 if per_replica else 0))
    # an .npz archive as numpy.savez lays it out, but with a fixed member date: the same counts give the same bytes (a
    # resumed run's file is the uninterrupted run's)
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED, allowZip64=True) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def cube_name(group, atom_type):
    """density_gGG_typeTT.cube (atom type 1-based)"""
    return f"density_g{int(group):02d}_type{int(atom_type) + 1:02d}.cube"


def write_cube(path, rho, box_matrix, bounds_lo, atoms=(), title=""):
    """A Gaussian cube file of rho (n2, n1, n0) in sites per cubic Angstrom: origin bounds_lo and the three voxel vectors
    (column k of box%matrix over n_k) in bohr, the values as they are (NOT per cubic bohr: the comment lines say so), the first
    cell axis outermost and the third fastest as the format has it.  atoms: (atomic number, x, y, z in Angstrom)."""
    rho = np.asarray(rho, dtype=np.float64)
    n = (rho.shape[2], rho.shape[1], rho.shape[0])
    m = np.asarray(box_matrix, dtype=np.float64).reshape(3, 3)
    lo = np.asarray(bounds_lo, dtype=np.float64)
    atoms = list(atoms)
    with open(path, "w") as f:
        f.write(f"number density of sites in 1/Angstrom^3 (not per bohr^3) {title}".rstrip() + "\n")
        f.write("lengths in bohr; loop order: cell axis 0 outer, axis 2 inner; maniac_mc_amd.density\n")
        f.write(f"{len(atoms):5d} {lo[0] / BOHR:12.6f} {lo[1] / BOHR:12.6f} {lo[2] / BOHR:12.6f}\n")
        for k in range(3):
            v = m[:, k] / n[k] / BOHR
            f.write(f"{n[k]:5d} {v[0]:12.6f} {v[1]:12.6f} {v[2]:12.6f}\n")
        for z, x, y, zc in atoms:
            f.write(f"{int(z):5d} {float(z):12.6f} {x / BOHR:12.6f} {y / BOHR:12.6f} {zc / BOHR:12.6f}\n")
        vals = np.ascontiguousarray(rho.transpose(2, 1, 0))
        for i0 in range(n[0]):
            for i1 in range(n[1]):
                row = vals[i0, i1]
                for j in range(0, n[2], 6):
                    f.write(" ".join(f"{x:12.5E}" for x in row[j:j + 6]) + "\n")


def read_cube(path):
    """A cube file back: dict(comments, origin (3,) and vectors (3, 3: row k = voxel vector k) in Angstrom, n (3,), atoms
    [(Z, x, y, z in Angstrom)], rho (n2, n1, n0))"""
    with open(path) as f:
        comments = [f.readline().rstrip("\n"), f.readline().rstrip("\n")]
        w = f.readline().split()
        n_atoms, origin = int(w[0]), np.array([float(x) for x in w[1:4]]) * BOHR
        n, vec = [], []
        for _ in range(3):
            w = f.readline().split()
            n.append(int(w[0])); vec.append([float(x) * BOHR for x in w[1:4]])
        atoms = []
        for _ in range(n_atoms):
            w = f.readline().split()
            atoms.append((int(w[0]), float(w[2]) * BOHR, float(w[3]) * BOHR, float(w[4]) * BOHR))
        vals = np.array(f.read().split(), dtype=np.float64)
    if vals.size != n[0] * n[1] * n[2]:
        raise ValueError(f"{path}: {vals.size} values for a grid of {n}")
    return dict(comments=comments, origin=origin, vectors=np.array(vec), n=np.array(n), atoms=atoms,
                rho=vals.reshape(n[0], n[1], n[2]).transpose(2, 1, 0))


class Sampler:
    """run_replicas' ``density`` option as one of its farm analyses ("adding a farm analysis")"""
    name = "density"

    def __init__(self, option, ctx):
        self.ctx = ctx
        self.spec = check_spec(option, ctx.topo)
        self.every = self.spec["every"]

    def check_size(self):
        """Once ctx holds the groups: the map every replica adds into, and the accumulators' size against MAX_BYTES"""
        ctx, per_replica = self.ctx, self.spec["per_replica"]
        self.group_of = np.arange(ctx.R) if per_replica else np.asarray(ctx.group)
        self.n_groups = ctx.R if per_replica else (len(ctx.fugacities) if ctx.fugacities is not None else 1)
        check_size(self.spec["grid"], len(self.spec["types"]), self.n_groups)

    def identity_array(self):
        return identity_array(self.spec)

    def configure(self, farm, root, resumed):
        farm.eng.density_configure(self.spec["grid"], self.spec["types"], self.group_of, self.n_groups)

    def sample(self, farm, block):
        farm.density_sample()

    def state(self, farm):
        return dict(zip(("density_hist", "density_samples"), farm.eng.density_read()))

    def load(self, farm, extra):
        farm.eng.density_load(extra["density_hist"], extra["density_samples"])

    def finish(self, farm, root, inp, dat):
        s, topo, system = self.spec, self.ctx.topo, self.ctx.system
        hist, samples = farm.eng.density_read()
        write_counts(os.path.join(root, "density_counts.npz"), hist, samples, self.group_of, self.ctx.group, s["types"], s["grid"],
                     s["every"], s["per_replica"])
        write_profiles(os.path.join(root, "density_profiles.dat"), hist, samples, s["types"], system.box_matrix)
        rho = number_density(hist, samples, system.box_matrix)
        atoms = [(atomic_number(dat["masses"][int(topo.atom_types[t, a]) - 1]), *xyz)
                 for t in range(topo.n_res) if topo.is_active[t] != 1
                 for mol in system.all_sites(t) for a, xyz in enumerate(mol.tolist())]
        for g in range(hist.shape[0]):
            for c, ty in enumerate(s["types"]):
                write_cube(os.path.join(root, cube_name(g, ty)), rho[g, c], system.box_matrix, system.bounds_lo, atoms,
                           title=f"map {g} atom type {ty + 1} samples {int(samples[g])}")
