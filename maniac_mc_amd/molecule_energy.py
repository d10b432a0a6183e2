"""Per-molecule removal energies of a replica farm (run_replicas(molecule_energy=...), --molecule-energy): the host side of the
engine's integer histograms (mgpu_molecule_energy_*, include/maniac_gpu.h).  Nothing here needs the library or a device.

For every molecule m of a selected ACTIVE residue type the engine forms u = E(X) - E(X without m), the energy the molecule
contributes to its configuration, and counts it into n_bins bins over [e_min, e_max) and one slot below, one above.  This
module restates the bin rule in numpy, pools the counts over the replicas of a fugacity group into the site-energy
distribution p(u) = H / (sum H  w), w the bin width, and writes

  <out>/molecule_energy_counts.npz   hist (R, n_sel, n_bins + 2), samples (R,), the spec and every replica's group;
  <out>/molecule_energy.dat          per fugacity group and type the bins' centre in kcal/mol, the pooled probability density
                                     (per kcal/mol, over the molecules inside the range), its standard error over the group's
                                     replicas and the pooled raw count; the counts below and above the range in the header.
"""
from __future__ import annotations

import math
import os

import numpy as np

from .system import KB_KCALMOL

MAX_BINS = 4096
MAX_TYPES = 8


def parse_spec(text):
    """--molecule-energy EMIN,EMAX,BINS[,EVERY] (kcal/mol) -> dict(e_min, e_max, n_bins, every); ValueError naming the switch."""
    parts = [p.strip() for p in str(text).split(",")]
    if len(parts) not in (3, 4):
        raise ValueError(f"--molecule-energy takes EMIN,EMAX,BINS[,EVERY], not {text!r}")
    try:
        e_min, e_max = float(parts[0]), float(parts[1])
        n_bins = int(parts[2])
        every = int(parts[3]) if len(parts) == 4 else 1
    except ValueError:
        raise ValueError(f"--molecule-energy takes EMIN,EMAX,BINS[,EVERY] (two numbers and integers), not {text!r}") from None
    if not (math.isfinite(e_min) and math.isfinite(e_max)):
        raise ValueError("--molecule-energy: EMIN and EMAX must be finite")
    if not e_min < e_max:
        raise ValueError("--molecule-energy: EMIN must be below EMAX")
    if n_bins < 1 or n_bins > MAX_BINS:
        raise ValueError(f"--molecule-energy: BINS must lie in [1, {MAX_BINS}]")
    if every < 1:
        raise ValueError("--molecule-energy: EVERY must be at least 1")
    return dict(e_min=e_min, e_max=e_max, n_bins=n_bins, every=every)


def parse_types(text, names):
    """--molecule-energy-types NAME,NAME with the input's residue names -> 0-based residue types in the order given;
    ValueError naming the switch for an unknown name, a duplicate or an empty list."""
    names = [str(n) for n in names]
    items = [x.strip() for x in str(text).split(",") if x.strip()]
    if not items:
        raise ValueError("--molecule-energy-types: expected NAME,NAME,..., got an empty list")
    out = []
    for n in items:
        if n not in names:
            raise ValueError(f"--molecule-energy-types: unknown residue name {n!r} (the input has {', '.join(names)})")
        if names.index(n) in out:
            raise ValueError(f"--molecule-energy-types: {n!r} is given twice")
        out.append(names.index(n))
    return out


def default_types(topo):
    """Every ACTIVE residue type, ascending"""
    return [t for t in range(topo.n_res) if int(topo.is_active[t]) == 1]


def check_spec(spec, topo):
    """run_replicas' ``molecule_energy`` dict -> dict(e_min, e_max (kcal/mol), n_bins, types, every), checked; ValueError
    naming what is wrong."""
    unknown = set(spec) - {"e_min", "e_max", "n_bins", "types", "every"}
    if unknown:
        raise ValueError(f"molecule_energy: takes e_min, e_max, n_bins, types and every ({sorted(unknown)} unknown)")
    for key in ("e_min", "e_max", "n_bins"):
        if key not in spec:
            raise ValueError(f"molecule_energy: needs e_min, e_max and n_bins ({key} is missing)")
    out = dict(e_min=float(spec["e_min"]), e_max=float(spec["e_max"]), n_bins=int(spec["n_bins"]), every=int(spec.get("every", 1)))
    if not (math.isfinite(out["e_min"]) and math.isfinite(out["e_max"])):
        raise ValueError("molecule_energy: e_min and e_max must be finite")
    if not out["e_min"] < out["e_max"]:
        raise ValueError("molecule_energy: e_min must be below e_max")
    if not 1 <= out["n_bins"] <= MAX_BINS:
        raise ValueError(f"molecule_energy: n_bins must lie in [1, {MAX_BINS}]")
    if out["every"] < 1:
        raise ValueError("molecule_energy: every must be at least 1")
    types = spec.get("types")
    types = default_types(topo) if types is None else [int(t) for t in types]
    if not types:
        raise ValueError("molecule_energy: the selection is empty (no active residue type)")
    seen = []
    for t in types:
        if not 0 <= t < topo.n_res:
            raise ValueError(f"molecule_energy: residue type {t} is outside the residue types [0, {topo.n_res - 1}]")
        if int(topo.is_active[t]) != 1:
            raise ValueError(f"molecule_energy: residue type {t} is not an active type")
        if t in seen:
            raise ValueError(f"molecule_energy: residue type {t} is given twice")
        seen.append(t)
    out["types"] = seen
    return out


def from_args(ap, a):
    """--molecule-energy, --molecule-energy-types of the parsed command line `a` -> run_replicas' ``molecule_energy`` dict, None
    without --molecule-energy; ap.error for the sub-option without it or an argument that does not parse.  The names of
    --molecule-energy-types are the input file's (a missing input file is reported by the caller)."""
    if a.molecule_energy is None and a.molecule_energy_types is not None:
        ap.error("--molecule-energy-types needs --molecule-energy EMIN,EMAX,BINS[,EVERY]")
    if a.molecule_energy is None:
        return None
    try:
        spec = parse_spec(a.molecule_energy)
        spec["types"] = None
        if a.molecule_energy_types is not None and os.path.isfile(a.maniac):
            from . import io_maniac
            names = [r.name for r in io_maniac.read_maniac_input(a.maniac).residues]
            spec["types"] = parse_types(a.molecule_energy_types, names)
    except ValueError as err:
        ap.error(str(err))
    return spec


def identity_array(spec):
    """What a resumed run's --molecule-energy must share with the checkpointed one's, as one float64 array"""
    return np.asarray([float(spec["e_min"]), float(spec["e_max"]), float(spec["n_bins"]), float(spec["every"])]
                      + [float(t) for t in spec["types"]], dtype=np.float64)


def kelvin_limits(spec):
    """(e_min, e_max) in K, the engine's unit: the option's kcal/mol divided by KB_KCALMOL, once"""
    return float(spec["e_min"]) / KB_KCALMOL, float(spec["e_max"]) / KB_KCALMOL


# ---- the bin rule -------------------------------------------------------------------------------------------------------------
def total_energy(components):
    """total = ((((nc + c) + r) + s) + i) of (..., 5) components: the engine's chain of rounded adds"""
    c = np.asarray(components, dtype=np.float64)
    return (((c[..., 0] + c[..., 1]) + c[..., 2]) + c[..., 3]) + c[..., 4]


def slot_index(u, e_min, e_max, n_bins):
    """The contract's slot of every total u (array), in the unit of e_min and e_max: 0 below e_min, 1 + min(n_bins - 1,
    floor((u - e_min) * inv_w)) below e_max, n_bins + 1 otherwise -- a total that is not a number included.  inv_w =
    n_bins / (e_max - e_min); the difference and the product are separate rounded operations, as on the device."""
    u = np.asarray(u, dtype=np.float64)
    e_min, e_max = np.float64(e_min), np.float64(e_max)
    inv_w = np.float64(n_bins) / (e_max - e_min)
    with np.errstate(invalid="ignore", over="ignore"):
        d = u - e_min
        x = d * inv_w
        inside = 1 + np.minimum(n_bins - 1, np.floor(np.where(u < e_max, x, 0.0)).astype(np.int64))
    return np.where(u < e_min, 0, np.where(u < e_max, inside, n_bins + 1)).astype(np.int64)


def histogram(u, e_min, e_max, n_bins):
    """The n_bins + 2 slot counts of the totals u (any shape), uint64"""
    return np.bincount(slot_index(u, e_min, e_max, n_bins).reshape(-1), minlength=n_bins + 2).astype(np.uint64)


def bin_centres(e_min, e_max, n_bins):
    w = (float(e_max) - float(e_min)) / n_bins
    return float(e_min) + (np.arange(n_bins, dtype=np.float64) + 0.5) * w


def density_of(hist, e_min, e_max):
    """p (..., n_bins) = inside counts / (their sum x bin width) of hist (..., n_bins + 2); zero where nothing lies inside"""
    h = np.asarray(hist, dtype=np.float64)[..., 1:-1]
    w = (float(e_max) - float(e_min)) / h.shape[-1]
    tot = h.sum(axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(tot > 0, h / (tot * w), 0.0)


# ---- the run's files ----------------------------------------------------------------------------------------------------------
MAGIC = "# molecule_energy.dat: per fugacity group and residue type the distribution of E(X) - E(X without m), kcal/mol\n"
COLUMNS = "#  group  sel  type           e_mid         density     density_sem            count\n"


def pooled(hist, group, e_min, e_max):
    """Per fugacity group g and selected type s: (g, s, density pooled over the group's replicas, its standard error over the
    replicas, the pooled raw counts (n_bins + 2)).  hist (R, n_sel, n_bins + 2): sums over each replica's samples."""
    hist = np.asarray(hist, dtype=np.uint64)
    group = np.asarray(group)
    out = []
    for g in sorted({int(v) for v in group}):
        sel = group == g
        h = hist[sel]
        n = int(sel.sum())
        total = h.sum(axis=0)
        p_pool = density_of(total, e_min, e_max)
        p_each = density_of(h, e_min, e_max)
        sem = np.std(p_each, axis=0, ddof=1) / math.sqrt(n) if n > 1 else np.zeros_like(p_pool)
        for s in range(hist.shape[1]):
            out.append((g, s, p_pool[s], sem[s], total[s]))
    return out


def write_dat(path, hist, group, types, names, e_min, e_max):
    """<out>/molecule_energy.dat; e_min, e_max in kcal/mol; residue types 1-based with their names"""
    n_bins = np.asarray(hist).shape[-1] - 2
    mid = bin_centres(e_min, e_max, n_bins)
    with open(path, "w") as f:
        f.write(MAGIC)
        for g, s, p, sem, count in pooled(hist, group, e_min, e_max):
            f.write(f"# group {g} sel {s} type {types[s] + 1} {names[types[s]]}: below {int(count[0])} above {int(count[-1])}\n")
            f.write(COLUMNS)
            for k in range(n_bins):
                f.write(f"{g:8d} {s:4d} {types[s] + 1:5d} {mid[k]:15.8f} {p[k]:15.8e} {sem[k]:15.8e} {int(count[1 + k]):16d}\n")


def read_dat(path):
    """molecule_energy.dat back: dict (group, sel) -> dict(type (1-based), name, below, above, e_mid, density, sem, count)"""
    out = {}
    with open(path) as f:
        if f.readline() != MAGIC:
            raise ValueError(f"{path}: not a molecule_energy.dat file")
        for line in f:
            w = line.split()
            if line.startswith("# group"):
                key = (int(w[2]), int(w[4]))
                out[key] = dict(type=int(w[6]), name=w[7].rstrip(":"), below=int(w[9]), above=int(w[11]), e_mid=[], density=[],
                                sem=[], count=[])
            elif not line.startswith("#"):
                d = out[(int(w[0]), int(w[1]))]
                d["e_mid"].append(float(w[3])); d["density"].append(float(w[4])); d["sem"].append(float(w[5]))
                d["count"].append(int(w[6]))
    for d in out.values():
        for k in ("e_mid", "density", "sem"):
            d[k] = np.array(d[k])
        d["count"] = np.array(d["count"], dtype=np.uint64)
    return out


def write_counts(path, hist, samples, group, spec):
    """<out>/molecule_energy_counts.npz: the raw accumulators per replica, the spec (limits in kcal/mol) and every replica's
    group.  An .npz archive as numpy.savez lays it out, but with a fixed member date: the same counts give the same bytes."""
    arrays = dict(hist=np.asarray(hist, dtype=np.uint64), samples=np.asarray(samples, dtype=np.uint64),
                  group=np.asarray(group, dtype=np.int64), types=np.asarray(spec["types"], dtype=np.int64),
                  e_min=np.float64(spec["e_min"]), e_max=np.float64(spec["e_max"]), n_bins=np.int64(spec["n_bins"]),
                  every=np.int64(spec["every"]))
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED, allowZip64=True) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def read_counts(path):
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


class Sampler:
    """run_replicas' ``molecule_energy`` option as one of its farm analyses ("adding a farm analysis")"""
    name = "molecule_energy"

    def __init__(self, option, ctx):
        self.ctx = ctx
        self.spec = check_spec(option, ctx.topo)
        self.every = self.spec["every"]

    def check_size(self):
        """(nothing of it depends on the groups)"""

    def identity_array(self):
        return identity_array(self.spec)

    def configure(self, farm, root, resumed):
        lo, hi = kelvin_limits(self.spec)
        farm.eng.molecule_energy_configure(self.spec["n_bins"], lo, hi, self.spec["types"])

    def sample(self, farm, block):
        farm.molecule_energy_sample()

    def state(self, farm):
        return dict(zip(("molecule_energy_hist", "molecule_energy_samples"), farm.eng.molecule_energy_read()))

    def load(self, farm, extra):
        farm.eng.molecule_energy_load(extra["molecule_energy_hist"], extra["molecule_energy_samples"])

    def finish(self, farm, root, inp, dat):
        s = self.spec
        hist, samples = farm.eng.molecule_energy_read()
        write_counts(os.path.join(root, "molecule_energy_counts.npz"), hist, samples, self.ctx.group, s)
        write_dat(os.path.join(root, "molecule_energy.dat"), hist, self.ctx.group, s["types"], self.ctx.residue_names,
                  s["e_min"], s["e_max"])
