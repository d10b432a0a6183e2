"""Radial distribution functions of a replica farm: the host side of the engine's integer histograms (mgpu_rdf_*,
include/maniac_gpu.h).  Nothing here needs the library or a device.

The engine counts; this module normalises:  g_p(r_b) = V sum H_p(b) / (sum E_p V_shell(b)),  V_shell(b) = 4 pi / 3
(r_{b+1}^3 - r_b^3), both sums over the samples and replicas pooled, E the count of ELIGIBLE pairs (every pair of atoms of the
selected types, whatever its distance).  With E in the denominator an ideal gas gives 1 at every N, which is the normalisation
a grand-canonical run with fluctuating N needs.
"""
from __future__ import annotations

import math
import os

import numpy as np

MAX_PAIRS = 8
MAX_BINS = 1024
ERROR_TOL = 1.0e-10


def parse_spec(text):
    """--rdf R_MAX,N_BINS[,EVERY] -> dict(r_max, n_bins, every); ValueError naming --rdf otherwise."""
    parts = [p.strip() for p in str(text).split(",")]
    if len(parts) not in (2, 3):
        raise ValueError(f"--rdf takes R_MAX,N_BINS[,EVERY], not {text!r}")
    try:
        r_max = float(parts[0])
        n_bins = int(parts[1])
        every = int(parts[2]) if len(parts) == 3 else 1
    except ValueError:
        raise ValueError(f"--rdf takes R_MAX,N_BINS[,EVERY] (a number and integers), not {text!r}") from None
    if not (r_max > 0.0) or not math.isfinite(r_max):
        raise ValueError("--rdf: R_MAX must be greater than 0")
    if n_bins < 1 or n_bins > MAX_BINS:
        raise ValueError(f"--rdf: N_BINS must lie in [1, {MAX_BINS}]")
    if every < 1:
        raise ValueError("--rdf: EVERY must be at least 1")
    return dict(r_max=r_max, n_bins=n_bins, every=every)


def parse_pairs(text):
    """--rdf-pairs 1-1,1-2 (atom type ids as in the data file, 1-based) -> [(a, b), ...] 0-based; ValueError otherwise."""
    pairs = []
    for item in str(text).split(","):
        ab = item.strip().split("-")
        if len(ab) != 2 or not all(v.strip().isdigit() for v in ab):
            raise ValueError(f"--rdf-pairs takes A-B,A-B,... (1-based atom type ids), not {text!r}")
        a, b = int(ab[0]), int(ab[1])
        if a < 1 or b < 1:
            raise ValueError("--rdf-pairs: atom type ids start at 1")
        pairs.append((a - 1, b - 1))
    return check_pairs(pairs)


def check_pairs(pairs, n_atom_types=None):
    """The pairs as a list of int tuples; ValueError for none, more than MAX_PAIRS, a duplicate or a type out of range."""
    pairs = [(int(a), int(b)) for a, b in pairs]
    if not pairs:
        raise ValueError("rdf: no atom-type pair is selected")
    if len(pairs) > MAX_PAIRS:
        raise ValueError(f"rdf: {len(pairs)} atom-type pairs are selected, the limit is {MAX_PAIRS}: name them with --rdf-pairs")
    seen = set()
    for a, b in pairs:
        if a < 0 or b < 0 or (n_atom_types is not None and max(a, b) >= n_atom_types):
            raise ValueError(f"rdf: atom type pair ({a + 1}, {b + 1}) is outside the data file's types")
        key = (min(a, b), max(a, b))
        if key in seen:
            raise ValueError(f"rdf: atom type pair {a + 1}-{b + 1} is given twice")
        seen.add(key)
    return pairs


def default_pairs(topo):
    """Every unordered pair of the atom types that occur in the ACTIVE residue types, 0-based, ascending."""
    types = sorted({int(topo.atom_types[t, a]) - 1 for t in range(topo.n_res) if topo.is_active[t] == 1
                    for a in range(int(topo.atoms_in_res[t]))})
    return [(a, b) for i, a in enumerate(types) for b in types[i:]]


def check_spec(spec, topo, box_matrix):
    """run_replicas' ``rdf`` dict -> dict(r_max, n_bins, pairs, every, include_intra), checked; ValueError naming what is wrong."""
    unknown = set(spec) - {"r_max", "n_bins", "pairs", "every", "include_intra"}
    if unknown or "r_max" not in spec or "n_bins" not in spec:
        raise ValueError(f"rdf: needs r_max and n_bins, and takes pairs, every and include_intra besides ({sorted(unknown)} unknown)")
    pairs = spec.get("pairs")
    pairs = check_pairs(default_pairs(topo) if pairs is None else pairs, topo.n_atom_types)
    out = dict(r_max=float(spec["r_max"]), n_bins=int(spec["n_bins"]), pairs=pairs, every=int(spec.get("every", 1)),
               include_intra=bool(spec.get("include_intra", False)))
    if not out["r_max"] > 0.0:
        raise ValueError("rdf: r_max must be greater than 0")
    if not 1 <= out["n_bins"] <= MAX_BINS:
        raise ValueError(f"rdf: n_bins must lie in [1, {MAX_BINS}]")
    if out["every"] < 1:
        raise ValueError("rdf: every must be at least 1")
    limit = half_width(box_matrix)
    if out["r_max"] > limit:
        raise ValueError(f"rdf: r_max {out['r_max']!r} exceeds half the smallest perpendicular width of the cell, {limit!r}")
    return out


def from_args(ap, a):
    """--rdf, --rdf-pairs, --rdf-intra of the parsed command line `a` -> run_replicas' ``rdf`` dict, None without --rdf;
    ap.error for a sub-option without --rdf or an argument that does not parse."""
    if a.rdf is None and (a.rdf_pairs is not None or a.rdf_intra):
        ap.error("--rdf-pairs and --rdf-intra need --rdf R_MAX,N_BINS[,EVERY]")
    if a.rdf is None:
        return None
    try:
        spec = parse_spec(a.rdf)
        spec["pairs"] = parse_pairs(a.rdf_pairs) if a.rdf_pairs is not None else None
        spec["include_intra"] = bool(a.rdf_intra)
    except ValueError as err:
        ap.error(str(err))
    return spec


def half_width(box_matrix):
    """Half the smallest perpendicular width of the cell: the largest r_max a histogram may have.  Orthorhombic: min L / 2;
    triclinic: width i = V / |a_j x a_k|, the cell vectors being the COLUMNS of box%matrix.  Plain rounded operations in the
    engine's order: the same double as mgpu_rdf_configure compares with."""
    m = [[float(v) for v in row] for row in np.asarray(box_matrix, dtype=np.float64).reshape(3, 3)]
    off = max(abs(m[0][1]), abs(m[0][2]), abs(m[1][0]), abs(m[1][2]), abs(m[2][0]), abs(m[2][1]))
    if not off > ERROR_TOL:
        return 0.5 * min(m[0][0], min(m[1][1], m[2][2]))
    v = [[m[0][k], m[1][k], m[2][k]] for k in range(3)]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

    bc = cross(v[1], v[2])
    vol = abs(v[0][0] * bc[0] + v[0][1] * bc[1] + v[0][2] * bc[2])
    least = 0.0
    for i in range(3):
        c = cross(v[(i + 1) % 3], v[(i + 2) % 3])
        w = vol / math.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
        if i == 0 or w < least:
            least = w
    return 0.5 * least


def volume(box_matrix):
    m = np.asarray(box_matrix, dtype=np.float64).reshape(3, 3)
    return abs(float(np.linalg.det(m)))


def bin_index(r2, r_max, n_bins):
    """The contract's binning of squared distances r2 (array): the bin of every entry, -1 where it is not counted (r2 not
    below r_max * r_max, or a bin index n_bins from rounding at the top edge)."""
    r2 = np.asarray(r2, dtype=np.float64)
    inv_dr = float(n_bins) / float(r_max)
    b = (np.sqrt(r2) * inv_dr).astype(np.int64)
    return np.where((r2 < float(r_max) * float(r_max)) & (b < n_bins), b, -1)


def shell_volumes(r_max, n_bins):
    edges = np.arange(n_bins + 1, dtype=np.float64) * (float(r_max) / n_bins)
    return 4.0 * math.pi / 3.0 * (edges[1:] ** 3 - edges[:-1] ** 3)


def normalise(hist, eligible, volume, r_max):
    """(r_mid (n_bins,), g): g = V hist / (eligible V_shell) for hist (..., n_bins) and eligible (...) pooled by the caller
    (summed over the samples and replicas wanted); zero where there are no eligible pairs."""
    hist = np.asarray(hist, dtype=np.float64)
    elig = np.asarray(eligible, dtype=np.float64)
    n_bins = hist.shape[-1]
    dr = float(r_max) / n_bins
    r_mid = (np.arange(n_bins, dtype=np.float64) + 0.5) * dr
    shell = shell_volumes(r_max, n_bins)
    e = elig[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(e > 0, float(volume) * hist / (e * shell), 0.0)
    return r_mid, g


def eligible_pairs(topo, n_mol, pairs, include_intra):
    """The number of eligible atom pairs of one configuration per selected pair, in closed form from the molecule counts
    n_mol (n_res,) and the site templates: with c[x] atoms of type x in all,  c[a] c[b]  (a != b)  or  c[a] (c[a] - 1) / 2
    (a == b) pairs, less -- without include_intra -- those inside one molecule."""
    n_types = topo.n_atom_types
    per_mol = np.zeros((topo.n_res, n_types), dtype=np.int64)      # atoms of every type in one molecule of residue type t
    for t in range(topo.n_res):
        for a in range(int(topo.atoms_in_res[t])):
            per_mol[t, int(topo.atom_types[t, a]) - 1] += 1
    n_mol = np.asarray(n_mol, dtype=np.int64).reshape(topo.n_res)
    total = (per_mol * n_mol[:, None]).sum(axis=0)
    out = np.zeros(len(pairs), dtype=np.uint64)
    for p, (a, b) in enumerate(pairs):
        if a == b:
            n = int(total[a]) * (int(total[a]) - 1) // 2
            intra = int(sum(int(n_mol[t]) * (int(per_mol[t, a]) * (int(per_mol[t, a]) - 1) // 2) for t in range(topo.n_res)))
        else:
            n = int(total[a]) * int(total[b])
            intra = int(sum(int(n_mol[t]) * int(per_mol[t, a]) * int(per_mol[t, b]) for t in range(topo.n_res)))
        out[p] = n if include_intra else n - intra
    return out


# ---- the run's files ------------------------------------------------------------------------------------------------------
HEADER = "#  group  pair  type_a  type_b           r_mid            g(r)         g_sem            count\n"


def pooled(hist, eligible, group, volume, r_max):
    """Per fugacity group g and pair p: (g index, p, g(r) pooled over the group's replicas, its standard error over the
    replicas, the pooled raw counts).  hist (R, n_pairs, n_bins), eligible (R, n_pairs): sums over each replica's samples."""
    hist = np.asarray(hist, dtype=np.uint64)
    eligible = np.asarray(eligible, dtype=np.uint64)
    group = np.asarray(group)
    out = []
    for g in sorted({int(v) for v in group}):
        sel = group == g
        h, e = hist[sel], eligible[sel]
        r_mid, g_pool = normalise(h.sum(axis=0), e.sum(axis=0), volume, r_max)
        _, g_each = normalise(h, e, volume, r_max)
        n = int(sel.sum())
        sem = np.std(g_each, axis=0, ddof=1) / math.sqrt(n) if n > 1 else np.zeros_like(g_pool)
        for p in range(hist.shape[1]):
            out.append((g, p, r_mid, g_pool[p], sem[p], h[:, p, :].sum(axis=0)))
    return out


def write_dat(path, hist, eligible, group, pairs, volume, r_max):
    """<out>/rdf.dat: per fugacity group and pair the bins' r_mid, pooled g(r), its standard error over the replicas and the
    pooled raw count; atom types 1-based as in the data file."""
    with open(path, "w") as f:
        f.write(HEADER)
        for g, p, r_mid, gr, sem, count in pooled(hist, eligible, group, volume, r_max):
            a, b = pairs[p]
            for k in range(r_mid.shape[0]):
                f.write(f"{g:8d} {p:5d} {a + 1:7d} {b + 1:7d} {r_mid[k]:15.8f} {gr[k]:15.8e} {sem[k]:13.6e} {int(count[k]):16d}\n")


def read_dat(path):
    """rdf.dat back: dict (group, pair) -> dict(types=(a, b) 1-based, r_mid, g, sem, count) in file order."""
    out = {}
    with open(path) as f:
        first = f.readline()
        if first != HEADER:
            raise ValueError(f"{path}: not an rdf.dat file")
        for line in f:
            w = line.split()
            key = (int(w[0]), int(w[1]))
            d = out.setdefault(key, dict(types=(int(w[2]), int(w[3])), r_mid=[], g=[], sem=[], count=[]))
            d["r_mid"].append(float(w[4])); d["g"].append(float(w[5])); d["sem"].append(float(w[6])); d["count"].append(int(w[7]))
    for d in out.values():
        for k in ("r_mid", "g", "sem"):
            d[k] = np.array(d[k])
        d["count"] = np.array(d["count"], dtype=np.uint64)
    return out


def write_counts(path, hist, eligible, samples, group, pairs, r_max, n_bins, every, include_intra):
    """<out>/rdf_counts.npz: the raw accumulators per replica, the spec and every replica's group"""
    arrays = dict(hist=np.asarray(hist, dtype=np.uint64), eligible=np.asarray(eligible, dtype=np.uint64),
                  samples=np.asarray(samples, dtype=np.uint64), group=np.asarray(group, dtype=np.int64),
                  pairs=np.asarray(pairs, dtype=np.int64).reshape(-1, 2), r_max=np.float64(r_max), n_bins=np.int64(n_bins),
                  every=np.int64(every), include_intra=np.int64(1 if include_intra else 0))
    # an .npz archive as numpy.savez lays it out, but with a fixed member date: the same counts give the same bytes (a
    # resumed run's file is the uninterrupted run's)
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_STORED, allowZip64=True) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(a), allow_pickle=False)


def identity_array(spec):
    """What a resumed run's --rdf must share with the checkpointed one's, as one float64 array"""
    flat = [float(spec["r_max"]), float(spec["n_bins"]), float(spec["every"]), float(1 if spec["include_intra"] else 0)]
    for a, b in spec["pairs"]:
        flat += [float(a), float(b)]
    return np.asarray(flat, dtype=np.float64)


class Sampler:
    """run_replicas' ``rdf`` option as one of its farm analyses ("adding a farm analysis")"""
    name = "rdf"

    def __init__(self, option, ctx):
        self.ctx = ctx
        self.spec = check_spec(option, ctx.topo, ctx.system.box_matrix)
        self.every = self.spec["every"]

    def check_size(self):
        """(nothing of it depends on the groups)"""

    def identity_array(self):
        return identity_array(self.spec)

    def configure(self, farm, root, resumed):
        farm.eng.rdf_configure(self.spec["n_bins"], self.spec["r_max"], self.spec["pairs"], self.spec["include_intra"])

    def sample(self, farm, block):
        farm.rdf_sample()

    def state(self, farm):
        return dict(zip(("rdf_hist", "rdf_eligible", "rdf_samples"), farm.eng.rdf_read()))

    def load(self, farm, extra):
        farm.eng.rdf_load(extra["rdf_hist"], extra["rdf_eligible"], extra["rdf_samples"])

    def finish(self, farm, root, inp, dat):
        s, box = self.spec, self.ctx.system.box_matrix
        hist, eligible, samples = farm.eng.rdf_read()
        write_counts(os.path.join(root, "rdf_counts.npz"), hist, eligible, samples, self.ctx.group, s["pairs"], s["r_max"],
                     s["n_bins"], s["every"], s["include_intra"])
        write_dat(os.path.join(root, "rdf.dat"), hist, eligible, self.ctx.group, s["pairs"], volume(box), s["r_max"])
