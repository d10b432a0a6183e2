"""Build / load the Fortran host side (maniac_mc_amd/fortran/*.f90 -> libmaniac_host.so) and drive it.

The Metropolis loop of the replica farm is Fortran (mc_farm.f90), as the north star asks: it calls
the HIP engine through the ISO_C_BINDING module maniac_gpu.f90 -> include/maniac_gpu.h.  Python only
creates the engine, hands over the initial configuration and asks for n steps.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import _lib
from .engine import Engine
from .system import System

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmaniac_host.so")
FSRC = [os.path.join(_HERE, "fortran", f) for f in ("maniac_gpu.f90", "maniac_output.f90", "mc_farm.f90", "mc_chain.f90")]

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def build(force: bool = False, verbose: bool = False) -> str:
    _lib.build()
    if not force and os.path.exists(LIB_PATH):
        if os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(f) for f in FSRC + [_lib.LIB_PATH]):
            return LIB_PATH
    moddir = os.path.join(_HERE, "..", "build", "fmod")
    os.makedirs(moddir, exist_ok=True)
    cmd = ["amdflang", "-O2", "-fopenmp", "-fPIC", "-shared", "-module-dir", moddir, "-o", LIB_PATH] + FSRC + \
          ["-L" + _HERE, "-lmaniac_hip", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib/llvm/lib"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


_host = None


def lib():
    global _host
    if _host is None:
        # the farm drives each lane from its own host thread with a nested OpenMP team: allow two active levels and
        # keep the inner teams alive between regions (must be in the environment before the OpenMP runtime starts)
        os.environ.setdefault("OMP_MAX_ACTIVE_LEVELS", "2")
        os.environ.setdefault("KMP_HOT_TEAMS_MAX_LEVEL", "2")
        os.environ.setdefault("KMP_HOT_TEAMS_MODE", "1")
        _lib.lib()       # libmaniac_hip.so first, so the dependency resolves in-tree
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run __graft_entry__.build() (needs amdflang)")
        L = C.CDLL(LIB_PATH)
        L.mfarm_create.restype = C.c_int
        L.mfarm_run.restype = C.c_int
        L.mfarm_set_gcmc.restype = C.c_int
        L.mfarm_set_replica.restype = C.c_int
        L.mfarm_set_reservoir.restype = C.c_int
        L.mfarm_get_reservoir.restype = C.c_int
        L.mfarm_write_block.restype = C.c_int
        L.mfarm_state_bytes.restype = C.c_longlong
        L.mfarm_state_export.restype = C.c_int
        L.mfarm_state_import.restype = C.c_int
        _host = L
    return _host


def set_chain_run(k: int = 0, depth: int = 3):
    """mchain_set_chain_run: the single-chain driver (mc_chain.f90) runs NVT blocks as chain runs of k steps per launch with
    `depth` launches in flight, where the engine takes them (Engine.chain_run_capacity: a triclinic box only after
    Engine.chain_run_set_triclinic); k = 0 switches the mode off."""
    lib().mchain_set_chain_run(C.c_int(int(k)), C.c_int(int(depth)))


def set_chain_run_gcmc(on: bool = False):
    """mchain_set_chain_run_gcmc: with set_chain_run on, blocks WITH insertions / deletions run as chain runs of by-count
    records too, where the engine takes the switch (Engine.chain_run_set_gc) and the run is not as-written."""
    lib().mchain_set_chain_run_gcmc(C.c_int(1 if on else 0))


def chain_run_gcmc_mode():
    """(gcmc, fallback_steps) of the last mchain_run: its blocks were grand-canonical chain runs; steps they took through the
    windows because a molecule count stood at an edge."""
    out = np.zeros(2, dtype=np.int32)
    lib().mchain_get_chain_run_gcmc(out.ctypes.data_as(_ip))
    return bool(out[0]), int(out[1])


def chain_run_mode():
    """(on, k, depth) of the last mchain_run: on = the run's blocks were chain runs, k and depth as the engine's capacity cut them."""
    out = np.zeros(3, dtype=np.int32)
    lib().mchain_get_chain_run(out.ctypes.data_as(_ip))
    return bool(out[0]), int(out[1]), int(out[2])


class FortranFarm:
    """R chains of `system` on one GPU, advanced by the Fortran driver (mc_farm.f90).

    NVT by default (translation / rotation).  ``gcmc=dict(p_translation=..., p_rotation=..., fugacity=...)``
    switches insertion / deletion on: ``fugacity`` in molecules per cubic Angstrom, scalar, per active
    type, or (n_active, R) for an isotherm sweep; ``mol_capacity`` bounds the molecule count per type.
    ``reservoir={t: off (n, n1, 3)}`` gives every chain a reservoir of residue type t (MANIAC's ``-r reservoir.data``;
    ``io_maniac.reservoir_offsets`` reads one): insertions of t copy a reservoir molecule unrotated and take it out of the
    reservoir, deletions put the box's last molecule of t into it, and an insertion from an empty reservoir is skipped.
    ``wide_triclinic=True`` (with ``triclinic_moves``): window mode also applies to a triclinic box with rigid molecules of 6
    to 63 sites (``Engine.farm_set_wide_triclinic``); off by default, and such a farm then keeps the batched path.
    ``initial=[R Systems]``: every chain starts from its own configuration (the topology and box of ``system``, counts within
    ``mol_capacity``; anything else raises ValueError before a farm slot is taken): one batched S(k) initialisation and one
    batched whole-system energy over all replicas, then ``mfarm_set_replica`` per chain.  Default: R copies of ``system``.
    """

    _live = None          # the farm created last that is still open (tests close leftovers through it)
    _slots = {}           # farm slot of the Fortran module (mfarm_select) -> the open farm that holds it
    MAX_FARMS = 8

    def __init__(self, system: System, n_replicas: int, device: int = 0, seed: int = 1,
                 translation_step: float = 0.3, rotation_step: float = 0.3, p_translation: float = 0.5,
                 rng_kind: int = 1, n_threads: int = 8, mol_capacity=None, gcmc=None,
                 n_lanes: int = 2, n_drivers: int = 1, device_build: bool = False, device_accept: bool = False,
                 window: bool = False, window_depth: int = 2, reservoir=None, triclinic_moves: bool = False,
                 wide_triclinic: bool = False, initial=None):
        self.H = lib()
        # mc_farm.f90 keeps up to MAX_FARMS farms; every call below selects this farm's slot first
        free = [k for k in range(FortranFarm.MAX_FARMS) if k not in FortranFarm._slots]
        if not free:
            raise RuntimeError(f"{FortranFarm.MAX_FARMS} FortranFarms are already open in this process: close() one first")
        self.slot = -1
        self.sys = system
        self.R = int(n_replicas)
        topo = system.topo
        if mol_capacity is None:
            mol_capacity = [max(1, int(n)) for n in system.n_mol]
        self.mol_capacity = [int(c) for c in mol_capacity]
        if initial is not None:
            initial = list(initial)
            self._check_initial(system, initial)
        self.eng = Engine(topo, system.box_matrix, system.bounds_lo, system.real_space_cutoff,
                          system.ewald_tolerance, self.R, device, self.mol_capacity,
                          triclinic_moves=bool(triclinic_moves) and system.is_triclinic())
        # wide_triclinic (with triclinic_moves): farm windows take rigid molecules of 6 to 63 sites in this triclinic box
        # (Engine.farm_set_wide_triclinic) -- set before mc_farm.f90 asks for the windows' capacity
        self.wide_triclinic = bool(wide_triclinic) and bool(triclinic_moves) and system.is_triclinic()
        if self.wide_triclinic:
            self.eng.farm_set_wide_triclinic(True)
        if initial is None:
            self.eng.load_system(system, 0)
        # device_build: the engine keeps the molecules' frames (com, offsets) and builds the trial moves itself; the
        # Fortran driver then holds no mirror of the coordinates (orthorhombic boxes; triclinic ones with triclinic_moves,
        # Engine.set_triclinic_moves -- without it a triclinic system's moves are built on the host, as they always were)
        self.triclinic_moves = bool(triclinic_moves) and system.is_triclinic()
        self.device_build = bool(device_build) and (not system.is_triclinic() or self.triclinic_moves)
        if initial is not None:
            # every replica its own configuration: one S(k) and one whole-system energy pass over all of them; the driver
            # is created with replica 0's state and told every replica's own below (mfarm_set_replica)
            for r, s_r in enumerate(initial):
                self.eng.load_system(s_r, r)
                if self.device_build:
                    for tt in range(topo.n_res):
                        if topo.is_active[tt]:
                            self.eng.set_frames(r, tt, s_r.com[tt], s_r.offsets[tt])
            self.eng.init_structure_factor_replicas()
            e_all = self.eng.system_energy_replicas()
            system = initial[0]
            e0 = dict(zip(("non_coulomb", "coulomb", "recip_coulomb", "ewald_self", "intra_coulomb"), e_all[0, :5]))
        else:
            if self.device_build:
                for tt in range(topo.n_res):
                    if topo.is_active[tt]:
                        self.eng.set_frames(0, tt, system.com[tt], system.offsets[tt])
            self.eng.init_structure_factor(0, True)
            for r in range(1, self.R):
                self.eng.replica_copy(r, 0)
            e0 = self.eng.system_energy(0)
        active = [t for t in range(topo.n_res) if topo.is_active[t]]
        self.active = np.array(active, dtype=np.int32)
        n1 = np.array([topo.atoms_in_res[t] for t in active], dtype=np.int32)
        nmol = np.array([system.n_mol[t] for t in active], dtype=np.int32)
        cap = np.array([self.mol_capacity[t] for t in active], dtype=np.int32)
        max_n1 = int(n1.max())
        tot = max(1, int(nmol.sum()))
        com = np.zeros((tot, 3))
        off = np.zeros((tot, max_n1, 3))
        pos = 0
        for k, t in enumerate(active):
            com[pos:pos + nmol[k]] = system.com[t]
            off[pos:pos + nmol[k], :n1[k]] = system.offsets[t]
            pos += nmol[k]
        energy0 = np.array([e0["non_coulomb"], e0["coulomb"], e0["recip_coulomb"], e0["ewald_self"],
                            e0["intra_coulomb"]])
        lo = np.ascontiguousarray(system.bounds_lo)
        length = np.ascontiguousarray(np.diag(system.box_matrix))
        self.slot = free[0]
        FortranFarm._slots[self.slot] = self
        self._select()
        # device_accept (with device_build): the engine also applies the acceptance rule and commits accepted candidates
        self.device_accept = bool(device_accept) and self.device_build
        # window (with device_build): one launch per lane step (mgpu_farm_window_submit): the engine builds, evaluates, decides
        # with the driver's draws and commits; the driver checks every decision.  Falls back to the batched path where the
        # one-launch kernel does not apply (mgpu_farm_window_capacity).
        want_window = bool(window) and self.device_build and not self.device_accept
        self.H.mfarm_configure(C.c_int((3 if want_window else (2 if self.device_accept else 1)) if self.device_build else 0))
        rc = self.H.mfarm_create(self.eng.h, C.c_int(self.R), C.c_int(len(active)), self.active.ctypes.data_as(_ip),
                                 n1.ctypes.data_as(_ip), nmol.ctypes.data_as(_ip), cap.ctypes.data_as(_ip),
                                 C.c_int(max_n1), com.ctypes.data_as(_dp), off.ctypes.data_as(_dp),
                                 energy0.ctypes.data_as(_dp), lo.ctypes.data_as(_dp), length.ctypes.data_as(_dp),
                                 C.c_double(system.temperature), C.c_double(translation_step),
                                 C.c_double(rotation_step), C.c_double(p_translation), C.c_int(seed),
                                 C.c_int(rng_kind), C.c_int(n_threads), C.c_int(n_lanes))
        _lib.check(rc)
        if initial is not None:
            for r, s_r in enumerate(initial):
                nm_r = np.array([s_r.n_mol[t] for t in active], dtype=np.int32)
                tot_r = max(1, int(nm_r.sum()))
                com_r = np.zeros((tot_r, 3))
                off_r = np.zeros((tot_r, max_n1, 3))
                pos = 0
                for k, t in enumerate(active):
                    com_r[pos:pos + nm_r[k]] = s_r.com[t]
                    off_r[pos:pos + nm_r[k], :n1[k]] = s_r.offsets[t]
                    pos += nm_r[k]
                e_r = np.ascontiguousarray(e_all[r, :5])
                rc = self.H.mfarm_set_replica(C.c_int(r), nm_r.ctypes.data_as(_ip), com_r.ctypes.data_as(_dp),
                                              off_r.ctypes.data_as(_dp), e_r.ctypes.data_as(_dp))
                if rc:
                    raise RuntimeError(f"mfarm_set_replica({r}): code {rc}")
        if system.is_triclinic():
            from .engine import box_prepare
            _, volume, reciprocal, _ = box_prepare(system.box_matrix)
            mat = np.asfortranarray(system.box_matrix, dtype=np.float64)
            rcp = np.asfortranarray(reciprocal, dtype=np.float64)
            self.H.mfarm_set_triclinic(mat.ctypes.data_as(_dp), rcp.ctypes.data_as(_dp), C.c_double(volume))
        self.H.mfarm_set_window_depth(C.c_int(int(window_depth)))
        mode = np.zeros(3)
        self.H.mfarm_window_mode(mode.ctypes.data_as(_dp))
        self.window = bool(mode[0])
        self.H.mfarm_set_drivers(C.c_int(max(1, int(n_drivers))))     # host threads that share the lanes (mc_farm.f90)
        self.n_drivers = max(1, int(n_drivers))
        self.max_n1 = max_n1
        self.n_lanes = max(1, min(int(n_lanes) if n_lanes > 0 else 2, 4, self.R))
        self.n_active = len(active)
        self.stats = np.zeros(3)
        FortranFarm._live = self
        if gcmc is not None:
            fug = np.asarray(gcmc["fugacity"], dtype=np.float64)
            if fug.ndim == 0:
                fug = np.full((self.R, self.n_active), float(fug))
            elif fug.ndim == 1:
                fug = np.tile(fug[None, :], (self.R, 1)) if fug.shape[0] == self.n_active and self.n_active > 1 \
                    else (np.tile(fug[:, None], (1, self.n_active)) if fug.shape[0] == self.R
                          else np.tile(fug[None, :], (self.R, 1)))
            fug = np.ascontiguousarray(fug.reshape(self.R, self.n_active))     # == Fortran (n_active, R)
            rc = self.H.mfarm_set_gcmc(C.c_double(gcmc["p_translation"]), C.c_double(gcmc["p_rotation"]),
                                       fug.ctypes.data_as(_dp))
            if rc:
                raise ValueError(f"mfarm_set_gcmc: bad probabilities / fugacity (code {rc})")
        for t, off in (reservoir or {}).items():
            n1 = int(topo.atoms_in_res[t])
            off = np.ascontiguousarray(np.asarray(off, dtype=np.float64).reshape(-1, n1, 3))
            _lib.check(self.H.mfarm_set_reservoir(C.c_int(int(t)), C.c_int(off.shape[0]), off.ctypes.data_as(_dp)))

    def _check_initial(self, system, initial):
        """`initial`: R Systems with the topology and the box of `system`, every count within mol_capacity."""
        if len(initial) != self.R:
            raise ValueError(f"initial: {len(initial)} systems for {self.R} replicas")
        topo = system.topo
        for r, s_r in enumerate(initial):
            tr = s_r.topo
            same = tr is topo or (tr.n_res == topo.n_res and all(
                np.array_equal(np.asarray(getattr(tr, a)), np.asarray(getattr(topo, a)))
                for a in ("atoms_in_res", "atom_types", "charges", "is_active", "epsilon", "sigma")))
            if not same:
                raise ValueError(f"initial[{r}]: another topology than the farm's system")
            if not (np.array_equal(np.asarray(s_r.box_matrix), np.asarray(system.box_matrix))
                    and np.array_equal(np.asarray(s_r.bounds_lo), np.asarray(system.bounds_lo))):
                raise ValueError(f"initial[{r}]: another box than the farm's system")
            for t in range(topo.n_res):
                if int(s_r.n_mol[t]) > self.mol_capacity[t]:
                    raise ValueError(f"initial[{r}]: {int(s_r.n_mol[t])} molecules of type {t} exceed the capacity "
                                     f"{self.mol_capacity[t]}")

    def _select(self):
        self.H.mfarm_select(C.c_int(self.slot))

    def audit(self, replicas=None):
        """Every listed chain's energy from scratch against its running energy, in K, from ONE system_energy_replicas call:
        recomputed (n, 6), running (n, 5), energy_deviation (n,) = the largest |running - recomputed| over the five components,
        a_deviation (n,) = max |A(k) - S(k)|.  replicas = None: all of them."""
        reps = np.arange(self.R, dtype=np.int32) if replicas is None else np.ascontiguousarray(replicas, dtype=np.int32).reshape(-1)
        recomputed, a_dev = self.eng.system_energy_replicas(reps, a_deviation=True)
        running = np.array([self.energy(int(r)) for r in reps]).reshape(-1, 5)
        return dict(recomputed=recomputed, running=running,
                    energy_deviation=np.max(np.abs(running - recomputed[:, :5]), axis=1) if len(reps) else np.zeros(0),
                    a_deviation=a_dev)

    def rdf_sample(self, replicas=None, chunk=None):
        """One sample of every listed chain (None: all) into the engine's histograms (Engine.rdf_configure first), from the
        coordinates the engine holds -- which are current between two run() calls in every farm mode."""
        self.eng.rdf_accumulate(replicas, chunk)
        self._select()

    def molecule_energy_sample(self, replicas=None, chunk=None):
        """One sample of every listed chain (None: all) into the engine's molecule-energy histograms
        (Engine.molecule_energy_configure first), from the coordinates the engine holds -- which are current between two run()
        calls in every farm mode."""
        self.eng.molecule_energy_accumulate(replicas, chunk)
        self._select()

    def density_sample(self, replicas=None, chunk=None):
        """One sample of every listed chain (None: all) into the engine's density maps (Engine.density_configure first), from
        the coordinates the engine holds -- which are current between two run() calls in every farm mode."""
        self.eng.density_accumulate(replicas, chunk)
        self._select()

    def energy_pairs_sample(self, pairs, replicas=None, chunk=None):
        """The energy by residue-type pair of every listed chain (None: all), (n, n_sel, 5) in K (Engine.energy_pairs_replicas),
        from the coordinates the engine holds -- which are current between two run() calls in every farm mode."""
        out = self.eng.energy_pairs_replicas(pairs, replicas, chunk)
        self._select()
        return out

    def run(self, n_steps: int) -> int:
        """Advance every chain by n_steps move selections; returns the moves accepted during this call."""
        self._select()
        before = self.stats[1]
        rc = self.H.mfarm_run(C.c_int(n_steps), self.stats.ctypes.data_as(_dp))
        _lib.check(rc)
        return int(self.stats[1] - before)

    def window_mode(self):
        """(window mode on, windows of a lane in flight, steps the device left to the driver so far)."""
        self._select()
        mode = np.zeros(3)
        self.H.mfarm_window_mode(mode.ctypes.data_as(_dp))
        return bool(mode[0]), int(mode[1]), int(mode[2])

    def recalibrate(self):
        self._select()
        s = np.zeros(2)
        self.H.mfarm_recalibrate(s.ctypes.data_as(_dp))
        return s

    def timers(self):
        """Host seconds in: generate, submit, wait-for-GPU, resolve, commit-submit."""
        t = np.zeros(7)
        self._select()
        self.H.mfarm_get_timers(t.ctypes.data_as(_dp))
        return dict(zip(("generate", "submit", "wait", "resolve", "commit", "gen_rng", "gen_gather"), t.tolist()))

    def counters(self):
        c = np.zeros(8)
        self._select()
        self.H.mfarm_get_counters(c.ctypes.data_as(_dp))
        names = ("trial_translations", "translations", "trial_rotations", "rotations", "trial_creations",
                 "creations", "trial_deletions", "deletions")
        return dict(zip(names, c.astype(np.int64).tolist()))

    def chain_counters(self):
        """Every chain's own counters, shape (R, 8), in the order of counters(); summed over the chains they are counters()."""
        c = np.zeros((self.R, 8))
        self._select()
        self.H.mfarm_get_chain_counters(c.ctypes.data_as(_dp))
        return c.astype(np.int64)

    def counts(self):
        """Current molecule counts, shape (R, n_active)."""
        c = np.zeros((self.R, self.n_active), dtype=np.int32)
        self._select()
        self.H.mfarm_get_counts(c.ctypes.data_as(_ip))
        return c

    def exchange_block(self, comm, n_bins=5001):
        """mfarm_exchange_block: every rank's {accepted, trials} and per-active-type histogram of its chains' molecule
        counts through the C-ABI communicator `comm` (exchange.CAbiComm).  Returns (sums[world, 2], hist[world, n_active,
        n_bins])."""
        self._select()
        sums = np.zeros((comm.world, 2))
        hist = np.zeros((comm.world, self.n_active, n_bins), dtype=np.int64)
        self.H.mfarm_exchange_block.restype = C.c_int
        rc = self.H.mfarm_exchange_block(comm.h, C.c_int(n_bins), C.c_int(comm.world), sums.ctypes.data_as(_dp),
                                         hist.ctypes.data_as(C.POINTER(C.c_longlong)))
        _lib.check(rc)
        return sums, hist

    def energy(self, replica: int):
        e = np.zeros(5)
        self._select()
        self.H.mfarm_get_energy(C.c_int(replica), e.ctypes.data_as(_dp))
        return e

    def molecule(self, replica: int, ia: int, slot: int):
        com = np.zeros(3)
        off = np.zeros((self.max_n1, 3))
        self._select()
        self.H.mfarm_get_molecule(C.c_int(replica), C.c_int(ia), C.c_int(slot), com.ctypes.data_as(_dp),
                                  off.ctypes.data_as(_dp))
        return com, off

    def reservoir(self, replica: int, ia: int):
        """chain `replica`'s reservoir of active type ia: offsets (n, n1, 3) -- the driver's mirror (host-built farms) or the
        engine's (device-built)"""
        n1 = int(self.sys.topo.atoms_in_res[int(self.active[ia])])
        cap = self.mol_capacity[int(self.active[ia])] + 4096
        off = np.zeros((cap, n1, 3))
        n = C.c_int()
        self._select()
        _lib.check(self.H.mfarm_get_reservoir(C.c_int(replica), C.c_int(ia), C.c_int(cap), C.byref(n), off.ctypes.data_as(_dp)))
        if n.value > cap:
            raise RuntimeError("reservoir larger than the buffer")
        return off[: n.value].copy()

    STATE_CHUNK_BYTES = 1 << 30       # an engine block's size at the types' capacities: larger farms are cut by the replica list

    def _state_chunks(self):
        """the replica lists of the engine blocks of a checkpoint: all R replicas in order, cut so that a block stays well
        below the engine's limit of 2^31 words"""
        topo = self.sys.topo
        per = 16 * (self.eng.nk + 1) * 2 + sum(8 * 3 * (2 * int(topo.atoms_in_res[t]) + 1) * int(self.mol_capacity[t]) * 2
                                               for t in range(topo.n_res))
        step = max(1, FortranFarm.STATE_CHUNK_BYTES // max(1, per))
        return [list(range(c0, min(self.R, c0 + step))) for c0 in range(0, self.R, step)]

    def checkpoint_state(self):
        """Everything the next run() reads, between two run() calls: dict(driver=the Fortran driver's block (mfarm_state_export:
        generator states, counts, running energies, step sizes, counters, and a host-built farm's mirror and reservoirs),
        engine=[the engine's blocks (Engine.state_export) of all R replicas, in order]), uint8 arrays.  restore_state puts them
        into a farm created the same way; the run then continues bit for bit on the same library build and GPU model."""
        self._select()
        n = int(self.H.mfarm_state_bytes())
        drv = np.zeros(n, dtype=np.uint8)
        rc = self.H.mfarm_state_export(drv.ctypes.data_as(C.c_void_p), C.c_longlong(n))
        if rc:
            raise RuntimeError(f"mfarm_state_export: code {rc}")
        return dict(driver=drv, engine=[self.eng.state_export(reps) for reps in self._state_chunks()])

    def restore_state(self, state):
        """The inverse of checkpoint_state, into a farm created with the same system, replicas, capacities, mode, generator
        and reservoirs; ValueError otherwise -- from the driver before anything has changed, from the engine (which checks each
        block against itself and writes nothing of a block it refuses) after the driver has taken its own."""
        chunks = self._state_chunks()
        blocks = list(state["engine"])
        if len(blocks) != len(chunks):
            raise ValueError(f"restore_state: {len(blocks)} engine blocks for {len(chunks)} replica lists")
        drv = np.ascontiguousarray(np.frombuffer(state["driver"], dtype=np.uint8)).copy()
        self._select()
        rc = self.H.mfarm_state_import(drv.ctypes.data_as(C.c_void_p), C.c_longlong(drv.shape[0]))
        if rc:
            raise ValueError(f"restore_state: the driver's block does not belong to a farm created like this one (code {rc})")
        for reps, block in zip(chunks, blocks):
            try:
                self.eng.state_import(reps, block)
            except _lib.MgpuError as err:
                raise ValueError(f"restore_state: the engine refuses its block: {err}") from None
        self._select()
        _lib.check(self.H.mfarm_run(C.c_int(0), self.stats.ctypes.data_as(_dp)))     # (no steps: the carried totals)

    @property
    def trials(self):
        return int(self.stats[0])

    @property
    def accepted(self):
        return int(self.stats[1])

    @property
    def skipped(self):
        return int(self.stats[2])

    def close(self):
        if FortranFarm._slots.get(getattr(self, "slot", -1)) is self:
            self._select()
            self.H.mfarm_destroy()
            del FortranFarm._slots[self.slot]
        if FortranFarm._live is self:
            FortranFarm._live = next(iter(FortranFarm._slots.values()), None)
        self.eng.close()
