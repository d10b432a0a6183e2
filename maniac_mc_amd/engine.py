"""Python mirror of the energy engine's C ABI (include/maniac_gpu.h) -- plumbing only.

Two layers:

* batched calls (``pair_energy_candidates`` ...): thin ctypes wrappers, one per C entry point;
* reference-named B = 1 seams (``ComputePairInteractionEnergy_singlemol`` ...): the same names,
  argument meaning (residue type, molecule index) and outputs as the Fortran procedures listed in
  SURVEY.md section 8(b), so parity tests read like calls into the reference.  Indices are 0-based.

Every call goes to the HIP library; nothing here computes energies on the host.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import MGPU_CREATION, MGPU_DELETION, MGPU_MOVE, MGPU_NONE, check
from .system import System, Topology

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def _d(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _i(a):
    return None if a is None else a.ctypes.data_as(_ip)


def _ints(x, n=None):
    a = np.ascontiguousarray(np.atleast_1d(x), dtype=np.int32)
    if n is not None and a.shape[0] == 1 and n != 1:
        a = np.full(n, int(a[0]), dtype=np.int32)
    return a


def box_prepare(box_matrix):
    """mgpu_box_prepare: box type, volume, ``box%reciprocal`` and ``box%metrics``."""
    L = _lib.lib()
    m = np.ascontiguousarray(box_matrix, dtype=np.float64).reshape(9)
    bt = C.c_int(); vol = C.c_double(); rcp = np.zeros(9); met = np.zeros(9)
    check(L.mgpu_box_prepare(_d(m), C.byref(bt), C.byref(vol), _d(rcp), _d(met)))
    return bt.value, vol.value, rcp.reshape(3, 3), met


def ewald_setup(metrics, rc, tol):
    """mgpu_ewald_setup (SetupEwald, prepare_utils.f90:103-214)."""
    L = _lib.lib()
    met = np.ascontiguousarray(metrics, dtype=np.float64)
    rc_ = C.c_double(rc); tol_ = C.c_double(tol); alpha = C.c_double(); scr = C.c_double(); fp = C.c_double()
    kmax = np.zeros(3, dtype=np.int32); nk = C.c_int()
    check(L.mgpu_ewald_setup(_d(met), C.byref(rc_), C.byref(tol_), C.byref(alpha), C.byref(scr), C.byref(fp),
                             _i(kmax), C.byref(nk)))
    return dict(rc=rc_.value, tol=tol_.value, alpha=alpha.value, screening=scr.value,
                fourier_precision=fp.value, kmax=kmax, nk=nk.value)


def ewald_kvectors(reciprocal, alpha, kmax, nk):
    """mgpu_ewald_kvectors (PrecomputeValidReciprocalVectors + ComputeReciprocalWeights)."""
    L = _lib.lib()
    rcp = np.ascontiguousarray(reciprocal, dtype=np.float64).reshape(9)
    km = np.ascontiguousarray(kmax, dtype=np.int32)
    kx = np.zeros(nk, np.int32); ky = np.zeros(nk, np.int32); kz = np.zeros(nk, np.int32)
    k2 = np.zeros(nk); ff = np.zeros(nk); w = np.zeros(nk)
    check(L.mgpu_ewald_kvectors(_d(rcp), C.c_double(alpha), _i(km), C.c_int(nk), _i(kx), _i(ky), _i(kz),
                                _d(k2), _d(ff), _d(w)))
    return dict(kx=kx, ky=ky, kz=kz, k2mag=k2, form_factor=ff, weights=w)


STATE_FLAGS = dict(in_range=1, frames_ok=2, frames_tight=4, frames_held=8, rsv_tight=16)


def state_unpack(block):
    """The pieces of a state block (Engine.state_export; layout: include/maniac_gpu.h).  Returns a list with one dict per listed
    replica: replica, A (n_slots, 2) in the engine's slot order, and per residue type the lists n, flags, pos (n, n1, 3) in the
    engine's site order, com (n, 3) / off (n, n1, 3) over the nf molecules of frames carried (None without frames), rsv
    (count, n1, 3) and rsv_cap (None / 0 without a reservoir).  Copies, bit for bit."""
    w = np.frombuffer(block, dtype=np.int64)
    f = np.frombuffer(block, dtype=np.float64)
    n, n_res, n_slots = int(w[1]), int(w[2]), int(w[3])
    types_at = 8 + 12
    reps_at = types_at + 2 * n_res
    recs_at = reps_at + 2 * n
    n1s = [int(w[types_at + 2 * t]) for t in range(n_res)]

    def planes(at, nm, n1):
        pw = (nm * n1 + 1) & ~1
        p = np.stack([f[at + d * pw: at + d * pw + nm * n1] for d in range(3)], axis=-1)
        return (p.reshape(nm, n1, 3) if n1 >= 64 else p.reshape(n1, nm, 3).transpose(1, 0, 2)).copy()

    out = []
    for i in range(n):
        a_at = int(w[reps_at + 2 * i + 1])
        rep = dict(replica=int(w[reps_at + 2 * i]), A=f[a_at: a_at + 2 * n_slots].reshape(n_slots, 2).copy(),
                   n=[], flags=[], pos=[], com=[], off=[], rsv=[], rsv_cap=[])
        for t in range(n_res):
            nm, nf, rcap, flags, pos_at, com_at, off_at, rsv_at = (int(v) for v in w[recs_at + 8 * (i * n_res + t):][:8])
            rep["n"].append(nm)
            rep["flags"].append(flags)
            rep["pos"].append(planes(pos_at, nm, n1s[t]))
            rep["com"].append(planes(com_at, nf, 1)[:, 0, :] if com_at >= 0 else None)
            rep["off"].append(planes(off_at, nf, n1s[t]) if off_at >= 0 else None)
            rep["rsv_cap"].append(rcap)
            if rsv_at >= 0:
                count = int(np.frombuffer(block, dtype=np.int32)[2 * rsv_at])
                rep["rsv"].append(f[rsv_at + 2: rsv_at + 2 + 3 * count * n1s[t]].reshape(count, n1s[t], 3).copy())
            else:
                rep["rsv"].append(None)
        out.append(rep)
    return out


class Engine:
    """One HIP device, R replicas of one (box, force field, k table)."""

    def __init__(self, topo: Topology, box_matrix, bounds_lo, real_space_cutoff, ewald_tolerance,
                 n_replicas: int = 1, device: int = 0, mol_capacity: Optional[Sequence[int]] = None,
                 triclinic_moves: bool = False):
        self.L = _lib.lib()
        self.topo = topo
        self.n_replicas = int(n_replicas)
        if mol_capacity is None:
            mol_capacity = [64] * topo.n_res
        self.mol_capacity = np.ascontiguousarray(mol_capacity, dtype=np.int32)
        self.h = C.c_void_p()
        bm = np.ascontiguousarray(box_matrix, dtype=np.float64).reshape(9)
        lo = np.ascontiguousarray(bounds_lo, dtype=np.float64)
        check(self.L.mgpu_engine_create(
            C.byref(self.h), C.c_int(device), C.c_int(self.n_replicas), C.c_int(topo.n_res),
            _i(topo.atoms_in_res), _i(self.mol_capacity), C.c_int(topo.max_atom), _i(topo.atom_types),
            _d(topo.charges), _i(topo.is_active), C.c_int(topo.n_atom_types), _d(topo.epsilon), _d(topo.sigma),
            _d(bm), _d(lo), C.c_double(real_space_cutoff), C.c_double(ewald_tolerance)))
        alpha = C.c_double(); rc = C.c_double(); tol = C.c_double(); vol = C.c_double(); bt = C.c_int()
        kmax = np.zeros(3, dtype=np.int32); nk = C.c_int()
        check(self.L.mgpu_engine_get_ewald(self.h, C.byref(alpha), C.byref(rc), C.byref(tol), _i(kmax),
                                           C.byref(nk), C.byref(vol), C.byref(bt)))
        self.alpha, self.rc, self.tol, self.volume = alpha.value, rc.value, tol.value, vol.value
        self.kmax, self.nk, self.box_type = kmax, nk.value, bt.value
        self.max_n1 = int(topo.atoms_in_res.max())
        if triclinic_moves:
            self.set_triclinic_moves(True)

    @classmethod
    def from_system(cls, system: System, n_replicas: int = 1, device: int = 0, mol_capacity=None,
                    extra_capacity: int = 8, triclinic_moves: bool = False):
        """Engine sized for ``system`` with every replica loaded with that configuration.  ``triclinic_moves``: device-built
        moves and farm windows for a triclinic box (set_triclinic_moves)."""
        if mol_capacity is None:
            mol_capacity = [int(n) + (extra_capacity if system.topo.is_active[t] else 0)
                            for t, n in enumerate(system.n_mol)]
            mol_capacity = [max(1, c) for c in mol_capacity]
        eng = cls(system.topo, system.box_matrix, system.bounds_lo, system.real_space_cutoff,
                  system.ewald_tolerance, n_replicas, device, mol_capacity, triclinic_moves)
        eng.load_system(system, 0)
        for r in range(1, n_replicas):
            eng.replica_copy(r, 0)
        return eng

    def close(self):
        if getattr(self, "h", None) is not None and self.h:
            self.L.mgpu_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- replica state -------------------------------------------------------------------
    def load_system(self, system: System, replica: int = 0):
        for t in range(self.topo.n_res):
            self.set_molecules(replica, t, system.all_sites(t))

    def set_molecules(self, replica, t, sites):
        sites = np.ascontiguousarray(sites, dtype=np.float64).reshape(-1, int(self.topo.atoms_in_res[t]), 3)
        check(self.L.mgpu_replica_set_molecules(self.h, C.c_int(replica), C.c_int(t), C.c_int(sites.shape[0]),
                                                _d(sites)))

    def get_molecules(self, replica, t):
        n = self.num_molecules(replica, t)
        sites = np.zeros((n, int(self.topo.atoms_in_res[t]), 3))
        nm = C.c_int()
        check(self.L.mgpu_replica_get_molecules(self.h, C.c_int(replica), C.c_int(t), C.byref(nm), _d(sites)))
        return sites

    def set_frames(self, replica, t, com, off):
        """mgpu_replica_set_frames: com (n, 3) and offsets (n, n1, 3) as the reference keeps them; the sites are com + off."""
        n1 = int(self.topo.atoms_in_res[t])
        com = np.ascontiguousarray(com, dtype=np.float64).reshape(-1, 3)
        off = np.ascontiguousarray(np.asarray(off, dtype=np.float64)[:, :n1, :]).reshape(-1, n1, 3)
        check(self.L.mgpu_replica_set_frames(self.h, C.c_int(replica), C.c_int(t), C.c_int(com.shape[0]), _d(com), _d(off)))

    def get_frames(self, replica, t):
        n = self.num_molecules(replica, t)
        n1 = int(self.topo.atoms_in_res[t])
        com = np.zeros((n, 3)); off = np.zeros((n, n1, 3)); nm = C.c_int()
        check(self.L.mgpu_replica_get_frames(self.h, C.c_int(replica), C.c_int(t), C.byref(nm), _d(com), _d(off)))
        return com, off

    def set_reservoir(self, replica, t, off, cap=0):
        """mgpu_replica_set_reservoir: the reservoir of (replica, t) holds the molecule offsets off (n, n1, 3); cap = 0 sizes it
        by the conservation bound (n + the type's capacity).  off of no molecules with cap = 0 removes it."""
        n1 = int(self.topo.atoms_in_res[t]) if 0 <= t < len(self.topo.atoms_in_res) else 1   # (a bad type: the engine refuses it)
        off = np.ascontiguousarray(np.asarray(off, dtype=np.float64).reshape(-1, n1, 3))
        check(self.L.mgpu_replica_set_reservoir(self.h, C.c_int(replica), C.c_int(t), C.c_int(off.shape[0]), C.c_int(cap), _d(off)))

    def get_reservoir(self, replica, t):
        """mgpu_replica_get_reservoir: the reservoir's molecule offsets (n, n1, 3) as the device holds them now."""
        n1 = int(self.topo.atoms_in_res[t])
        nr = C.c_int()
        check(self.L.mgpu_replica_get_reservoir(self.h, C.c_int(replica), C.c_int(t), C.byref(nr), None))
        off = np.zeros((nr.value, n1, 3))
        if nr.value:
            check(self.L.mgpu_replica_get_reservoir(self.h, C.c_int(replica), C.c_int(t), C.byref(nr), _d(off)))
        return off

    def farm_snapshot_raw(self, replicas):
        """mgpu_farm_snapshot_submit + _wait for the replica list: (the engine's pinned block as a ctypes pointer, its length in
        doubles).  The block stays valid until the next snapshot; its layout is include/maniac_gpu.h's."""
        reps = _ints(replicas)
        nbytes = C.c_longlong()
        check(self.L.mgpu_farm_snapshot_submit(self.h, C.c_int(reps.shape[0]), _i(reps), C.byref(nbytes)))
        ptr = C.c_void_p()
        check(self.L.mgpu_farm_snapshot_wait(self.h, C.byref(ptr), C.byref(nbytes)))
        return ptr, nbytes.value // 8

    def farm_snapshot(self, replicas, chunk=None):
        """The frames and reservoirs of the listed replicas in one launch per chunk of `chunk` replicas (default: chunks of
        about 256 MB at the types' capacities).  Returns (counts (n, n_res) int32, com, off, rsv): com[i][t] (n, 3) and
        off[i][t] (n, n1, 3) are what get_frames(replicas[i], t) returns (None for a type without frames), rsv[i][t] the
        offsets get_reservoir returns (None without a reservoir)."""
        reps = [int(r) for r in np.atleast_1d(np.asarray(replicas, dtype=np.int64))]
        n_res = self.topo.n_res
        n1s = [int(self.topo.atoms_in_res[t]) for t in range(n_res)]
        if chunk is None:
            per = sum(3 * (1 + n1s[t]) * int(self.mol_capacity[t]) * 8 for t in range(n_res))
            chunk = max(1, (256 << 20) // max(1, per))
        counts = np.zeros((len(reps), n_res), dtype=np.int32)
        com, off, rsv = [], [], []
        for c0 in range(0, max(1, len(reps)), int(chunk)):
            part = reps[c0:c0 + int(chunk)]
            if not part:
                break
            ptr, n_dbl = self.farm_snapshot_raw(part)
            block = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(n_dbl,))
            hdr = block[: 4 * len(part) * n_res].view(np.int64).reshape(len(part), n_res, 4)
            for i in range(len(part)):
                ci, oi, ri = [], [], []
                for t in range(n_res):
                    n, nr, at, rat = (int(v) for v in hdr[i, t])
                    counts[c0 + i, t] = n
                    if at >= 0:
                        ci.append(block[at: at + 3 * n].reshape(n, 3).copy())
                        oi.append(block[at + 3 * n: at + 3 * n * (1 + n1s[t])].reshape(n, n1s[t], 3).copy())
                    else:
                        ci.append(None); oi.append(None)
                    ri.append(block[rat: rat + 3 * nr * n1s[t]].reshape(nr, n1s[t], 3).copy() if rat >= 0 else None)
                com.append(ci); off.append(oi); rsv.append(ri)
        return counts, com, off, rsv

    def state_export(self, replicas, copy=True):
        """mgpu_state_export_submit + _wait: the whole resident state of the listed replicas (any order, any subset, each once) as
        one block -- a uint8 array, a copy of the engine's pinned buffer (copy=False: a view of it, valid until the next export
        or the engine's close); include/maniac_gpu.h has the layout, state_unpack reads it."""
        reps = _ints(replicas) if len(np.atleast_1d(replicas)) else np.zeros(0, np.int32)
        nbytes = C.c_longlong()
        check(self.L.mgpu_state_export_submit(self.h, C.c_int(reps.shape[0]), _i(reps), C.byref(nbytes)))
        ptr = C.c_void_p()
        check(self.L.mgpu_state_export_wait(self.h, C.byref(ptr), C.byref(nbytes)))
        block = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(nbytes.value,))
        return block.copy() if copy else block

    def state_import(self, replicas, block):
        """mgpu_state_import: the block of a state_export into the listed replicas of this engine (as many as the block holds).
        The engine checks the block against itself first and writes nothing where it does not fit."""
        reps = _ints(replicas) if len(np.atleast_1d(replicas)) else np.zeros(0, np.int32)
        buf = np.ascontiguousarray(np.frombuffer(block, dtype=np.uint8))
        check(self.L.mgpu_state_import(self.h, C.c_int(reps.shape[0]), _i(reps), buf.ctypes.data_as(C.c_void_p),
                                       C.c_longlong(buf.shape[0])))

    def move_trial(self, replica, t, m, move, u, translation_step, rotation_step, lane=0):
        """Device-built trials (mgpu_move_trial_submit + wait): (old[n,5], new[n,5])."""
        m = _ints(m); n = m.shape[0]
        replica = _ints(replica, n); t = _ints(t, n); move = _ints(move, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(n, 5)
        old = np.zeros((n, 5)); new = np.zeros((n, 5))
        self._last_stride = 0
        check(self.L.mgpu_move_trial_submit(self.h, C.c_int(lane), C.c_int(n), _i(replica), _i(t), _i(m), _i(move), _d(u),
                                            C.c_double(translation_step), C.c_double(rotation_step)))
        check(self.L.mgpu_gcmc_trial_wait(self.h, C.c_int(lane), _d(old), _d(new)))
        return old, new

    def move_trial_decide(self, replica, t, m, move, u, translation_step, rotation_step, accept_u, accept_pref, temperature,
                          lane=0):
        """Device-built trials decided and committed on the device (mgpu_move_trial_decide_submit + wait):
        (old[n,5], new[n,5], accepted[n])."""
        m = _ints(m); n = m.shape[0]
        replica = _ints(replica, n); t = _ints(t, n); move = _ints(move, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(n, 5)
        au = np.ascontiguousarray(accept_u, dtype=np.float64).reshape(n)
        ap = np.ascontiguousarray(accept_pref, dtype=np.float64).reshape(n)
        old = np.zeros((n, 5)); new = np.zeros((n, 5)); acc = np.zeros(n, np.int32)
        self._last_stride = 0
        check(self.L.mgpu_move_trial_decide_submit(self.h, C.c_int(lane), C.c_int(n), _i(replica), _i(t), _i(m), _i(move), _d(u),
                                                   C.c_double(translation_step), C.c_double(rotation_step), _d(au), _d(ap),
                                                   C.c_double(temperature)))
        check(self.L.mgpu_trial_decide_wait(self.h, C.c_int(lane), _d(old), _d(new), _i(acc)))
        return old, new, acc

    def farm_window_capacity(self):
        n = C.c_int(0); d = C.c_int(0)
        check(self.L.mgpu_farm_window_capacity(self.h, C.byref(n), C.byref(d)))
        return n.value, d.value

    def farm_set_wide_triclinic(self, on=True):
        """mgpu_farm_set_wide_triclinic: farm windows take rigid molecules of 6 to 63 sites in a triclinic box (off by default;
        the single-chain paths have chain_set_wide_triclinic).  Needs set_triclinic_moves as every farm window of such a box.
        Refused (MgpuError, the switch unchanged) for an orthorhombic box, and switched off while a farm window is uncollected."""
        check(self.L.mgpu_farm_set_wide_triclinic(self.h, C.c_int(1 if on else 0)))

    def farm_window_submit(self, replica, t, m, move, u, translation_step, rotation_step, accept_u, accept_pref, temperature,
                           forced=None, lane=0, slot_u=None):
        """mgpu_farm_window_submit: one launch evaluates, decides and commits one step of every chain given."""
        m = _ints(m); n = m.shape[0]
        replica = _ints(replica, n); t = _ints(t, n); move = _ints(move, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(n, 5)
        au = np.ascontiguousarray(accept_u, dtype=np.float64).reshape(n)
        ap = np.ascontiguousarray(accept_pref, dtype=np.float64).reshape(n)
        fo = _ints(0 if forced is None else forced, n)
        su = None if slot_u is None else np.ascontiguousarray(slot_u, dtype=np.float64).reshape(n)
        check(self.L.mgpu_farm_window_submit(self.h, C.c_int(lane), C.c_int(n), _i(replica), _i(t), _i(m), _i(move), _i(fo), _d(u),
                                             _d(au), _d(ap), _d(su), C.c_double(translation_step), C.c_double(rotation_step),
                                             C.c_double(temperature)))
        return n

    def farm_window_wait(self, n, lane=0):
        """The lane's oldest window: (old[n,5], new[n,5], verdict[n])."""
        old = np.zeros((n, 5)); new = np.zeros((n, 5)); v = np.zeros(n, np.int32)
        check(self.L.mgpu_farm_window_wait(self.h, C.c_int(lane), _d(old), _d(new), _i(v)))
        return old, new, v

    def farm_window_flush(self):
        check(self.L.mgpu_farm_window_flush(self.h))

    def farm_window_stats(self):
        w = C.c_longlong(0); u = C.c_longlong(0)
        check(self.L.mgpu_farm_window_get_stats(self.h, C.byref(w), C.byref(u)))
        return w.value, u.value

    # ---- chain runs (mgpu_chain_run_*): launches of one chain queued back to back, continuing from a cursor on the device
    def chain_run_capacity(self):
        """(max_k, max_in_flight, ring_steps); all 0 where the path does not apply."""
        k = C.c_int(0); d = C.c_int(0); r = C.c_int(0)
        check(self.L.mgpu_chain_run_capacity(self.h, C.byref(k), C.byref(d), C.byref(r)))
        return k.value, d.value, r.value

    def chain_run_set_triclinic(self, on=True):
        """mgpu_chain_run_set_triclinic: a triclinic box takes chain runs (off by default).  Refused (MgpuError, the switch
        unchanged) for an orthorhombic box, without set_triclinic_moves, while a run is open, and -- switching it off -- while
        chain_run_set_gc is on."""
        check(self.L.mgpu_chain_run_set_triclinic(self.h, C.c_int(1 if on else 0)))

    def chain_run_open(self, replica, k, translation_step, rotation_step, temperature):
        check(self.L.mgpu_chain_run_open(self.h, C.c_int(replica), C.c_int(k), C.c_double(translation_step), C.c_double(rotation_step),
                                         C.c_double(temperature)))

    def chain_run_push(self, t, m, move, u, accept_u):
        m = _ints(m); n = m.shape[0]
        t = _ints(t, n); move = _ints(move, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(n, 5)
        au = np.ascontiguousarray(accept_u, dtype=np.float64).reshape(n)
        check(self.L.mgpu_chain_run_push(self.h, C.c_int(n), _i(t), _i(m), _i(move), _d(u), _d(au)))
        return n

    def chain_run_set_wide(self, on=True):
        """mgpu_chain_run_set_wide: the engine's runs also take rigid molecules of 6 to 63 sites (off by default: such an
        engine reports capacity 0).  Refused (MgpuError, the switch unchanged) while a run is open, and switching it on for a
        triclinic box or an engine with a reservoir.  Works with chain_run_set_gc / chain_run_push_gc."""
        check(self.L.mgpu_chain_run_set_wide(self.h, C.c_int(1 if on else 0)))

    def chain_run_set_gc(self, on=True):
        """mgpu_chain_run_set_gc: the engine's runs are those of a grand-canonical block (off by default): by-count records
        through chain_run_push_gc.  Refused (MgpuError, the switch unchanged) for a triclinic box unless
        chain_run_set_triclinic is on, with a reservoir, and while a run is open."""
        check(self.L.mgpu_chain_run_set_gc(self.h, C.c_int(1 if on else 0)))

    def chain_run_push_gc(self, t, move, u, accept_u, sel_u, phi_v):
        """By-count records (moves 0-4): the launch that takes one picks slot min(int(sel_u N), N - 1) and forms the prefactor
        phi_v / (N + 1) (insertion) or N / phi_v (deletion) from the count N it finds."""
        move = _ints(move); n = move.shape[0]
        t = _ints(t, n)
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(n, 5)
        au = np.ascontiguousarray(accept_u, dtype=np.float64).reshape(n)
        su = np.ascontiguousarray(np.broadcast_to(np.asarray(sel_u, dtype=np.float64), (n,)))
        pv = np.ascontiguousarray(np.broadcast_to(np.asarray(phi_v, dtype=np.float64), (n,)))
        check(self.L.mgpu_chain_run_push_gc(self.h, C.c_int(n), _i(t), _i(move), _d(u), _d(au), _d(su), _d(pv)))
        return n

    def chain_run_launch(self, n_launches=1):
        check(self.L.mgpu_chain_run_launch(self.h, C.c_int(n_launches)))

    def chain_run_collect(self, max_steps, wait=True):
        """(old[n,5], new[n,5], verdict[n], stalled_at): the next steps in order; an undecided step is the last row (verdict 2)."""
        old = np.zeros((max_steps, 5)); new = np.zeros((max_steps, 5)); v = np.zeros(max_steps, np.int32)
        n = C.c_int(0); st = C.c_int(-1)
        check(self.L.mgpu_chain_run_collect(self.h, C.c_int(max_steps), C.c_int(1 if wait else 0), _d(old), _d(new), _i(v), C.byref(n),
                                            C.byref(st)))
        return old[:n.value], new[:n.value], v[:n.value], st.value

    def chain_run_force(self, step, accept):
        check(self.L.mgpu_chain_run_force(self.h, C.c_int(step), C.c_int(1 if accept else 0)))

    def chain_run_close(self):
        check(self.L.mgpu_chain_run_close(self.h))

    def chain_run_stats(self):
        """(launches, steps, void_launches, undecided) since the engine was created."""
        a = [C.c_longlong(0) for _ in range(4)]
        check(self.L.mgpu_chain_run_get_stats(self.h, *[C.byref(x) for x in a]))
        return tuple(x.value for x in a)

    def chain_run_launches(self, max_launches=1024):
        """[(first step, steps consumed)] of the launches seen since the run was opened, oldest first."""
        f = np.zeros(max_launches, np.int32); c = np.zeros(max_launches, np.int32); n = C.c_int(0)
        check(self.L.mgpu_chain_run_get_launches(self.h, C.c_int(max_launches), _i(f), _i(c), C.byref(n)))
        return [(int(f[i]), int(c[i])) for i in range(n.value)]

    def gcmc_trial_decide(self, replica, t, m, kind, sites, accept_u, accept_pref, temperature, lane=0):
        """Host-built rows, decided and committed on the device: (old[n,5], new[n,5], accepted[n])."""
        n, replica, t, m, sites = self._cand(replica, t, m, sites)
        kind = _ints(kind, n)
        au = np.ascontiguousarray(accept_u, dtype=np.float64).reshape(n)
        ap = np.ascontiguousarray(accept_pref, dtype=np.float64).reshape(n)
        old = np.zeros((n, 5)); new = np.zeros((n, 5)); acc = np.zeros(n, np.int32)
        self._last_stride = sites.shape[1]
        check(self.L.mgpu_gcmc_trial_decide_submit(self.h, C.c_int(lane), C.c_int(n), _i(replica), _i(t), _i(m), _i(kind),
                                                   _d(sites), C.c_int(sites.shape[1]), _d(au), _d(ap), C.c_double(temperature)))
        check(self.L.mgpu_trial_decide_wait(self.h, C.c_int(lane), _d(old), _d(new), _i(acc)))
        return old, new, acc

    def num_molecules(self, replica, t):
        n = C.c_int()
        check(self.L.mgpu_replica_num_molecules(self.h, C.c_int(replica), C.c_int(t), C.byref(n)))
        return n.value

    def set_num_molecules(self, replica, t, n):
        check(self.L.mgpu_replica_set_num_molecules(self.h, C.c_int(replica), C.c_int(t), C.c_int(n)))

    def replica_copy(self, dst, src):
        check(self.L.mgpu_replica_copy(self.h, C.c_int(dst), C.c_int(src)))

    def structure_factor_add(self, replica, t, sites):
        """A(k) += sum_a q_a exp(i k . sites_a) for one molecule of type t; nothing else changes."""
        a = np.ascontiguousarray(sites, dtype=np.float64)[: int(self.topo.atoms_in_res[t])]
        check(self.L.mgpu_structure_factor_add(self.h, C.c_int(replica), C.c_int(t), _d(np.ascontiguousarray(a))))

    def replace_molecule(self, replica, t, m_dst, m_src):
        check(self.L.mgpu_replica_replace_molecule(self.h, C.c_int(replica), C.c_int(t), C.c_int(m_dst),
                                                   C.c_int(m_src)))

    def kvectors(self):
        nk = self.nk
        kx = np.zeros(nk, np.int32); ky = np.zeros(nk, np.int32); kz = np.zeros(nk, np.int32)
        k2 = np.zeros(nk); ff = np.zeros(nk); w = np.zeros(nk)
        check(self.L.mgpu_engine_get_kvectors(self.h, _i(kx), _i(ky), _i(kz), _d(k2), _d(ff), _d(w)))
        return dict(kx=kx, ky=ky, kz=kz, k2mag=k2, form_factor=ff, weights=w)

    # ---- static energies -----------------------------------------------------------------
    def system_energy(self, replica=0):
        out = np.zeros(6)
        check(self.L.mgpu_system_energy(self.h, C.c_int(replica), _d(out)))
        return dict(non_coulomb=out[0], coulomb=out[1], recip_coulomb=out[2], ewald_self=out[3],
                    intra_coulomb=out[4], total=out[5])

    def init_structure_factor(self, replica=0, full=True):
        check(self.L.mgpu_init_structure_factor(self.h, C.c_int(replica), C.c_int(1 if full else 0)))

    def _replica_list(self, replicas):
        if replicas is None:
            return np.arange(self.n_replicas, dtype=np.int32)
        return np.ascontiguousarray(replicas, dtype=np.int32).reshape(-1)

    def system_energy_replicas(self, replicas=None, chunk=None, a_deviation=False):
        """ComputeSystemEnergy of many replicas in one call: an (n, 6) array whose row i is system_energy(replicas[i]) bit for
        bit (non_coulomb, coulomb, recip_coulomb, ewald_self, intra_coulomb, total); with a_deviation also the (n,) array
        max |A(k) - S(k)| per replica.  replicas = None: all of them; chunk = replicas per device pass (None: the engine's)."""
        r = self._replica_list(replicas)
        n = r.shape[0]
        out = np.zeros((n, 6))
        dev = np.zeros(n) if a_deviation else None
        check(self.L.mgpu_system_energy_replicas(self.h, C.c_int(n), _i(r), C.c_int(0 if chunk is None else int(chunk)),
                                                 _d(out), _d(dev)))
        return (out, dev) if a_deviation else out

    def init_structure_factor_replicas(self, replicas=None, full=True):
        """init_structure_factor for many replicas in one call (None: all of them)."""
        r = self._replica_list(replicas)
        check(self.L.mgpu_init_structure_factor_replicas(self.h, C.c_int(r.shape[0]), _i(r), C.c_int(1 if full else 0)))

    def energy_pairs_replicas(self, pairs, replicas=None, chunk=None):
        """mgpu_energy_pairs_replicas: the energy by residue-type pair of many replicas in one call, an (n, n_sel, 5) array in K
        (non_coulomb, coulomb, recip_coulomb, ewald_self, intra_coulomb) for the unordered pairs [(a, b), ...] of 0-based
        residue types (at most 36, a == b allowed).  replicas = None: all of them; chunk as system_energy_replicas takes it."""
        pairs = [(int(a), int(b)) for a, b in pairs]
        ra = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int32)
        rb = np.ascontiguousarray([p[1] for p in pairs], dtype=np.int32)
        r = self._replica_list(replicas)
        n = r.shape[0]
        out = np.zeros((n, len(pairs), 5))
        check(self.L.mgpu_energy_pairs_replicas(self.h, C.c_int(n), _i(r), C.c_int(0 if chunk is None else int(chunk)),
                                                C.c_int(len(pairs)), _i(ra) if pairs else None, _i(rb) if pairs else None,
                                                _d(out) if out.size else None))
        return out

    # ---- radial distribution functions ---------------------------------------------------
    def rdf_configure(self, n_bins, r_max, pairs, include_intra=False):
        """mgpu_rdf_configure: histograms of n_bins bins up to r_max for the unordered pairs [(a, b), ...] of 0-based atom types
        (at most 8), zeroed, for every replica.  pairs = [] frees them."""
        pairs = [(int(a), int(b)) for a, b in pairs]
        ta = np.ascontiguousarray([p[0] for p in pairs], dtype=np.int32)
        tb = np.ascontiguousarray([p[1] for p in pairs], dtype=np.int32)
        check(self.L.mgpu_rdf_configure(self.h, C.c_int(int(n_bins)), C.c_double(float(r_max)), C.c_int(len(pairs)),
                                        _i(ta) if pairs else None, _i(tb) if pairs else None, C.c_int(1 if include_intra else 0)))
        self.rdf_shape = (len(pairs), int(n_bins)) if pairs else None

    def _rdf_shape(self):
        shape = getattr(self, "rdf_shape", None)
        if shape is None:
            raise _lib.MgpuError(5, "no histogram is configured (Engine.rdf_configure)")
        return shape

    def rdf_accumulate(self, replicas=None, chunk=None):
        """mgpu_rdf_accumulate_replicas: one sample of every listed replica (None: all) from the resident coordinates."""
        r = self._replica_list(replicas)
        check(self.L.mgpu_rdf_accumulate_replicas(self.h, C.c_int(r.shape[0]), _i(r), C.c_int(0 if chunk is None else int(chunk))))

    def _accum_call(self, name, ids, shapes=(), arrays=None, what=""):
        """mgpu_<name>, one of the rdf / density read, load and reset calls, on the entries `ids`.  Its uint64 buffers, one per
        entry of `shapes` (the per-entry shape of an accumulator segment), are zeroed and returned (arrays None: a read;
        no shapes: a reset) or are `arrays`, which must have those shapes (a load; ValueError naming `what` otherwise)."""
        n = ids.shape[0]
        if arrays is None:
            bufs = [np.zeros((n,) + tuple(s), dtype=np.uint64) for s in shapes]
        else:
            bufs = [np.ascontiguousarray(a, dtype=np.uint64) for a in arrays]
            if [b.shape for b in bufs] != [(n,) + tuple(s) for s in shapes]:
                raise ValueError(f"{name}: arrays of shapes {', '.join(str(b.shape) for b in bufs)} for {n} {what}")
        check(getattr(self.L, "mgpu_" + name)(self.h, C.c_int(n), _i(ids), *[b.ctypes.data_as(C.POINTER(C.c_ulonglong)) for b in bufs]))
        return tuple(bufs)

    def rdf_read(self, replicas=None):
        """mgpu_rdf_read: (hist (n, n_pairs, n_bins), eligible (n, n_pairs), samples (n,)) of the listed replicas, uint64."""
        r = self._replica_list(replicas)
        np_, nb = self._rdf_shape()
        return self._accum_call("rdf_read", r, ((np_, nb), (np_,), ()))

    def rdf_load(self, hist, eligible, samples, replicas=None):
        """mgpu_rdf_load: overwrite the listed replicas' accumulators with arrays shaped as rdf_read returns them."""
        r = self._replica_list(replicas)
        np_, nb = self._rdf_shape()
        self._accum_call("rdf_load", r, ((np_, nb), (np_,), ()), (hist, eligible, samples), f"replicas of {np_} pairs and {nb} bins")

    def rdf_reset(self, replicas=None):
        """mgpu_rdf_reset: zero the listed replicas' accumulators (None: all)."""
        self._accum_call("rdf_reset", self._replica_list(replicas))

    # ---- density maps --------------------------------------------------------------------
    def density_configure(self, grid, types, group_of=None, n_groups=None):
        """mgpu_density_configure: maps of grid = (n0, n1, n2) voxels along the three cell vectors for the channels `types`
        (0-based atom types, at most 8), zeroed.  group_of (R,): the map every replica adds into, -1 for a replica that is
        never counted (None: all replicas into map 0); n_groups: None = the largest entry + 1.  types = [] frees them."""
        types = np.ascontiguousarray([int(t) for t in types], dtype=np.int32)
        grid = np.ascontiguousarray([int(v) for v in grid], dtype=np.int32)
        if grid.shape != (3,):
            raise ValueError(f"density_configure: the grid takes three voxel counts, not {grid.tolist()}")
        if group_of is None:
            group_of = np.zeros(self.n_replicas, dtype=np.int32)
        group_of = np.ascontiguousarray(group_of, dtype=np.int32)
        if group_of.shape != (self.n_replicas,):
            raise ValueError(f"density_configure: group_of takes one entry per replica ({self.n_replicas}), not {group_of.shape}")
        if n_groups is None:
            n_groups = max(1, int(group_of.max()) + 1)
        check(self.L.mgpu_density_configure(self.h, _i(grid), C.c_int(types.shape[0]), _i(types) if types.size else None,
                                            C.c_int(int(n_groups)), _i(group_of)))
        self.density_shape = (int(n_groups), types.shape[0], int(grid[2]), int(grid[1]), int(grid[0])) if types.size else None

    def _density_groups(self, groups):
        shape = getattr(self, "density_shape", None)
        if shape is None:
            raise _lib.MgpuError(5, "no density map is configured (Engine.density_configure)")
        g = np.arange(shape[0], dtype=np.int32) if groups is None else np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        return g, shape[1:]

    def density_accumulate(self, replicas=None, chunk=None):
        """mgpu_density_accumulate_replicas: one sample of every listed replica (None: all) from the resident coordinates."""
        r = self._replica_list(replicas)
        check(self.L.mgpu_density_accumulate_replicas(self.h, C.c_int(r.shape[0]), _i(r), C.c_int(0 if chunk is None else int(chunk))))

    def density_read(self, groups=None):
        """mgpu_density_read: (hist (n, n_channels, n2, n1, n0), samples (n,)) of the listed groups (None: all), uint64."""
        g, per = self._density_groups(groups)
        return self._accum_call("density_read", g, (per, ()))

    def density_load(self, hist, samples, groups=None):
        """mgpu_density_load: overwrite the listed groups' accumulators with arrays shaped as density_read returns them."""
        g, per = self._density_groups(groups)
        self._accum_call("density_load", g, (per, ()), (hist, samples), f"groups of maps {per}")

    def density_reset(self, groups=None):
        """mgpu_density_reset: zero the listed groups' accumulators (None: all)."""
        self._accum_call("density_reset", self._density_groups(groups)[0])

    # ---- per-molecule removal energies ---------------------------------------------------
    def molecule_energies_replicas(self, types, replicas=None, chunk=None):
        """mgpu_molecule_energies_replicas: (energies (n, rows, 5) float64 in K, counts (n, n_sel) int32) of the listed replicas
        (None: all) for the ACTIVE 0-based residue `types`: row (capacities of types[:s]).sum() + m holds E(X) - E(X without m)
        of molecule m of types[s] (non_coulomb, coulomb, recip_coulomb, ewald_self, intra_coulomb); rows from a count on are 0."""
        types = _ints([int(t) for t in types]) if len(types) else np.zeros(0, dtype=np.int32)
        r = self._replica_list(replicas)
        n = r.shape[0]
        rows = int(sum(int(self.mol_capacity[t]) for t in types if 0 <= t < self.topo.n_res))
        out = np.zeros((n, rows, 5))
        counts = np.zeros((n, types.shape[0]), dtype=np.int32)
        check(self.L.mgpu_molecule_energies_replicas(self.h, C.c_int(n), _i(r), C.c_int(0 if chunk is None else int(chunk)),
                                                     C.c_int(types.shape[0]), _i(types) if types.size else None, _d(out), _i(counts)))
        return out, counts

    def molecule_energy_configure(self, n_bins, e_min, e_max, types):
        """mgpu_molecule_energy_configure: histograms of n_bins bins over [e_min, e_max) K (and one slot below, one above) of the
        molecules' total removal energy for the ACTIVE 0-based residue `types`, zeroed, for every replica.  types = [] frees them."""
        types = _ints([int(t) for t in types]) if len(types) else np.zeros(0, dtype=np.int32)
        check(self.L.mgpu_molecule_energy_configure(self.h, C.c_int(int(n_bins)), C.c_double(float(e_min)), C.c_double(float(e_max)),
                                                    C.c_int(types.shape[0]), _i(types) if types.size else None))
        self.molecule_energy_shape = (types.shape[0], int(n_bins) + 2) if types.size else None

    def _molecule_energy_shape(self):
        shape = getattr(self, "molecule_energy_shape", None)
        if shape is None:
            raise _lib.MgpuError(5, "no histogram is configured (Engine.molecule_energy_configure)")
        return shape

    def molecule_energy_accumulate(self, replicas=None, chunk=None):
        """mgpu_molecule_energy_accumulate_replicas: one sample of every listed replica (None: all) from the resident coordinates."""
        r = self._replica_list(replicas)
        check(self.L.mgpu_molecule_energy_accumulate_replicas(self.h, C.c_int(r.shape[0]), _i(r), C.c_int(0 if chunk is None else int(chunk))))

    def molecule_energy_read(self, replicas=None):
        """mgpu_molecule_energy_read: (hist (n, n_sel, n_bins + 2), samples (n,)) of the listed replicas, uint64."""
        return self._accum_call("molecule_energy_read", self._replica_list(replicas), (self._molecule_energy_shape(), ()))

    def molecule_energy_load(self, hist, samples, replicas=None):
        """mgpu_molecule_energy_load: overwrite the listed replicas' accumulators with arrays shaped as molecule_energy_read returns them."""
        ns, slots = self._molecule_energy_shape()
        self._accum_call("molecule_energy_load", self._replica_list(replicas), ((ns, slots), ()), (hist, samples),
                         f"replicas of {ns} types and {slots} slots")

    def molecule_energy_reset(self, replicas=None):
        """mgpu_molecule_energy_reset: zero the listed replicas' accumulators (None: all)."""
        self._accum_call("molecule_energy_reset", self._replica_list(replicas))

    def structure_factor(self, replica=0):
        a = np.zeros((self.nk, 2))
        check(self.L.mgpu_get_structure_factor(self.h, C.c_int(replica), _d(a)))
        return a[:, 0] + 1j * a[:, 1]

    def set_structure_factor(self, z, replica=0):
        a = np.ascontiguousarray(np.stack([np.real(z), np.imag(z)], axis=1), dtype=np.float64)
        check(self.L.mgpu_set_structure_factor(self.h, C.c_int(replica), _d(a)))

    # ---- batched candidates --------------------------------------------------------------
    def _cand(self, replica, t, m, sites):
        m = _ints(m)
        n = m.shape[0]
        replica = _ints(replica, n)
        t = _ints(t, n)
        if sites is not None:
            sites = np.ascontiguousarray(sites, dtype=np.float64)
            if sites.ndim == 2:
                sites = sites[None]
            assert sites.shape[0] == n and sites.shape[2] == 3
        return n, replica, t, m, sites

    def pair_energy_candidates(self, replica, t, m, sites=None, use_resident=None):
        n, replica, t, m, sites = self._cand(replica, t, m, sites)
        if use_resident is None:
            use_resident = np.full(n, 1 if sites is None else 0, dtype=np.int32)
        use_resident = _ints(use_resident, n)
        e_nc = np.zeros(n); e_c = np.zeros(n)
        stride = 1 if sites is None else sites.shape[1]
        check(self.L.mgpu_pair_energy_candidates(self.h, C.c_int(n), _i(replica), _i(t), _i(m), _i(use_resident),
                                                 _d(sites), C.c_int(stride), _d(e_nc), _d(e_c)))
        return e_nc, e_c

    def recip_energy_candidates(self, replica, t, m, kind, sites=None):
        n, replica, t, m, sites = self._cand(replica, t, m, sites)
        kind = _ints(kind, n)
        u = np.zeros(n)
        stride = 1 if sites is None else sites.shape[1]
        check(self.L.mgpu_recip_energy_candidates(self.h, C.c_int(n), _i(replica), _i(t), _i(m), _i(kind),
                                                  _d(sites), C.c_int(stride), _d(u)))
        return u

    def intra_energy_candidates(self, replica, t, m, sites=None, use_resident=None):
        n, replica, t, m, sites = self._cand(replica, t, m, sites)
        if use_resident is None:
            use_resident = np.full(n, 1 if sites is None else 0, dtype=np.int32)
        use_resident = _ints(use_resident, n)
        u = np.zeros(n)
        stride = 1 if sites is None else sites.shape[1]
        check(self.L.mgpu_intra_energy_candidates(self.h, C.c_int(n), _i(replica), _i(t), _i(m), _i(use_resident),
                                                  _d(sites), C.c_int(stride), _d(u)))
        return u

    def recip_form(self, n1_max, commit=False):
        """mgpu_recip_form: the form of the reciprocal update for molecules of up to n1_max sites, as a trial
        (commit=False) or a commit takes it -- dict(form= one of _lib.RECIP_FORMS, site_states= per LDS tile,
        rows_per_tile= of the XY table (0: none), site_tiles=)."""
        out = np.zeros(4, np.int32)
        check(self.L.mgpu_recip_form(self.h, C.c_int(int(n1_max)), C.c_int(_lib.RECIP_COMMIT if commit else _lib.RECIP_TRIAL), _i(out)))
        return dict(form=_lib.RECIP_FORMS[int(out[0])], site_states=int(out[1]), rows_per_tile=int(out[2]), site_tiles=int(out[3]))

    def pair_layout(self):
        """mgpu_pair_layout: dict(flat= pair_flat_kernel in use, groups= / planes= of the frozen layout its eligibility was
        judged on, frozen_batch= the residue type pair_frozen_kernel batches now (-1: none), site_major= per residue type:
        0 plane-major, 1 site-major, 2 frozen)."""
        out = np.zeros(_lib.PAIR_LAYOUT_LEN, np.int32)
        check(self.L.mgpu_pair_layout(self.h, _i(out)))
        return dict(flat=bool(out[0]), groups=int(out[1]), planes=int(out[2]), frozen_batch=int(out[3]),
                    site_major=[int(v) for v in out[4:4 + self.topo.n_res]])

    def self_energy(self, t):
        e = C.c_double()
        check(self.L.mgpu_self_energy(self.h, C.c_int(t), C.byref(e)))
        return e.value

    def trial_energy_candidates(self, replica, t, m, sites):
        n, replica, t, m, sites = self._cand(replica, t, m, sites)
        old = np.zeros((n, 3)); new = np.zeros((n, 3))
        check(self.L.mgpu_trial_energy_candidates(self.h, C.c_int(n), _i(replica), _i(t), _i(m), _d(sites),
                                                  C.c_int(sites.shape[1]), _d(old), _d(new)))
        return old, new

    def gcmc_trial(self, replica, t, m, kind, sites, lane=0):
        """Mixed batch (moves, creations, deletions): (old[n,5], new[n,5]) as ComputeOld/NewEnergy fill them."""
        n, replica, t, m, sites = self._cand(replica, t, m, sites)
        kind = _ints(kind, n)
        old = np.zeros((n, 5)); new = np.zeros((n, 5))
        self._last_stride = sites.shape[1]
        check(self.L.mgpu_gcmc_trial_submit(self.h, C.c_int(lane), C.c_int(n), _i(replica), _i(t), _i(m), _i(kind),
                                            _d(sites), C.c_int(sites.shape[1])))
        check(self.L.mgpu_gcmc_trial_wait(self.h, C.c_int(lane), _d(old), _d(new)))
        return old, new

    def chain_window_capacity(self):
        n = C.c_int(0)
        check(self.L.mgpu_chain_window_capacity(self.h, C.byref(n)))
        return n.value

    def chain_window(self, replica, t, m, kind, sites, accept_u, accept_pref, temperature, recip_energy, link=None):
        """mgpu_chain_window: one launch evaluates the window's steps (all trials of replica's current state), decides
        them in order and commits the first accepted one.  Returns (old[n,5], new[n,5], first_accepted, undecided)."""
        kind = np.ascontiguousarray(kind, dtype=np.int32)
        n = kind.shape[0]
        t = _ints(t, n); m = _ints(m, n)
        link = _ints(-1 if link is None else link, n)
        sites = np.ascontiguousarray(sites, dtype=np.float64)
        assert sites.ndim == 3 and sites.shape[0] == n and sites.shape[2] == 3
        u = np.ascontiguousarray(accept_u, dtype=np.float64); pref = np.ascontiguousarray(accept_pref, dtype=np.float64)
        assert u.shape == (n,) and pref.shape == (n,)
        old = np.zeros((n, 5)); new = np.zeros((n, 5))
        first = C.c_int(-1); und = C.c_int(-1)
        check(self.L.mgpu_chain_window(self.h, C.c_int(int(replica)), C.c_int(n), _i(t), _i(m), _i(kind), _i(link), _d(sites),
                                       C.c_int(sites.shape[1]), _d(u), _d(pref), C.c_double(temperature), C.c_double(recip_energy),
                                       _d(old), _d(new), C.byref(first), C.byref(und)))
        return old, new, first.value, und.value

    def chain_set_margin(self, rel):
        check(self.L.mgpu_chain_set_margin(self.h, C.c_double(rel)))

    def chain_set_wide(self, on=True):
        """mgpu_chain_set_wide: single-chain windows also take rigid molecules of 6 to 63 sites (off by default)."""
        check(self.L.mgpu_chain_set_wide(self.h, C.c_int(1 if on else 0)))

    def chain_set_wide_triclinic(self, on=True):
        """mgpu_chain_set_wide_triclinic: the single-chain one-launch paths (windows under chain_set_wide, runs under
        chain_run_set_wide) take rigid molecules of 6 to 63 sites in a triclinic box (off by default; farm windows never).
        Refused (MgpuError, the switch unchanged) for an orthorhombic box, while a run is open, and switched off while
        chain_run_set_wide is on."""
        check(self.L.mgpu_chain_set_wide_triclinic(self.h, C.c_int(1 if on else 0)))

    def chain_set_timing(self, on=True):
        check(self.L.mgpu_chain_set_timing(self.h, C.c_int(1 if on else 0)))

    def chain_timing(self):
        """Stage times (us) of the last window: see include/maniac_gpu.h."""
        us = np.zeros(15)
        check(self.L.mgpu_chain_get_timing(self.h, _d(us)))
        return us

    def chain_stats(self):
        w = C.c_longlong(0); u = C.c_longlong(0)
        check(self.L.mgpu_chain_get_stats(self.h, C.byref(w), C.byref(u)))
        return w.value, u.value

    def commit_lane(self, lane, replica, t, m, kind, accept, sites=None, sync=True):
        """mgpu_commit_submit (+ synchronize unless sync=False); sites=None reuses the rows of the lane's last trial."""
        n, replica, t, m, sites = self._cand(replica, t, m, sites)
        kind = _ints(kind, n)
        accept = _ints(accept, n)
        stride = self._last_stride if sites is None else sites.shape[1]
        check(self.L.mgpu_commit_submit(self.h, C.c_int(lane), C.c_int(n), _i(replica), _i(t), _i(m), _i(kind),
                                        _d(sites), C.c_int(stride), _i(accept)))
        if sync:
            self.synchronize()

    def commit_candidates(self, replica, t, m, kind, sites, accept):
        n, replica, t, m, sites = self._cand(replica, t, m, sites)
        kind = _ints(kind, n)
        accept = _ints(accept, n)
        stride = 1 if sites is None else sites.shape[1]
        check(self.L.mgpu_commit_candidates(self.h, C.c_int(n), _i(replica), _i(t), _i(m), _i(kind), _d(sites),
                                            C.c_int(stride), _i(accept)))

    # ---- reference-named B = 1 seams ------------------------------
    def ComputeSystemEnergy(self, replica=0):
        """energy_utils.f90:18-35"""
        return self.system_energy(replica)

    def ComputePairInteractionEnergy_singlemol(self, residue_type, molecule_index, sites=None, replica=0):
        """energy_utils.f90:374-442 -> (e_non_coulomb, e_coulomb)"""
        a, b = self.pair_energy_candidates(replica, residue_type, molecule_index, sites)
        return float(a[0]), float(b[0])

    def ComputeRecipEnergySingleMol(self, residue_type, molecule_index, sites=None, is_creation=False,
                                    is_deletion=False, replica=0):
        """ewald_energy.f90:191-274 (non-mutating: commit applies the update)"""
        kind = MGPU_CREATION if is_creation else (MGPU_DELETION if is_deletion else
                                                  (MGPU_NONE if sites is None else MGPU_MOVE))
        return float(self.recip_energy_candidates(replica, residue_type, molecule_index, kind, sites)[0])

    def ComputeEwaldSelfInteractionSingleMol(self, residue_type):
        """ewald_energy.f90:308-336"""
        return self.self_energy(residue_type)

    def ComputeIntraResidueRealCoulombEnergySingleMol(self, residue_type, molecule_index, sites=None, replica=0):
        """ewald_energy.f90:371-411"""
        return float(self.intra_energy_candidates(replica, residue_type, molecule_index, sites)[0])

    def set_triclinic_moves(self, on=True):
        """Device-built moves (move_trial, move_trial_decide) and farm windows in a triclinic box: off by default, and then
        refused / capacity 0 there.  Changes nothing for an orthorhombic engine."""
        check(self.L.mgpu_set_triclinic_moves(self.h, C.c_int(1 if on else 0)))

    def set_host_team(self, n_threads):
        """Host threads the candidate loops inside submit / wait / commit may use (mgpu_set_host_team)."""
        check(self.L.mgpu_set_host_team(self.h, C.c_int(int(n_threads))))

    def phase_factors(self, theta, k):
        """(cos, sin)(k * theta) as the device's phase tables hold them (mgpu_phase_factors; ewald_phase.f90:100-109)."""
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        k = np.ascontiguousarray(k, dtype=np.int32)
        n = theta.shape[0]
        c, s = np.empty(n), np.empty(n)
        check(self.L.mgpu_phase_factors(self.h, C.c_int(n), _d(theta), _i(k), _d(c), _d(s)))
        return c, s

    # ---- measurement ---------------------------------------------------------------------
    def synchronize(self):
        check(self.L.mgpu_synchronize(self.h))

    def profile_enable(self, on=True):
        check(self.L.mgpu_profile_enable(self.h, C.c_int(1 if on else 0)))

    def profile_reset(self):
        check(self.L.mgpu_profile_reset(self.h))

    def profile_get(self, kernel):
        n = C.c_longlong(); ms = C.c_double()
        check(self.L.mgpu_profile_get(self.h, C.c_int(kernel), C.byref(n), C.byref(ms)))
        return n.value, ms.value
