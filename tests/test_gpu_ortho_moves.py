"""Device-built moves in ORTHORHOMBIC cells held to the oracle bit for bit: the centres trial_frame builds (translation:
ApplyPBC of com + the ROUNDED displacement (u - 1/2) step; insertion: lo + the ROUNDED product L u) must be the oracle's doubles,
unrotated offsets the frames' own, rotated offsets the oracle's within tests/ortho_cases.py's K_ROT ulps of the two mixed
components.  Every path that holds an instance of the construction takes the same cases (tests/ortho_cases.py: two cells, a
1-site, a 3-site and a plane-major 6-site type): the batched build, farm windows with and without a reservoir on the engine,
for the small types and for the 6-site type, chain runs and grand-canonical chain runs, and a 200-step walk through farm
windows.  The oracle's ApplyPBC and RotationMatrix are pinned to the compiled reference by tests/test_oracle_pin.py.
Reference: src/translation.f90:93-112, src/geometry_utils.f90:167-220, src/monte_carlo_utils.f90:30-92,
src/create_molecule.f90:166-207, src/helper_utils.f90:39-77."""
import numpy as np
import pytest

from maniac_mc_amd._lib import MGPU_CREATION, MGPU_MOVE
from maniac_mc_amd.engine import Engine
from tests import ortho_cases as oc

gpu = pytest.mark.gpu

V_REJ, V_ACC, V_UND, V_IDLE = 0, 1, 2, 5
TWO_PI = 2.0 * np.pi
# path -> (residue types its cases use, the engine holds a reservoir on a replica of its own)
PATHS = {"batched": ((0, 1, 2), False),
         "window": ((0, 1), False),                 # farm_window_kernel's instances for <= 5 sites, RSV = false
         "window_rsv": ((0, 1), True),              #   ... RSV = true
         "window_wide": ((2,), False),              # the instances for 6 to 63 sites
         "window_wide_rsv": ((2,), True)}


def _caps(s):
    return [int(n) + 3 for n in s.n_mol]


def _active(s):
    return [t for t in range(s.topo.n_res) if s.topo.is_active[t]]


def _engine(s, starts, extra=0):
    """One replica per entry of starts = [(t, m, centre) or None] (+ `extra` more), each holding the cell with that one centre
    replaced, resident frames and a fresh A(k)."""
    n = len(starts)
    eng = Engine.from_system(s, n_replicas=n + extra, mol_capacity=_caps(s))
    for r in range(n + extra):
        if r:
            eng.replica_copy(r, 0)
        for tt in _active(s):
            com = s.com[tt].copy()
            if r < n and starts[r] is not None and starts[r][0] == tt:
                com[starts[r][1]] = starts[r][2]
            eng.set_frames(r, tt, com, s.offsets[tt])
        eng.init_structure_factor(r, True)
    return eng


def _step(eng, path, rep, t, m, move, u, ts, rs, T):
    """every candidate built on the device and accepted"""
    n = len(rep)
    if path == "batched":
        eng.move_trial(rep, t, m, move, u, ts, rs)
        eng.commit_lane(0, rep, t, m, np.where(move == 3, MGPU_CREATION, MGPU_MOVE).astype(np.int32), np.ones(n, np.int32))
    else:
        eng.farm_window_submit(rep, t, m, move, u, ts, rs, np.full(n, 0.5), np.ones(n), T, forced=np.ones(n, np.int32))
        _, _, v = eng.farm_window_wait(n)
        assert np.all(v == V_ACC), v


class Tally:
    """what differed from the oracle, counted over a test so that a failure reports how much, not only where first"""

    def __init__(self):
        self.n = {1: 0, 2: 0, 3: 0}
        self.bad_moves = {1: 0, 3: 0}
        self.bad_coords = {1: 0, 3: 0}
        self.first = {}
        self.ratio = 0.0
        self.rotated = 0

    def centre(self, mv, got, want, where):
        diff = int(np.sum(got != want))
        self.bad_moves[mv] += int(diff > 0)
        self.bad_coords[mv] += diff
        if diff and mv not in self.first:
            self.first[mv] = (where, got.tolist(), want.tolist())

    def report(self):
        return (f"translations: {self.bad_moves[1]} of {self.n[1]} centres ({self.bad_coords[1]} coordinates) differ from the "
                f"oracle; insertions: {self.bad_moves[3]} of {self.n[3]} ({self.bad_coords[3]} coordinates); first: {self.first}; "
                f"rotated offsets: {self.rotated} molecules, largest |d| / (2^-52 (|x| + |y|)) = {self.ratio:.3f}")


def _check(s, P, tally, eng, rep, t, m, move, u, before, ts, rs, tag):
    """The frames read back against the oracle's composition of the same move from the frames read before it."""
    for c in range(len(rep)):
        r, tt, mm, mv = int(rep[c]), int(t[c]), int(m[c]), int(move[c])
        n1 = int(s.topo.atoms_in_res[tt])
        com_b, off_b = before[c]
        com_a, off_a = eng.get_frames(r, tt)
        where = (tag, c, tt, mm)
        tally.n[mv] += 1
        slot, n_b = mm, com_b.shape[0]
        if mv == 1:
            tally.centre(1, com_a[mm], oc.translated(s, P, com_b[mm], u[c], ts), where)
            assert np.array_equal(off_a[mm], off_b[mm]), where                  # the offsets come back unchanged, bit for bit
        elif mv == 2:
            assert np.array_equal(com_a[mm], com_b[mm]), where                  # a rotation keeps its centre bit for bit
            theta, off0 = (u[c, 3] - 0.5) * rs, off_b[mm]
        else:
            slot = n_b
            assert com_a.shape[0] == n_b + 1, where
            tally.centre(3, com_a[slot], oc.inserted(s, u[c]), where)
            theta, off0 = u[c, 3] * TWO_PI, off_b[0]                            # molecule 1 of the type (create_molecule.f90:197-199)
        if mv != 1:
            if theta == 0.0 or (mv == 3 and n1 == 1):                           # cs = 1, sn = 0, or no rotation at all
                assert np.array_equal(off_a[slot], off0), where
            else:
                axis = oc.axis_of(u[c, 4])
                ratio, third = oc.rotation_ratio(off_a[slot], oc.rotated(P, off0, axis, theta), off0, axis)
                assert third, where
                tally.ratio = max(tally.ratio, ratio)
                tally.rotated += 1
        assert np.array_equal(eng.get_molecules(r, tt)[slot], com_a[slot][None, :] + off_a[slot]), where   # sites = com + off
        rest = np.arange(n_b) != mm if mv != 3 else np.ones(n_b, bool)
        assert np.array_equal(com_a[:n_b][rest], com_b[rest]) and np.array_equal(off_a[:n_b][rest], off_b[rest]), where


# ---------------------------------------------------------------------------------------------------------------------
# 0. the cases can see the fault (no GPU)
@pytest.mark.parametrize("name", oc.CELLS)
def test_the_cases_are_what_they_claim(name, refcpu_mod):
    """On the CPU: what one fused multiply-add per axis would give (exact rational arithmetic, rounded once) differs from the
    reference's rounded-product-then-sum on at least 10 translated coordinates of each cell and on at least 10 inserted
    coordinates of the cell whose bounds_lo is not zero.  In the cubic cell bounds_lo = 0 and an insertion's centre is
    0 + L u: the sum is exact and round(L u + 0) == round(L u) + 0 for every u, so NO inserted coordinate of that cell can
    tell the two apart -- asserted as such; its translations can.  The start centres lie where they are said to lie, and the
    plain-Python wrap used for the fused variant is the oracle's ApplyPBC on these inputs."""
    s = oc.cell(name)
    P = refcpu_mod.RefCPU(s, mol_capacity=max(_caps(s)))
    lo, L = s.bounds_lo, oc.edges(s)
    step = oc.t_step(s)
    recs = oc.first_round(s)
    assert len(recs) <= 160
    n_tr = n_in = far = zero_disp = on_top = below = 0
    for t, m, mv, u, start in recs:
        assert 0.0 <= u.min() and u.max() < 1.0
        if mv == 1:
            com0 = s.com[t][m] if start is None else start
            target = com0 + (u[:3] - 0.5) * step
            unfused = oc.wrap_stated(s, target)
            assert np.array_equal(unfused, P.apply_pbc(target))
            assert np.array_equal(unfused, oc.translated(s, P, com0, u, step))
            n_tr += int(np.sum(unfused != oc.translated_fused(s, com0, u, step)))
            far += int(np.max(np.abs(com0 - (lo + 0.5 * L))) > 100.0)
            if np.all(u[:3] == 0.5):
                zero_disp += 1
                assert np.array_equal(target, com0)
                on_top += int(np.sum((target - lo == L) & (unfused == lo)))                         # x == L wraps to lo
                below += int(np.sum((target < lo) & (target - lo > -1e-9) & (unfused == lo + L)))   # x just below 0: lo + L
        elif mv == 3:
            n_in += int(np.sum(oc.inserted(s, u) != oc.inserted_fused(s, u)))
    print(f"[{name}] a fused multiply-add would move {n_tr} translated and {n_in} inserted coordinates of the first round")
    assert n_tr >= 10
    if np.all(lo == 0.0):
        assert n_in == 0
    else:
        assert n_in >= 10
    assert far >= 6 and zero_disp >= 12 and on_top >= 1 and below >= 3
    assert step > 2.0 * L.max()
    axes = [oc.axis_of(x) for x in oc.axis_draws()]
    # 1/3 and 2/3 as doubles lie BELOW the thirds, yet 3.0 * u rounds up to 1.0 and 2.0: they select the next axis, their lower
    # neighbours the axis before
    assert axes == [1, 2, 1, 2, 3, 2, 3, 3]


# ---------------------------------------------------------------------------------------------------------------------
# 1. geometry, path by path
@gpu
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", oc.CELLS)
def test_device_built_geometry_is_the_oracles_bit_for_bit(name, path, refcpu_mod):
    """tests/ortho_cases.py's first round (centres on and beside the faces, far outside, draws at the ends of [0, 1), zero
    angles, axes at the thirds) and then rounds of ordinary translations from wherever the round before left the molecules (300
    or more, from inside the cell), every candidate accepted: centres np.array_equal to the oracle's, unrotated offsets
    unchanged, rotated ones within K_ROT.  A window path takes the records of its own residue types only (a window with a
    6-site record launches the instance for 6 to 63 sites, one without the instance for up to 5); with `_rsv` a replica that
    takes no record holds a reservoir, so every launch is the engine-with-reservoirs instance and builds the same geometry.
    K_ROT = 2: the largest ratio measured on an MI355X over this file and tests/test_gpu_gcmc.py is 0.702 (a 6-site molecule
    of the batched and the wide-window cases; 0.527 for the 3-site type, 0.538 in the grand-canonical runs)."""
    types, rsv = PATHS[path]
    s = oc.cell(name)
    P = refcpu_mod.RefCPU(s, mol_capacity=max(_caps(s)))
    recs = [rc for rc in oc.first_round(s) if rc[0] in types]
    n = len(recs)
    eng = _engine(s, [None if rc[4] is None else (rc[0], rc[1], rc[4]) for rc in recs], extra=int(rsv))
    if rsv:
        eng.set_reservoir(n, 1, s.offsets[1][:2])
    if path != "batched":
        assert eng.farm_window_capacity()[0] >= n
    ts, T = oc.t_step(s), float(s.temperature)
    rng = np.random.default_rng(3)
    rep = np.arange(n, dtype=np.int32)
    tally = Tally()
    for rnd in range(1 + -(-300 // n)):                       # the later rounds hold at least 300 ordinary translations
        if rnd == 0:
            t = np.array([rc[0] for rc in recs], np.int32)
            m = np.array([rc[1] for rc in recs], np.int32)
            move = np.array([rc[2] for rc in recs], np.int32)
            u = np.array([rc[3] for rc in recs])
        else:
            t = rng.choice(types, n).astype(np.int32)
            m = np.array([rng.integers(0, oc.N_MOL[tt]) for tt in t], np.int32)
            move = np.ones(n, np.int32)
            u = rng.random((n, 5))
        before = [eng.get_frames(int(rep[c]), int(t[c])) for c in range(n)]
        _step(eng, path, rep, t, m, move, u, ts, oc.R_STEP, T)
        _check(s, P, tally, eng, rep, t, m, move, u, before, ts, oc.R_STEP, rnd)
    print(f"[{name} {path}] {tally.report()}")
    assert tally.bad_moves == {1: 0, 3: 0}, tally.report()
    assert tally.ratio <= oc.K_ROT, tally.report()
    assert tally.n[1] >= 300 + 20
    if len(types) == 3:
        assert tally.n[1] >= 300 + 72 and tally.n[2] >= 20 and tally.n[3] >= 36 and tally.rotated >= 30
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. chain runs
def _admitted(s, com, off, rng, t, m, move, make, d_min=2.4):
    """Draws for one step that leave every site at least d_min from every other molecule's: the step's probability is then
    positive, and a draw of accept_u = 0 is accepted (never undecided: that needs the probability to underflow)."""
    for _ in range(200):
        u = rng.random(5)
        c, o = make(u)
        if oc.closest_approach(s, com, off, t, m if move != 3 else None, c[None, :] + o) >= d_min:
            return u, c, o
    raise AssertionError("no admissible step found")


def _collect(eng, n):
    vs = []
    while len(vs) < n:
        _, _, v, st = eng.chain_run_collect(n - len(vs), wait=True)
        assert st == -1 and len(v) > 0, (st, v)
        vs.extend(int(x) for x in v)
    return vs


@gpu
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("name", oc.CELLS)
def test_a_chain_run_of_translations_is_the_oracles_walk(name, wide, refcpu_mod):
    """24 translations of a few molecules pushed into one run (k = 4), accept_u = 0 and steps that leave no overlap, so the
    rule accepts each: the frames after the run are the oracle's composition applied 24 times, np.array_equal.  narrow: the
    6-site type inactive, chain_run_kernel's instance for <= 5 sites; wide: chain_run_set_wide, all three types."""
    s = oc.cell(name, wide_active=wide)
    P = refcpu_mod.RefCPU(s, mol_capacity=max(_caps(s)))
    eng = _engine(s, [None])
    if wide:
        eng.chain_run_set_wide(True)
    max_k, depth, ring = eng.chain_run_capacity()
    assert max_k >= 4 and depth >= 24 and ring >= 24
    types = _active(s)
    ts, T = oc.t_step(s), float(s.temperature)
    rng = np.random.default_rng(19)
    n = 24
    com = [c.copy() for c in s.com]
    off = [o.copy() for o in s.offsets]
    t = rng.choice(types, n).astype(np.int32)
    m = rng.integers(0, 2, n).astype(np.int32)
    u = np.zeros((n, 5))
    for i in range(n):
        tt, mm = int(t[i]), int(m[i])
        u[i], c, _ = _admitted(s, com, off, rng, tt, mm, 1, lambda x: (oc.translated(s, P, com[tt][mm], x, ts), off[tt][mm]))
        com[tt][mm] = c
    eng.chain_run_open(0, 4, ts, oc.R_STEP, T)
    eng.chain_run_push(t, m, np.ones(n, np.int32), u, np.zeros(n))
    for _ in range(8):
        eng.chain_run_launch(3)
    v = _collect(eng, n)
    eng.chain_run_close()
    assert v == [V_ACC] * n, v
    bad = 0
    for tt in types:
        com_d, off_d = eng.get_frames(0, tt)
        bad += int(np.sum(com_d != com[tt]))
        assert np.array_equal(off_d, off[tt]), tt
        assert np.array_equal(eng.get_molecules(0, tt), com_d[:, None, :] + off_d), tt
    assert bad == 0, f"{bad} centre coordinates differ from the oracle's walk"
    eng.close()


@gpu
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("name", oc.CELLS)
def test_a_grand_canonical_run_inserts_at_the_oracles_centres(name, wide, refcpu_mod):
    """Insertions by count through chain_run_push_gc (accept_u = 0, no overlap): the device completes each record from the
    count it finds and appends the molecule; its centre is lo + L u with the product rounded before the sum, np.array_equal;
    u[3] = 0 leaves molecule 1's offsets bit for bit, any other angle within K_ROT."""
    s = oc.cell(name, wide_active=wide)
    P = refcpu_mod.RefCPU(s, mol_capacity=max(_caps(s)))
    eng = _engine(s, [None])
    if wide:
        eng.chain_run_set_wide(True)
    eng.chain_run_set_gc(True)
    assert eng.chain_run_capacity()[0] >= 4
    types = _active(s)
    T = float(s.temperature)
    rng = np.random.default_rng(29)
    com = [c.copy() for c in s.com]
    off = [o.copy() for o in s.offsets]
    t = np.repeat(types, 2).astype(np.int32)
    n = len(t)
    u = np.zeros((n, 5))
    thetas = []
    for i in range(n):
        tt = int(t[i])
        n1 = int(s.topo.atoms_in_res[tt])

        def make(x, tt=tt, n1=n1, plain=(i % 2 == 0)):
            if plain:
                x[3] = 0.0
            o = off[tt][0] if n1 == 1 or x[3] == 0.0 else oc.rotated(P, off[tt][0], oc.axis_of(x[4]), x[3] * TWO_PI)
            return oc.inserted(s, x), o
        u[i], c, o = _admitted(s, com, off, rng, tt, None, 3, make)
        com[tt] = np.vstack([com[tt], c])
        off[tt] = np.concatenate([off[tt], o[None]])
        thetas.append(u[i, 3] * TWO_PI)
    eng.chain_run_open(0, 4, 1.0, oc.R_STEP, T)
    eng.chain_run_push_gc(t, np.full(n, 3, np.int32), u, np.zeros(n), rng.random(n), np.full(n, 50.0))
    for _ in range(n):
        eng.chain_run_launch(1)
    v = _collect(eng, n)
    eng.chain_run_close()
    assert v == [V_ACC] * n, v
    bad, worst = 0, 0.0
    for tt in types:
        com_d, off_d = eng.get_frames(0, tt)
        n0 = int(s.n_mol[tt])
        assert com_d.shape[0] == n0 + 2
        assert np.array_equal(com_d[:n0], s.com[tt]) and np.array_equal(off_d[:n0], s.offsets[tt])
        bad += int(np.sum(com_d[n0:] != com[tt][n0:]))
        for j in range(2):
            i = int(np.flatnonzero(t == tt)[j])
            if thetas[i] == 0.0 or off_d.shape[1] == 1:
                assert np.array_equal(off_d[n0 + j], s.offsets[tt][0]), (tt, j)
            else:
                axis = oc.axis_of(u[i, 4])
                ratio, third = oc.rotation_ratio(off_d[n0 + j], off[tt][n0 + j], s.offsets[tt][0], axis)
                assert third
                worst = max(worst, ratio)
        assert np.array_equal(eng.get_molecules(0, tt), com_d[:, None, :] + off_d), tt
    print(f"[{name} gc run {'wide' if wide else 'narrow'}] rotated offsets: largest ratio {worst:.3f}")
    assert bad == 0, f"{bad} of {3 * n} inserted centre coordinates differ from lo + L u"
    assert worst <= oc.K_ROT
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. a walk
@gpu
@pytest.mark.parametrize("name", oc.CELLS)
def test_a_walk_of_200_forced_translations_stays_on_the_oracles(name, refcpu_mod):
    """One 1-site particle, 200 forced translations through farm windows with a step of 0.8 max(L): after every step the
    centre read back equals the oracle's walk (its own composition from the start, not from the device's last value)."""
    s = oc.cell(name)
    P = refcpu_mod.RefCPU(s, mol_capacity=max(_caps(s)))
    eng = _engine(s, [None])
    assert eng.farm_window_capacity()[0] >= 1
    ts, T = 0.8 * float(np.max(oc.edges(s))), float(s.temperature)
    rng = np.random.default_rng(13)
    com = s.com[0][3].copy()
    first_bad, crossed = None, 0
    for i in range(200):
        u = rng.random((1, 5))
        raw = com + (u[0, :3] - 0.5) * ts
        crossed += int(np.any((raw < s.bounds_lo) | (raw >= s.bounds_lo + oc.edges(s))))
        com = oc.translated(s, P, com, u[0], ts)
        _step(eng, "window", [0], [0], [3], np.array([1], np.int32), u, ts, oc.R_STEP, T)
        if first_bad is None and not np.array_equal(eng.get_frames(0, 0)[0][3], com):
            first_bad = i
    assert first_bad is None, f"the walk left the oracle's at step {first_bad}"
    assert crossed >= 50
    assert np.array_equal(eng.get_frames(0, 0)[0][np.arange(oc.N_MOL[0]) != 3], s.com[0][np.arange(oc.N_MOL[0]) != 3])
    eng.close()
