"""What the three one-launch paths admit (mgpu_chain_window, mgpu_farm_window_*, mgpu_chain_run_*; DESIGN sections 4.3, 4.4):
the capacities they report for a table of small engines, and the FIRST refusal -- status code and text -- of calls that break
two rules at once.  The expected values are literals recorded from the build before the admission rules were gathered into
one table and one function (window_types_build, window_admission in csrc/mgpu_windows.hip): they pin that the rules did not
move.  Then two engines in one process whose WIDE single-chain windows opt in to different amounts of dynamic LDS beyond
64 KiB, run in turn: the opt-in belongs to the kernel function, not to an engine."""
import numpy as np
import pytest

from maniac_mc_amd import synth
from maniac_mc_amd._lib import MGPU_MOVE, MgpuError
from maniac_mc_amd.engine import Engine
from tests import triclinic_cases
from tests.test_gpu_chain_wide import _same_state, _twin, _window
from tests.test_gpu_farm_window_wide import _env, _shell, _system, _water
from tests.test_gpu_topology_edges import _engine, _four_types

pytestmark = pytest.mark.gpu

R = 2


def _triple(e):
    return (e.chain_window_capacity(), e.farm_window_capacity()[0], e.chain_run_capacity()[0])


def observed_capacities():
    """[(label, (chain_window_capacity, farm_window_capacity()[0], chain_run_capacity()[0]))]"""
    out = []
    e = Engine.from_system(synth.spce_box(5), n_replicas=R)
    out.append(("spce5", _triple(e)))
    e.close()
    ads = synth.rigid_adsorbate_box(n_mol=6, n_sites=24, L=26.0)
    for label, env in (("ads24", {}), ("ads24 no-mfma", {"MGPU_RECIP_NO_MFMA": "1"}), ("ads24 per-k", {"MGPU_RECIP_PER_K": "1"})):
        with _env(**env):
            e = Engine.from_system(ads, n_replicas=R)
        out.append((label, _triple(e)))
        e.chain_set_wide(True)
        out.append((label + " wide", _triple(e)))
        e.close()
    for name in triclinic_cases.CELLS:
        s = triclinic_cases.cell(name)
        e = Engine.from_system(s, n_replicas=R)
        out.append((name, _triple(e)))
        e.set_triclinic_moves(True)
        out.append((name + " moves", _triple(e)))
        e.chain_run_set_triclinic(True)
        out.append((name + " moves runs", _triple(e)))
        e.close()
    s = synth.spce_box(5)
    e = Engine.from_system(s, n_replicas=R)
    e.set_reservoir(0, 0, s.offsets[0][:2].copy())
    out.append(("spce5 reservoir", _triple(e)))
    e.close()
    s64, c64 = _four_types(True)
    e = _engine(s64, {}, c64, R=R)
    out.append(("four types + active 64-site type", _triple(e)))
    e.close()
    e = Engine.from_system(synth.framework_water_box(n_water=8), n_replicas=R)
    out.append(("framework + 8 water", _triple(e)))
    e.close()
    return out


# recorded from the build before the change (see the module's docstring)
CAPACITIES = [
    ('spce5', (16, 2, 16)),
    ('ads24', (0, 2, 0)),
    ('ads24 wide', (16, 2, 0)),
    ('ads24 no-mfma', (0, 2, 0)),
    ('ads24 no-mfma wide', (16, 2, 0)),
    ('ads24 per-k', (0, 0, 0)),
    ('ads24 per-k wide', (0, 0, 0)),
    ('mild', (16, 0, 0)),
    ('mild moves', (16, 2, 0)),
    ('mild moves runs', (16, 2, 16)),
    ('sheared', (16, 0, 0)),
    ('sheared moves', (16, 2, 0)),
    ('sheared moves runs', (16, 2, 16)),
    ('spce5 reservoir', (16, 2, 0)),
    ('four types + active 64-site type', (0, 0, 0)),
    ('framework + 8 water', (16, 2, 16)),
]


def test_capacities_are_the_recorded_ones():
    got = observed_capacities()
    for row in got:
        print(row)
    assert got == CAPACITIES


def _refusal(call):
    try:
        call()
    except MgpuError as err:
        return (err.code, str(err))
    return (0, "no refusal")


def observed_refusals():
    """[(label, (status code, text))]: every call breaks two rules; the entry point reports the one it tests first"""
    out = []
    s = synth.spce_box(5)
    e = Engine.from_system(s, n_replicas=R)
    e.init_structure_factor(0, True)
    T = float(s.temperature)
    row = e.get_molecules(0, 0)[:1].copy()
    rows17 = np.repeat(row, 17, axis=0)
    # ---- chain_window
    out.append(("chain_window: window size and replica out of range", _refusal(
        lambda: e.chain_window(5, [0] * 17, [0] * 17, [MGPU_MOVE] * 17, rows17, [0.5] * 17, [1.0] * 17, T, 0.0))))
    out.append(("chain_window: unknown kind and residue type out of range", _refusal(
        lambda: e.chain_window(0, [9], [0], [7], row, [0.5], [1.0], T, 0.0))))
    out.append(("chain_window: molecule beyond the site stride and a bad link", _refusal(
        lambda: e.chain_window(0, [0], [0], [MGPU_MOVE], row[:, :2], [0.5], [1.0], T, 0.0, link=[5]))))
    # (water and an INACTIVE 24-site type: what a record of that type meets is the path's own rule for the type)
    sm = _system(np.diag([36.0, 36.0, 36.0]), [(*_water(), 10), (*_shell(24, seed=21), 3)], active=[1, 0], seed=21)
    mix = Engine.from_system(sm, n_replicas=R, mol_capacity=[12, 5])
    wide_row = mix.get_molecules(0, 1)[:1].copy()
    out.append(("chain_window: a row of 24 sites with wide windows off and a bad link", _refusal(
        lambda: mix.chain_window(0, [1], [0], [MGPU_MOVE], wide_row, [0.5], [1.0], T, 0.0, link=[5]))))
    mix.chain_set_wide(True)
    out.append(("chain_window: the same row with wide windows on", _refusal(
        lambda: mix.chain_window(0, [1], [0], [MGPU_MOVE], wide_row, [0.5], [1.0], T, 0.0, link=[5]))))
    # ---- farm_window_submit
    u5 = np.full((3, 5), 0.5)
    out.append(("farm_window_submit: unknown move code and replica out of range", _refusal(
        lambda: e.farm_window_submit([7], [0], [0], [9], u5[:1], 0.5, 0.5, [0.5], [1.0], T))))
    out.append(("farm_window_submit: too many chains and a temperature of zero", _refusal(
        lambda: e.farm_window_submit([0, 1, 0], [0] * 3, [0] * 3, [1] * 3, u5, 0.5, 0.5, [0.5] * 3, [1.0] * 3, 0.0))))
    fw = Engine.from_system(synth.framework_water_box(n_water=8), n_replicas=R)
    out.append(("farm_window_submit: a type windows do not take and no frames", _refusal(
        lambda: fw.farm_window_submit([0], [0], [0], [1], u5[:1], 0.5, 0.5, [0.5], [1.0], T))))
    fw.close()
    # ---- chain_run_open
    out.append(("chain_run_open: replica and steps per launch out of range", _refusal(lambda: e.chain_run_open(5, 99, 0.5, 0.5, T))))
    out.append(("chain_run_open: steps per launch out of range and a temperature of zero", _refusal(lambda: e.chain_run_open(0, 99, 0.5, 0.5, 0.0))))
    out.append(("chain_run_open: a temperature of zero and no frames", _refusal(lambda: e.chain_run_open(0, 4, 0.5, 0.5, 0.0))))
    rs = Engine.from_system(s, n_replicas=R)
    rs.set_reservoir(0, 0, s.offsets[0][:2].copy())
    out.append(("chain_run_open: reservoirs and replica out of range", _refusal(lambda: rs.chain_run_open(5, 4, 0.5, 0.5, T))))
    rs.close()
    # ---- chain_run_push (a run open, nothing launched)
    e.set_frames(0, 0, s.com[0], s.offsets[0])
    e.chain_run_open(0, 4, 0.5, 0.5, T)
    out.append(("chain_run_push: an insertion and residue type out of range", _refusal(lambda: e.chain_run_push([9], [0], [3], u5[:1], [0.5]))))
    out.append(("chain_run_push: unknown move code and residue type out of range", _refusal(lambda: e.chain_run_push([9], [0], [7], u5[:1], [0.5]))))
    out.append(("chain_run_push: residue type and molecule out of range", _refusal(lambda: e.chain_run_push([5], [99999], [1], u5[:1], [0.5]))))
    out.append(("chain_run_push: beyond the ring and an insertion", _refusal(
        lambda: e.chain_run_push([0] * 5000, [0] * 5000, [3] * 5000, np.full((5000, 5), 0.5), [0.5] * 5000))))
    e.chain_run_close()
    e.close()
    mix.set_frames(0, 0, sm.com[0], sm.offsets[0])
    mix.chain_run_open(0, 4, 0.5, 0.5, T)
    out.append(("chain_run_push: an inactive type and molecule out of range", _refusal(lambda: mix.chain_run_push([1], [99999], [1], u5[:1], [0.5]))))
    mix.chain_run_close()
    mix.close()
    return out


# recorded from the build before the change (see the module's docstring)
REFUSALS = [
    ('chain_window: window size and replica out of range', (1, 'maniac_gpu error 1: chain_window: window size out of range')),
    ('chain_window: unknown kind and residue type out of range', (1, 'maniac_gpu error 1: chain_window: unknown candidate kind')),
    ('chain_window: molecule beyond the site stride and a bad link',
     (1, 'maniac_gpu error 1: chain_window: molecule too large for the one-launch path')),
    ('chain_window: a row of 24 sites with wide windows off and a bad link',
     (1, 'maniac_gpu error 1: chain_window: molecule too large for the one-launch path')),
    ('chain_window: the same row with wide windows on', (1, 'maniac_gpu error 1: chain_window: bad link')),
    ('farm_window_submit: unknown move code and replica out of range', (1, 'maniac_gpu error 1: farm_window_submit: unknown move code')),
    ('farm_window_submit: too many chains and a temperature of zero', (1, 'maniac_gpu error 1: farm_window_submit: number of chains out of range')),
    ('farm_window_submit: a type windows do not take and no frames',
     (1, 'maniac_gpu error 1: farm_window_submit: molecule too large for the one-launch path')),
    ('chain_run_open: replica and steps per launch out of range', (1, 'maniac_gpu error 1: chain_run_open: replica out of range')),
    ('chain_run_open: steps per launch out of range and a temperature of zero',
     (1, 'maniac_gpu error 1: chain_run_open: steps per launch out of range')),
    ('chain_run_open: a temperature of zero and no frames', (1, 'maniac_gpu error 1: chain_run_open: temperature must be positive')),
    ('chain_run_open: reservoirs and replica out of range',
     (5, 'maniac_gpu error 5: chain_run_open: not available for this engine (mgpu_chain_run_capacity)')),
    ('chain_run_push: an insertion and residue type out of range',
     (1, 'maniac_gpu error 1: chain_run_push: insertions and deletions do not ride in a run (moves only)')),
    ('chain_run_push: unknown move code and residue type out of range', (1, 'maniac_gpu error 1: chain_run_push: unknown move code')),
    ('chain_run_push: residue type and molecule out of range', (1, 'maniac_gpu error 1: chain_run_push: residue type out of range or not active')),
    ('chain_run_push: beyond the ring and an insertion',
     (1, 'maniac_gpu error 1: chain_run_push: beyond the ring (steps pushed and not yet collected: mgpu_chain_run_capacity)')),
    ('chain_run_push: an inactive type and molecule out of range',
     (1, 'maniac_gpu error 1: chain_run_push: residue type out of range or not active')),
]


def test_first_refusals_are_the_recorded_ones():
    got = observed_refusals()
    for row in got:
        print(row)
    assert got == REFUSALS


def test_two_engines_with_different_wide_lds_in_one_process():
    """MGPU_RECIP_NO_MFMA=1: 24- and 32-site molecules in the 26 A box take the vector wide form; the WIDE single-chain window's
    k role then needs 66 688 bytes of dynamic LDS for 24 sites and 66 560 for 32 (kmax 7 7 7, 82 rows, a 33 840-byte Coulomb
    table) -- both beyond 64 KiB, the first engine's the larger (asserted below from each engine's kmax and tile; the pair role,
    the table + 21.5 KiB, is the same for both and smaller).  A window on the first engine, one on the second, one on the
    first again: energies, first_accepted and the state afterwards are a twin engine's on the batched path every time."""
    pairs, k_lds = [], []
    for n_sites in (24, 32):
        s = synth.rigid_adsorbate_box(n_mol=6, n_sites=n_sites, L=26.0, seed=17)
        A, B = _twin(s, [8], env={"MGPU_RECIP_NO_MFMA": "1"})
        assert A.recip_form(n_sites)["form"] == "wide-vector" and B.recip_form(n_sites)["form"] == "wide-vector"
        assert A.chain_window_capacity() >= 2
        # the k role's dynamic LDS from the engine's own form (window_k_lds_bytes over recip_wide_lds_bytes, csrc/mgpu_internal.h):
        # candidate row | two intra tiles | 1-D tables | XY tile | charges
        f, ktot = A.recip_form(n_sites), int(np.sum(A.kmax)) + 3
        nss, rpt = f["site_states"], f["rows_per_tile"]
        k_lds.append(64 * 3 * 8 + 2 * 64 * 32 + nss * ktot * 16 + rpt * nss * 16 + nss * 8)
        pairs.append((s, A, B))
    print("k role LDS", k_lds)
    assert k_lds[0] > k_lds[1] > 64 * 1024, k_lds          # both opt in, and the second engine asks for less than the first
    rng = np.random.default_rng(29)
    kinds = np.full(2, MGPU_MOVE, np.int32)
    zeros = np.zeros(2, np.int32)
    for i in (0, 1, 0):
        s, A, B = pairs[i]
        t, m, sites = _window(rng, B, s, [0], kinds, 0)
        u, pref = np.array([0.999999, 0.0]), np.array([1e-200, 1.0])       # step 0 rejected, step 1 accepted
        e_recip = B.system_energy(0)["recip_coulomb"]
        old_b, new_b = B.gcmc_trial(zeros, t, m, kinds, sites)
        old_a, new_a, first, und = A.chain_window(0, t, m, kinds, sites, u, pref, float(s.temperature), e_recip)
        assert (first, und) == (1, -1)
        assert np.array_equal(old_a, old_b) and np.array_equal(new_a, new_b)
        B.commit_lane(0, zeros, t, m, kinds, np.array([0, 1], np.int32))
        _same_state(A, B, s.topo.n_res)
    for _, A, B in pairs:
        A.close(); B.close()
