"""The layers above the engine on a TRICLINIC box with rigid molecules of 6 to 63 sites: the Fortran farm (mc_farm.f90 through
FortranFarm(wide_triclinic=True): window mode, which such a farm did not have) against its device mode -- the batched device-built
steps -- on the tilted 24-site box and the 3 + 24 mixture of tests/test_gpu_chain_wide_triclinic.py, NVT and grand-canonical, with
tests/test_gpu_triclinic_moves.py's farm invariants and the same energies, counters and frames bit for bit; and replica runs
(run_replicas(wide_triclinic=True)) of the committed inputs tests/golden/runs_wide_triclinic/{cage6_tri_nvt, cage24_tri_gcmc}: mode
`windows` runs as windows and writes the bytes mode `device` writes (tests/test_gpu_replicas.py's comparison); without the flag it
raises the ValueError it always raised."""
import os

import numpy as np
import pytest

from maniac_mc_amd.replicas import run_replicas
from tests.test_gpu_chain_wide_triclinic import print_redraws, tri_box  # noqa: F401  (print_redraws: autouse fixture)
from tests.test_gpu_replicas import _tree, _without_dir
from tests.test_gpu_triclinic_moves import _farm, _farm_invariants, _farm_state
from tests.util import GOLDEN

pytestmark = pytest.mark.gpu

TRI = os.path.join(GOLDEN, "runs_wide_triclinic")


@pytest.mark.parametrize("gcmc", [False, True], ids=["nvt", "gcmc"])
@pytest.mark.parametrize("cell", ["mild", "sheared"])
@pytest.mark.parametrize("name", ["24", "3+24"])
def test_fortran_farm_window_mode_is_its_device_mode(name, cell, gcmc):
    """device mode and window mode from one seed: both keep the farm's invariants (running energies against a from-scratch
    evaluation, A(k) against a fresh S(k), the farm's molecules against the device's) and are equal BIT FOR BIT in trial counts,
    molecule counts, energies, coordinates and A(k).  Window mode asked for without wide_triclinic stays on the batched path."""
    s, _, cap = tri_box(name, cell)
    R, steps = 6, 60
    kw = {}
    if gcmc:
        V = abs(float(np.linalg.det(s.box_matrix)))
        kw = dict(mol_capacity=cap, gcmc=dict(p_translation=0.25, p_rotation=0.25, fugacity=2.0 * np.array([float(n) for n in s.n_mol]) / V))
    states, trials = {}, {}
    for mode, mk in (("device", dict(device_build=True)), ("window", dict(device_build=True, window=True, wide_triclinic=True)),
                     ("window asked for, switch off", dict(device_build=True, window=True))):
        farm = _farm(s, R, steps, **mk, **kw)
        assert farm.device_build and not farm.device_accept
        assert farm.window == (mode == "window"), mode
        assert farm.wide_triclinic == (mode == "window")
        _farm_invariants(farm, R, steps)
        states[mode] = _farm_state(farm, R)
        trials[mode] = (farm.trials, farm.skipped, farm.accepted, farm.counts().copy(), farm.counters())
        if mode == "window":
            windows, in_flight, left = farm.window_mode()
            assert windows and in_flight >= 1
            print(f"[{name} {cell} {'gcmc' if gcmc else 'nvt'}] windows: accepted {farm.accepted} of {farm.trials}, left to the driver {left}")
        farm.close()
    for other in ("window", "window asked for, switch off"):
        assert trials["device"][:3] == trials[other][:3] and np.array_equal(trials["device"][3], trials[other][3]), other
        assert trials["device"][4] == trials[other][4], other
        (e_d, x_d, A_d), (e_w, x_w, A_w) = states["device"], states[other]
        for r in range(R):
            assert np.array_equal(e_d[r], e_w[r]) and np.array_equal(A_d[r], A_w[r]), (other, r)
            assert all(np.array_equal(p, q) for p, q in zip(x_d[r], x_w[r])), (other, r)


def _run(case, out, **kw):
    d = os.path.join(TRI, case, "inputs")
    return run_replicas(os.path.join(d, "system.maniac"), os.path.join(d, "system.data"), os.path.join(d, "system.inc"), str(out), **kw)


@pytest.mark.parametrize("case", ["cage6_tri_nvt", "cage24_tri_gcmc"])
def test_replica_runs_in_windows_mode_write_the_bytes_of_device_mode(case, tmp_path):
    kw = dict(replicas=4, seed=7, nb_block=3, nb_step=40, frames=(0, 2))
    trees = {}
    for mode, extra in (("windows", dict(wide_triclinic=True)), ("device", {})):
        res = _run(case, tmp_path / mode, mode=mode, **extra, **kw)
        assert res["mode"] == mode, res["mode"]
        assert res["accepted"] > 0
        trees[mode] = _tree(tmp_path / mode)
    assert sorted(trees["windows"]) == sorted(trees["device"]) and len(trees["windows"]) > 4
    for name in trees["windows"]:
        assert _without_dir(trees["windows"][name], tmp_path) == _without_dir(trees["device"][name], tmp_path), name
    # the flag does not move `auto`, and `device` does not read it
    assert _run(case, tmp_path / "auto", mode="auto", wide_triclinic=True, **kw)["mode"] == "host"


@pytest.mark.parametrize("case", ["cage6_tri_nvt", "cage24_tri_gcmc"])
def test_without_the_flag_windows_mode_stops_as_it_always_did(case, tmp_path):
    with pytest.raises(ValueError, match="the engine's one-launch farm window does not apply to this system"):
        _run(case, tmp_path / "out", replicas=4, seed=7, nb_block=1, nb_step=10, mode="windows")
