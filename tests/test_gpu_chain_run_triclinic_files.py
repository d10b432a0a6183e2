"""The single-chain driver's chain-run mode on the reference's TRICLINIC run (tests/golden/runs/spce_triclinic_nvt):
run_simulation(chain_run=(k, depth), chain_run_triclinic=True) runs each block as launches queued back to back that build
and wrap their moves on the device, and must still write the reference's files character for character -- the comparison
tests/test_gpu_chain_run_files.py makes; without the switch the same input keeps its windows."""
import pytest

from tests.test_gpu_chain_run_files import _run, _same_files
from tests.util import TOL_K

pytestmark = pytest.mark.gpu
CASE = "spce_triclinic_nvt"


def test_a_triclinic_chain_run_writes_the_reference_files(tmp_path):
    res, out = _run(CASE, tmp_path, chain_run=(4, 3), chain_run_triclinic=True)
    cr = res["chain_run"]
    print(f"{CASE}: {cr}")
    assert cr["on"] and (cr["k"], cr["depth"]) == (4, 3)
    assert 0 < cr["launches"] - cr["void_launches"] <= cr["launches"] < cr["steps"]    # some launch consumed more than one step
    assert res["chain_windows"][0] == 0                                # no window was launched
    for k, v in res["energy"].items():
        assert abs(v - res["recomputed_energy"][k]) <= 1e-9 * max(1.0, abs(v)) + 50 * TOL_K, k
    # (a step inside the 16-ulp margin is decided by the loop's own exp and forced: the files hold either way)
    _same_files(CASE, out)


def test_without_the_switch_a_triclinic_input_keeps_its_windows(tmp_path):
    res, out = _run(CASE, tmp_path, chain_run=(4, 3))
    assert not res["chain_run"]["on"] and res["chain_run"]["launches"] == 0
    assert res["chain_windows"][0] > 0
    _same_files(CASE, out)


def test_the_switch_needs_a_chain_run(tmp_path):
    with pytest.raises(ValueError):
        _run(CASE, tmp_path, chain_run_triclinic=True)
