"""No GPU.  tests/test_gpu_triclinic_moves.py holds the device's triclinic trial geometry to oracle/refcpu.c's
refcpu_apply_pbc BIT FOR BIT, at inputs chosen to sit on the edges of the wrap.  This file shows the authority is sound
there: on those inputs, in both cells, refcpu_apply_pbc returns the doubles of the compiled reference's ApplyPBC
(src/geometry_utils.f90:167-220) -- against its stored answers (tests/golden/triclinic_wrap_pins.npz, written by
tests/golden/make_triclinic_wrap_pins.py: a digest of 60 000 wrapped points per cell) and, where the compiled reference is
present, against the library itself, point by point."""
import hashlib
import os

import numpy as np
import pytest

from tests import triclinic_cases as tc
from tests.util import GOLDEN


@pytest.mark.parametrize("name", tc.CELLS)
def test_refcpu_apply_pbc_is_the_references_on_the_edge_inputs(name, refcpu_mod):
    s = tc.cell(name)
    assert s.is_triclinic()
    pts = tc.wrap_inputs(s)
    P = refcpu_mod.RefCPU(s)
    mine = np.array([P.apply_pbc(p) for p in pts])
    pins = np.load(os.path.join(GOLDEN, "triclinic_wrap_pins.npz"))
    assert len(pts) == int(pins[name + "_n"]) == 60000
    assert hashlib.sha256(np.ascontiguousarray(mine).tobytes()).hexdigest() == str(pins[name])
    # ... and the arithmetic the engine's header states for the device is that arithmetic, written out
    assert np.array_equal(tc.apply_pbc_stated(s, P.box()[2], pts), mine)
    from oracle import reflib
    if reflib.available():
        R = reflib.Reference(s)
        ref = np.array([R.apply_pbc(p) for p in pts])
        R.close()
        diff = np.flatnonzero(np.any(mine != ref, axis=1))
        assert diff.size == 0, (name, diff.size, pts[diff[:3]], mine[diff[:3]], ref[diff[:3]])


@pytest.mark.parametrize("name", tc.CELLS)
def test_the_edge_inputs_sit_on_the_edges_of_the_wrap(name, refcpu_mod):
    """The lo + M^T f family really does put ApplyPBC's fractional coordinates within 1e-16 of 0 and of 1 -- and ApplyPBC is
    not the identity on a point inside the cell: the reference maps pos to lo + M frac(M^-T (pos - lo)), M and its
    transpose both, which is why the device applies it ALWAYS and has no "already inside" shortcut."""
    s = tc.cell(name)
    P = refcpu_mod.RefCPU(s)
    rcp = P.box()[2]
    pts = tc.edge_points(s, 4000, 7, True)
    v = pts - s.bounds_lo
    f = np.stack([(rcp[i, 0] * v[:, 0] + rcp[i, 1] * v[:, 1]) + rcp[i, 2] * v[:, 2] for i in range(3)], axis=1)
    d = np.abs(f - np.rint(f))
    assert np.mean(d < 1e-12) > 0.5 and np.any((d > 0) & (d < 1e-12))
    inside = tc.cart(s, np.random.default_rng(3).uniform(0.05, 0.95, (500, 3)))
    back = np.array([P.apply_pbc(p) for p in inside])
    assert np.max(np.abs(back - inside)) > 1e-3
