"""GPU: the walls of a box (k_box_walls) past its first trip -- tests/test_writer_trips_gpu.py's scheme for this sweep.

A sweep's grid is capped at the resident workgroups, so a store of more than ``CAP = compute_units * 8 * 256`` slots sends every
workgroup through the loop's body again: the second trip is the first in which the wave-wide ballots at the head of the body run
behind a divergent ``continue``.  The edge scene (tests/box_walls_reference.py) at ``N2 = CAP + 2049 + 13`` slots (two trips, a
ragged last wave) in f64 and f32 and at ``N3 = 2 * CAP + 77`` (three trips, workgroups whose trip counts differ by one) in f64, with
mixed walls ("periodic", "mirror", "open") and with mirrors alone, every slot and the eight counts against the restatement.

``has_work`` (the conditions of tests/test_writer_trips_gpu.py, on the restatement's own mask of the slots that are written: the
lanes that stay in the body behind the ``continue``) is held from CAP on: between 10 % and 90 % cross a wall, there are waves that
cross in part below CAP and from there on, with lane 0 idle beside a crossing lane and with lane 0 crossing beside an idle lane.
tests/test_writer_walls_cpu.py needs no device to see that this file names the case.

The restatement these cases are compared with is light._box_walls, the numpy one, for their size; tests/test_writer_walls_cpu.py holds
it bit for bit to the independent loop on Python floats on the edge scene, and tests/test_writer_walls_gpu.py compares the device with
that loop directly.
"""
import numpy as np
import pytest

import writer_reference as W
from box_walls_reference import BOXES, WALLS, check_box_walls, scene, upload_state
from physicl_amd import light
from test_writer_trips_gpu import has_work, slots

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cap(dev):
    return dev.info()["compute_units"] * 8 * 256


@pytest.mark.parametrize("size, dtype", [("N2", "f64"), ("N2", "f32"), ("N3", "f64")])
@pytest.mark.parametrize("walls", ["mixed", "mirror"])
def test_the_walls_past_one_trip(dev, cap, walls, size, dtype):
    n, modes, (lo, hi) = slots(cap, size), WALLS[walls], BOXES["high"]
    state = scene(n, lo, hi, np.float32 if dtype == "f32" else np.float64)
    fields, kind = upload_state(state)
    dev.store_alloc(n, dtype)
    dev.upload_state(dict(fields, id_base=W.ID_BASE, kind=kind))       # plain Objects among the photons: the kinds travel
    before = W.snapshot(dev)
    what = "box walls trips %s %s %s" % (walls, size, dtype)
    counts = dev.box_walls(modes, lo, hi)
    ref = check_box_walls(before, W.snapshot(dev), counts, modes, lo, hi, what, restate=light._box_walls)
    has_work(ref["written"], cap, what)
    assert 0 < ref["moving"][cap:].mean() < 0.95 and (np.asarray(ref["crossed"])[:, :] > 0).all(), what
    assert ref["multi"][cap:].any() and (ref["folded"] & ~ref["multi"])[cap:].any(), what
    if walls == "mixed":
        assert ref["parked"][cap:].any() and ref["folded"][cap:].any(), what
