"""GPU: pcl_step_phase_grid past its first trip ("Trips"; tests/test_writer_trips_gpu.py says what a second and a third
trip are the first to do).  ``TRIP_CASES`` names the test for every kernel of ``build.LATER``; tests/test_build_later_cpu.py holds the
table against the build's, on a machine without a GPU.

``N2 = CAP + 2049 + 13`` slots in f64 and f32 and ``N3 = 2 * CAP + 77`` in f64, ``CAP = compute_units * 8 * 256``: every slot against
the restatement (grid_phase_reference.check_grid), and test_writer_trips_gpu.has_work's conditions (a)-(c) from CAP on, on the
restatement's mask of the re-directed slots.  The scene is the 4 x 4 x 4 box with three mixtures and cells that are left alone: a
scattered lane may leave the body through the map or stay in it, so a wave's lanes part ways behind the ballots."""
import numpy as np
import pytest

import writer_reference as W
from grid_phase_reference import call, check_grid, scenes, state_of
from layered_phase_reference import C, SEED
from test_writer_trips_gpu import ID_BASE, N_PASS, ROOM, SIZES, has_work, slots

pytestmark = pytest.mark.gpu

TRIP_CASES = {"k_phase_grid": ("test_writers_grid_phase_trips_gpu.py", "test_the_sweep_past_one_trip")}
SCENE = scenes()["xyz"]


@pytest.fixture(scope="module")
def dev():
    from physicl_amd import _hip
    d = _hip.Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("size, dtype", SIZES)
def test_the_sweep_past_one_trip(dev, size, dtype):
    cap = dev.info()["compute_units"] * 8 * 256
    n = slots(cap, size)
    what = "grid phase n=%d %s" % (n, dtype)
    dev.store_alloc(n + ROOM, dtype)
    dev.upload_state(dict(state_of(n, dtype), id_base=ID_BASE))
    assert dev.is_uniform() and dev.count == n > cap
    before = W.snapshot(dev)
    answer = call(dev, SCENE, N_PASS)
    ref = check_grid(before, W.snapshot(dev), answer, SCENE, C, SEED, N_PASS, what)
    assert dev.count == n and min(answer[2]) > 0 and min(answer[3]) > 0 and answer[1] < answer[0], what
    has_work(ref["redirected"], cap, what)
    has_work(ref["scattered"], cap, what + " [scattered]")
