"""GPU: pcl_step_absorb_grid past its first trip ("Trips"; tests/test_writer_trips_gpu.py says what a second and a third
trip are the first to do).  ``TRIP_CASES`` names the test for every kernel of ``build.MORE``; tests/test_grid_absorb_build_cpu.py holds
the table against the build's, on a machine without a GPU.

``N2 = CAP + 2049 + 13`` slots in f64 and f32 and ``N3 = 2 * CAP + 77`` in f64, ``CAP = compute_units * 8 * 256``, in both forms -- 16 x
16 x 16 cells with k alone (LDS) and with both tables (device memory): every slot against the restatement
(grid_absorb_reference.check_grid_absorb), and test_writer_trips_gpu.has_work's conditions (a)-(c) from CAP on, on the restatement's
mask of the absorbed.  The population is the edge scene, tiled: an absorbed lane leaves the body behind the ballots, its neighbours
stay, and a wave's run of absorptions in one cell is carried from trip to trip or ended by another cell."""
import numpy as np
import pytest

import writer_reference as W
from grid_absorb_reference import CENTER, SEED, check_grid_absorb, grid_edges, scene, tables
from test_writer_trips_gpu import ID_BASE, N_PASS, ROOM, SIZES, has_work, np_type, slots

pytestmark = pytest.mark.gpu

TRIP_CASES = {"k_absorb_grid": ("test_grid_absorb_trips_gpu.py", "test_the_sweep_past_one_trip")}
AXES, BINS = ("x", "y", "z"), (16, 16, 16)
EDGES = grid_edges(AXES, BINS)
BLOCK = 8192                                                           # the scene's length; tiled up to n


@pytest.fixture(scope="module")
def dev():
    from physicl_amd import _hip
    d = _hip.Device(0)
    yield d
    d.close()


def state_of(n, dtype):
    s = scene(BLOCK, AXES, EDGES, np_type(dtype))
    reps = -(-n // BLOCK)
    return {f: np.tile(a, (reps,) + (1,) * (a.ndim - 1))[:n] for f, a in s.items()}


@pytest.mark.parametrize("which", ["k", "both"])
@pytest.mark.parametrize("size, dtype", SIZES)
def test_the_sweep_past_one_trip(dev, size, dtype, which):
    from physicl_amd import _hip
    cap = dev.info()["compute_units"] * 8 * 256
    n = slots(cap, size)
    what = "grid absorb n=%d %s %s" % (n, dtype, which)
    assert _hip.absorb_grid_lds_form(1 if which == "k" else 2, 51, 4096) == (which == "k")
    p, om = tables(BINS, which)
    dev.store_alloc(n + ROOM, dtype)
    dev.upload_state(dict(state_of(n, dtype), id_base=ID_BASE))
    assert dev.is_uniform() and dev.count == n > cap
    before = W.snapshot(dev)
    answer = dev.absorb_grid(p, om, AXES, EDGES, CENTER, None, SEED, N_PASS)
    ref = check_grid_absorb(before, W.snapshot(dev), answer, p, om, AXES, EDGES, CENTER, None, SEED, N_PASS, what)
    assert dev.count == n and 0 < answer[0][2] + answer[0][3] < answer[0][0] < n, what
    assert int(np.asarray(answer[1])[np.asarray(answer[1]) > 0].size) > 1000, what          # the absorbed stand in many cells
    has_work(ref["absorbed"], cap, what)
