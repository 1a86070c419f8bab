"""GPU: pcl_step_plane_flux past its first trip ("Trips"; tests/test_writer_trips_gpu.py says what a second and a third
trip are the first to do).  The sweep's row in ``build.ROWS`` names this file's test as its trip case; tests/test_plane_flux_build_cpu.py
holds the row to it on a machine without a GPU.

``N2 = CAP + 2049 + 13`` slots in f64 and f32 and ``N3 = 2 * CAP + 77`` in f64, ``CAP = compute_units * 8 * 256``, in both forms -- 3
levels x 8 x 16 columns (768 cells: LDS) and x 32 x 32 (6144 cells: device memory): the counts and every cell of the maps equal the
restatement's, and test_writer_trips_gpu.has_work's conditions (a)-(c) from CAP on hold on the restatement's mask of crossers -- the
lanes that stay in the body behind the ballots, in part of a wave, with and without lane 0.  tests/test_plane_flux_cpu.py checks the
scene against has_work without a device."""
import numpy as np
import pytest

from plane_flux_reference import crossers, scene
from test_writer_trips_gpu import ROOM, SIZES, has_work, slots

pytestmark = pytest.mark.gpu

TRIP_AXIS, TRIP_LEVELS = "z", [-0.5, 0.0, 0.5]
FORMS = {"lds": [np.linspace(-3, 3, 9), np.linspace(-3, 3, 17)], "global": [np.linspace(-3, 3, 33), np.linspace(-3, 3, 33)]}


def state_of(n, dtype):
    return scene(n, dtype)


@pytest.fixture(scope="module")
def dev():
    from physicl_amd import _hip
    d = _hip.Device(0)
    yield d
    d.close()


@pytest.mark.parametrize("size, dtype", SIZES)
def test_the_sweep_past_one_trip(dev, size, dtype):
    from physicl_amd import _hip, light_grid
    cap = dev.info()["compute_units"] * 8 * 256
    n = slots(cap, size)
    r, dr, E, photon = st = state_of(n, dtype)
    what = "plane flux n=%d %s" % (n, dtype)
    has_work(crossers(st, TRIP_AXIS, TRIP_LEVELS), cap, what)
    dev.store_alloc(n + ROOM, dtype)
    dev.upload_state(dict(r=r, dr=dr, E=E))
    assert dev.count == n > cap
    for form, edges in FORMS.items():
        assert _hip.plane_flux_lds_form(3, len(edges[0]) - 1, len(edges[1]) - 1, 0) == (form == "lds")
        want = light_grid._plane_flux_maps(r, dr, E, photon, TRIP_AXIS, TRIP_LEVELS, edges)
        got = dev.plane_flux(TRIP_AXIS, TRIP_LEVELS, edges)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (what, form)
        assert got[0].min() > 1000 and np.count_nonzero(got[1]) > got[1].size // 2, (what, form)
