"""CPU: PositionGridMeasureStep and Device.position_grid without a GPU.

* the numpy restatement (tests/grid_reference.py) equals ``numpy.histogramdd`` for 1-, 2- and 3-axis Cartesian grids, with
  values exactly on inner and outer edges, NaN, +-inf and out-of-range points; the radius axis is the q form;
* the constructor's checks;
* what ``Device.position_grid`` / ``DeviceGroup.position_grid`` put over the C ABI and hand back, on a stand-in for the
  library in the manner of tests/test_binding_marshal_cpu.py;
* (the unit's build is held in tests/test_build_cpu.py);
* the host path -- the step called on host-resident Python objects -- and the ``every=`` run counter;
* two gloo ranks on the host side of the collective all-reduce to the unsharded grid.
"""
import os
import re

import numpy as np
import pytest

import physicl_amd as phys
import rank_world
from physicl_amd import _hip, build, light
from grid_reference import position_grid

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------ the restatement
def points(rng, n, edges3):
    """Positions around three axes' edges: inside, exactly on every edge, just outside, NaN and +-inf."""
    r = rng.uniform(-1.5, 1.5, size=(n, 3))
    for k, e in enumerate(edges3):
        on = rng.integers(0, n, size=4 * len(e))
        r[on, k] = np.tile(e, 4)                                  # on inner and outer edges
        r[rng.integers(0, n, size=3), k] = [np.nextafter(e[0], -INF), np.nextafter(e[-1], INF), np.nextafter(e[-1], -INF)]
    r[5, 0], r[6, 1], r[7, 2], r[8, 0], r[9, 1] = NAN, INF, -INF, INF, NAN
    return r


@pytest.mark.parametrize("axes", [("x",), ("y",), ("z",), ("y", "z"), ("z", "x"), ("x", "y", "z"), ("z", "y", "x")])
def test_restatement_equals_histogramdd(axes):
    rng = np.random.default_rng(3)
    edges3 = [np.linspace(-1.0, 1.0, 11), np.array([-1.25, -0.5, -0.25, 0.0, 0.75, 1.0]), np.geomspace(0.01, 1.2, 8)]
    r = points(rng, 5000, edges3)
    cols = ["xyz".index(a) for a in axes]
    edges = [edges3[c] for c in cols]
    want = np.histogramdd(r[:, cols][np.all(np.isfinite(r[:, cols]), axis=1)], bins=edges)[0]     # (histogramdd refuses non-finite samples)
    got = position_grid(r, axes, edges)
    assert got.dtype == np.int64 and got.shape == tuple(len(e) - 1 for e in edges)
    assert np.array_equal(got, want.astype(np.int64)) and 0 < got.sum() < len(r)
    assert np.array_equal(light._grid_of_positions(r, axes, edges, np.zeros(3)), got)             # the host path's own statement


def test_restatement_radius_axis_is_the_q_form():
    rng = np.random.default_rng(4)
    c = np.array([0.25, -0.5, 1.0])
    r = rng.normal(size=(4000, 3)) + c
    e = np.array([0.0, 0.5, 1.0, 1.5, 2.5])
    r[0] = c                                                      # q = 0: on the first edge
    r[1] = c + [1.5, 0, 0]                                        # q = 2.25 = 1.5 * 1.5: on an inner edge, upper bin
    r[2] = c + [0, 0, -2.5]                                       # on the last edge: closed
    r[3] = c + [0, 3.0, 0]                                        # outside
    r[4] = [NAN, 0, 0]
    d = r - c
    q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    want = np.histogram(q[np.isfinite(q)], bins=e * e)[0]
    got = position_grid(r, ("r",), [e], c)
    assert np.array_equal(got, want) and got.sum() < len(r)
    assert np.array_equal(light._grid_of_positions(r, ("r",), [e], c), got)
    two = position_grid(r, ("r", "x"), [e, np.linspace(-2, 2, 5)], c)
    assert two.shape == (4, 4) and np.array_equal(two, light._grid_of_positions(r, ("r", "x"), [e, np.linspace(-2, 2, 5)], c))
    assert np.array_equal(two.sum(axis=1), position_grid(r[np.abs(r[:, 0]) <= 2], ("r",), [e], c))


# ------------------------------------------------------------------------------------------------ constructor
E2 = [0.0, 1.0, 2.0]


@pytest.mark.parametrize("kw", [
    dict(axes=(), edges=[]), dict(axes=("x", "y", "z", "r"), edges=[E2] * 4), dict(axes=("x", "x"), edges=[E2, E2]),
    dict(axes=("w",), edges=[E2]), dict(axes=(0,), edges=[E2]), dict(axes=3, edges=[E2]), dict(axes=("x",), edges=[E2, E2]),
    dict(axes=("x", "y"), edges=[E2]), dict(axes=("x",), edges=[[1.0]]), dict(axes=("x",), edges=[np.arange(1026.0)]),
    dict(axes=("x",), edges=[[1.0, 1.0, 2.0]]), dict(axes=("x",), edges=[[1.0, 3.0, 2.0]]), dict(axes=("x",), edges=[[1.0, NAN, 2.0]]),
    dict(axes=("x",), edges=[[1.0, 2.0, INF]]), dict(axes=("x",), edges=[[[1.0, 2.0], [3.0, 4.0]]]), dict(axes=("x",), edges="abc"),
    dict(axes=("x", "y", "z"), edges=[np.arange(1025.0), np.arange(1025.0), np.arange(3.0)]),       # 2^21 cells
    dict(axes=("r",), edges=[[-1.0, 1.0]]), dict(axes=("r",), edges=[[0.0, 1e200]]), dict(axes=("r",), edges=[[0.0, 1e-200, 2e-200]]),
    dict(axes=("x",), edges=[E2], center=(0, NAN, 0)), dict(axes=("x",), edges=[E2], center=(0, 0)), dict(axes=("x",), edges=[E2], center="c"),
    dict(axes=("x",), edges=[E2], every=0), dict(axes=("x",), edges=[E2], every=-3), dict(axes=("x",), edges=[E2], every=1.5),
    dict(axes=("x",), edges=[E2], every=True)])
def test_malformed_steps_are_refused_at_construction(kw):
    with pytest.raises(ValueError):
        light.PositionGridMeasureStep(None, **kw)


def test_accepted_forms():
    s = light.PositionGridMeasureStep(None, ("r", "x"), [np.arange(1025), [0, 1]], center=(6371000, 0, 0), every=32, measure_n=False)
    assert s.axes == ("r", "x") and s.edges[0].dtype == np.float64 and len(s.edges[0]) == 1025 and s.center.tolist() == [6371000.0, 0.0, 0.0]
    assert s.every == 32 and s._fuse_role == "snapshot" and s._n_planes() == 0 and s._plane_rows() == [] and s.data == []
    s = light.PositionGridMeasureStep(None, "yz", [E2, E2])                                      # a string reads as its letters
    assert s.axes == ("y", "z") and s.every == 1 and s.measure_n is True
    s = light.PositionGridMeasureStep(None, ["x", "y", "z"], [np.arange(1025.0), np.arange(1025.0), np.arange(2.0)])   # 2^20 cells: the most
    m = light.PositionGridMeasureStep(None, ("x",), [phys.Measurement(np.array([1.0, 2.0, 4.0]), "m**1")])
    assert type(m.edges[0]) is np.ndarray and m.edges[0].tolist() == [1.0, 2.0, 4.0]             # a Measurement: by its stored value
    assert phys.light.PositionGridMeasureStep is light.PositionGridMeasureStep


# ------------------------------------------------------------------------------------------------ binding
class FakeLib:
    """Records the call with the arrays behind its pointers; answers cells 1000, 1001, ..."""

    def __init__(self):
        self.calls = []

    def _grid(self, name, handle, n_axes, coords, n_bins, edges, center, out):
        at = lambda addr, dt, n: np.ctypeslib.as_array((np.ctypeslib.as_ctypes_type(dt) * n).from_address(addr))     # noqa: E731
        nb = at(n_bins, np.int32, n_axes).tolist()
        self.calls.append((name, handle, n_axes, at(coords, np.int32, n_axes).tolist(), nb, at(edges, np.float64, sum(nb) + n_axes).tolist(),
                           None if center is None else at(center, np.float64, 3).tolist()))
        cells = int(np.prod(nb))
        at(out, np.int64, cells)[:] = 1000 + np.arange(cells)
        return 0

    def pcl_step_position_grid(self, *a):
        return self._grid("pcl_step_position_grid", *a)

    def pcl_group_step_position_grid(self, *a):
        return self._grid("pcl_group_step_position_grid", *a)


@pytest.mark.parametrize("cls,handle,entry", [(_hip.Device, "ctx", "pcl_step_position_grid"), (_hip.DeviceGroup, "g", "pcl_group_step_position_grid")])
def test_position_grid_marshalling(cls, handle, entry):
    d = cls.__new__(cls)
    d.lib = FakeLib()
    setattr(d, handle, None)
    grid = d.position_grid(("r", "z", "x"), [[0, 1, 2], [-1, 3], [1, 2, 4, 8]], center=(1.5, -2, 0.25))
    (name, h, n_axes, coords, n_bins, edges, center), = d.lib.calls
    assert name == entry and h is None and n_axes == 3 and coords == [3, 2, 0] and n_bins == [2, 1, 3]
    assert edges == [0.0, 1.0, 2.0, -1.0, 3.0, 1.0, 2.0, 4.0, 8.0] and center == [1.5, -2.0, 0.25]      # (the edges as given: the library squares)
    assert grid.dtype == np.int64 and grid.shape == (2, 1, 3) and grid.reshape(-1).tolist() == list(range(1000, 1006))  # C order
    grid = d.position_grid("y", [np.linspace(0, 1, 5)])
    assert d.lib.calls[1][2:] == (1, [1], [4], [0.0, 0.25, 0.5, 0.75, 1.0], None) and grid.shape == (4,)   # no centre: NULL
    with pytest.raises(ValueError):
        d.position_grid(("x", "y"), [[0, 1]])


def test_prototypes_constants_and_multidevice_sum():
    assert "pcl_step_position_grid" in _hip.EXPORTS and "pcl_group_step_position_grid" in _hip.EXPORTS
    assert len(_hip._PROTOTYPES["pcl_step_position_grid"]) == 7 == len(_hip._PROTOTYPES["pcl_group_step_position_grid"])
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "physicl_hip.h")).read()
    for name, value in (("PCL_GRID_X", 0), ("PCL_GRID_Y", 1), ("PCL_GRID_Z", 2), ("PCL_GRID_RADIUS", 3), ("PCL_GRID_MAX_AXES", 3),
                        ("PCL_GRID_MAX_BINS", 1024)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value
    assert "#define PCL_GRID_MAX_CELLS (1 << 20)" in header and "sqrt(q)" in header
    assert _hip.GRID_COORDS == {"x": 0, "y": 1, "z": 2, "r": 3}
    assert (_hip.GRID_MAX_AXES, _hip.GRID_MAX_BINS, _hip.GRID_MAX_CELLS) == (3, 1024, 1 << 20)
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def position_grid(self, axes, edges, center=None):
            return np.full((2, 3), self.k, dtype=np.int64)
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    got = md.position_grid(("x", "y"), [E2, [0, 1, 2, 3]])
    md._pool.shutdown()
    assert got.dtype == np.int64 and got.tolist() == [[111] * 3] * 2


# ------------------------------------------------------------------------------------------------ host path
def host_sim(r, objects=0):
    sim = phys.Simulation(cl_on=False)               # (cl_on=True opens its device at once)
    objs = [light.PhotonObject(E=1.0, v=light.c * [1, 0, 0]) for _ in range(len(r) - objects)] + [phys.Object() for _ in range(objects)]
    for o, rr in zip(objs, r):
        o.r = np.array(rr, dtype=np.float64)
    sim.add_objs(objs)
    return sim


def test_host_path_gives_the_restatement_s_rows(tmp_path):
    rng = np.random.default_rng(8)
    ex, ey = np.linspace(-1, 1, 5), np.array([-1.0, 0.0, 0.5, 1.0])
    r = points(rng, 300, [ex, ey, ex])
    sim = host_sim(r, objects=20)                    # plain Objects count like photons
    sim.t = 0.25
    out = tmp_path / "grid.csv"
    a = light.PositionGridMeasureStep(str(out), ("x", "y"), [ex, ey])
    b = light.PositionGridMeasureStep(None, ("r",), [[0.0, 0.5, 1.0, 2.0]], center=(0.5, 0, 0), measure_n=False)
    a.run(sim)
    b.run(sim)
    assert sim._dev is None                          # nothing was uploaded for a measurement of host-resident objects
    (row,), (rowb,) = a.data, b.data
    assert row.dtype == object and len(row) == 3 and row[0] == 0.25 and row[1] == 300
    assert row[2].dtype == np.int64 and np.array_equal(row[2], position_grid(r, ("x", "y"), [ex, ey])) and 0 < row[2].sum() < 300
    assert len(rowb) == 2 and rowb[0] == 0.25 and np.array_equal(rowb[1], position_grid(r, ("r",), [[0.0, 0.5, 1.0, 2.0]], (0.5, 0, 0)))
    a.terminate(sim)
    assert out.read_text() == "0.25, 300, %s\n" % row[2].tolist()       # the grid reads as a nested plain list
    b.terminate(sim)                                 # no file asked for: nothing written


def test_every_counts_the_step_s_own_runs_from_one():
    sim = host_sim(np.zeros((3, 3)))
    s = light.PositionGridMeasureStep(None, ("x",), [[-1.0, 1.0]], every=3)
    assert s._passes_to_record() == 3
    for m in range(1, 11):
        sim.t = float(m)
        s.run(sim)
        assert s._passes_to_record() == 3 - m % 3
    assert [row[0] for row in s.data] == [3.0, 6.0, 9.0] and all(row[2].tolist() == [3] for row in s.data)
    assert not s._advance(1) and s._advance(1) and s._passes_to_record() == 3 and not s._advance(0)      # runs 11, 12: the 12th records
    assert s._advance(6) and not s._advance(5) and s._advance(1)                                           # 18; 23; 24


def test_snapshot_steps_ride_at_the_end_of_a_fused_group_only():
    from physicl_amd import newton
    sim = phys.Simulation(cl_on=False, rng="philox")
    sim.cl_on = True                                 # (plan as a device run would; no device is opened by planning)
    g1, g2 = (light.PositionGridMeasureStep(None, ("x",), [[-1.0, 1.0]], every=4) for _ in range(2))
    steps = [phys.UpdateTimeStep(lambda s: 1.0), newton.NewtonianKinematicsStep(), light.ScatterIsotropicStep(n=1.0, A=1e-9),
             light.ScatterSignMeasureStep(None), g1, newton.NewtonianKinematicsStep(), light.ScatterDeleteStep(1.0, 1e-9), g2]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    plan = sim._build_plan()
    assert [k for k, _ in plan] == ["single", "fused", "fused"] and plan[1][1][-1] is g1 and plan[2][1][-1] is g2
    sim._plan, sim._hip = plan, _hip
    assert not sim._multi_eligible() and "PositionGridMeasureStep" in sim.launch_note            # g1 is not behind the last light step
    sim.launch_note = None
    sim.steps.pop(4)
    sim._plan = sim._build_plan()
    assert sim._multi_eligible() and sim.launch_note is None
    sim.steps.pop(7)                                 # without such a step: as before
    sim._plan = sim._build_plan()
    assert sim._multi_eligible() and sim.launch_note is None


def test_passes_that_were_never_k_eligible_answer_as_before():
    from physicl_amd import newton
    sim = phys.Simulation(cl_on=False, rng="philox")
    sim.cl_on, sim._hip = True, _hip
    sim._plan = sim._build_plan()                    # no steps at all: an empty plan
    assert sim._plan == [] and sim._multi_eligible() is False and sim.launch_note is None
    sim.exit = lambda s: True
    sim._run_pass_locked()                           # ... and a pass of it idles, as it always did
    assert sim.launch_note is None and not sim.schedule
    g = light.PositionGridMeasureStep(None, ("x",), [[-1.0, 1.0]])
    # the step behind a measure_E step is a plan item of its own: the pass is not K-eligible whatever it holds, and says nothing
    for k, s in enumerate([phys.UpdateTimeStep(lambda s: 1.0), newton.NewtonianKinematicsStep(), light.ScatterIsotropicStep(n=1.0, A=1e-9),
                           light.ScatterMeasureStep(None, measure_locs=[[0.0, NAN, NAN]], measure_E=True), g]):
        sim.add_step(k, s)
    sim._plan = sim._build_plan()
    assert [k for k, _ in sim._plan] == ["single", "fused", "single", "single"] and sim._plan[-1][1] is g
    assert sim._multi_eligible() is False and sim.launch_note is None


# ------------------------------------------------------------------------------------------------ collective
GLOO_WORKER = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from physicl_amd import light
from physicl_amd.dist import CounterComm
comm = CounterComm.from_env(backend="gloo")
rng = np.random.default_rng(2)
r = rng.uniform(-1, 1, size=(5000, 3))
lo, hi = (0, len(r)) if comm.world == 1 else ((0, 0) if comm.rank == 0 else (0, len(r)))   # rank 0 of a sharded run holds an empty shard
if comm.world == 3:
    lo, hi = comm.shard(len(r))
class Dev:
    count = hi - lo
    def position_grid(self, axes, edges, center=None):
        return light._grid_of_positions(r[lo:hi], axes, edges, center)
class Sim:
    t = 0.5
    _dev = Dev()
    def _global(self, values):
        return comm.allreduce_sum(values) if comm.world > 1 else np.asarray(values, dtype=np.int64)
Sim.comm = comm
step = light.PositionGridMeasureStep(None, ("x", "r"), [np.linspace(-1, 1, 65), np.linspace(0, 1.5, 65)], every=2)   # 1 + 4096 values: three collectives
for _ in range(4):
    step._device_run(Sim())
print(json.dumps({"rank": comm.rank, "rows": [[x.tolist() if isinstance(x, np.ndarray) else float(x) for x in row] for row in step.data]}))
comm.close()
"""


def run_gloo_world(world):
    return rank_world.run_world(GLOO_WORKER % {"root": os.path.dirname(os.path.dirname(os.path.abspath(__file__)))}, world, timeout=300)


def test_world2_gloo_grids_equal_the_unsharded_grid():
    """Two processes, gloo on the CPU: rank 0 holds an empty shard, rank 1 what the single process holds -- both record the single
    process's rows, two of the four runs (every=2); three ranks with a shard each do, too."""
    one = run_gloo_world(1)[0]
    two = run_gloo_world(2)
    three = run_gloo_world(3)
    assert two[0]["rows"] == two[1]["rows"] == one["rows"] and len(one["rows"]) == 2
    assert three[0]["rows"] == three[2]["rows"] == one["rows"]
    t, n, grid = one["rows"][0]
    assert (t, n) == (0.5, 5000.0) and np.array(grid).shape == (64, 64) and 0 < np.sum(grid) <= 5000
