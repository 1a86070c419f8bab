"""CPU: DetectorMeasureStep and Device.detector_image without a GPU.

* the numpy restatement the package answers with (light._detector_image) agrees with a per-particle Python loop written from the
  header's text (tests/detector_reference.py) on drawn pencils, on the planted edge cases and on what they must give by hand;
* a photon sent from a known direction through the aperture's centre lands in the pixel worked out by hand;
* every refusal of ``_check_detector`` and of the constructor; every PCL_ERR_ARG of both entry points with a NULL context; the
  header's limits against ``_hip``;
* the TallyStep wiring on a stand-in device (rows, ``frames``, the exposure, ``out_fn``), the MultiDevice sum on stand-in shards, the
  binding on a stand-in library, the host-plugin path on Python objects;
* both entry points declared; the sweep's element of the build table (tests/test_build_cpu.py holds the kernel's assembly to its
  budget, as every sweep's).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import physicl_amd as phys
from physicl_amd import _hip, build, light
from detector_reference import (ALIGNED, E_BANDS, EVERY, PLANTED, X33, Y17, configs, detector_image_loop, planted_answers,
                                planted_state, scene, tilted_frame)

NAN, INF = float("nan"), float("inf")
ROOT = os.path.dirname(build.HERE)
ENTRIES = ("pcl_step_detector_image", "pcl_group_step_detector_image")


def same(a, b):
    return len(a) == len(b) == 2 and all(x.dtype == np.int64 and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", sorted(configs()))
def test_planted_cases_by_hand_and_against_the_loop(name):
    cfg = configs()[name]
    st = planted_state(cfg)
    got = light._detector_image(*st, **cfg)
    assert same(got, detector_image_loop(*st, **cfg))
    if name.startswith("aligned_33x17"):                   # exact there: every planted case by hand
        through, seen, cells = planted_answers(cfg["E_edges"] is not None)
        want = np.zeros_like(got[1])
        for cell, k in cells.items():
            want[cell] = k
        assert got[0].tolist() == [through, seen] and np.array_equal(got[1], want)
    if name == "aligned_1x1":                              # one pixel over [-0.5, 0.5]: cases 5 and 13 lie outside it
        assert got[0].tolist() == [9, 6] and got[1].tolist() == [[[6]]]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(configs()))
def test_restatement_equals_the_loop_on_drawn_pencils(name, dtype):
    cfg = configs()[name]
    for N in (1, 65, 700):
        st = scene(N, dtype, name)
        counts, image = got = light._detector_image(*st, **cfg)
        assert same(got, detector_image_loop(*st, **cfg)), N
        assert image.shape == (1 if cfg["E_edges"] is None else 4, len(cfg["y_edges"]) - 1, len(cfg["x_edges"]) - 1)
        assert image.sum() <= counts[1] <= counts[0] <= N
    assert 0 < counts[1] < counts[0] < 700 and 0 < image.sum() and (image.sum() < counts[1]) == (cfg["E_edges"] is not None)
    assert np.count_nonzero(image) >= (2 if image.size > 4 else 1)


def test_the_scene_holds_the_planted_cases():
    r, dr, E, photon = scene(2049, "f64", "aligned_33x17_bands")
    pr, pm, pE, pph = planted_state(configs()["aligned_33x17_bands"])
    for at in (0, EVERY, 30 * EVERY):
        k = slice(at, at + len(PLANTED))
        assert np.array_equal(r[k], pr, equal_nan=True) and np.array_equal(dr[k], pm) and np.array_equal(E[k], pE, equal_nan=True)
        assert np.array_equal(photon[k], pph)
    r32 = scene(2049, "f32", "aligned_33x17_bands")[0]
    assert r32.dtype == np.float32 and np.array_equal(r32[:len(PLANTED)].astype(np.float64), pr, equal_nan=True)    # dyadic: exact in fp32


@pytest.mark.parametrize("col,row", [(0, 0), (16, 8), (32, 16), (5, 11), (27, 2)])
def test_a_photon_from_a_known_direction_lands_in_its_pixel(col, row):
    """Through the aperture's centre, from the direction of the middle of pixel (row, col) of a tilted camera."""
    step = light.DetectorMeasureStep(None, (3.0, -2.0, 0.5), normal=(1.0, 2.0, -2.0), radius=0.1, pixels=(33, 17), fov=(0.6, 0.4), up=(0.0, 0.0, 1.0))
    e1, e2, n = step.frame
    assert np.allclose(step.frame @ step.frame.T, np.eye(3), atol=1e-15) and np.allclose(n, np.array([1.0, 2.0, -2.0]) / 3.0)
    assert np.allclose(step.x_edges, np.linspace(-np.tan(0.6), np.tan(0.6), 34)) and np.allclose(step.y_edges, np.linspace(-np.tan(0.4), np.tan(0.4), 18))
    tx, ty = 0.5 * (step.x_edges[col] + step.x_edges[col + 1]), 0.5 * (step.y_edges[row] + step.y_edges[row + 1])
    came_from = n + tx * e1 + ty * e2                       # the direction towards the scene, gnomonic (tx, ty)
    m = -0.8 * came_from                                    # it moves the other way, from in front of the plane to behind it
    r = step.position + 0.5 * m
    counts, image = light._detector_image([r], [m], [2.0], [True], step.position, step.frame, step.radius, step.x_edges, step.y_edges)
    assert counts.tolist() == [1, 1] and image[0, row, col] == 1 and image.sum() == 1
    counts, image = light._detector_image([r - m], [-m], [2.0], [True], step.position, step.frame, step.radius, step.x_edges, step.y_edges)
    assert counts.tolist() == [0, 0] and image.sum() == 0    # the same way back: back to front, not a crossing


# ------------------------------------------------------------------------------------------------ refusals
GOOD = dict(position=(0.5, -1.0, 2.0), frame=ALIGNED, radius=0.25, x_edges=X33, y_edges=Y17, E_edges=E_BANDS)
BAD = [
    dict(position=(0.0, NAN, 0.0)), dict(position=(0.0, INF, 0.0)), dict(frame=np.where(np.eye(3) > 0, NAN, 0.0)),
    dict(frame=np.array([[1.0, 0, 0], [0, INF, 0], [0, 0, 1.0]])), dict(frame=np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 0]])),      # a zero n
    dict(radius=0.0), dict(radius=-1.0), dict(radius=NAN), dict(radius=INF), dict(radius=1e200),
    dict(x_edges=np.array([0.0, 0.0, 1.0])), dict(x_edges=np.array([0.0, NAN, 1.0])), dict(x_edges=np.array([0.0, 1.0, INF])),
    dict(x_edges=np.array([1.0, 0.5])), dict(x_edges=np.array([0.5])), dict(x_edges=np.linspace(-1, 1, 1026)),
    dict(y_edges=np.array([0.0, 1.0, 1.0])), dict(y_edges=np.array([NAN, 1.0])), dict(y_edges=np.array([0.5])), dict(y_edges=np.linspace(-1, 1, 1026)),
    dict(E_edges=np.array([1.0, 1.0, 2.0])), dict(E_edges=np.array([1.0, NAN])), dict(E_edges=np.array([1.0, INF])), dict(E_edges=np.array([2.0, 1.0])),
    dict(E_edges=np.array([1.0])), dict(E_edges=np.linspace(1, 2, 1026)),
    dict(x_edges=np.linspace(-1, 1, 1025), y_edges=np.linspace(-1, 1, 1025), E_edges=np.array([1.0, 2.0, 3.0])),        # 2 x 1024 x 1024 cells
    dict(x_edges=np.linspace(-1, 1, 1025), y_edges=np.linspace(-1, 1, 1026), E_edges=None),
]


@pytest.mark.parametrize("kw", BAD, ids=[",".join(sorted(kw)) + "-%d" % k for k, kw in enumerate(BAD)])
def test_check_detector_refuses(kw):
    with pytest.raises(ValueError):
        light._check_detector(**dict(GOOD, **kw))


def test_check_detector_accepts_and_gives_float64():
    p, f, radius, x, y, e = light._check_detector((1, 2, 3), [1, 0, 0, 0, 1, 0, 0, 0, 1], 2, [0, 1], range(3), None)
    assert p.dtype == f.dtype == x.dtype == y.dtype == np.float64 and f.shape == (3, 3) and radius == 2.0 and e is None
    assert p.tolist() == [1.0, 2.0, 3.0] and x.tolist() == [0.0, 1.0] and y.tolist() == [0.0, 1.0, 2.0]
    light._check_detector(**dict(GOOD, x_edges=np.linspace(-1, 1, 1025), y_edges=np.linspace(-1, 1, 1025), E_edges=None))     # 2**20 cells: the most
    light._check_detector(**dict(GOOD, x_edges=[0.0, 1.0], y_edges=np.linspace(-1, 1, 1025), E_edges=np.linspace(1, 2, 1025)))
    with pytest.raises(ValueError, match="position"):
        light._check_detector(**dict(GOOD, position=(0, 0)))
    with pytest.raises(ValueError, match="frame"):
        light._check_detector(**dict(GOOD, frame=np.eye(2)))
    with pytest.raises(ValueError):
        light._check_detector(**dict(GOOD, radius="r"))


@pytest.mark.parametrize("kw", [
    dict(normal=(0, 0, 0)), dict(normal=(0, NAN, 1)), dict(normal=(0, 1)), dict(normal="n"), dict(normal=(0, 0, 1), up=(0, 0, 2)),
    dict(normal=(0, 0, 1), up=(0, 0, 0)), dict(normal=(0, 0, 1), up=(0, INF, 0)), dict(normal=(0, 0, 1), up=(1, 0)),
    dict(normal=(0, 0, 1), radius=0.0), dict(normal=(0, 0, 1), position=(0, NAN, 0)), dict(normal=(0, 0, 1), pixels=(0, 4)),
    dict(normal=(0, 0, 1), pixels=(4,)), dict(normal=(0, 0, 1), pixels=(1025, 4)), dict(normal=(0, 0, 1), fov=0.0), dict(normal=(0, 0, 1), fov=np.pi / 2),
    dict(normal=(0, 0, 1), fov=(0.5, NAN)), dict(normal=(0, 0, 1), fov=(0.1, 0.2, 0.3)), dict(normal=(0, 0, 1), x_edges=[0.0, 0.0], y_edges=[0.0, 1.0]),
    dict(normal=(0, 0, 1), E_bins=[1.0]), dict(normal=(0, 0, 1), pixels=(1024, 1024), E_bins=[1.0, 2.0, 3.0])])
def test_malformed_steps_are_refused_at_construction(kw):
    with pytest.raises(ValueError):
        light.DetectorMeasureStep(None, **dict(dict(position=(0, 0, 0), radius=1.0), **kw))


def test_accepted_forms_and_the_frame():
    s = light.DetectorMeasureStep(None, (6371000, 0, 0), (1, 0, 0), 50.0)
    assert s.image.shape == (1, 64, 64) and s.image.dtype == np.int64 and not s.image.any() and (s.through, s.seen) == (0, 0)
    assert s.frame[2].tolist() == [1.0, 0.0, 0.0] and s.frame[0].tolist() == [0.0, 1.0, 0.0] and s.frame[1].tolist() == [0.0, 0.0, 1.0]    # up: the first of the least aligned axes
    assert np.allclose(s.x_edges, np.linspace(-1, 1, 65)) and s.E_bins is None and s.frames is False and s.measure_n is True
    assert s._fuse_role is None and s._device_native and s.data == [] and s.position.tolist() == [6371000.0, 0.0, 0.0]
    s = light.DetectorMeasureStep(None, (0, 0, 0), (0, 0, -2), 1, pixels=(3, 2), fov=0.5, E_bins=[1, 2, 4], frames=True, measure_n=False)
    assert s.image.shape == (2, 2, 3) and s.frame[2].tolist() == [0.0, 0.0, -1.0] and len(s.x_edges) == 4 and len(s.y_edges) == 3
    assert np.allclose(s.x_edges[[0, -1]], [-np.tan(0.5), np.tan(0.5)]) and np.allclose(s.y_edges, s.x_edges[[0, -1]].mean() + np.tan(0.5) * np.array([-1, 0, 1]))
    s = light.DetectorMeasureStep(None, (0, 0, 0), (1, 1, 0), 1, x_edges=[-0.25, 0.5], y_edges=[0.0, 0.125, 0.25], fov=0.1, pixels=(9, 9))
    assert s.x_edges.tolist() == [-0.25, 0.5] and s.y_edges.tolist() == [0.0, 0.125, 0.25]                 # explicit edges win
    assert np.allclose(s.frame @ s.frame.T, np.eye(3), atol=1e-15) and np.allclose(np.cross(s.frame[2], s.frame[0]), s.frame[1])
    assert s.frame[0].tolist() == [0.0, 0.0, 1.0]           # n has no z: z is the least aligned axis
    assert np.allclose(tilted_frame() @ tilted_frame().T, np.eye(3), atol=1e-15) and np.all(np.abs(tilted_frame()) > 0.05)
    import physicl.light
    assert physicl.light.DetectorMeasureStep is light.DetectorMeasureStep is phys.light.DetectorMeasureStep


# ------------------------------------------------------------------------------------------------ TallyStep wiring
class Dev:
    count = 7

    def __init__(self):
        self.calls = []

    def detector_image(self, position, frame, radius, x_edges, y_edges, E_edges=None):
        self.calls.append((position, frame, radius, x_edges, y_edges, E_edges))
        k = len(self.calls)
        return np.array([5 * k, 3 * k], dtype=np.int64), np.arange(6, dtype=np.int64).reshape(1, 2, 3) * k


class Sim:
    t, launch_note, steps_per_launch = 0.5, None, None

    def __init__(self):
        self._dev, self.chunks = Dev(), []

    def _k_wanted(self):
        return 32

    def _global(self, values):
        self.chunks.append(len(values))
        return np.asarray(values, dtype=np.int64) * 2               # two ranks with the same tallies


def test_the_step_on_a_stand_in_device(tmp_path):
    out = tmp_path / "camera.csv"
    sim = Sim()
    step = light.DetectorMeasureStep(str(out), (0, 0, 0), (0, 0, 1), 1.0, pixels=(3, 2), fov=0.5, frames=True)
    step._device_run(sim)
    step._device_run(sim)
    assert "DetectorMeasureStep" in sim.launch_note and sim.launch_note.startswith("one launch per light step")
    assert sim.chunks == [1 + 2 + 6] * 2                   # one collective per pass: N, the two counts, the image
    (p, f, radius, x, y, e), _ = sim._dev.calls
    assert p is step.position and f is step.frame and radius == 1.0 and x is step.x_edges and y is step.y_edges and e is None
    a, b = step.data
    assert list(a[:4]) == [0.5, 14, 10, 6] and list(b[:4]) == [0.5, 14, 20, 12] and len(a) == 5
    assert a[4].tolist() == [[[0, 2, 4], [6, 8, 10]]] and b[4].tolist() == [[[0, 4, 8], [12, 16, 20]]] and b[4].dtype == np.int64
    assert step.image.tolist() == (a[4] + b[4]).tolist() and (step.through, step.seen) == (20, 12)          # the exposure; the last pass's counts
    step.terminate(sim)
    assert out.read_text() == "0.5, 14, 10, 6, %s\n0.5, 14, 20, 12, %s\n" % (a[4].tolist(), b[4].tolist())
    bare = light.DetectorMeasureStep(None, (0, 0, 0), (0, 0, 1), 1.0, pixels=(3, 2), fov=0.5, measure_n=False)
    sim2 = Sim()
    sim2.launch_note, sim2.steps_per_launch = None, 1
    sim2._k_wanted = lambda: 1                              # one pass per launch was asked for: nothing to say
    bare._device_run(sim2)
    assert sim2.launch_note is None and list(bare.data[0]) == [0.5, 10, 6] and bare.image.sum() == 30
    bare.terminate(sim2)                                    # no file asked for: nothing written


def test_a_loop_with_the_step_is_planned_one_launch_per_light_step():
    from physicl_amd import newton
    sim = phys.Simulation(cl_on=False, rng="philox")
    sim.cl_on, sim._hip = True, _hip                        # (plan as a device run would; no device is opened by planning)
    cam = light.DetectorMeasureStep(None, (0, 0, 0), (0, 0, 1), 1.0)
    steps = [phys.UpdateTimeStep(lambda s: 1.0), newton.NewtonianKinematicsStep(), light.ScatterIsotropicStep(n=1.0, A=1e-9), cam]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim._plan = sim._build_plan()
    assert [k for k, _ in sim._plan] == ["single", "fused", "single"] and sim._plan[-1][1] is cam
    assert sim._multi_eligible() is False


def test_multidevice_sums_the_shards():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def detector_image(self, position, frame, radius, x_edges, y_edges, E_edges=None):
            return np.array([2 * self.k, self.k], dtype=np.int64), np.full((1 if E_edges is None else 2, 2, 3), self.k, dtype=np.int64)
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    counts, image = md.detector_image((0, 0, 0), ALIGNED, 1.0, [0, 1, 2, 3], [0, 1, 2])
    banded = md.detector_image((0, 0, 0), ALIGNED, 1.0, [0, 1, 2, 3], [0, 1, 2], [1.0, 2.0, 3.0])
    md._pool.shutdown()
    assert counts.dtype == np.int64 and counts.tolist() == [222, 111] and image.dtype == np.int64 and image.tolist() == [[[111] * 3] * 2]
    assert banded[1].shape == (2, 2, 3) and np.all(banded[1] == 111)


# ------------------------------------------------------------------------------------------------ binding
class FakeLib:
    """Records the call with the arrays behind its pointers; answers counts 1000, 1001 and cells 2000, 2001, ..."""

    def __init__(self):
        self.calls = []

    def _call(self, name, handle, position, frame, radius, x_edges, nx, y_edges, ny, E_edges, nE, counts, image):
        at = lambda addr, dt, n: np.ctypeslib.as_array((np.ctypeslib.as_ctypes_type(dt) * n).from_address(addr))     # noqa: E731
        self.calls.append((name, handle, at(position, np.float64, 3).tolist(), at(frame, np.float64, 9).tolist(), radius,
                           at(x_edges, np.float64, nx + 1).tolist(), nx, at(y_edges, np.float64, ny + 1).tolist(), ny,
                           None if E_edges is None else at(E_edges, np.float64, nE + 1).tolist(), nE))
        at(counts, np.int64, 2)[:] = [1000, 1001]
        at(image, np.int64, max(nE, 1) * ny * nx)[:] = 2000 + np.arange(max(nE, 1) * ny * nx)
        return 0

    def pcl_step_detector_image(self, *a):
        return self._call("pcl_step_detector_image", *a)

    def pcl_group_step_detector_image(self, *a):
        return self._call("pcl_group_step_detector_image", *a)


@pytest.mark.parametrize("cls,handle,entry", [(_hip.Device, "ctx", ENTRIES[0]), (_hip.DeviceGroup, "g", ENTRIES[1])])
def test_detector_image_marshalling(cls, handle, entry):
    d = cls.__new__(cls)
    d.lib = FakeLib()
    setattr(d, handle, None)
    counts, image = d.detector_image((1, 2, 3), [[0, 1, 0], [0, 0, 1], [1, 0, 0]], 2, [-1, 0, 1, 2], [0, 1, 2], E_edges=[1, 2, 4])
    assert d.lib.calls[0] == (entry, None, [1.0, 2.0, 3.0], [0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0], 2.0, [-1.0, 0.0, 1.0, 2.0], 3,
                              [0.0, 1.0, 2.0], 2, [1.0, 2.0, 4.0], 2)
    assert counts.dtype == np.int64 and counts.tolist() == [1000, 1001]
    assert image.dtype == np.int64 and image.shape == (2, 2, 3) and image.reshape(-1).tolist() == list(range(2000, 2012))      # C order: band, row, column
    counts, image = d.detector_image((1, 2, 3), np.eye(3), 2, [0, 1], [0, 1, 2])
    assert d.lib.calls[1][9:] == (None, 0) and image.shape == (1, 2, 1)                                       # no bands: NULL and 0


def test_header_limits_prototypes_and_the_build_table():
    text = open(build.ABI_HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and len(_hip._PROTOTYPES[entry]) == 12
    for name, value in (("PCL_DETECTOR_MAX_PIXELS", _hip.DETECTOR_MAX_PIXELS), ("PCL_DETECTOR_MAX_BANDS", _hip.DETECTOR_MAX_BANDS),
                        ("PCL_DETECTOR_MAX_CELLS", _hip.DETECTOR_MAX_CELLS)):
        (found,) = re.findall(r"#define\s+%s\s+(\(1 << \d+\)|\d+)" % name, code)
        assert eval(found) == value, name
    assert (_hip.DETECTOR_MAX_PIXELS, _hip.DETECTOR_MAX_BANDS, _hip.DETECTOR_MAX_CELLS) == (1024, 1024, 1 << 20)
    assert 3 * 1025 * 8 < 64 * 1024                         # the largest call's three edge tables fit the LDS a launch may ask for
    assert "wavelength-dependent scatter" in " ".join(text[text.index("What a radiometer sees"):text.index("#define PCL_DETECTOR_MAX_PIXELS")].split())
    assert hasattr(_hip.Device, "detector_image") and hasattr(_hip.DeviceGroup, "detector_image")
    # the table: the unit for crossing tallies holds the sweep behind the shells', described as every sweep is (tests/test_build_cpu.py)
    (unit,) = [u for u in build.ADDONS if os.path.basename(u["src"]) == "pcl_shell.hip"]
    assert unit["sweeps"][1] == dict(entries=ENTRIES, kernel="k_detector_image", count=2)


# ------------------------------------------------------------------------------------------------ the library
def abi_args(**kw):
    """(what must stay alive, the arguments behind the handle, (counts, image)) of a call; ``kw`` replaces arguments, None: NULL."""
    a = dict(position=np.array([0.5, -1.0, 2.0]), frame=ALIGNED.reshape(-1).copy(), radius=0.25, x_edges=np.array([-1.0, 0.0, 1.0]), nx=2,
             y_edges=np.array([-1.0, 1.0]), ny=1, E_edges=np.array([1.0, 2.0, 3.0]), nE=2, counts=np.full(2, -7, np.int64),
             image=np.full(4, -7, np.int64))
    a.update(kw)
    p = lambda x: None if x is None else x.ctypes.data      # noqa: E731
    args = (p(a["position"]), p(a["frame"]), ctypes.c_double(a["radius"]), p(a["x_edges"]), a["nx"], p(a["y_edges"]), a["ny"], p(a["E_edges"]),
            a["nE"], p(a["counts"]), p(a["image"]))
    return a, args, (a["counts"], a["image"])


def frame_with(k, value):
    f = ALIGNED.reshape(-1).copy()
    f[k] = value
    return f


BAD_CALLS = [
    dict(position=None), dict(frame=None), dict(x_edges=None), dict(y_edges=None), dict(E_edges=None), dict(counts=None), dict(image=None),
    dict(position=np.array([0.0, NAN, 0.0])), dict(position=np.array([INF, 0.0, 0.0])), dict(frame=frame_with(0, NAN)), dict(frame=frame_with(4, INF)),
    dict(frame=frame_with(8, 0.0)),                          # a zero n
    dict(radius=0.0), dict(radius=-0.25), dict(radius=NAN), dict(radius=INF), dict(radius=1e200),
    dict(x_edges=np.array([0.0, 0.0, 1.0])), dict(x_edges=np.array([0.0, NAN, 1.0])), dict(x_edges=np.array([0.0, 1.0, INF])), dict(x_edges=np.array([0.0, 1.0, 0.5])),
    dict(y_edges=np.array([1.0, 1.0])), dict(y_edges=np.array([NAN, 1.0])), dict(y_edges=np.array([1.0, -1.0])),
    dict(E_edges=np.array([1.0, 1.0, 2.0])), dict(E_edges=np.array([1.0, NAN, 2.0])), dict(E_edges=np.array([1.0, 2.0, INF])),
    dict(nx=0), dict(nx=-1), dict(nx=1025, x_edges=np.linspace(-1, 1, 1026)), dict(ny=0), dict(ny=1025, y_edges=np.linspace(-1, 1, 1026)),
    dict(nE=-1), dict(nE=1025, E_edges=np.linspace(1, 2, 1026)),
    dict(nx=1024, x_edges=np.linspace(-1, 1, 1025), ny=1024, y_edges=np.linspace(-1, 1, 1025)),              # 2 x 1024 x 1024 cells
    dict(nx=1024, x_edges=np.linspace(-1, 1, 1025), ny=2, y_edges=np.array([0.0, 1.0, 2.0]), nE=1024, E_edges=np.linspace(1, 2, 1025)),
]


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context, which is refused as well); the outputs stay as they
    were."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in [{}] + BAD_CALLS:
        keep, args, (counts, image) = abi_args(**kw)
        assert lib.pcl_step_detector_image(None, *args) == -2, kw
        assert lib.pcl_group_step_detector_image(None, *args) != 0, kw
        assert (counts is None or (counts == -7).all()) and (image is None or (image == -7).all()), kw


# ------------------------------------------------------------------------------------------------ host path
def test_host_path_gives_the_restatement_s_rows(tmp_path):
    cfg = configs()["tilted_1x1_bands"]
    n, n_obj = 300, 20
    r, dr, E, _ = (np.asarray(a, dtype=np.float64) for a in scene(n, "f64", "tilted_1x1_bands"))
    E = np.where(np.isnan(E), 2.0, E)
    sim = phys.Simulation(cl_on=False)                      # (cl_on=True opens its device at once)
    objs = [light.PhotonObject(E=E[k], v=light.c * [1, 0, 0]) for k in range(n - n_obj)] + [phys.Object() for _ in range(n_obj)]
    for o, rr, mm in zip(objs, r, dr):
        o.r, o.dr = np.array(rr, dtype=np.float64), np.array(mm, dtype=np.float64)
    sim.add_objs(objs)
    sim.t = 0.25
    ph = np.arange(n) < n - n_obj
    out = tmp_path / "camera.csv"
    kw = dict(position=cfg["position"], normal=cfg["frame"][2], radius=cfg["radius"], up=cfg["frame"][0])
    a = light.DetectorMeasureStep(str(out), x_edges=cfg["x_edges"], y_edges=cfg["y_edges"], E_bins=E_BANDS, frames=True, **kw)
    b = light.DetectorMeasureStep(None, pixels=(9, 5), fov=(0.9, 0.7), measure_n=False, **kw)
    assert np.allclose(a.frame, cfg["frame"], atol=1e-15)
    for _ in range(2):
        a.run(sim)
        b.run(sim)
    assert sim._dev is None                                 # nothing was uploaded for a measurement of host-resident objects
    counts, image = light._detector_image(r, dr, E, ph, a.position, a.frame, a.radius, a.x_edges, a.y_edges, E_BANDS)
    assert same((counts, image), detector_image_loop(r, dr, E, ph, a.position, a.frame, a.radius, a.x_edges, a.y_edges, E_BANDS))
    row = a.data[1]
    assert row.dtype == object and len(row) == 5 and list(row[:4]) == [0.25, n, counts[0], counts[1]] and np.array_equal(row[4], image)
    assert 0 < image.sum() < counts[1] < counts[0] < n and np.array_equal(a.image, 2 * image) and (a.through, a.seen) == tuple(counts)
    wide = light._detector_image(r, dr, E, ph, b.position, b.frame, b.radius, b.x_edges, b.y_edges)
    assert list(b.data[0]) == [0.25, wide[0][0], wide[0][1]] and np.array_equal(b.image, 2 * wide[1]) and np.count_nonzero(b.image) >= 2
    a.terminate(sim)
    assert out.read_text() == ("0.25, %d, %d, %d, %s\n" % (n, counts[0], counts[1], image.tolist())) * 2
