"""CPU: BoxBoundaryStep (light.BoxBoundaryStep, light._box_walls, pcl_step_box_walls' description) without a device.

* light._box_walls, the numpy restatement, against the per-photon loop of tests/box_walls_reference.py on the edge scene, bit for bit,
  for fp64 and for fp32 stored values, every kind of wall alone and mixed, both boxes; what the rule promises of its images
  (periodic in [lo, hi), mirror in [lo, hi] with |v| kept, a single bounce equal to 2w - x to an ulp of L, open parks).
* every ValueError of the constructor; the host-resident path on Python objects; a second run parks nothing new.
* the sweep's element of the build table, the header's text; the refusals of the library without a device.
"""
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from box_walls_reference import (BAD_CALLS, BOXES, C, GOOD_CALLS, MODE_CODES, N_EDGE, WALLS, abi_args, assert_every_outcome, box_walls_loop,
                                 scene)
from physicl_amd import _hip, build, light, tally
from writer_reference import same_bits

ENTRIES = ("pcl_step_box_walls", "pcl_group_step_box_walls")
FIELDS = ("r", "v", "dr", "dv")


def both(state, modes, lo, hi, dtype):
    args = (state["r"], state["v"], state["dr"], state["dv"], state["photon"], modes, lo, hi)
    return light._box_walls(*args, dtype=dtype), box_walls_loop(*args, dtype=dtype)


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("box", sorted(BOXES))
@pytest.mark.parametrize("walls", sorted(WALLS) + ["x only", "y and z"])
def test_the_restatement_is_the_loop_bit_for_bit(walls, box, dtype):
    modes = WALLS.get(walls) or {"x only": ("mirror", None, None), "y and z": (None, "open", "periodic")}[walls]
    lo, hi = BOXES[box]
    assert N_EDGE % 64 and N_EDGE % 256 and N_EDGE > 2048 + 64
    state = scene(N_EDGE, lo, hi, dtype)
    mine, loop = both(state, modes, lo, hi, dtype)
    what = "%s %s %s" % (walls, box, np.dtype(dtype).name)
    assert mine["counts"].tolist() == loop["counts"].tolist() and mine["crossed"].tolist() == loop["crossed"].tolist(), what
    for f in FIELDS + ("moving", "parked", "folded", "multi", "written"):
        assert same_bits(mine[f], loop[f]), (what, f)
    assert_every_outcome(loop, modes, what)
    assert mine["counts"].dtype == np.int64 and mine["crossed"].shape == (3, 2) and mine["counts"][2:].tolist() == mine["crossed"].reshape(-1).tolist()
    # what is never touched
    still = ~loop["written"]
    for f in FIELDS:
        assert same_bits(loop[f][still], state[f][still]), (what, f)
    assert not loop["written"][~state["photon"]].any() and not loop["moving"][~state["photon"]].any()
    at_rest = (state["v"] == 0).all(axis=1)
    assert at_rest.sum() > 50 and not loop["written"][at_rest].any() and loop["moving"][np.isnan(state["v"][:, 0]) & state["photon"]].all()
    lo, hi = np.array(lo), np.array(hi)
    for a, m in enumerate(modes):
        x0, x1 = state["r"][:, a], loop["r"][:, a]
        fin = np.isfinite(x0)
        assert same_bits(x1[~fin], x0[~fin]), what                     # NaN and +-inf: the axis is skipped
        if m is None or m == "open":
            assert same_bits(x1, x0), (what, a)
        if m == "periodic" and dtype is np.float64:
            who = loop["folded"] & fin
            assert ((x1[who] >= lo[a]) & (x1[who] < hi[a])).all(), (what, a)
            assert (x1[loop["moving"] & ~loop["parked"] & fin] < hi[a]).all() and (x1[loop["moving"] & ~loop["parked"] & fin] >= lo[a]).all()
        if m == "mirror" and dtype is np.float64:
            who = loop["folded"] & fin
            assert ((x1[who] >= lo[a]) & (x1[who] <= hi[a])).all(), (what, a)
    if dtype is np.float64 and "open" not in modes:
        assert same_bits(np.abs(loop["v"]), np.abs(state["v"])) and same_bits(np.abs(loop["dv"]), np.abs(state["dv"]))
        assert same_bits(np.abs(loop["dr"]), np.abs(state["dr"]))      # a mirror only turns the axis round: |v| is kept
    if walls == "periodic":
        for f in ("v", "dr", "dv"):
            assert same_bits(loop[f], state[f]), (what, f)             # periodic writes r alone
    if walls == "open":
        assert same_bits(loop["r"], state["r"]) and same_bits(loop["dr"], state["dr"])
        assert not loop["v"][loop["parked"]].any() and not loop["dv"][loop["parked"]].any()
        assert int(loop["parked"].sum()) == int(loop["crossed"].sum())  # counted once, for the first open axis


@pytest.mark.parametrize("box", sorted(BOXES))
def test_a_single_bounce_is_2w_minus_x_to_an_ulp_of_the_box(box):
    lo, hi = (np.array(x) for x in BOXES[box])
    L = hi - lo
    rng = np.random.RandomState(1)
    n = 4000
    r = lo + L * rng.uniform(-1.0, 2.0, size=(n, 3))
    v = np.tile([C, 0.0, 0.0], (n, 1))
    ref = box_walls_loop(r, v, np.ones((n, 3)), np.ones((n, 3)), np.ones(n, dtype=bool), ("mirror",) * 3, lo, hi)
    for a in range(3):
        below, above = r[:, a] < lo[a], r[:, a] > hi[a]
        want = np.where(below, 2 * lo[a] - r[:, a], np.where(above, 2 * hi[a] - r[:, a], r[:, a]))
        assert below.sum() > 500 and above.sum() > 500
        assert np.abs(ref["r"][:, a] - want).max() <= np.spacing(L[a]) and not ref["multi"].any()
        flipped = below | above
        assert (ref["v"][flipped, a] == -v[flipped, a]).all() and (ref["dr"][flipped, a] == -1.0).all() and (ref["dv"][~flipped, a] == 1.0).all()


def test_open_walls_come_first_and_count_the_first_axis():
    lo, hi = BOXES["unit"]
    r = np.array([[3.0, 0.0, 5.0], [-3.0, 6.5, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [1.0, 1.0, np.nextafter(1.0, 2.0)], [9.0, 0.0, 0.0]])
    v = np.tile([0.0, C, 0.0], (len(r), 1))
    one = np.ones((len(r), 3))
    for restate in (light._box_walls, box_walls_loop):
        ref = restate(r, v, one, one, np.ones(len(r), dtype=bool), ("periodic", "mirror", "open"), lo, hi)
        # slot 0: outside on x (periodic) and z (open): parked, counted for z alone, r untouched; slot 3: x == hi is outside for periodic
        assert ref["parked"].tolist() == [True, False, False, False, True, False] and ref["crossed"].tolist() == [[1, 2], [0, 1], [0, 2]]
        assert same_bits(ref["r"][0], r[0]) and not ref["v"][0].any() and not ref["dv"][0].any() and ref["dr"][0].tolist() == [1, 1, 1]
        assert ref["r"][1].tolist() == [-1.0, -0.5, 0.0] and ref["v"][1].tolist() == [0.0, -C, 0.0]     # x: -3 -> -1; y: 6.5 -> 3 bounces
        assert ref["dr"][1].tolist() == [1.0, -1.0, 1.0] and ref["dv"][1].tolist() == [1.0, -1.0, 1.0]
        assert ref["r"][3].tolist() == [-1.0, 1.0, 1.0] and ref["r"][5].tolist() == [-1.0, 0.0, 0.0]
        assert ref["multi"].tolist() == [False, True, False, False, False, True] and ref["counts"][:2].tolist() == [6, 2]
        two = restate(r, v, one, one, np.ones(len(r), dtype=bool), ("open", None, "open"), lo, hi)
        assert two["crossed"].tolist() == [[1, 2], [0, 0], [0, 1]] and two["parked"].tolist() == [True, True, False, False, True, True]


# ------------------------------------------------------------------------------------------------ the step on the host
class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed = 0.25, 5

    def __init__(self, objs, py=False, steps=None):
        self.objects, self.py, self.steps = objs, py, steps or {}

    def _py_semantics(self):
        return self.py


def objects(state):
    out = []
    for k in range(len(state["photon"])):
        if state["photon"][k]:
            o = phys.light.PhotonObject(E=np.double(state["E"][k]), v=phys.light.c * [1, 0, 0])
        else:
            o = phys.Object()
        o.r = phys.Measurement(np.array(state["r"][k]), "m**1")
        o.v, o.dv = np.array(state["v"][k]), np.array(state["dv"][k])
        o.dr = phys.Measurement(np.array(state["dr"][k]), "m**1")
        out.append(o)
    return out


def test_constructor_keeps_what_it_was_given():
    step = phys.light.BoxBoundaryStep((-1, -2, -3), (1, 2, 3), out_fn="rows.csv")
    assert step.lo.tolist() == [-1, -2, -3] and step.hi.tolist() == [1, 2, 3] and step.walls == ("periodic",) * 3
    assert step.lo.dtype == step.hi.dtype == np.float64
    assert (step._pass, step.data, step.out_fn, step.moving, step.multi, step.parked) == (0, [], "rows.csv", 0, 0, 0)
    assert step.crossed.shape == (3, 2) and step.crossed.dtype == np.int64 and not step.crossed.any()
    assert step._writes == ("r", "dr", "v", "dv")
    mixed = phys.light.BoxBoundaryStep(BOXES["high"][0], BOXES["high"][1], walls=["periodic", None, "open"])
    assert mixed.walls == ("periodic", None, "open")
    assert phys.light.BoxBoundaryStep((0, 0, 0), (1, 1, 1), "mirror").walls == ("mirror",) * 3
    free = phys.light.BoxBoundaryStep((np.nan, 0, 5), (np.inf, 1, 5), walls=(None, "open", None))         # no wall: the bounds are ignored
    assert free.walls == (None, "open", None)
    in_metres = phys.light.BoxBoundaryStep(phys.Measurement(np.array([0.0, 0.0, 0.0]), "m**1"), (1, 1, 1))
    assert in_metres.lo.tolist() == [0, 0, 0]
    import phys.light as short
    cls = light.BoxBoundaryStep
    assert short.BoxBoundaryStep is cls is phys.light.BoxBoundaryStep
    assert cls.__mro__[1] is tally.WriterStep and not set(vars(cls)) & {"run", "_device_run", "_reduce"}
    assert tally.writer_family(step) == cls._STREAM != tally.writer_family(light.RefractiveSurfaceStep(1.0, 1.33)) and "_STREAM" in vars(cls)
    assert "one launch per light step" in cls._NOTE and "BoxBoundaryStep" in cls._NOTE and cls._NOTE != light.RefractiveSurfaceStep._NOTE
    assert cls.terminate is tally.TallyStep.terminate and "image positions" in " ".join(cls.__doc__.split())
    assert _hip.WALL_MODES == MODE_CODES


@pytest.mark.parametrize("kw, word", [
    (dict(walls="closed"), "walls must be one of"), (dict(walls=("periodic", "mirror")), "walls must be one of"), (dict(walls=5), "walls must be one of"),
    (dict(walls=("periodic", "mirror", 3)), "walls must be one of"), (dict(walls=None), "a wall on one axis at least"),
    (dict(walls=(None, None, None)), "a wall on one axis at least"), (dict(lo="abc"), "lo must be three numbers"), (dict(lo=(0, 0)), "lo must be three numbers"),
    (dict(hi=5.0), "hi must be three numbers"), (dict(hi=(1, 1, 1, 1)), "hi must be three numbers"), (dict(lo=(np.nan, 0, 0)), "axis x"),
    (dict(hi=(1, np.inf, 1)), "axis y"), (dict(lo=(0, 0, 1)), "axis z"), (dict(lo=(0, 0, 2)), "axis z"),
    (dict(lo=(-1e308, 0, 0), hi=(1e308, 1, 1)), "axis x"), (dict(walls=("open", None, None), lo=(3, 0, 0)), "hi - lo > 0")])
def test_constructor_refusals(kw, word):
    args = dict(lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), walls="periodic")
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        phys.light.BoxBoundaryStep(**args)


@pytest.mark.parametrize("py", [False, True])
@pytest.mark.parametrize("walls", sorted(WALLS))
def test_host_resident_objects_get_the_restatement_s_state(tmp_path, walls, py):
    lo, hi = BOXES["unit"]
    modes = WALLS[walls]
    state = scene(400, lo, hi)
    state["r"][~np.isfinite(state["r"])] = 0.25                         # (a Measurement of the host path holds numbers)
    objs = objects(state)
    before = {f: tally.vec3(objs, f) for f in FIELDS}
    E0 = tally.photon_energies(objs, phys.light.PhotonObject)[0]
    step = phys.light.BoxBoundaryStep(lo, hi, modes, out_fn=str(tmp_path / "walls.csv"))
    sim = HostSim(objs, py=py, steps={0: phys.newton.NewtonianKinematicsStep(), 1: step})
    step.run(sim)                                                      # reads no dv rule: works under cl_on=False as well
    ref = box_walls_loop(before["r"], before["v"], before["dr"], before["dv"], state["photon"], modes, lo, hi)
    assert_every_outcome(ref, modes, "host " + walls)
    assert (step.moving, step.multi) == tuple(ref["counts"][:2].tolist()) and same_bits(step.crossed, ref["crossed"]) and step._pass == 1
    assert step.parked == int(ref["parked"].sum()) == sum(int(ref["crossed"][a].sum()) for a in range(3) if modes[a] == "open")
    row = list(step.data[0])
    assert row[:3] == [0.25, step.moving, step.multi] and same_bits(row[3], ref["crossed"]) and sim.launch_note is None
    after = {f: tally.vec3(objs, f) for f in FIELDS}
    for f in FIELDS:
        assert same_bits(after[f], ref[f]), (walls, f)
    assert same_bits(tally.photon_energies(objs, phys.light.PhotonObject)[0], E0)
    if walls in ("mirror", "periodic"):
        assert same_bits(np.abs(after["v"]), np.abs(before["v"]))      # mirror keeps |v|; periodic leaves v, dr and dv untouched
    if walls == "periodic":
        assert all(same_bits(after[f], before[f]) for f in ("v", "dr", "dv"))
    first = (step.moving, step.parked, step.crossed.copy())
    step.run(sim)                                                      # a second run: everybody is inside or at rest
    assert step._pass == 2 and step.parked == 0 and not step.crossed.any() and step.multi == 0
    assert step.moving == first[0] - first[1]
    for f in FIELDS:
        assert same_bits(tally.vec3(objs, f), after[f]), (walls, f)
    step.terminate(sim)
    lines = open(str(tmp_path / "walls.csv")).read().splitlines()
    assert len(lines) == 2 and lines[0] == "0.25, %d, %d, %s" % (first[0], int(ref["counts"][1]), first[2].tolist())


def test_a_simulation_of_python_objects_runs_the_step_behind_newton():
    """Through ``Simulation`` with host-resident Python objects: Newton moves them out of a small periodic box, the step hands
    them back in, pass by pass."""
    lo, hi = (0.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    rng = np.random.RandomState(4)
    photons = []
    for k in range(40):
        d = rng.normal(size=3)
        o = phys.light.PhotonObject(E=np.double(2.0), v=phys.light.c * [1, 0, 0])
        o.v, o.dv = C * d / np.sqrt((d * d).sum()), np.zeros(3)
        o.r = phys.Measurement(np.array([0.5, 0.0, 0.0]), "m**1")
        photons.append(o)
    step = phys.light.BoxBoundaryStep(lo, hi, ("periodic", "mirror", "mirror"))
    speed = [np.sqrt((np.asarray(o.v, dtype=np.float64) ** 2).sum()) for o in photons]
    sim = phys.Simulation(cl_on=False, seed=5)
    sim.add_objs(photons)
    sim.add_step(0, step)
    crossed = np.zeros((3, 2), dtype=np.int64)
    for n_pass in range(12):
        for o in photons:                                              # a Newton move of 0.7: more than half the box in x
            move = np.asarray(o.v, dtype=np.float64) * (0.7 / C)
            o.r = phys.Measurement(np.asarray(o.r, dtype=np.float64) + move, "m**1")
            o.dr = phys.Measurement(move, "m**1")
        step.run(sim)
        crossed += step.crossed
        r = tally.vec3(photons, "r")
        assert ((r[:, 0] >= 0.0) & (r[:, 0] < 1.0) & (np.abs(r[:, 1:]) <= 1.0).all(axis=1)).all() and step.moving == 40
    assert (crossed > 0).all() and step._pass == 12 == len(step.data)
    for o, s in zip(photons, speed):
        assert abs(np.sqrt((np.asarray(o.v, dtype=np.float64) ** 2).sum()) - s) <= 2 * np.spacing(s)


def test_device_run_hands_the_walls_to_the_device_and_reduces_once():
    class Dev:
        count = 9
        calls = []

        def box_walls(self, *a):
            Dev.calls.append(a)
            return np.array([9, 1, 1, 2, 0, 0, 3, 4])

    class Sim:
        t, seed, launch_note, steps = 0.5, 1, None, {}
        _dev, globals_ = Dev(), []

        def _k_wanted(self):
            return 4

        def _global(self, flat):
            Sim.globals_.append(list(flat))
            return 2 * np.asarray(flat)
    step = phys.light.BoxBoundaryStep((0, 0, 0), (1, 2, 3), ("periodic", None, "open"))
    sim = Sim()
    step._device_run(sim)
    (a,) = Dev.calls
    assert a[0] == ("periodic", None, "open") and a[1].tolist() == [0, 0, 0] and a[2].tolist() == [1, 2, 3] and len(a) == 3
    assert Sim.globals_ == [[9, 9, 1, 1, 2, 0, 0, 3, 4]] and sim.launch_note == step._NOTE and sim._scattered is True
    assert (step.moving, step.multi, step.parked) == (18, 2, 14) and step.crossed.tolist() == [[2, 4], [0, 0], [6, 8]]
    assert list(step.data[0])[:3] == [0.5, 18, 2] and step._n_pass == 1


def test_multi_device_sums_the_shards_counts():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def box_walls(self, *a, **kw):
            return self.k * np.arange(8)
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    counts = md.box_walls(("periodic",) * 3, (0, 0, 0), (1, 1, 1))
    md._pool.shutdown()
    assert np.asarray(counts).tolist() == (111 * np.arange(8)).tolist()


def test_binding_marshals_the_call():
    import ctypes

    def entry(handle, modes, lo, hi, counts):
        dbl = lambda q: np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_double)), (3,)).tolist()            # noqa: E731
        seen.append((handle, np.ctypeslib.as_array(ctypes.cast(modes, ctypes.POINTER(ctypes.c_int32)), (3,)).tolist(), dbl(lo), dbl(hi)))
        np.ctypeslib.as_array(ctypes.cast(counts, ctypes.POINTER(ctypes.c_int64)), (8,))[:] = np.arange(8)
        return 0
    seen = []
    counts = _hip._box_walls(entry, "h", ("periodic", None, "open"), (0, 1, 2), [3.5, 4, 5])
    assert counts.tolist() == list(range(8)) and counts.dtype == np.int64
    _hip._box_walls(entry, "g", (2, 2, 0), np.zeros(3), np.ones(3))
    assert seen == [("h", [1, 0, 3], [0.0, 1.0, 2.0], [3.5, 4.0, 5.0]), ("g", [2, 2, 0], [0.0, 0.0, 0.0], [1.0, 1.0, 1.0])]
    assert len(_hip._PROTOTYPES[ENTRIES[0]]) == len(_hip._PROTOTYPES[ENTRIES[1]]) == 5


# ------------------------------------------------------------------------------------------------ the library
def surface_unit():
    (unit,) = [u for u in build.ADDONS if os.path.basename(u["src"]) == "pcl_surface.hip"]
    return unit


def test_header_prototypes_and_the_build_table():
    text = open(build.ABI_HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and len(_hip._PROTOTYPES[entry]) == 5
    for name, value in (("NONE", 0), ("PERIODIC", 1), ("MIRROR", 2), ("OPEN", 3)):
        assert re.search(r"#define PCL_WALL_%s %d\b" % (name, value), code), name
    assert re.search(r"#define PCL_ABI_VERSION 1\b", code)
    flat = " ".join(text.split()).replace("* ", "")
    for line in ("s = x - lo; n = floor(s / L); f = min(max(s - n*L, 0), L)", "y = lo + f; if not (y < hi): y = lo; r_a = y",
                 "h = n 0.5; odd = floor(h) != h; y = odd ? hi - f : lo + f; y = min(max(y, lo), hi)", "v_a = -v_a, dv_a = -dv_a, dr_a = -dr_a",
                 "above = x >= hi (PCL_WALL_PERIODIC", "above = x > hi (PCL_WALL_MIRROR, PCL_WALL_OPEN", "-0.0 counts as 0; a NaN in v: moving",
                 "for the FIRST such axis a in the order x, y, z", "r and dr are left alone", "n < -1 or n > 1", "48 B a slot",
                 "The call takes no seed, no pass and no c", "0-5 and 8-26 are taken", "moving, multi, crossed[3][2]",
                 "is not written at all", "fmin and fmax"):
        assert line in flat, line                                      # the rule is written out
    assert hasattr(_hip.Device, "box_walls") and hasattr(_hip.DeviceGroup, "box_walls")
    from physicl_amd.multidev import MultiDevice
    assert hasattr(MultiDevice, "box_walls")
    # the table: the unit of the writer sweeps holds this one last, described as every sweep is (tests/test_build_cpu.py checks it as one)
    assert surface_unit()["sweeps"][-1] == dict(entries=ENTRIES, kernel="k_box_walls", count=2)
    assert build.csrc_sha() == "b54e0443ee3f400f"                       # the tuned core has not moved
    src = open(os.path.join(build.CSRC, "pcl_surface.hip")).read()
    body = src[src.index("void __launch_bounds__(kBlock) k_box_walls"):src.index("struct walls_spec")]
    assert src.index("k_box_walls(walls_args<T> a)") > src.index("int group_scatter_grid(")                # at the end of the unit
    assert "pcl_philox" not in body and "id_of(" not in body and "asm" not in body and "flush_cells(" not in body
    assert body.index("if (!work) continue;") > body.rindex("__ballot(") and "balanced_grid" in src[src.index("int launch_walls("):]


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context and a NULL group, refused as well); the counts stay as
    they were."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in BAD_CALLS + GOOD_CALLS:                                   # a good call without a context is refused, too
        keep, args, counts = abi_args(**kw)
        assert lib.pcl_step_box_walls(None, *args) == -2, kw
        assert (lib.pcl_group_step_box_walls(None, *args) == -2) or kw in GOOD_CALLS, kw
        assert lib.pcl_group_step_box_walls(None, *args) != 0, kw
        assert counts is None or (counts == -7).all(), kw
