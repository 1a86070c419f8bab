"""GPU: BoxBoundaryStep (pcl_step_box_walls, light.BoxBoundaryStep).

* ``Device.box_walls`` against the per-photon loop of tests/box_walls_reference.py (Python floats, no light.py) on the edge scene,
  uploaded explicitly and downloaded before and after the call, N = 3001 (a tile and a half, a ragged last wave), fp64 and fp32
  stores, each kind of wall alone and the mixed ("periodic", "mirror", "open"), both boxes, on a uniform store and on one with plain
  Objects and ids of its own: every slot of r, v, dr and dv and the eight counts bit for bit, no tolerance; a second call on what
  the first left; walls on one axis and on two; the refusals, an empty store, no store; a device group.
* through ``Simulation``: 500 photons, 20 passes of Newton, a GridScatterStep and the box (mirror in x, periodic in y and z), every
  pass replayed from the probed state in front of the step with light._box_walls, the numpy restatement the host path answers with
  (tests/test_writer_walls_cpu.py holds it bit for bit to the loop), every photon in [lo, hi) on the periodic axes after every pass.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
import writer_reference as W
from box_walls_reference import (BAD_CALLS, BOXES, C, GOOD_CALLS, N_EDGE, WALLS, abi_args, assert_every_outcome, box_walls_loop,
                                 check_box_walls, scene, upload_state)
from physicl_amd import light
from writer_reference import same_bits

pytestmark = pytest.mark.gpu

ID_BASE = W.ID_BASE
FIELDS = ("r", "v", "dr", "dv")


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


def np_type(dtype):
    return np.float32 if dtype == "f32" else np.float64


def upload(dev, state, dtype, mixed=False, ids=None):
    fields, kind = upload_state(state)
    fields = dict(fields, id_base=ID_BASE)
    if ids is not None:
        fields["id"] = ids
    if mixed:
        fields["kind"] = kind
    dev.store_alloc(len(state["E"]), dtype)
    dev.upload_state(fields)
    return W.snapshot(dev)


def check_call(dev, before, modes, lo, hi, what, every=True):
    counts = dev.box_walls(modes, lo, hi)
    after = W.snapshot(dev)
    ref = check_box_walls(before, after, counts, modes, lo, hi, what)
    if every:
        assert_every_outcome(ref, modes, what)
    return counts, after, ref


@pytest.mark.parametrize("mixed", [False, True], ids=["uniform", "objects"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("box", sorted(BOXES))
@pytest.mark.parametrize("walls", sorted(WALLS))
def test_every_particle_against_the_plain_loop(dev, walls, box, dtype, mixed):
    modes, (lo, hi) = WALLS[walls], BOXES[box]
    state = scene(N_EDGE, lo, hi, np_type(dtype))
    ids = ID_BASE + 3 * np.random.RandomState(5).permutation(N_EDGE).astype(np.int64) if mixed else None
    before = upload(dev, state, dtype, mixed=mixed, ids=ids)
    assert dev.is_uniform() != mixed
    what = "%s %s %s %s" % (walls, box, dtype, "objects" if mixed else "uniform")
    counts, after, ref = check_call(dev, before, modes, lo, hi, what)
    assert counts.dtype == np.int64 and counts.shape == (8,)
    if mixed:
        obj = ~state["photon"]
        a, b = W.wide(after), W.wide(before)
        assert obj.sum() > 200 and not ref["written"][obj].any() and all(same_bits(a[f][obj], b[f][obj]) for f in FIELDS)
    else:
        assert counts[0] > ref["moving"][state["photon"]].sum()        # without kinds the Objects' slots are photons
    # a second call on what the first left: nobody is outside a wall any more, and who was parked is at rest
    again, last, ref2 = check_call(dev, after, modes, lo, hi, what + ", second call", every=False)
    if dtype == "f64":                                                 # (an fp32 store rounds an image once more: it may land on hi)
        assert not again[1:].any() and again[0] == counts[0] - int(ref["parked"].sum()), what
        W.assert_same_state(last, after, what + ": the second call writes nothing")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("modes", [("mirror", None, None), (None, "open", "periodic"), (None, None, "periodic"), ("open", "open", None)],
                         ids=["x", "yz", "z", "xy"])
def test_axes_without_a_wall_are_not_read(dev, modes, dtype):
    lo, hi = BOXES["high"]
    before = upload(dev, scene(N_EDGE, lo, hi, np_type(dtype)), dtype, mixed=True)
    bad = [np.nan if m is None else x for m, x in zip(modes, lo)], [-np.inf if m is None else x for m, x in zip(modes, hi)]
    counts, after, ref = check_call(dev, before, modes, bad[0], bad[1], "%r %s" % (modes, dtype))
    for a, m in enumerate(modes):
        if m is None or m == "open":
            assert same_bits(W.wide(after)["r"][:, a], W.wide(before)["r"][:, a])


def test_refused_calls_an_empty_store_and_no_store(dev, hip):
    lo, hi = BOXES["unit"]
    before = upload(dev, scene(300, lo, hi), "f64")
    for kw in BAD_CALLS:
        keep, args, counts = abi_args(**kw)
        assert dev.lib.pcl_step_box_walls(dev.ctx, *args) == -2, kw
        assert counts is None or (counts == -7).all(), kw
    W.assert_same_state(W.snapshot(dev), before, "a refused call writes nothing")
    with pytest.raises(hip.HipError) as e:
        dev.box_walls((None, None, None), lo, hi)
    assert e.value.code == -2
    for kw in GOOD_CALLS:
        keep, good, counts = abi_args(**kw)
        assert dev.lib.pcl_step_box_walls(dev.ctx, *good) == 0, kw
        assert (counts[8:] == -7).all() and (counts[:8] >= 0).all() and counts[0] > 0      # eight counts, no more
    dev.set_count(0, 0)
    empty = dev.box_walls(("periodic", "mirror", "open"), lo, hi)
    assert empty.shape == (8,) and not empty.any()
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.box_walls("periodic periodic periodic".split(), lo, hi)
    assert e.value.code == -3
    bare.close()


def test_device_group_gives_the_unsharded_store(dev, hip):
    n = 3 * 2048 + 77
    lo, hi = BOXES["unit"]
    modes = WALLS["mixed"]
    before = upload(dev, scene(n, lo, hi), "f64")
    whole = dev.box_walls(modes, lo, hi)
    with hip.DeviceGroup([0, 0]) as g:
        g.store_alloc(n)
        g.fill_photons(n, ID_BASE, C, 1.0, 2.0, 5)
        for i in range(2):                                             # the shards' rows through their own contexts
            a, b = g.shard(n, i)
            ctx = hip.c_void_p()
            hip.check(g.lib.pcl_group_ctx(g.g, i, hip.byref(ctx)))
            for f, name in ((f, name) for name in FIELDS for f in hip.FIELD_GROUPS[name]):
                col = np.ascontiguousarray(before[name][f - hip.FIELD_GROUPS[name][0]][a:b])
                hip.check(g.lib.pcl_store_upload(ctx, f, col.ctypes.data, 0, b - a))
            col = np.ascontiguousarray(before["E"][a:b])
            hip.check(g.lib.pcl_store_upload(ctx, hip.E, col.ctypes.data, 0, b - a))
        got = g.box_walls(modes, lo, hi)
        assert got.tolist() == whole.tolist() and (whole[2:].reshape(3, 2) > 0).all() and whole[1] > 0
        for f in range(hip.E + 1):
            assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            g.box_walls(modes, hi, lo)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 500, 20
STEP = 0.5                             # length of a move: the box is 4 wide, so walls are met from the fourth pass on
DT = STEP / C
SIM_LO, SIM_HI = (0.0, -2.0, -2.0), (4.0, 2.0, 2.0)
SIM_WALLS = ("mirror", "periodic", "periodic")
SIM_EDGES = [np.linspace(0.0, 4.0, 9), np.linspace(-2.0, 2.0, 9), np.linspace(-2.0, 2.0, 9)]
ix, iy, iz = np.indices((8, 8, 8))
FIELD_K = np.where((iy + iz) % 2 == 0, 1.2, 0.0)                       # columns along x, cloudy and clear in a checkerboard
STATE = ("r", "v", "dr", "dv", "E", "id")


class Look(phys.DeviceStep):
    """The store as it stands, pass by pass."""
    _fuse_role = None

    def __init__(self):
        self.states = []

    def _device_run(self, sim):
        self.states.append({f: sim.download(f) for f in STATE})


def test_a_cloud_field_in_a_box_replays_from_the_probed_states():
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=lambda s: len(s.ts) >= PASSES)
    src = phys.light.PhotonSource(origin=(2.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), angular="isotropic")
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    field = phys.light.GridScatterStep(FIELD_K, ("x", "y", "z"), SIM_EDGES)
    box = phys.light.BoxBoundaryStep(SIM_LO, SIM_HI, SIM_WALLS)
    looks = [Look(), Look()]
    steps = [phys.UpdateTimeStep(lambda s: np.double(DT)), phys.newton.NewtonianKinematicsStep(), field, looks[0], box, looks[1]]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    note = sim.launch_note
    sim.close(download=False)
    assert box._pass == PASSES == len(box.data) == len(field.data) and note is not None and "one launch per light step" in note
    total = np.zeros((3, 2), dtype=np.int64)
    lo, hi = np.array(SIM_LO), np.array(SIM_HI)
    for k in range(PASSES):
        s0, s1 = (look.states[k] for look in looks)
        row = box.data[k]
        what = "pass %d" % (k + 1)
        counts = np.concatenate([[row[1], row[2]], np.asarray(row[3]).reshape(-1)])
        check_box_walls(s0, s1, counts, SIM_WALLS, SIM_LO, SIM_HI, what, restate=light._box_walls)
        r = W.wide(s1)["r"]
        assert ((r[:, 1:] >= lo[1:]) & (r[:, 1:] < hi[1:])).all() and ((r[:, 0] >= lo[0]) & (r[:, 0] <= hi[0])).all(), what
        assert int(row[1]) == N_SIM and int(row[2]) == 0, what         # everybody moves; a move is an eighth of the box
        total += np.asarray(row[3])
    print("crossed over %d passes: %s; scattered %d" % (PASSES, total.tolist(), sum(int(row[2]) for row in field.data)))
    assert (total > 0).all() and sum(int(row[2]) for row in field.data) > 0
