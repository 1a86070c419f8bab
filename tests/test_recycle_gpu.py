"""GPU: RecycleStep (pcl_step_recycle_spent, light.RecycleStep).

* ``Device.recycle_spent`` against the numpy restatement (light._recycle_spent) on a state that is uploaded explicitly
  (tests/recycle_reference.py: ``layout``), downloaded before and after the call: N at the wave, workgroup and tile edges and one
  size at which a workgroup takes more than one trip, fp64 and fp32 stores, without and with a spectrum.  Tallies are exact; every
  field of every particle that is not spent is bit-identical, without a spectrum all of E, ids and kinds always; dr and dv of the
  spent are exactly 0, table energies the restatement's bit for bit; v and r of the spent lie within the bounds
  tests/test_gpu_source.py states for the same arithmetic (exact for a beam and a point).
* each angular and each spatial mode; a store with explicit ids in scrambled order and plain Objects; two passes; either
  criterion alone; the refusals; an empty store; a device group; the step through ``Simulation``.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import light
from recycle_reference import BAD_CALLS, C, CDF, CENTER, FIELDS, GRID, ID_BASE, SEED, TOP, abi_args, check_recycle, expected_masks, \
    layout, source, wide
from writer_reference import same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 2047, 2048, 2049]


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


def upload(dev, n, dtype, ids=None, kind=None):
    state = dict(layout(n, np.float32 if dtype == "f32" else np.float64), id_base=ID_BASE)
    if ids is not None:
        state["id"] = ids
    if kind is not None:
        state["kind"] = kind
    dev.store_alloc(n, dtype)
    dev.upload_state(state)
    return dev.download_state()


def check_call(dev, n, dtype, src, n_pass, top=TOP, at_rest=True, spectrum=None, ids=None, kind=None):
    before = upload(dev, n, dtype, ids, kind)
    photon = None if kind is None else kind != 0
    counts = dev.recycle_spent(src, C, at_rest, top, CENTER, spectrum, SEED, n_pass)
    after = dev.download_state()
    what = "recycle n=%d %s %s/%s pass %d%s%s" % (n, dtype, src.angular, src.spatial, n_pass, " table" if spectrum else "", " ids" if ids is not None else "")
    ref = check_recycle(before, after, counts, src, top, CENTER, at_rest, spectrum, SEED, n_pass, what, photon)
    if kind is not None:
        assert np.array_equal(dev.download_kind(), kind), what
    rest, gone = expected_masks(n, at_rest, top is not None, photon)
    assert np.array_equal(ref["at_rest"], rest) and np.array_equal(ref["escaped"], gone), what
    # behind the step no photon is spent: the source lies inside the top
    assert dev.recycle_spent(src, C, at_rest, top, CENTER, spectrum, SEED, n_pass + 1) == (0, 0), what
    again = dev.download_state()
    for f in FIELDS + ("E",):
        assert same_bits(np.asarray(again[f]), np.asarray(after[f])), (what, f)
    return counts, before, after, ref


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_particle_against_the_numpy_restatement(dev, n, dtype):
    src = source("cone", "gaussian")
    for n_pass, spectrum in ((1, None), (2, (GRID, CDF))):
        counts, _, _, _ = check_call(dev, n, dtype, src, n_pass, spectrum=spectrum)
        assert dev.is_uniform()
        if n >= 255:
            assert counts[0] > 0 and counts[1] > 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_workgroup_takes_more_than_one_trip(dev, dtype):
    n = dev.info()["compute_units"] * 8 * 256 + 77                     # just above the grid's cap of resident workgroups
    counts, _, _, _ = check_call(dev, n, dtype, source("isotropic", "disc"), 3, spectrum=(GRID, CDF))
    assert counts[0] > n // 4 and counts[1] > n // 10


@pytest.mark.parametrize("angular, spatial", [("beam", "point"), ("isotropic", "disc"), ("cone", "gaussian"), ("lambertian", "point"),
                                              ("beam", "disc")])
def test_each_mode_of_the_source(dev, angular, spatial):
    for dtype in ("f64", "f32"):
        check_call(dev, 2049, dtype, source(angular, spatial), 4)
    check_call(dev, 2049, "f64", source(angular, spatial, oblique=False), 5)


def test_either_criterion_alone(dev):
    src = source()
    rest_only, _, _, _ = check_call(dev, 4097, "f64", src, 1, top=None)
    top_only, _, _, _ = check_call(dev, 4097, "f64", src, 1, at_rest=False)
    both, _, _, _ = check_call(dev, 4097, "f64", src, 1)
    assert rest_only[1] == 0 and top_only[0] == 0 and rest_only[0] == both[0] > 0
    assert top_only[1] > both[1] > 0                                   # at rest outside the top: counted as at rest when both are on


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_store_that_is_not_uniform(dev, hip, dtype):
    n = 2049
    ids = ID_BASE + 3 * np.random.RandomState(5).permutation(n).astype(np.int64)            # explicit, not consecutive
    kind = np.where(np.arange(n) % 4 == 1, hip.KIND_OBJECT, hip.KIND_PHOTON).astype(np.uint8)
    counts, before, after, ref = check_call(dev, n, dtype, source(), 6, spectrum=(GRID, CDF), ids=ids, kind=kind)
    assert not dev.is_uniform() and counts[0] > 0 and counts[1] > 0
    obj = kind == hip.KIND_OBJECT
    b, a = wide(before), wide(after)
    for f in FIELDS:                                                   # Objects at rest or outside are untouched
        assert same_bits(a[f][obj], b[f][obj]), f
    assert not ref["spent"][obj].any() and ((np.arange(n) % 3 == 0) & obj).any()
    # the draws follow the ids: the same ids in store order give other photons the draws
    plain = light._recycle_spent(b["r"], b["v"], np.asarray(before["E"], dtype=np.float64), ~obj, ID_BASE + np.arange(n), source(), TOP,
                                 CENTER, True, (GRID, CDF), C, SEED, 6)
    assert not np.array_equal(plain["v"][ref["spent"]], ref["v"][ref["spent"]])


def test_two_passes_give_a_slot_two_directions(dev):
    src = source()
    out = []
    for n_pass in (1, 2):
        _, _, after, ref = check_call(dev, 2049, "f64", src, n_pass)
        out.append((wide(after), ref["spent"]))
    spent = out[0][1]
    assert np.array_equal(spent, out[1][1]) and spent.sum() > 500
    assert not (out[0][0]["v"][spent] == out[1][0]["v"][spent]).all(axis=1).any()
    assert not (out[0][0]["r"][spent] == out[1][0]["r"][spent]).all(axis=1).any()


def test_refused_calls_and_an_empty_store(dev, hip):
    before = upload(dev, 300, "f64")
    for kw in BAD_CALLS:
        keep, args, counts = abi_args(hip, **kw)
        assert dev.lib.pcl_step_recycle_spent(dev.ctx, *args) == -2, kw
        assert counts is None or (counts == -7).all(), kw
    after = dev.download_state()
    for f in FIELDS:
        for k in range(3):
            assert same_bits(after[f][k], before[f][k]), f
    assert same_bits(after["E"], before["E"])
    keep, good, counts = abi_args(hip)
    rest, gone = expected_masks(300)
    assert dev.lib.pcl_step_recycle_spent(dev.ctx, *good) == 0 and counts.tolist() == [rest.sum(), gone.sum(), -7, -7]      # two values, no more
    assert np.isin(dev.download(hip.E)[rest | gone], GRID).all()
    dev.set_count(0, 0)
    assert dev.recycle_spent(source(), C, True, TOP, CENTER, None, SEED, 1) == (0, 0)
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.recycle_spent(source(), C, True, TOP, CENTER, None, SEED, 1)
    assert e.value.code == -3
    bare.close()


def test_device_group_gives_the_unsharded_store(dev, hip):
    n = 3 * 2048 + 77
    src = source("lambertian", "gaussian")
    before = upload(dev, n, "f64")
    whole = dev.recycle_spent(src, C, True, TOP, CENTER, (GRID, CDF), SEED, 4)
    with hip.DeviceGroup([0, 0]) as g:
        g.store_alloc(n)
        g.fill_photons(n, ID_BASE, C, 1.0, 2.0, SEED)
        for i in range(2):                                             # the shards' rows through their own contexts
            lo, hi = g.shard(n, i)
            ctx = hip.c_void_p()
            hip.check(g.lib.pcl_group_ctx(g.g, i, hip.byref(ctx)))
            for f, name in ((f, name) for name in FIELDS for f in hip.FIELD_GROUPS[name]):
                col = np.ascontiguousarray(before[name][f - hip.FIELD_GROUPS[name][0]][lo:hi])
                hip.check(g.lib.pcl_store_upload(ctx, f, col.ctypes.data, 0, hi - lo))
            col = np.ascontiguousarray(before["E"][lo:hi])
            hip.check(g.lib.pcl_store_upload(ctx, hip.E, col.ctypes.data, 0, hi - lo))
        got = g.recycle_spent(src, C, True, TOP, CENTER, (GRID, CDF), SEED, 4)
        assert got == whole and whole[0] > 0 and whole[1] > 0
        for f in range(hip.E + 1):
            assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            g.recycle_spent(src, C, False, None, CENTER, None, SEED, 4)                     # neither criterion
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 4096, 20
STEP = 0.5                             # length of a move: A*n*|dr| = 0.5, about half of the photons interact per pass
DT = STEP / C
GROUND, TOP_SIM = 1.0, 4.0
SRC_SIM = dict(origin=(2.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), angular="isotropic")


def atmosphere(passes, recycle=True, devices=None):
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, devices=devices, exit=lambda s: len(s.ts) >= passes)
    src = phys.light.PhotonSource(**SRC_SIM)
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
    sim.add_step(3, phys.light.AbsorptionStep(omega0=0.5))
    sim.add_step(4, phys.light.SurfaceReflectStep(GROUND, albedo=0.0))
    step = phys.light.RecycleStep(src, top=TOP_SIM)
    if recycle:
        sim.add_step(5, step)
    return sim, step


def run(sim):
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    return sim


def spent_now(sim):
    r, v = sim.download("r"), sim.download("v")
    rest = (v == 0).all(axis=1)
    gone = ~rest & ((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2] > TOP_SIM * TOP_SIM)
    return int(rest.sum()), int(gone.sum())


class Count(phys.DeviceStep):
    """Behind the RecycleStep: the store's count, pass by pass."""
    _fuse_role = None

    def __init__(self):
        self.counts = []

    def _device_run(self, sim):
        self.counts.append(sim._dev.count)


class AllButTheLast(phys.light.RecycleStep):
    """The twin's step: it stops in front of the last pass's sweep and downloads what that sweep would find."""
    found = None

    def _device_run(self, sim):
        if self._pass == PASSES - 1:
            self.found = spent_now(sim)
            return
        phys.light.RecycleStep._device_run(self, sim)


def test_the_population_is_constant_and_the_counts_are_the_spent_photons():
    sim, step = atmosphere(PASSES)
    look = Count()
    sim.add_step(6, look)
    run(sim)
    rows = [[int(x) for x in row[1:]] for row in step.data]
    assert len(rows) == PASSES == step._pass and look.counts == [N_SIM] * PASSES and len(sim.objects) == N_SIM       # the count never changes
    assert step.recycled == sum(rows[-1]) and all(a > 0 for a, _ in rows) and sum(b for _, b in rows) > 0
    print("recycled per pass (at rest, escaped):", rows)
    assert spent_now(sim) == (0, 0)                                    # behind the step nobody is spent
    assert "one launch per light step" in sim.launch_note
    assert sim.schedule["fused"] == PASSES and not sim.schedule["fused_multi"]
    ids = sim.download("id")
    assert np.array_equal(np.sort(ids), np.arange(N_SIM) + ids.min())  # ids are never written
    sim.close(download=False)

    # a twin with the same seed, stopped one step earlier: a download finds the photons the last sweep counted
    twin, _ = atmosphere(PASSES, recycle=False)
    twin_step = AllButTheLast(phys.light.PhotonSource(**SRC_SIM), top=TOP_SIM)
    twin.add_step(5, twin_step)
    run(twin)
    assert [[int(x) for x in row[1:]] for row in twin_step.data] == rows[:-1]
    assert list(twin_step.found) == rows[-1], (twin_step.found, rows[-1])
    twin.close(download=False)


def test_without_the_step_the_spent_photons_pile_up():
    sim, _ = atmosphere(PASSES, recycle=False)
    run(sim)
    rest, gone = spent_now(sim)
    assert rest > N_SIM // 2 and rest + gone > 0.9 * N_SIM             # after 20 passes nearly everybody is dead weight
    sim.close(download=False)


def test_two_contexts_on_one_gpu_give_the_unsharded_run():
    out = []
    for devices in (None, [0, 0]):
        sim, step = atmosphere(6, devices=devices)
        run(sim)
        order = np.argsort(sim.download("id"))
        out.append((sim.download("r")[order], sim.download("v")[order], [[int(x) for x in row[1:]] for row in step.data]))
        sim.close(download=False)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and min(row[0] for row in out[0][2]) > 0
