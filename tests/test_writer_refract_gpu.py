"""GPU: RefractiveSurfaceStep (pcl_step_refract_surface, light.RefractiveSurfaceStep).

* ``Device.refract_surface`` against the numpy restatement (light._refract_surface) WITHOUT A TOLERANCE: a state that is uploaded
  explicitly (tests/refract_reference.py: ``scene`` -- a sphere of radius 1, n_inside = 1.5, a third of the photons crossing inward,
  a third outward, a third not at all, and every special slot of it), downloaded before and after the call; r, v, dr and dv of every
  slot bit for bit, and the six counts.  N at the wave and tile edges, several tiles with a ragged tail, one size past the grid's
  first stride, a capacity beyond N, fp64 and fp32 stores, fresnel True and False, two consecutive passes.
* everybody crossing; nobody crossing (the store untouched bit for bit); scrambled ids and plain Objects; the refusals; an empty
  store; no store; a device group of two shards; the step through ``Simulation``: a beam through a drop of n = 4/3 with a shell tally
  of the same radius in front, with cl_on=True and cl_on=False.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from refract_reference import BAD_CALLS, C, COUNTS, FIELDS, GLASS, GLASS_PLAIN, ID_BASE, SEED, abi_args, check_refract, scene
from writer_reference import same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 2047, 2048, 2049, 4097, 3 * 2048 + 77]       # wave and tile edges (tests/test_reemit_gpu.py's, and the issue's)
ROOM = 300                                                             # capacity beyond N


def first_stride(dev):
    """A sweep's grid is capped at 8 resident workgroups of 256 slots on each CU: slots from here on take a second trip."""
    return dev.info()["compute_units"] * 8 * 256


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


def upload(dev, n, dtype, mixed=False, **kw):
    """The scene in a fresh store; ``mixed``: its scrambled ids and plain Objects as well.  (the downloaded state, who is a photon)"""
    T = np.float32 if dtype == "f32" else np.float64
    s = scene(n, T, nan_v=False, **kw)                                 # (a NaN in v: a NaN's payload is nobody's rule; the CPU tests have it)
    up = {f: s[f] for f in FIELDS}
    up.update(E=np.ones(n), id_base=ID_BASE)
    photon = None
    if mixed:
        up.update(id=s["id"], kind=s["photon"].astype(np.uint8))
        photon = s["photon"]
    dev.store_alloc(n + ROOM, dtype)
    dev.upload_state(up)
    return dev.download_state(), photon


def call(dev, cfg, n_pass, seed=SEED):
    return dev.refract_surface(cfg["radius"], cfg["n_inside"], cfg["n_outside"], cfg["center"], cfg["fresnel"], C, seed, n_pass)


def sweep_and_check(dev, before, cfg, n_pass, what, photon=None):
    counts = call(dev, cfg, n_pass)
    after = dev.download_state()
    return counts, after, check_refract(before, after, counts, cfg, SEED, n_pass, what, photon)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_slot_against_the_numpy_restatement(dev, n, dtype):
    for name, cfg in (("fresnel", GLASS), ("plain", GLASS_PLAIN)):
        before, _ = upload(dev, n, dtype)
        total = np.zeros(6, dtype=np.int64)
        for n_pass in (1, 2):                                          # two consecutive passes: the pass counter moves
            counts, before, ref = sweep_and_check(dev, before, cfg, n_pass, "refract n=%d %s %s pass %d" % (n, dtype, name, n_pass))
            total += counts
            assert dev.count == n and dev.is_uniform()
        if n >= 2047:
            assert (total[[0, 2, 4]] > 0).all() and (total[[1, 3]] > 0).all() == cfg["fresnel"], total


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_past_the_grid_s_first_stride(dev, dtype):
    cap = first_stride(dev)
    n = cap + 2049
    before, _ = upload(dev, n, dtype)
    counts, after, ref = sweep_and_check(dev, before, GLASS, 3, "refract n=%d %s" % (n, dtype))
    tail = ref["crossed"][cap:]                                        # the second trip had work
    assert tail.sum() > 500 and min(counts[:5]) > 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_everybody_crossing_and_nobody_crossing(dev, dtype):
    n = 4097
    before, _ = upload(dev, n, dtype, everybody=True)
    counts, after, ref = sweep_and_check(dev, before, GLASS, 1, "everybody %s" % dtype)
    assert ref["crossed"].mean() > 0.9 and sum(counts[:5]) == ref["crossed"].sum()
    before, _ = upload(dev, n, dtype, nobody=True)
    counts, after, ref = sweep_and_check(dev, before, GLASS, 1, "nobody %s" % dtype)
    assert counts.tolist() == [0] * 6 and not ref["crossed"].any()
    for f in FIELDS:                                                   # the store is untouched, bit for bit
        for k in range(3):
            assert same_bits(after[f][k], before[f][k]), f
    assert same_bits(after["E"], before["E"]) and np.array_equal(after["id"], before["id"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_store_that_is_not_uniform(dev, hip, dtype):
    n = 2049
    before, photon = upload(dev, n, dtype, mixed=True)
    counts, after, ref = sweep_and_check(dev, before, GLASS, 6, "mixed %s" % dtype, photon)
    assert not dev.is_uniform() and min(counts[:5]) > 0
    obj = dev.download_kind() == hip.KIND_OBJECT
    assert np.array_equal(obj, np.arange(n) % 17 == 0) and not ref["crossed"][obj].any()      # kinds are never written, Objects never cross
    # the draws follow the ids: the same state with ids in store order reflects other photons
    plain, _ = upload(dev, n, dtype)
    other = call(dev, GLASS, 6)
    assert other[1] + other[3] > 0 and not same_bits(np.stack(dev.download_state()["v"], 1), np.stack(after["v"], 1))


def test_refused_calls_an_empty_store_and_no_store(dev, hip):
    before, _ = upload(dev, 300, "f64")
    for kw in BAD_CALLS:
        keep, args, counts = abi_args(**kw)
        assert dev.lib.pcl_step_refract_surface(dev.ctx, *args) == -2, kw
        assert counts is None or (counts == -7).all(), kw
    after = dev.download_state()
    for f in FIELDS:
        for k in range(3):
            assert same_bits(after[f][k], before[f][k]), f
    keep, good, counts = abi_args()                                    # six counts, no more
    assert dev.lib.pcl_step_refract_surface(dev.ctx, *good) == 0 and (counts[:6] >= 0).all() and counts[6:].tolist() == [-7, -7]
    assert counts[:5].sum() > 0
    dev.set_count(0, 0)
    assert call(dev, GLASS, 1).tolist() == [0] * 6
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        call(bare, GLASS, 1)
    assert e.value.code == -3
    bare.close()


def test_device_group_gives_the_unsharded_store(dev, hip):
    n = 3 * 2048 + 77
    before, _ = upload(dev, n, "f64")
    whole = call(dev, GLASS, 4)
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
        got = call(g, GLASS, 4)
        assert got.tolist() == whole.tolist() and min(whole[:5]) > 0   # the counts are global
        for name in FIELDS:                                            # the union of the shards is the unsharded run, bit for bit
            for f in hip.FIELD_GROUPS[name]:
                assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            call(g, dict(GLASS, n_inside=-1.5), 4)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 512, 120
RADIUS = 1.0
DT = RADIUS / 50 / C                   # c*dt = radius / 50


def drop(cl_on):
    """A beam through a drop of n = 4/3: the rows of the step and of the shell in front of it, the final state, the launch note."""
    sim = phys.Simulation(cl_on=cl_on, rng="philox", seed=7, exit=lambda s: len(s.ts) >= PASSES)
    src = phys.light.PhotonSource(origin=(-1.01, 0.0, 0.0), direction=(1.0, 0.0, 0.0), angular="beam", spatial="disc", radius=0.9)
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    shell = phys.light.ShellCrossingMeasureStep(None, [RADIUS])
    step = phys.light.RefractiveSurfaceStep(RADIUS, 4.0 / 3.0)
    sim.add_step(2, shell)
    sim.add_step(3, step)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    rows = [[int(x) for x in list(row)[1:]] for row in step.data]
    crossings = [[int(row[2][0]), int(row[3][0])] for row in shell.data]                  # out, in
    state = {f: sim.download(f) for f in ("r", "v", "dr", "dv")}
    note = sim.launch_note
    sim.close(download=False)
    return rows, crossings, state, note, step


def test_a_beam_through_a_drop_agrees_with_the_shell_in_front():
    rows, crossings, state, note, step = drop(True)
    assert len(rows) == PASSES == step._pass
    for (i_t, i_r, o_t, o_r, o_tot, over), (out, inn) in zip(rows, crossings):
        assert inn == i_t + i_r and out == o_t + o_r + o_tot and over == 0
    sums = np.sum(rows, axis=0)
    print("the drop's counts over %d passes:" % PASSES, dict(zip(COUNTS, sums.tolist())))
    assert sums[0] > N_SIM // 2 and sums[2] > N_SIM // 2 and sums[1] > 0 and sums[5] == 0 and sums[0] + sums[1] == N_SIM
    assert "one launch per light step" in note and ("RefractiveSurfaceStep" in note or "ShellCrossingMeasureStep" in note)
    assert [getattr(step, name) for name in COUNTS] == rows[-1]
    speed = np.sqrt((state["v"] ** 2).sum(axis=1))
    assert np.max(np.abs(speed - C)) < 1e-9 * C                        # directions change, speeds do not
    # the same script under the reference's Python semantics: the step reads no dv rule
    rows_py, crossings_py, state_py, _, _ = drop(False)
    assert rows_py == rows and crossings_py == crossings
    for f in state:
        assert same_bits(state_py[f], state[f]), f
