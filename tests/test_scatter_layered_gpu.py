"""GPU: LayeredScatterStep (pcl_step_scatter_layered, light.LayeredScatterStep).

* ``Device.scatter_layered`` against the numpy restatement (light._scatter_layered) on a state that is uploaded explicitly
  (tests/path_absorb_reference.py: ``layout``, with its planted slots: at rest, -0.0, NaN, on the first, an inner and the last radius,
  on band edges, outside), downloaded before and after the call: N at the wave, workgroup and tile edges and one size just past the
  first trip of the balanced grid, fp64 and fp32 stores, ``first`` 0 and 1, 0 and 3 layers by 0, 3 and 1024 bands, p = 0, p = 1 and
  mixed, uniform stores and stores with explicit ids and plain Objects.  Who is exposed, who is hit, every cell, the rows that are not
  written and the dv = 0 rows have no tolerance; v and dv of the hit rows have the bound tests/writer_reference.py derives for a
  direction made by frame / polar / turned (the one tests/test_reemit_gpu.py applies).  Cases of 64 slots or more hold every outcome
  (tests/scatter_layered_reference.py: ``assert_every_outcome``, on the numpy side).
* two passes; the refusals; an empty store; a device group.
* through ``Simulation``: 8 passes of Newton, ScatterIsotropicStep, LayeredScatterStep (``first`` resolved to False), LayeredPhaseStep,
  AbsorptionStep and a ground, every writer behind the scatter step replayed with its numpy restatement from the probed state in
  front of it; and a second simulation without the ScatterIsotropicStep, where ``first`` resolves to True.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
import writer_reference as W
from layered_phase_reference import check_layered
from physicl_amd import light
from scatter_layered_reference import BAD_CALLS, C, CENTER, ID_BASE, SEED, abi_args, assert_every_outcome, check_scatter_layered, layout, tables
from writer_reference import same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]
SHAPES = [(L, B) for L in (0, 3) for B in (0, 3, 1024)]
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


def upload(dev, n, dtype, ids=None, kind=None):
    state = dict(layout(n, np.float32 if dtype == "f32" else np.float64), id_base=ID_BASE)
    if ids is not None:
        state["id"] = ids
    if kind is not None:
        state["kind"] = kind
    dev.store_alloc(n, dtype)
    dev.upload_state(state)
    return W.snapshot(dev)


def mixed_store(hip, n):
    ids = ID_BASE + 3 * np.random.RandomState(5).permutation(n).astype(np.int64)            # explicit, not consecutive
    kind = np.where(np.arange(n) % 4 == 1, hip.KIND_OBJECT, hip.KIND_PHOTON).astype(np.uint8)
    return ids, kind


def check_call(dev, n, dtype, cfg, first, n_pass, ids=None, kind=None, before=None, every=True):
    p, edges, E_edges = cfg
    before = upload(dev, n, dtype, ids, kind) if before is None else before
    answer = dev.scatter_layered(p, edges, CENTER, E_edges, first, C, SEED, n_pass)
    after = W.snapshot(dev)
    what = "layered scatter n=%d %s %dx%d first=%d pass %d%s" % (n, dtype, p.shape[0], p.shape[1], first, n_pass, " ids" if ids is not None else "")
    ref = check_scatter_layered(before, after, answer, p, edges, CENTER, E_edges, first, C, SEED, n_pass, what)
    if every and n >= 64:
        assert_every_outcome(ref, W.wide(before)["v"], W.photons(before), edges, E_edges, what)
    return answer, before, after, ref


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_particle_against_the_numpy_restatement(dev, hip, n, dtype, first):
    for n_pass, (L, B) in enumerate(SHAPES, start=1):
        check_call(dev, n, dtype, tables(L, B), first, n_pass)
        assert dev.is_uniform()
    for p in (0.0, 1.0):
        answer, _, _, _ = check_call(dev, n, dtype, tables(3, 3, p), first, 7, every=False)
        assert answer[1] == (answer[0] if p else 0)
    ids, kind = mixed_store(hip, n)
    for L, B in ((3, 1024), (0, 0)):
        _, before, after, ref = check_call(dev, n, dtype, tables(L, B), first, 8, ids=ids, kind=kind)
        obj = kind == hip.KIND_OBJECT
        b, a = W.wide(before), W.wide(after)
        for f in FIELDS:                                               # plain Objects are untouched, first or not
            assert same_bits(a[f][obj], b[f][obj]), f
        assert not dev.is_uniform() or n == 1


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_just_past_the_first_trip_of_the_balanced_grid(dev, hip, dtype):
    n = dev.info()["compute_units"] * 8 * 256 + 2049 + 13              # the grid's cap of resident workgroups, a ragged last wave
    cap = n - 2049 - 13
    cfg = tables(3, 3)
    before = upload(dev, n, dtype)
    for first, n_pass in ((1, 3), (0, 4)):                             # the second call on what the first left
        answer, before, after, ref = check_call(dev, n, dtype, cfg, first, n_pass, before=before)
        later = ref["scattered"][cap:]
        assert 0.1 < later.mean() < 0.9 and 0 < ref["exposed"][cap:].mean() < 0.9, first    # the second trip has work, and idle lanes
        assert (np.asarray(answer[2]) > 0).sum() == (cfg[0] > 0).sum()
        before = after


def test_two_passes_draw_twice(dev):
    n = 2049
    cfg = tables(3, 0)
    first, before, after, ref1 = check_call(dev, n, "f64", cfg, 1, 1)
    second, _, after2, ref2 = check_call(dev, n, "f64", cfg, 1, 2, before=after)             # on what the first pass left
    assert second[0] > 0 and not np.array_equal(ref2["scattered"], ref1["scattered"])
    behind, _, after3, ref3 = check_call(dev, n, "f64", cfg, 0, 3, before=W.snapshot(dev))   # first = 0 behind it: the marks survive
    kept = ref2["scattered"] & ~ref3["scattered"] & np.isfinite(ref2["dv"]).all(axis=1)
    assert kept.any() and same_bits(W.wide(after3)["dv"][kept], W.wide(after2)["dv"][kept]) and W.wide(after3)["dv"][kept].any(axis=1).all()


def test_refused_calls_and_an_empty_store(dev, hip):
    before = upload(dev, 300, "f64")
    for kw in BAD_CALLS:
        keep, args, (counts, cells) = abi_args(**kw)
        assert dev.lib.pcl_step_scatter_layered(dev.ctx, *args) == -2, kw
        assert (counts is None or (counts == -7).all()) and (cells is None or (cells == -7).all()), kw
    W.assert_same_state(W.snapshot(dev), before, "a refused call writes nothing")
    with pytest.raises(ValueError, match="p holds"):
        dev.scatter_layered([0.5, 0.5], [1.0, 2.0, 2.5, 3.0], CENTER, None, True, C, SEED, 1)
    keep, good, (counts, cells) = abi_args()
    assert dev.lib.pcl_step_scatter_layered(dev.ctx, *good) == 0
    p, edges, E_edges = tables(3, 3)
    ref = check_scatter_layered(before, W.snapshot(dev), (counts[0], counts[1], cells[:9].reshape(3, 3)), p, edges, CENTER, E_edges, 1, C, 1, 1,
                                "by hand")
    assert ref["scattered"].any() and (counts[2:] == -7).all() and (cells[9:] == -7).all()  # two counts and nine cells, no more
    dev.set_count(0, 0)
    empty = dev.scatter_layered(p, edges, CENTER, E_edges, True, C, SEED, 1)
    assert empty[:2] == (0, 0) and empty[2].tolist() == [[0] * 3] * 3
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.scatter_layered(0.5, None, None, None, True, C, SEED, 1)
    assert e.value.code == -3
    bare.close()


@pytest.mark.parametrize("first", [0, 1])
def test_device_group_gives_the_unsharded_store(dev, hip, first):
    n = 3 * 2048 + 77
    p, edges, E_edges = tables(3, 3)
    before = upload(dev, n, "f64")
    whole = dev.scatter_layered(p, edges, CENTER, E_edges, first, C, SEED, 4)
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
        got = g.scatter_layered(p, edges, CENTER, E_edges, first, C, SEED, 4)
        assert got[:2] == whole[:2] and got[2].tolist() == whole[2].tolist() and 0 < whole[1] < whole[0]
        for f in range(hip.E + 1):
            assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            g.scatter_layered(np.full((3, 3), 1.5), edges, CENTER, E_edges, first, C, SEED, 4)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 4096, 8
STEP = 0.5                             # length of a move: A*n*|dr| = 0.25, a quarter of the photons scatter in the clear air per pass
DT = STEP / C
GROUND = 1.0
SRC_SIM = dict(origin=(2.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), angular="isotropic")
CLOUD_EDGES = np.array([1.0, 2.5, 4.0])
CLOUD_BANDS = np.array([1.0, 2.0, 3.0])
CLOUD_K = np.array([[1.2, 0.0], [0.2, 0.6]])          # per unit length: tau = k * STEP; the lower layer is clear in the upper band
LAWS, WEIGHTS = ["rayleigh", ("hg", 0.85)], [[0.2, 0.8], [1.0, 0.0]]
OMEGA0 = (0.9, 1.0)
STATE = ("r", "v", "dr", "dv", "E", "id")


class Look(phys.DeviceStep):
    """The store as it stands, pass by pass."""
    _fuse_role = None

    def __init__(self):
        self.states = []

    def _device_run(self, sim):
        self.states.append({f: sim.download(f) for f in STATE})


def atmosphere(passes, air=True, devices=None):
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, devices=devices, exit=lambda s: len(s.ts) >= passes)
    src = phys.light.PhotonSource(**SRC_SIM)
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    cloud = phys.light.LayeredScatterStep(CLOUD_K, CLOUD_EDGES, (0, 0, 0), CLOUD_BANDS)
    phase = phys.light.LayeredPhaseStep(LAWS, WEIGHTS, edges=CLOUD_EDGES)
    medium = phys.light.AbsorptionStep(OMEGA0, edges=CLOUD_EDGES)
    floor = phys.light.SurfaceReflectStep(GROUND, albedo=0.5)
    looks = [Look() for _ in range(5)]
    steps = [phys.UpdateTimeStep(lambda s: np.double(DT)), phys.newton.NewtonianKinematicsStep()]
    if air:
        steps.append(phys.light.ScatterIsotropicStep(A=np.double(0.5), n=np.double(1.0)))
    steps += [looks[0], cloud, looks[1], phase, looks[2], medium, looks[3], floor, looks[4]]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    out = dict(cloud=cloud, phase=phase, medium=medium, floor=floor, looks=looks, seed=sim.seed, note=sim.launch_note,
               final={f: sim.download(f) for f in STATE})
    sim.close(download=False)
    return out


def replay(run, first):
    c_lit = light._c_h_literals()[0]
    cloud, phase, medium, floor = run["cloud"], run["phase"], run["medium"], run["floor"]
    p = light._path_probability(CLOUD_K, c_lit, DT)
    assert p[0, 1] == 0.0 and cloud.first is first and cloud._pass == PASSES == len(cloud.data)
    assert run["note"] == cloud._NOTE                                  # the first writer of the pass says why
    cells = np.zeros((2, 2), dtype=np.int64)
    for k in range(PASSES):
        s0, s1, s2, s3, s4 = (look.states[k] for look in run["looks"])
        what = "pass %d" % (k + 1)
        row = cloud.data[k]
        ref = check_scatter_layered(s0, s1, (row[1], row[2], row[3]), p, CLOUD_EDGES, np.zeros(3), CLOUD_BANDS, first, c_lit, run["seed"],
                                    k + 1, what + " cloud")
        marked = W.wide(s0)["dv"].any(axis=1) & ~ref["scattered"]       # in front of the cloud: the clear air's hits, or what the last pass left
        if first:                                                      # the first scatterer wipes them: dv != 0 reads "scattered in this pass"
            assert not W.wide(s1)["dv"][~ref["scattered"]].any(), what
        else:                                                          # behind the clear air they survive where the cloud did not hit
            assert marked.any() and same_bits(W.wide(s1)["dv"][marked], W.wide(s0)["dv"][marked]), what
        prow = phase.data[k]
        ref_p = check_layered(s1, s2, (prow[1], prow[2], prow[3], prow[4]), LAWS, WEIGHTS, CLOUD_EDGES, np.zeros(3), c_lit, run["seed"], k + 1,
                              what + " phase")
        assert ref_p["scattered"][ref["scattered"] & np.isfinite(W.wide(s0)["v"]).all(axis=1)].all(), what    # the cloud's hits are re-directed
        mrow = medium.data[k]
        W.check_absorb(s2, s3, (mrow[1], mrow[2], mrow[3], None), OMEGA0, CLOUD_EDGES, np.zeros(3), None, run["seed"], k + 1, what + " medium")
        assert int(mrow[1]) >= int(row[2]), what                        # every hit of the cloud interacts with the medium
        W.check_surface(s3, s4, (floor.data[k][1], floor.data[k][2]), GROUND, np.zeros(3), 0.5, "lambertian", c_lit, run["seed"], k + 1,
                        1.001 * STEP, what + " ground")
        assert np.asarray(row[3])[0, 1] == 0 and int(row[2]) <= int(row[1]) <= N_SIM, what
        cells += np.asarray(row[3])
    print("scattered by cell over %d passes: %s" % (PASSES, cells.tolist()))
    assert cells[0, 0] > 0 and cells[1, 0] > 0 and cells[1, 1] > 0
    for f in STATE:                                                    # nothing moves behind the last probe
        assert same_bits(run["final"][f], run["looks"][4].states[-1][f]), f


def test_a_cloud_behind_the_clear_air_replays_from_the_probed_states():
    replay(atmosphere(PASSES, air=True), False)


def test_a_cloud_in_vacuum_is_the_first_scatterer():
    replay(atmosphere(PASSES, air=False), True)


def test_two_contexts_on_one_gpu_give_the_unsharded_run():
    one, both = atmosphere(PASSES), atmosphere(PASSES, devices=[0, 0])
    rows = lambda run: [[np.asarray(x).tolist() for x in row] for row in run["cloud"].data]                 # noqa: E731
    assert rows(one) == rows(both) and both["cloud"].first is False
    a, b = np.argsort(both["final"]["id"], kind="stable"), np.argsort(one["final"]["id"], kind="stable")
    for f in STATE:
        assert same_bits(both["final"][f][a], one["final"][f][b]), f
