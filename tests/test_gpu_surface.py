"""GPU: SurfaceReflectStep (pcl_step_surface_reflect, light.SurfaceReflectStep).

* ``Device.surface_reflect`` against the numpy restatement (light._surface_bounce) on the state downloaded before and after the
  call: N at the wave, workgroup and tile edges, fp64 and fp32 stores, both modes, albedo 1, 0 and 0.5, and a store with
  explicit ids in scrambled order and every 7th particle a plain Object (the path that stages ids and kinds).  Counts are
  exact, untouched particles bit-identical in all twelve rows and in E, specular rows and the rows of absorbed photons
  bit-identical to numpy, lambertian rows within the bounds below.
* through ``Simulation``: a one-shell ShellCrossingMeasureStep before the step counts what the step bounces, nothing is left
  inside the sphere, the scatter step draws what it draws without the step, ``launch_note`` names the step; two contexts on
  one GPU give the unsharded run's photons and counts; host-resident objects get the restatement's state.

Bounds for the lambertian rows (everything up to sin / cos is bit for bit the restatement's: the hit point, the normal, the
frame, mu and s are IEEE operations both sides perform alike; sin / cos are the project's pcl_sincos_2pi on the device and
libm in numpy):

* v, per component: the derivation of tests/test_gpu_source.py holds unchanged -- the project's contract for a direction built
  from its sincos is 4 ulp(c), and behind the sincos  v_k = c * ((s*cos)*e1_k + (s*sin)*e2_k + mu*nrm_k)  performs the same
  DIR_OPS = 8 rounded operations per component (s*cos, *e1_k, s*sin, *e2_k, +, mu*nrm_k, +, c*); this kernel adds none:
  4 + 8/2 = 8 ulp(c).  An fp32 store holds the fp64 value rounded once more: 8.5 ulp of float32 c.
* r - center, per component: dr_k = w*dir_k carries dir_k's share of that bound -- 7.5 ulp(c)/c relative to 1 (the c* is not
  performed), times w -- plus POS_OPS = 3 more rounded operations (w*, x_k +, center_k +), each worth half an ulp of the
  largest magnitude in play, |center_k| + R + w <= MAG: (w/c) * 7.5 ulp(c) + 3/2 ulp(MAG).  fp32: one float32 ulp(MAG) more.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import light
from surface_reference import C, CENTER, RADIUS, SEED, cloud, ulp
from writer_reference import DIR_OPS, DIR_ULP, POS_OPS, lambertian_position_bound      # the derivation above, kept in one place

pytestmark = pytest.mark.gpu

assert (DIR_OPS, POS_OPS, DIR_ULP) == (8, 3, 8.0)
W_MAX = 2.8 * RADIUS                   # the longest move of surface_reference.cloud
MAG = float(np.max(np.abs(CENTER))) + RADIUS + W_MAX
POS_BOUND = lambertian_position_bound(W_MAX, MAG, C)
assert POS_BOUND == W_MAX / C * (DIR_ULP - 0.5) * ulp(C) + POS_OPS / 2 * ulp(MAG)
SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]
FIELDS = ("r", "v", "dr", "dv")
ID_BASE = 7_000_000_001


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


def upload(dev, n, dtype, ids=None, kind=None, seed=1):
    r, dr, v = cloud(n, seed=seed + n, dtype=np.float32 if dtype == "f32" else np.float64)
    dev.store_alloc(n, dtype)
    rng = np.random.RandomState(n)
    state = {"r": r, "v": v, "dr": dr, "dv": rng.normal(size=(n, 3)), "E": 1.0 + rng.uniform(size=n), "id_base": ID_BASE}
    if ids is not None:
        state["id"] = ids
    if kind is not None:
        state["kind"] = kind
    dev.upload_state(state)
    return dev.download_state()


def arrays(s):
    return {f: np.stack(s[f], 1).astype(np.float64) for f in FIELDS}


def check_call(dev, n, dtype, mode, albedo, n_pass, ids=None, kind=None):
    before = upload(dev, n, dtype, ids, kind)
    b = arrays(before)
    np_dtype = np.float32 if dtype == "f32" else np.float64
    photon = np.ones(n, dtype=bool) if kind is None else kind != 0
    ref = light._surface_bounce(b["r"], b["dr"], b["v"], photon, before["id"], RADIUS, CENTER, albedo, mode, C, SEED, n_pass, np_dtype)
    counts = dev.surface_reflect(RADIUS, CENTER, albedo, mode, C, SEED, n_pass)
    after = dev.download_state()
    a = arrays(after)
    assert counts == (int(ref["reflected"].sum()), int(ref["absorbed"].sum())), (n, dtype, mode, albedo)
    assert np.array_equal(after["E"], before["E"]) and np.array_equal(after["id"], before["id"]) and dev.count == n
    hit, refl, gone = ref["hit"], ref["reflected"], ref["absorbed"]
    for f in FIELDS:                                                   # untouched: bit-identical, dv included
        assert np.array_equal(a[f][~hit], b[f][~hit]), f
    exact = hit if mode == "specular" else gone
    for f in FIELDS:
        assert np.array_equal(a[f][exact], ref[f][exact]), (f, n, dtype, mode, albedo)
    worst = (0.0, 0.0)
    if mode == "lambertian" and refl.any():
        if dtype == "f64":
            v_unit, v_bound, r_bound = ulp(C), DIR_ULP, POS_BOUND
        else:
            v_unit, v_bound, r_bound = ulp(C, np.float32), DIR_ULP + 0.5, POS_BOUND + ulp(MAG, np.float32)
        v_err = np.max(np.abs(a["v"][refl] - ref["v"][refl])) / v_unit
        r_err = np.max(np.abs((a["r"][refl] - CENTER) - (ref["r"][refl] - CENTER)))
        dr_err = np.max(np.abs(a["dr"][refl] - ref["dr"][refl]))
        dv_err = np.max(np.abs(a["dv"][refl] - ref["dv"][refl])) / v_unit
        print("surface n=%d %s albedo %g: v %.3g ulp(c) (bound %g), r %.3g (bound %.3g), dr %.3g, dv %.3g ulp(c)"
              % (n, dtype, albedo, v_err, v_bound, r_err, r_bound, dr_err, dv_err))
        assert v_err <= v_bound
        assert r_err <= r_bound and dr_err <= r_bound
        assert dv_err <= v_bound + 1.0                                 # dv = v - v_old: one more rounding, of a value up to 2c
        worst = (v_err, r_err / r_bound)
    return counts, worst


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_particle_against_the_numpy_restatement(dev, n, dtype):
    total = 0
    for mode in ("specular", "lambertian"):
        for k, albedo in enumerate((1.0, 0.0, 0.5)):
            (refl, gone), _ = check_call(dev, n, dtype, mode, albedo, 1 + k)
            assert (gone == 0) if albedo == 1.0 else (refl == 0) if albedo == 0.0 else True
            total += refl + gone
    assert total == 6 * ((n + 1) // 2)                                 # even slots are hit, whatever becomes of them


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [65, 2049, 4097])
def test_explicit_ids_and_kinds_give_the_same_photons(dev, hip, n, dtype):
    """The path that downloads ids and kinds and stages them behind the counters: ids in scrambled order, every 7th a plain Object."""
    ids = ID_BASE + np.random.RandomState(5).permutation(n).astype(np.int64)
    kind = np.where(np.arange(n) % 7 == 0, hip.KIND_OBJECT, hip.KIND_PHOTON).astype(np.uint8)
    for mode in ("specular", "lambertian"):
        (refl, gone), _ = check_call(dev, n, dtype, mode, 0.5, 3, ids=ids, kind=kind)
        assert not dev.is_uniform() and refl > 0 and (n < 100 or gone > 0)
        assert refl + gone == int(((np.arange(n) % 2 == 0) & (kind != 0)).sum())
    # explicit ids that turn out to be id[0] + index (nothing is staged), all photons
    check_call(dev, n, dtype, "lambertian", 0.5, 3, ids=ID_BASE + np.arange(n, dtype=np.int64))
    # a photon is its id's photon wherever it stands: the scrambled store's photon with id j is the plain store's
    plain = upload(dev, n, dtype)
    dev.surface_reflect(RADIUS, CENTER, 0.5, "lambertian", C, SEED, 9)
    v_plain = arrays(dev.download_state())["v"]
    order = np.random.RandomState(6).permutation(n)
    dev.upload_state({f: np.stack(plain[f], 1)[order] for f in FIELDS} | {"E": plain["E"][order], "id": plain["id"][order]})
    dev.surface_reflect(RADIUS, CENTER, 0.5, "lambertian", C, SEED, 9)
    assert np.array_equal(arrays(dev.download_state())["v"], v_plain[order])


def test_refused_calls_and_an_empty_store(dev, hip):
    before = upload(dev, 300, "f64")
    bad = [dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=1e200), dict(center=(0, np.inf, 0)), dict(albedo=-0.1),
           dict(albedo=1.5), dict(albedo=np.nan), dict(mode=2), dict(mode=-1), dict(c=np.nan)]
    for kw in bad:
        args = dict(radius=RADIUS, center=CENTER, albedo=1.0, mode="specular", c=C, seed=SEED, n_pass=1)
        args.update(kw)
        with pytest.raises(hip.HipError) as e:
            dev.surface_reflect(**args)
        assert e.value.code == -2, kw
    assert dev.lib.pcl_step_surface_reflect(dev.ctx, RADIUS, None, 1.0, 0, C, 1, 1, None) == -2
    after = dev.download_state()
    for f in FIELDS:
        for k in range(3):
            assert np.array_equal(after[f][k], before[f][k]), f
    dev.set_count(0, 0)
    assert dev.surface_reflect(RADIUS, CENTER, 0.5, "lambertian", C, SEED, 1) == (0, 0)
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.surface_reflect(RADIUS, CENTER, 1.0, "specular", C, SEED, 1)
    assert e.value.code == -3
    bare.close()


def test_device_group_gives_the_unsharded_store(dev, hip):
    n = 3 * 2048 + 77
    before = upload(dev, n, "f64")
    whole = dev.surface_reflect(RADIUS, CENTER, 0.5, "lambertian", C, SEED, 4)
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
        assert g.surface_reflect(RADIUS, CENTER, 0.5, "lambertian", C, SEED, 4) == whole
        for f in range(hip.E):
            assert np.array_equal(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            g.surface_reflect(RADIUS, CENTER, 2.0, "lambertian", C, SEED, 4)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 5000, 30
STEP = 0.5                             # length of a move, in units of which the sphere has radius 10
DT = STEP / C


class InsideProbe(phys.DeviceStep):
    """Behind the ground: the smallest squared distance from the centre in the store, pass by pass."""
    _fuse_role = None

    def __init__(self):
        self.q_min, self.at_rest = [], []

    def _device_run(self, sim):
        d = sim.download("r") - CENTER
        self.q_min.append(float(np.min((d * d).sum(axis=1))))
        self.at_rest.append(int(np.sum(~sim.download("v").any(axis=1))))


def ground_sim(albedo=1.0, mode="lambertian", passes=PASSES, devices=None, shell=True, ground=True, probe=False, n=N_SIM):
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, devices=devices, exit=lambda s: len(s.ts) >= passes)
    src = phys.light.PhotonSource(origin=CENTER + [RADIUS + 1.0, 0.0, 0.0], angular="isotropic")
    sim.add_objs(phys.light.generate_photons_bulk(n, min=1.0, max=3.0, seed=7, source=src))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(0.6), n=np.double(1.0)))       # 0.3 per move
    tally = phys.light.ShellCrossingMeasureStep(None, [RADIUS], center=CENTER) if shell else None
    floor = phys.light.SurfaceReflectStep(RADIUS, center=CENTER, albedo=albedo, mode=mode) if ground else None
    look = InsideProbe() if probe else None
    for k, s in enumerate(x for x in (tally, floor, look) if x is not None):
        sim.add_step(3 + k, s)
    return sim, tally, floor, look


def run(sim):
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    return sim


@pytest.mark.parametrize("albedo, mode", [(1.0, "lambertian"), (0.4, "specular")])
def test_the_shell_before_the_step_counts_what_the_step_bounces(albedo, mode):
    sim, tally, floor, look = ground_sim(albedo, mode, probe=True)
    run(sim)
    assert len(tally.data) == len(floor.data) == PASSES
    came_in = [int(row[3][0]) for row in tally.data]
    bounced = [int(row[1]) + int(row[2]) for row in floor.data]
    assert came_in == bounced and sum(bounced) > N_SIM // 10
    assert min(look.q_min) >= RADIUS * RADIUS * (1 - 1e-12)            # nobody is left inside the sphere
    if albedo == 1.0:
        assert all(int(row[2]) == 0 for row in floor.data) and look.at_rest[-1] == 0
    else:                                                              # absorbed photons stay, at rest, and are not hit again
        gone = np.cumsum([int(row[2]) for row in floor.data])
        assert look.at_rest == gone.tolist() and gone[-1] > 50 and sum(int(row[1]) for row in floor.data) > 50
    assert len(sim.objects) == N_SIM and "one launch per light step" in sim.launch_note
    assert not sim.schedule["fused_multi"]                             # one launch per light step
    sim.close(download=False)


def test_the_scatter_step_draws_what_it_draws_without_the_step():
    hits, state = [], []
    for ground in (True, False):
        sim, _, floor, _ = ground_sim(shell=False, ground=ground, passes=1)
        run(sim)
        hits.append(sim.hits)
        if ground:
            assert "SurfaceReflectStep" in sim.launch_note and floor.reflected + floor.absorbed == 0    # one unit up, half a unit moved
        state.append((sim.download("r"), sim.download("v")))
        sim.close(download=False)
    assert hits[0] == hits[1] > N_SIM // 5
    assert np.array_equal(state[0][0], state[1][0]) and np.array_equal(state[0][1], state[1][1])
    # ... and over a longer run the ground changes where photons are, not which numbers the scatter step draws for an id:
    # the launch counter is the scatter step's own
    sim, _, floor, _ = ground_sim(shell=False, passes=6)
    run(sim)
    assert sim._launch == 6 and floor._pass == 6
    sim.close(download=False)


def test_two_contexts_on_one_gpu_give_the_unsharded_run():
    out = []
    for devices in (None, [0, 0]):
        sim, tally, floor, _ = ground_sim(0.5, "lambertian", passes=10, devices=devices, n=3 * 2048 + 77)
        run(sim)
        order = np.argsort(sim.download("id"))
        out.append((sim.download("r")[order], sim.download("v")[order], [list(map(int, row[1:])) for row in floor.data],
                    [int(row[3][0]) for row in tally.data]))
        sim.close(download=False)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and out[0][3] == out[1][3] and sum(a + b for a, b in out[0][2]) > 200
    assert any(b for _, b in out[0][2]) and any(a for a, _ in out[0][2])


def test_host_resident_objects_get_the_device_s_state():
    """The same explicit objects bounced by ``step.run(sim)`` on the host and on the device (specular: bit for bit)."""
    n = 300
    r, dr, v = cloud(n, seed=4)
    got = []
    for where in ("host", "device"):
        objs = []
        for k in range(n):
            o = phys.light.PhotonObject(E=phys.Measurement(np.double(1e-19), "J**1"), v=phys.light.c * [1, 0, 0]) if k % 5 else phys.Object()
            o.r, o.dr = phys.Measurement._from_code(r[k], units="m**1"), phys.Measurement._from_code(dr[k], units="m**1")
            if k % 5:
                o.v = np.array(v[k])
            objs.append(o)
        sim = phys.Simulation(cl_on=True, rng="philox", seed=SEED)
        sim.add_objs(objs)
        step = phys.light.SurfaceReflectStep(RADIUS, center=CENTER, albedo=0.5, mode="specular")
        if where == "device":
            sim._to_device()
        step.run(sim)
        got.append(((step.reflected, step.absorbed), np.array([np.asarray(o.r, dtype=np.float64) for o in sim.objects]),
                    np.array([np.asarray(o.v, dtype=np.float64) for o in sim.objects]),
                    np.array([np.asarray(o.dr, dtype=np.float64) for o in sim.objects])))
        sim.close(download=False)
    assert got[0][0] == got[1][0] and min(got[0][0]) > 20
    for k in (1, 2, 3):
        assert np.array_equal(got[0][k], got[1][k]), k
