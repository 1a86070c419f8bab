"""GPU: photon sources for bulk generation (pcl_store_apply_source, light.PhotonSource, generate_photons_bulk(..., source=)).

* exact: the default source changes nothing; a point source puts every photon on ``origin``; axis-aligned beams are exact; E, dr,
  dv and the ids are the plain fill's for every source and every energy form; a sharded fill holds the slices of the unsharded
  one bit for bit (two stores, a DeviceGroup, Simulation(devices=[0, 0]));
* against the numpy restatement of the draws (tests/source_reference.py), every photon, every angular x spatial combination, an
  oblique axis with a far origin and an axis-aligned one at the origin, fp64 and fp32 -- bounds below;
* the distributions' own 5-sigma conditions of tests/test_source_cpu.py on the device arrays, same n and seed;
* end to end: a sourced Simulation keeps the K-passes-per-launch schedule and its counter rows are the oracle chain's, started
  from the state downloaded after the fill; delete until empty; a tracked subset; a sourced batch is an ordinary store (the
  downloaded state uploaded into a second store runs bit-identically); refused calls leave the store as it was.

Bounds against the restatement (mu, s, rho of the disc and the angles are IEEE operations both sides perform alike; sin / cos are
the project's pcl_sincos_2pi on the device and libm in numpy, the gaussian's log is OCML's on the device):

* direction, per component: the project's contract for a direction built from its sincos is 4 ulp(c) (tests/test_gpu_parity.py);
  behind the sincos  v_k = c * ((s*cos)*e1_k + (s*sin)*e2_k + mu*d_k)  performs DIR_OPS = 8 rounded operations per component
  (s*cos, *e1_k, s*sin, *e2_k, +, mu*d_k, +, c*), each worth at most half an ulp(c): 4 + 8/2 = 8 ulp(c).  An fp32 store holds the
  fp64 value rounded once more: 8.5 ulp of float32 c.
* position (disc, gaussian), r - origin per component in units of ulp(9 * radius) (9 > sqrt(-2 ln 2^-53), the largest rho / sigma):
  measured on the first MI355X run of this file: largest deviation POS_MEASURED_ULP = 1.0 (disc and gaussian alike, fp64, 100003
  photons per case); the bound is four times that.  An fp32 store holds the fp64 value rounded once: the two roundings
  differ by at most one float32 ulp at the magnitude of r, |origin| + 9 * radius.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from oracle import physicl_oracle as orc
from source_reference import check_cone, check_disc, check_gaussian, check_isotropic, check_lambertian, source_state

pytestmark = pytest.mark.gpu

light = phys.light
C = 299792458.0
SEED = 0x5EED50C5                      # tests/test_source_cpu.py's
N_STAT = 1 << 20
DIR_OPS = 8
DIR_ULP = 4 + DIR_OPS / 2
POS_MEASURED_ULP = 1.0
POS_ULP = 4 * POS_MEASURED_ULP
assert POS_ULP <= 64
E_LO, E_HI = 2.8e-19, 9.9e-19
FIELDS13 = ("r", "v", "dr", "dv")
ANGULAR = {"beam": {}, "isotropic": {}, "cone": {"half_angle": 0.3}, "lambertian": {}}
SPATIAL = {"point": {}, "disc": {}, "gaussian": {}}


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture()
def make_store(hip):
    devs = []

    def make(capacity, dtype="f64"):
        d = hip.Device(0)
        d.store_alloc(capacity, dtype)
        devs.append(d)
        return d
    yield make
    for d in devs:
        d.close()


def planck_table():
    cdf, grid = orc.planck_table(E_LO, E_HI, 5800.0, 200)
    return np.asarray(cdf), np.asarray(grid)


def fill(dev, hip, n, id_base=0, energy="power", seed=SEED):
    if energy == "table":
        cdf, grid = planck_table()
        dev.fill_photons_table(n, id_base, C, cdf, grid[:len(cdf)], seed)
    else:
        dev.fill_photons(n, id_base, C, E_LO, E_HI, seed)
        if energy == "fn_vec":                               # what Simulation._upload_locked does with a user's sampler
            u = np.random.RandomState(5).power(3, n)
            dev.upload(hip.E, (E_LO + (E_HI - E_LO) * u).astype(dev.np_dtype))


def state_equal(a, b, fields=FIELDS13 + ("E", "id")):
    for f in fields:
        if f in ("E", "id"):
            assert np.array_equal(a[f], b[f]), f
        else:
            for k in range(3):
                assert np.array_equal(a[f][k], b[f][k]), (f, k)


def src_of(angular, spatial, origin, direction, radius):
    return light.PhotonSource(origin=origin, direction=direction, angular=angular, spatial=spatial,
                              radius=None if spatial == "point" else radius, **ANGULAR[angular])


# ------------------------------------------------------------------------------------------------ exact
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_default_source_leaves_the_fill_as_it_is(make_store, hip, dtype):
    n = 3 * 2048 + 77
    a, b = make_store(n, dtype), make_store(n, dtype)
    fill(a, hip, n, 11)
    fill(b, hip, n, 11)
    b.apply_source(light.PhotonSource(), C, SEED)
    sa, sb = a.download_state(), b.download_state()
    state_equal(sa, sb)
    assert np.all(sb["v"][0] == C) and not np.any(sb["v"][1]) and not np.any(sb["r"][0]) and b.is_uniform()


AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_point_source_and_axis_aligned_beams_are_exact(make_store, hip, dtype):
    n = 2048 + 301
    plain = make_store(n, dtype)
    fill(plain, hip, n)
    sp = plain.download_state()
    origin = (6371000.0, -12.5, 0.1)
    for axis in AXES:
        d = make_store(n, dtype)
        fill(d, hip, n)
        d.apply_source(light.PhotonSource(origin=origin, direction=axis), C, SEED)
        s = d.download_state()
        for k in range(3):
            assert np.all(s["r"][k] == d.np_dtype(origin[k])), (axis, k)
            assert np.all(s["v"][k] == d.np_dtype(C * axis[k])) and not np.any(np.signbit(s["v"][k]) & (s["v"][k] == 0)), (axis, k)
        state_equal(sp, s, ("dr", "dv", "E", "id"))
        d.close()


SOURCES = [("isotropic", "point"), ("cone", "disc"), ("lambertian", "gaussian"), ("beam", "gaussian")]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("energy", ["power", "table", "fn_vec"])
def test_energies_increments_and_ids_are_the_plain_fill_s(make_store, hip, energy, dtype):
    n = 2 * 2048 + 5
    plain = make_store(n, dtype)
    fill(plain, hip, n, 40, energy)
    sp = plain.download_state()
    assert len(np.unique(sp["E"])) > 100
    for angular, spatial in SOURCES:
        d = make_store(n, dtype)
        fill(d, hip, n, 40, energy)
        d.apply_source(src_of(angular, spatial, (6371000.0, 0, 0), (1, -2, 0.5), 1e6), C, SEED)
        s = d.download_state()
        state_equal(sp, s, ("dr", "dv", "E", "id"))
        assert d.is_uniform() and not np.array_equal(s["r"][0], sp["r"][0])
        d.close()


# ------------------------------------------------------------------------------------------------ exact: shards
N_SHARD = 3 * 2048 + 77
SHARD_SRC = dict(origin=(6371000.0, 5.0, -3.0), direction=(1, -2, 0.5), angular="lambertian", spatial="gaussian", radius=1e6)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("k", [1, 2048, 4097])
def test_two_stores_hold_the_slices_of_the_unsharded_store(make_store, hip, k, dtype):
    src = light.PhotonSource(**SHARD_SRC)
    whole = make_store(N_SHARD, dtype)
    fill(whole, hip, N_SHARD)
    whole.apply_source(src, C, SEED)
    sw = whole.download_state()
    for lo, hi in ((0, k), (k, N_SHARD)):
        part = make_store(hi - lo, dtype)
        fill(part, hip, hi - lo, lo)
        part.apply_source(src, C, SEED)
        s = part.download_state()
        assert np.array_equal(s["id"], sw["id"][lo:hi]) and np.array_equal(s["E"], sw["E"][lo:hi])
        for f in FIELDS13:
            for j in range(3):
                assert np.array_equal(s[f][j], sw[f][j][lo:hi]), (f, j, lo)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_device_group_holds_the_unsharded_store(make_store, hip, dtype):
    src = light.PhotonSource(**SHARD_SRC)
    whole = make_store(N_SHARD, dtype)
    fill(whole, hip, N_SHARD, 9)
    whole.apply_source(src, C, SEED)
    with hip.DeviceGroup([0, 0]) as g:
        g.store_alloc(N_SHARD, dtype)
        g.fill_photons(N_SHARD, 9, C, E_LO, E_HI, SEED)
        g.apply_source(src, C, SEED)
        assert np.array_equal(g.download_ids(), whole.download_ids())
        for f in range(hip.NFIELDS):
            assert np.array_equal(g.download(f), whole.download(f)), f
        # a refused source is refused before any shard is written
        bad = light.PhotonSource(**SHARD_SRC)
        bad.radius = -1.0
        with pytest.raises(hip.HipError) as e:
            g.apply_source(bad, C, SEED)
        assert e.value.code == -2
        for f in range(hip.NFIELDS):
            assert np.array_equal(g.download(f), whole.download(f)), f


def sourced_sim(n, source, *, devices=None, seed=77, passes=64, delete=False, trace=None, energy=None, spl=None):
    sim = phys.Simulation(cl_on=True, seed=seed, devices=devices, exit=lambda s: len(s.ts) >= passes, steps_per_launch=spl)
    sim.add_objs(light.generate_photons_bulk(n, seed=seed, source=source, **(energy or dict(min=E_LO, max=E_HI))))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    if delete:
        sim.add_step(2, light.ScatterDeleteStep(np.double(DEL_N), np.double(DEL_A)))
    else:
        sim.add_step(2, light.ScatterIsotropicStep(A=1.0, n=A_KERNEL, variable_n=True, variable_n_fn=EXPR_RADIAL))
    sign = light.ScatterSignMeasureStep(None, True)
    planes = light.ScatterMeasureStep(None, True, PLANES)
    sim.add_step(3, sign)
    sim.add_step(4, planes)
    tp = None
    if trace:
        tp = light.TracePathMeasureStep(None, track=trace)
        sim.add_step(5, tp)
    return sim, sign, planes, tp


def run(sim):
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    return sim


# the reference's radial atmosphere (examples/presentation_example_2.ipynb's expression about the Earth's centre); the kernel's A
# (the user's ``n``: physicl/light.py:287) makes a 3 km step at the surface scatter with probability 0.3
EXPR_RADIAL = "2.5E+25 * exp(-1 * (sqrt(pow(r0[gid], 2) + pow(r1[gid], 2) + pow(r2[gid], 2)) - 6371000.0)/(8600.0))"
DT = 1e-5
A_KERNEL = 4e-30
DEL_N, DEL_A = 1e-2, 1e-2              # ScatterDeleteStep(n, A): removal probability A * n * |dr| = 0.3 per 3 km step
SURFACE = (6371000.0, 0.0, 0.0)
PLANES = [[6371000.0 + 5000.0, np.nan, np.nan], [np.nan, 0.0, np.nan]]


def test_simulation_over_two_contexts_starts_from_the_same_photons():
    n = N_SHARD
    src = light.PhotonSource(origin=SURFACE, direction=(1, -2, 0.5), angular="cone", half_angle=0.3, spatial="disc", radius=1e6)
    out = []
    for devices in (None, [0, 0]):
        sim, sign, planes, _ = sourced_sim(n, src, devices=devices, passes=8)
        first = {f: sim.download(f) for f in ("r", "v", "E", "id")}
        run(sim)
        out.append((first, [[float(x) for x in r] for r in sign.data + planes.data], {f: sim.download(f) for f in ("r", "v", "dr", "dv")}))
        sim.close(download=False)
    for f in out[0][0]:
        assert np.array_equal(out[0][0][f], out[1][0][f]), f
    assert out[0][1] == out[1][1]
    for f in out[0][2]:
        assert np.array_equal(out[0][2][f], out[1][2][f]), f


# ------------------------------------------------------------------------------------------------ against the restatement
GEOMETRY = {"oblique_far": ((6371000.0, 0.0, 0.0), (1, -2, 0.5), 1e6), "axis_at_origin": ((0.0, 0.0, 0.0), (0, 0, -1), 2.5)}


def check_source(d, src, id_base, angular, spatial, geometry, dtype):
    """The store of ``d`` behind ``apply_source(src, C, SEED)`` on a fill with ids from ``id_base``, every photon against the numpy
    restatement under the bounds of the module's docstring (tests/test_writer_trips_gpu.py runs it past a sweep's first trip).
    (r, v) as downloaded, widened."""
    radius = GEOMETRY[geometry][2]
    s = d.download_state()
    n = len(s["E"])
    ref = source_state(src, np.arange(n, dtype=np.uint64) + np.uint64(id_base), SEED, C)
    v, r = np.stack(s["v"], 1).astype(np.float64), np.stack(s["r"], 1).astype(np.float64)
    if dtype == "f64":
        dir_err = np.max(np.abs(v - ref["v"])) / np.spacing(C)
        pos_err = np.max(np.abs((r - src.origin) - (ref["r"] - src.origin))) / np.spacing(9.0 * radius)
        print("source %s/%s %s f64: direction %.3g ulp(c) (bound %g), position %.3g ulp(9 radius) (bound %g)"
              % (angular, spatial, geometry, dir_err, DIR_ULP, pos_err, POS_ULP))
        assert dir_err <= DIR_ULP
        assert pos_err <= (POS_ULP if spatial != "point" else 0.0)
        assert np.max(np.abs(np.sqrt(np.sum((v / C) ** 2, axis=1)) - 1.0)) <= 1e-15
    else:
        ref_v, ref_r = ref["v"].astype(np.float32).astype(np.float64), ref["r"].astype(np.float32).astype(np.float64)
        dir_err = np.max(np.abs(v - ref_v)) / float(np.spacing(np.float32(C)))
        pos_unit = float(np.spacing(np.float32(np.max(np.abs(src.origin)) + 9.0 * radius)))
        pos_err = np.max(np.abs(r - ref_r)) / pos_unit
        print("source %s/%s %s f32: direction %.3g ulp32(c), position %.3g ulp32(|origin| + 9 radius)" % (angular, spatial, geometry, dir_err, pos_err))
        assert dir_err <= DIR_ULP + 0.5
        assert pos_err <= (1.0 if spatial != "point" else 0.0)
    if angular == "beam":
        assert np.array_equal(v, np.broadcast_to((C * src.d).astype(d.np_dtype).astype(np.float64), v.shape))
    if spatial != "point":                                   # in the plane through origin perpendicular to d
        off = (r - src.origin) @ src.d
        assert np.max(np.abs(off)) <= (1e-9 if dtype == "f64" else 2.0) * max(radius, 1.0)
    return r, v


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("geometry", sorted(GEOMETRY))
@pytest.mark.parametrize("spatial", sorted(SPATIAL))
@pytest.mark.parametrize("angular", sorted(ANGULAR))
def test_every_photon_against_the_numpy_restatement(make_store, hip, angular, spatial, geometry, dtype):
    n, id_base = 100_003, 7_000_000_001
    origin, direction, radius = GEOMETRY[geometry]
    src = src_of(angular, spatial, origin, direction, radius)
    d = make_store(n, dtype)
    fill(d, hip, n, id_base)
    d.apply_source(src, C, SEED)
    check_source(d, src, id_base, angular, spatial, geometry, dtype)


# ------------------------------------------------------------------------------------------------ the distributions
@pytest.fixture(scope="module")
def stat_store(hip):
    d = hip.Device(0)
    d.store_alloc(N_STAT)

    def sample(src):
        d.fill_photons(N_STAT, 0, C, E_LO, E_HI, SEED)
        d.apply_source(src, C, SEED)
        return np.stack([d.download(f) for f in hip.FIELD_GROUPS["r"]], 1), np.stack([d.download(f) for f in hip.FIELD_GROUPS["v"]], 1)
    yield sample
    d.close()


def test_device_isotropic(stat_store):
    _, v = stat_store(light.PhotonSource(direction=(1, -2, 0.5), angular="isotropic"))
    check_isotropic(v / C)


def test_device_cone(stat_store):
    _, v = stat_store(light.PhotonSource(direction=(0, 0, -1), angular="cone", half_angle=0.3))
    check_cone(v[:, 2] / -C, 0.3)                            # mu = v . d / c: one exact sign and one division for an axis-aligned d


def test_device_lambertian(stat_store):
    _, v = stat_store(light.PhotonSource(direction=(0, 1, 0), angular="lambertian"))
    check_lambertian(v[:, 1] / C)


def test_device_disc_and_gaussian(stat_store):
    r, _ = stat_store(light.PhotonSource(direction=(0, 0, 1), spatial="disc", radius=2.5))
    assert not np.any(r[:, 2])
    check_disc(np.hypot(r[:, 0], r[:, 1]), 2.5)
    r, _ = stat_store(light.PhotonSource(direction=(0, 0, 1), spatial="gaussian", radius=3.0))
    check_gaussian(np.hypot(r[:, 0], r[:, 1]), 3.0)
    assert np.all(np.isfinite(r))


# ------------------------------------------------------------------------------------------------ end to end
N_E2E = 4096 * 3 + 5


def soa(first):
    n = len(first["E"])
    return {"r": [np.ascontiguousarray(first["r"][:, k]) for k in range(3)], "v": [np.ascontiguousarray(first["v"][:, k]) for k in range(3)],
            "dr": [np.zeros(n)] * 3, "dv": [np.zeros(n)] * 3, "E": first["E"].copy(), "id": first["id"].copy()}


def crossings(st):
    return [int(orc.plane_crossings(st["r"], st["dr"], loc)) for loc in PLANES]


def test_isotropic_point_source_in_the_radial_atmosphere_against_the_oracle_chain():
    """64 passes of Newton + radial variable-n scatter + sign and plane counters from an isotropic point source on the Earth's
    surface: the schedule is the one the run takes without a source, the rows are the oracle chain's started from the downloaded
    initial state, final v within 4 ulp(c), r within the bound that follows (tests/test_gpu_multi.py)."""
    K = 64
    src = light.PhotonSource(origin=SURFACE, angular="isotropic")
    plain, _, _, _ = sourced_sim(N_E2E, None, passes=K)
    run(plain)
    sim, sign, planes, _ = sourced_sim(N_E2E, src, passes=K)
    first = {f: sim.download(f) for f in ("r", "v", "E", "id")}
    assert np.all(first["r"] == SURFACE) and len(np.unique(first["v"][:, 0])) > N_E2E // 2
    run(sim)
    assert dict(sim.schedule) == dict(plain.schedule) and sim.schedule["fused_multi"] == 2 and len(sim.ts) == K
    plain.close(download=False)
    st, ref_sign, ref_planes, hits = soa(first), [], [], 0
    for k in range(K):
        orc.step_newton(st, DT)
        hit = orc.step_scatter_isotropic(st, orc.philox_draws(77, 1 + k, st["id"]), A_KERNEL, 1.0, C, n_expr=EXPR_RADIAL)
        hits = int(hit.sum())
        ref_sign.append([N_E2E] + [int((st["v"][j] > 0).sum()) for j in range(3)])
        ref_planes.append([N_E2E] + crossings(st))
    assert [[int(x) for x in r[1:]] for r in sign.data] == ref_sign
    assert [[int(x) for x in r[1:]] for r in planes.data] == ref_planes
    assert sim.hits == hits and sum(r[1] for r in ref_planes) > 0 and 0 < ref_sign[-1][1] < N_E2E
    v_tol = 4 * np.spacing(C)
    assert np.max(np.abs(sim.download("v") - np.stack(st["v"], 1))) <= v_tol
    assert np.max(np.abs(sim.download("r") - np.stack(st["r"], 1))) <= K * DT * v_tol + np.spacing(2 * SURFACE[0]) * K
    sim.close(download=False)


def test_sourced_delete_run_until_empty_against_the_oracle_chain():
    src = light.PhotonSource(origin=SURFACE, angular="isotropic")
    sim, sign, planes, _ = sourced_sim(N_E2E, src, passes=10 ** 6, delete=True, seed=21)
    sim.exit = lambda s: len(s.objects) == 0
    first = {f: sim.download(f) for f in ("r", "v", "E", "id")}
    ids_per_pass = []
    run(sim)
    st, alive = soa(first), []
    step = 0
    while len(st["id"]):
        step += 1
        orc.step_newton(st, DT)
        _, _, rand = orc.philox_draws(21, step, st["id"])
        orc.step_scatter_delete(st, rand, DEL_N, DEL_A)
        alive.append(len(st["id"]))
        ids_per_pass.append(st["id"].copy())
    assert [int(r[1]) for r in sign.data] == alive and alive[-1] == 0 and len(alive) > 10 and len(sim.objects) == 0
    assert [int(r[1]) for r in planes.data] == alive
    sim.close(download=False)
    # the survivors' ids pass by pass: the same run stopped after 1, 5 and 12 passes
    for stop in (1, 5, 12):
        part, _, _, _ = sourced_sim(N_E2E, src, passes=stop, delete=True, seed=21)
        run(part)
        assert np.array_equal(part.download("id"), ids_per_pass[stop - 1]), stop
        part.close(download=False)


def test_tracked_photons_start_at_the_source_s_positions_plus_one_move():
    src = light.PhotonSource(origin=SURFACE, direction=(1, 0, 0), angular="lambertian", spatial="gaussian", radius=1000.0)
    plain, _, _, _ = sourced_sim(N_E2E, None, passes=40, trace=64)
    run(plain)
    sim, _, _, tp = sourced_sim(N_E2E, src, passes=40, trace=64)
    first = {f: sim.download(f) for f in ("r", "v")}
    run(sim)
    assert dict(sim.schedule) == dict(plain.schedule) and sim.schedule["fused_multi"] >= 1
    plain.close(download=False)
    assert len(tp.data) == 1 + 64
    for i in range(64):
        path = np.asarray(tp.data[1 + i][1:], dtype=np.float64).reshape(-1, 3)
        assert len(path) == 40
        assert np.array_equal(path[0], first["r"][i] + first["v"][i] * DT), i
    last = sim.download("r")
    for i in range(64):
        assert np.array_equal(np.asarray(tp.data[1 + i][1:], dtype=np.float64).reshape(-1, 3)[-1], last[i])
    sim.close(download=False)


def test_custom_id_info_sees_the_store_s_photon_not_the_default_one():
    """The synthetic photon a custom ``id_info_fn`` is handed on a device-traced batch carries the store's r and v (looked up when
    the rows of the launch are filed, like its E: here behind the run's only launch), not r = 0 and v = (c, 0, 0)."""
    src = light.PhotonSource(origin=SURFACE, direction=(0, 0, -1))
    sim, _, _, _ = sourced_sim(4099, src, passes=3)
    tp = light.TracePathMeasureStep(None, id_info_fn=lambda o: (float(np.asarray(o.E)), np.asarray(o.r).tolist(), np.asarray(o.v).tolist()), track=3)
    sim.add_step(5, tp)
    E = sim.download("E")
    run(sim)
    assert sim.schedule["fused_multi"] == 1
    r_end, v_end = sim.download("r"), sim.download("v")
    for i in range(3):
        e, r, v = tp.data[1 + i][0]
        assert e == E[i] and r == r_end[i].tolist() and v == v_end[i].tolist()
        assert r[0] == SURFACE[0] or v != [0.0, 0.0, -C]         # (fell along -z from the surface unless it was scattered)
        assert r != [0.0, 0.0, 0.0] and v != [C, 0.0, 0.0]
    sim.close(download=False)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_sourced_batch_is_an_ordinary_store(make_store, hip, dtype):
    n, K = N_E2E, 32
    src = light.PhotonSource(origin=SURFACE, direction=(1, -2, 0.5), angular="cone", half_angle=0.3, spatial="disc", radius=1e4)
    a = make_store(n, dtype)
    fill(a, hip, n, 123)
    a.apply_source(src, C, SEED)
    s = a.download_state()
    b = make_store(n, dtype)
    b.upload_state({"r": np.stack(s["r"], 1), "v": np.stack(s["v"], 1), "E": s["E"], "id_base": 123})
    sc = dict(A=A_KERNEL, n=1.0, flags=hip.SCATTER_VARIABLE_N, c=C, h=6.62607015e-34, n_expr=EXPR_RADIAL, rng_mode=hip.RNG_PHILOX, seed=5, step=1)
    rows_a = a.step_fused_multi(DT, K, sc, PLANES, raw=True)
    rows_b = b.step_fused_multi(DT, K, sc, PLANES, raw=True)
    assert np.array_equal(rows_a, rows_b) and rows_a[:, -1].sum() > 0
    state_equal(a.download_state(), b.download_state())


# ------------------------------------------------------------------------------------------------ refusals
def raw_source(hip, **kw):
    class Raw:
        origin, e1, e2, d = (0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)
        angular, spatial, cos_half_angle, radius = 1, 1, 0.5, 1.0
    r = Raw()
    for k, v in kw.items():
        setattr(r, k, v)
    return r


BAD = [dict(angular=4), dict(angular=-1), dict(spatial=3), dict(spatial=-1), dict(origin=(0.0, np.nan, 0.0)), dict(origin=(np.inf, 0.0, 0.0)),
       dict(e1=(np.nan, 0.0, 0.0)), dict(e2=(0.0, np.inf, 0.0)), dict(d=(0.0, 0.0, np.nan)),
       dict(angular=2, cos_half_angle=1.5), dict(angular=2, cos_half_angle=-1.0000001), dict(angular=2, cos_half_angle=np.nan),
       dict(radius=-1.0), dict(radius=np.inf), dict(radius=np.nan), dict(spatial=2, radius=-0.5)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_refused_calls_leave_the_store_unchanged(make_store, hip, dtype):
    n = 2048 + 9
    d = make_store(n, dtype)
    fill(d, hip, n, 3)
    before = d.download_state()
    for kw in BAD:
        with pytest.raises(hip.HipError) as e:
            d.apply_source(raw_source(hip, **kw), C, SEED)
        assert e.value.code == -2, kw
    assert d.lib.pcl_store_apply_source(d.ctx, None, C, SEED) == -2 and d.lib.pcl_store_apply_source(None, None, C, SEED) == -2
    with pytest.raises(hip.HipError) as e:
        d.apply_source(raw_source(hip), np.nan, SEED)
    assert e.value.code == -2
    state_equal(before, d.download_state())
    # explicit ids (or kinds): not a freshly filled population
    d.upload_ids(before["id"])
    with pytest.raises(hip.HipError) as e:
        d.apply_source(raw_source(hip), C, SEED)
    assert e.value.code == -3
    state_equal(before, d.download_state())
    k = make_store(n, dtype)
    fill(k, hip, n, 3)
    k.upload_kind(np.ones(n, dtype=np.uint8))
    with pytest.raises(hip.HipError) as e:
        k.apply_source(raw_source(hip), C, SEED)
    assert e.value.code == -3
    state_equal(before, k.download_state())
    # no store at all; an empty one is fine
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.apply_source(raw_source(hip), C, SEED)
    assert e.value.code == -3
    bare.store_alloc(16, dtype)
    bare.fill_photons(0, 0, C, E_LO, E_HI, SEED)
    bare.apply_source(raw_source(hip), C, SEED)
    assert bare.count == 0
    bare.close()
