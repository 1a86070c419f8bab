"""GPU: PhaseFunctionStep (pcl_step_phase_redirect, light.PhaseFunctionStep).

* ``Device.phase_redirect`` against the numpy restatement (light._phase_redirect) on the state downloaded before and after the
  call: N at the wave, workgroup and tile edges, fp64 and fp32 stores, the three phase functions (Henyey-Greenstein with g =
  0.85 and g = -0.5), a uniform store and a store with explicit ids in scrambled order and every 7th particle a plain Object
  (the path that stages ids and kinds).  Counts are exact, particles that are not re-directed bit-identical in all twelve rows
  and in E, re-directed rows within the bounds below.
* through ``Simulation``: every pass re-directs exactly the photons the scatter step hit, the scatter step draws what it
  draws without the step, the mean cosine of the scattering angle is g, one launch per light step and ``launch_note`` names
  the step; two contexts on one GPU give the unsharded call's store.

Bounds for the re-directed rows: those tests/test_gpu_surface.py derives for its lambertian rows, and for the same reason.
Everything up to sin / cos is bit for bit the restatement's (the old velocity, its unit vector, the frame, mu and s are IEEE
operations both sides perform alike); sin / cos are the project's pcl_sincos_2pi on the device and libm in numpy.  The project's
contract for a direction built from its sincos is 4 ulp(c), and behind the sincos  v_k = c * ((s*cos)*e1_k + (s*sin)*e2_k +
mu*w_k)  performs DIR_OPS = 8 rounded operations per component: 4 + 8/2 = 8 ulp(c); an fp32 store holds the fp64 value rounded
once more: 8.5 ulp of float32 c.  dv = v - v_old is one more rounding, of a value up to 2c: one ulp(c) more.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import light
from phase_reference import C, SEED, cloud, ulp
from writer_reference import DIR_OPS, DIR_ULP      # the derivation above, kept in one place

pytestmark = pytest.mark.gpu

assert (DIR_OPS, DIR_ULP) == (8, 8.0)
SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]
LAWS = [("isotropic", 0.0), ("hg", 0.85), ("hg", -0.5), ("rayleigh", 0.0), ("hg", 1e-12), ("hg", -1e-300)]
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
    v, dv = cloud(n, seed=seed + n, dtype=np.float32 if dtype == "f32" else np.float64)
    dev.store_alloc(n, dtype)
    rng = np.random.RandomState(n)
    state = {"r": rng.normal(size=(n, 3)), "v": v, "dr": rng.normal(size=(n, 3)), "dv": dv, "E": 1.0 + rng.uniform(size=n), "id_base": ID_BASE}
    if ids is not None:
        state["id"] = ids
    if kind is not None:
        state["kind"] = kind
    dev.upload_state(state)
    return dev.download_state()


def arrays(s):
    return {f: np.stack(s[f], 1).astype(np.float64) for f in FIELDS}


def check_call(dev, n, dtype, phase, g, n_pass, ids=None, kind=None):
    before = upload(dev, n, dtype, ids, kind)
    b = arrays(before)
    np_dtype = np.float32 if dtype == "f32" else np.float64
    photon = np.ones(n, dtype=bool) if kind is None else kind != 0
    ref = light._phase_redirect(b["v"], b["dv"], photon, before["id"], phase, g, C, SEED, n_pass, np_dtype)
    count = dev.phase_redirect(phase, g, C, SEED, n_pass)
    after = dev.download_state()
    a = arrays(after)
    go = ref["redirected"]
    assert count == int(go.sum()) == int(((np.arange(n) % 3 == 0) & photon).sum()), (n, dtype, phase, g)
    assert np.array_equal(after["E"], before["E"]) and np.array_equal(after["id"], before["id"]) and dev.count == n
    for f in FIELDS:                                                   # not re-directed: bit-identical; r and dr: everybody
        assert np.array_equal(a[f][~go], b[f][~go]), f
    assert np.array_equal(a["r"], b["r"]) and np.array_equal(a["dr"], b["dr"])
    worst = (0.0, 0.0)
    if go.any():
        v_unit, v_bound = (ulp(C), DIR_ULP) if dtype == "f64" else (ulp(C, np.float32), DIR_ULP + 0.5)
        v_err = np.max(np.abs(a["v"][go] - ref["v"][go])) / v_unit
        dv_err = np.max(np.abs(a["dv"][go] - ref["dv"][go])) / v_unit
        print("phase n=%d %s %s g=%g: v %.3g ulp(c) (bound %g), dv %.3g ulp(c) (bound %g)" % (n, dtype, phase, g, v_err, v_bound, dv_err, v_bound + 1))
        assert v_err <= v_bound
        assert dv_err <= v_bound + 1.0                                 # dv = v - v_old: one more rounding, of a value up to 2c
        worst = (v_err, dv_err)
    return count, worst


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_particle_against_the_numpy_restatement(dev, hip, n, dtype):
    ids = ID_BASE + np.random.RandomState(5).permutation(n).astype(np.int64)
    kind = np.where(np.arange(n) % 7 == 0, hip.KIND_OBJECT, hip.KIND_PHOTON).astype(np.uint8)
    for k, (phase, g) in enumerate(LAWS):
        count, _ = check_call(dev, n, dtype, phase, g, 1 + k)
        assert dev.is_uniform() and count == (n + 2) // 3              # every third slot was scattered
        # the path that downloads ids and kinds and stages them behind the counter
        check_call(dev, n, dtype, phase, g, 1 + k, ids=ids, kind=kind)
        assert not dev.is_uniform()


def test_a_photon_is_its_id_s_photon_wherever_it_stands(dev):
    n = 2049
    check_call(dev, n, "f64", "rayleigh", 0.0, 3, ids=ID_BASE + np.arange(n, dtype=np.int64))   # ids that are id[0] + index: nothing is staged
    plain = upload(dev, n, "f64")
    dev.phase_redirect("rayleigh", 0.0, C, SEED, 9)
    v_plain = arrays(dev.download_state())["v"]
    order = np.random.RandomState(6).permutation(n)
    dev.upload_state({f: np.stack(plain[f], 1)[order] for f in FIELDS} | {"E": plain["E"][order], "id": plain["id"][order]})
    dev.phase_redirect("rayleigh", 0.0, C, SEED, 9)
    assert np.array_equal(arrays(dev.download_state())["v"], v_plain[order])
    dev.upload_state({f: np.stack(plain[f], 1) for f in FIELDS} | {"E": plain["E"], "id": plain["id"]})
    dev.phase_redirect("rayleigh", 0.0, C, SEED, 10)                   # another pass: other draws
    assert not np.array_equal(arrays(dev.download_state())["v"], v_plain)


def test_refused_calls_and_an_empty_store(dev, hip):
    before = upload(dev, 300, "f64")
    bad = [dict(phase=3), dict(phase=-1), dict(g=1.0), dict(g=-1.0), dict(g=1.5), dict(g=np.nan), dict(g=np.inf), dict(c=np.nan), dict(c=np.inf)]
    for kw in bad:
        args = dict(phase="hg", g=0.5, c=C, seed=SEED, n_pass=1)
        args.update(kw)
        with pytest.raises(hip.HipError) as e:
            dev.phase_redirect(**args)
        assert e.value.code == -2, kw
    assert dev.lib.pcl_step_phase_redirect(dev.ctx, 1, 0.5, C, 1, 1, None) == -2
    after = dev.download_state()
    for f in FIELDS:
        for k in range(3):
            assert np.array_equal(after[f][k], before[f][k]), f
    assert dev.phase_redirect("rayleigh", 7.0, C, SEED, 1) == 100     # g is looked at by hg alone
    dev.set_count(0, 0)
    assert dev.phase_redirect("hg", 0.5, C, SEED, 1) == 0
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.phase_redirect("hg", 0.5, C, SEED, 1)
    assert e.value.code == -3
    bare.close()


def test_device_group_gives_the_unsharded_store(dev, hip):
    n = 3 * 2048 + 77
    before = upload(dev, n, "f64")
    whole = dev.phase_redirect("hg", 0.85, C, SEED, 4)
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
        assert g.phase_redirect("hg", 0.85, C, SEED, 4) == whole == (n + 2) // 3
        for f in range(hip.E):
            assert np.array_equal(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            g.phase_redirect("hg", 1.0, C, SEED, 4)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES, G = 4097, 6, 0.85
STEP = 0.5                             # length of a move: A*n*|dr| = 0.5, about half of the photons scatter per pass
DT = STEP / C


class Probe(phys.DeviceStep):
    """Behind the phase step: the scatter step's hit count of this pass, and the cosines between the velocities before and after
    the scatter of the photons it hit."""
    _fuse_role = None

    def __init__(self):
        self.hits, self.cosines, self.speed_err = [], [], []

    def _device_run(self, sim):
        self.hits.append(sim.hits)
        v, dv = sim.download("v"), sim.download("dv")
        hit = dv.any(axis=1)
        old = (v - dv)[hit]
        self.cosines.append((v[hit] * old).sum(axis=1) / np.sqrt((v[hit] ** 2).sum(axis=1) * (old ** 2).sum(axis=1)))
        self.speed_err.append(float(np.max(np.abs(np.sqrt((v ** 2).sum(axis=1)) - C))))


def phase_sim(with_step=True, passes=PASSES, devices=None, probe=True):
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, devices=devices, exit=lambda s: len(s.ts) >= passes)
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=phys.light.PhotonSource(angular="isotropic")))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
    step = phys.light.PhaseFunctionStep("hg", G) if with_step else None
    look = Probe() if probe else None
    for k, s in enumerate(x for x in (step, look) if x is not None):
        sim.add_step(3 + k, s)
    return sim, step, look


def run(sim):
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    return sim


def test_every_pass_redirects_the_photons_the_scatter_step_hit():
    sim, step, look = phase_sim()
    run(sim)
    redirected = [int(row[1]) for row in step.data]
    assert len(step.data) == PASSES and redirected == look.hits and step._pass == PASSES == sim._launch
    assert all(N_SIM // 3 < h < 2 * N_SIM // 3 for h in look.hits)     # about half scatter per pass
    assert [len(c) for c in look.cosines] == look.hits
    mu = np.concatenate(look.cosines)
    second = (1 + 2 * G * G) / 3                                       # the law's <mu^2>; <mu> = g, within 5 sigma
    assert abs(mu.mean() - G) <= 5 * np.sqrt((second - G * G) / len(mu)), mu.mean()
    assert max(look.speed_err) <= 8 * ulp(C)
    assert sim.schedule["fused"] == PASSES and not sim.schedule["fused_multi"]                      # one launch per light step
    assert "one launch per light step" in sim.launch_note and "PhaseFunctionStep" in sim.launch_note
    assert len(sim.objects) == N_SIM
    sim.close(download=False)


def test_the_scatter_step_draws_what_it_draws_without_the_step():
    hits, scattered, r = [], [], []
    for with_step in (True, False):
        sim, step, _ = phase_sim(with_step, passes=1, probe=False)
        run(sim)
        hits.append(sim.hits)
        scattered.append(sim.download("dv").any(axis=1))
        r.append(sim.download("r"))
        if with_step:
            assert step.redirected == sim.hits
            v_with = sim.download("v")
        else:
            assert not np.array_equal(sim.download("v")[scattered[0]], v_with[scattered[0]])       # the step gave them other directions
            assert np.array_equal(sim.download("v")[~scattered[0]], v_with[~scattered[0]])
        sim.close(download=False)
    assert hits[0] == hits[1] > N_SIM // 3 and np.array_equal(scattered[0], scattered[1]) and np.array_equal(r[0], r[1])


def test_two_contexts_on_one_gpu_give_the_unsharded_run():
    out = []
    for devices in (None, [0, 0]):
        sim, step, _ = phase_sim(passes=4, devices=devices, probe=False)
        run(sim)
        order = np.argsort(sim.download("id"))
        out.append((sim.download("r")[order], sim.download("v")[order], [int(row[1]) for row in step.data]))
        sim.close(download=False)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and min(out[0][2]) > N_SIM // 3


def test_host_resident_objects_get_the_device_s_counts():
    """The same explicit objects re-directed by ``step.run(sim)`` on the host and on the device: the same photons, the same
    state within the bound of the parity test."""
    n = 300
    v, dv = cloud(n, seed=4)
    got = []
    for where in ("host", "device"):
        objs = []
        for k in range(n):
            o = phys.light.PhotonObject(E=phys.Measurement(np.double(1e-19), "J**1"), v=phys.light.c * [1, 0, 0]) if k % 5 else phys.Object()
            o.v, o.dv = np.array(v[k]), np.array(dv[k])
            objs.append(o)
        sim = phys.Simulation(cl_on=True, rng="philox", seed=SEED)
        sim.add_objs(objs)
        step = phys.light.PhaseFunctionStep("rayleigh")
        if where == "device":
            sim._to_device()
        step.run(sim)
        got.append((step.redirected, np.array([np.asarray(o.v, dtype=np.float64) for o in sim.objects]),
                    np.array([np.asarray(o.dv, dtype=np.float64) for o in sim.objects])))
        sim.close(download=False)
    assert got[0][0] == got[1][0] == int(((np.arange(n) % 3 == 0) & (np.arange(n) % 5 != 0)).sum())
    c_code = light._c_h_literals()[0]
    assert np.max(np.abs(got[0][1] - got[1][1])) <= DIR_ULP * ulp(c_code) and np.max(np.abs(got[0][2] - got[1][2])) <= (DIR_ULP + 1) * ulp(c_code)
