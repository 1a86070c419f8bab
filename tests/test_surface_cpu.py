"""CPU: SurfaceReflectStep -- the constructor's refusals, the numpy restatement of the sweep (light._surface_bounce) on seeded
clouds, degenerate inputs, the host-resident path, the plan the step makes, the header's mode constants and the refusals that
need no device (the unit's build is held in tests/test_build_cpu.py)."""
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import _hip, build, light
from surface_reference import C, CENTER, RADIUS, SEED, cloud, ulp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000
ALL = np.ones(N, dtype=bool)
IDS = np.arange(N) + 7_000_000_001


def bounce(mode="lambertian", albedo=1.0, n_pass=1, seed=SEED, state=None, photon=ALL, ids=IDS, dtype=np.float64):
    r, dr, v = state if state is not None else cloud(N)
    return (r, dr, v), light._surface_bounce(r, dr, v, photon, ids, RADIUS, CENTER, albedo, mode, C, seed, n_pass, dtype)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw, word", [
    (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=np.nan), "radius"), (dict(radius=np.inf), "radius"),
    (dict(radius=1e200), "radius"), (dict(radius="x"), "radius"),
    (dict(radius=1.0, center=(0, np.nan, 0)), "center"), (dict(radius=1.0, center=(0, 0)), "center"), (dict(radius=1.0, center=(np.inf, 0, 0)), "center"),
    (dict(radius=1.0, albedo=-0.1), "albedo"), (dict(radius=1.0, albedo=1.0000001), "albedo"), (dict(radius=1.0, albedo=np.nan), "albedo"),
    (dict(radius=1.0, mode="mirror"), "mode"), (dict(radius=1.0, mode=1), "mode"), (dict(radius=1.0, mode=None), "mode")])
def test_constructor_refusals_name_the_argument(kw, word):
    with pytest.raises(ValueError, match=word):
        phys.light.SurfaceReflectStep(**kw)


def test_constructor_keeps_what_it_was_given():
    s = phys.light.SurfaceReflectStep(6371000.0, center=(1, 2, 3), albedo=0.3, mode="specular")
    assert s.radius == 6371000.0 and s.center.tolist() == [1.0, 2.0, 3.0] and s.albedo == 0.3 and s.mode == "specular"
    assert s._fuse_role is None and s._device_native and s.data == [] and (s.reflected, s.absorbed) == (0, 0)
    d = phys.light.SurfaceReflectStep(1.0)
    assert d.albedo == 1.0 and d.mode == "lambertian" and d.out_fn is None
    assert _hip.SURFACE_MODES == {"lambertian": 0, "specular": 1}


# ------------------------------------------------------------------------------------------------ the restatement
def test_philox_block_is_the_library_s():
    from oracle.physicl_oracle import philox4x32_10, u53
    ids = np.array([0, 1, 5, 2 ** 33 + 7, 2 ** 40, 2 ** 63 - 1], dtype=np.uint64)
    seed = 0x0123456789ABCDEF
    for word2, word3 in ((1, 8), (1, 9), (0xFFFFFFFF, 8), (77, 9)):
        got = light._philox_block(ids, seed, word2, word3)
        w = philox4x32_10(ids & np.uint64(0xFFFFFFFF), ids >> np.uint64(32), np.uint64(word2), np.uint64(word3), seed & 0xFFFFFFFF, seed >> 32)
        assert np.array_equal(got[0], u53(w[0], w[1])) and np.array_equal(got[1], u53(w[2], w[3]))


@pytest.mark.parametrize("mode", ["lambertian", "specular"])
def test_reflected_photons_leave_the_sphere_at_the_speed_of_light(mode):
    (r, dr, v), o = bounce(mode)
    hit, refl = o["hit"], o["reflected"]
    assert np.array_equal(hit, np.arange(N) % 2 == 0) and np.array_equal(refl, hit) and not o["absorbed"].any()
    q = ((o["r"] - CENTER) ** 2).sum(axis=1)
    assert np.all(q[refl] >= RADIUS * RADIUS * (1 - 1e-12))
    speed = np.sqrt((o["v"][refl] ** 2).sum(axis=1))
    assert np.max(np.abs(speed - C)) <= 8 * ulp(C)
    t = o["t"][hit]
    assert np.all((t >= 0) & (t <= 1)) and np.all(np.isnan(o["t"][~hit]))
    # p + m is the old position (about the centre), and x = p + t*m lies on the sphere
    p = (r - CENTER) - dr
    assert np.max(np.abs((p + dr) - (r - CENTER))) <= 2 * ulp(2 * RADIUS)
    assert np.max(np.abs(np.sqrt((o["x"][hit] ** 2).sum(axis=1)) - RADIUS)) <= 1e-13 * RADIUS
    # the rest of the move is flown along the new direction: |dr_new| = (1 - t)|dr_old|, dr_new parallel to v_new
    w = (1 - t) * np.sqrt((dr[hit] ** 2).sum(axis=1))
    assert np.allclose(np.sqrt((o["dr"][hit] ** 2).sum(axis=1)), w, rtol=1e-14, atol=0)
    assert np.allclose(o["dr"][hit] * C, o["v"][hit] * w[:, None], rtol=1e-13, atol=1e-6)
    assert np.array_equal(o["dv"][hit], o["v"][hit] - v[hit])
    # what is not hit is not touched
    for name, old in (("r", r), ("dr", dr), ("v", v)):
        assert np.array_equal(o[name][~hit], old[~hit]), name


def test_specular_mirrors_the_normal_component():
    (r, dr, v), o = bounce("specular")
    hit = o["hit"]
    vn_old, vn_new = (v[hit] * o["nrm"][hit]).sum(axis=1), (o["v"][hit] * o["nrm"][hit]).sum(axis=1)
    assert np.all(vn_old < 0) and np.max(np.abs(vn_new + vn_old)) <= 16 * ulp(C)
    tang_old, tang_new = v[hit] - vn_old[:, None] * o["nrm"][hit], o["v"][hit] - vn_new[:, None] * o["nrm"][hit]
    assert np.max(np.abs(tang_new - tang_old)) <= 16 * ulp(C)
    assert np.all(np.isnan(o["mu"]))                                   # no draw


def test_lambertian_is_cosine_weighted_about_the_normal():
    from source_reference import check_lambertian
    _, o = bounce("lambertian")
    hit = o["hit"]
    mu = (o["v"][hit] * o["nrm"][hit]).sum(axis=1) / C
    assert np.max(np.abs(mu - o["mu"][hit])) <= 1e-14
    check_lambertian(o["mu"][hit])                                     # mu > 0 always, the mean within 5 sigma of 2/3
    _, again = bounce("lambertian", n_pass=2)
    assert not np.array_equal(again["mu"][hit], o["mu"][hit])          # the pass counter is a counter word
    _, other = bounce("lambertian", seed=SEED + 1)
    assert not np.array_equal(other["mu"][hit], o["mu"][hit])


@pytest.mark.parametrize("mode", ["lambertian", "specular"])
def test_albedo_decides_the_outcome(mode):
    (r, dr, v), full = bounce(mode)
    _, o = bounce(mode, albedo=0.3)
    hit = o["hit"]
    n_hit = int(hit.sum())
    assert np.array_equal(hit, full["hit"]) and np.array_equal(o["reflected"] | o["absorbed"], hit) and not (o["reflected"] & o["absorbed"]).any()
    share = o["reflected"].sum() / n_hit
    assert abs(share - 0.3) <= 5 * np.sqrt(0.3 * 0.7 / n_hit), share
    refl, gone = o["reflected"], o["absorbed"]
    for name in ("r", "v", "dr", "dv"):                                # a reflected photon is the albedo-1 photon
        assert np.array_equal(o[name][refl], full[name][refl]), name
    assert not o["v"][gone].any() and np.array_equal(o["dv"][gone], 0.0 - v[gone])
    assert np.array_equal(o["r"][gone], CENTER + o["x"][gone]) and np.array_equal(o["dr"][gone], o["x"][gone] - ((r - CENTER) - dr)[gone])
    _, none = bounce(mode, albedo=0.0)
    assert np.array_equal(none["absorbed"], hit) and not none["reflected"].any()
    # an absorbed photon is at rest on the sphere: the next pass does not see it again
    _, nxt = bounce(mode, albedo=0.0, n_pass=2, state=(none["r"], np.zeros_like(dr), none["v"]))
    assert not nxt["hit"][gone].any()


def test_fp32_rows_are_the_fp64_results_rounded_once():
    state = cloud(N, dtype=np.float32)
    _, o64 = bounce("specular", albedo=0.5, state=state)
    _, o32 = bounce("specular", albedo=0.5, state=state, dtype=np.float32)
    for name in ("r", "v", "dr", "dv"):
        assert np.array_equal(o32[name], o64[name].astype(np.float32).astype(np.float64)), name


def test_grazing_and_degenerate_inputs():
    R = RADIUS
    r = np.array([[R - 1.0, 0, 0],        # 0: was exactly on the sphere, moving in: hit at t = 0
                  [R - 1.0, 0, 0],        # 1: dr = 0 inside: not hit
                  [np.nan, 0, 0],         # 2: NaN in r
                  [R - 1.0, 0, 0],        # 3: a plain Object
                  [R, 0, 0],              # 4: ends exactly on the sphere: outside, not hit
                  [R - 1.0, 0, 0],        # 5: NaN in dr
                  [R - 1.0, 0, 0],        # 6: came from infinitely far: no hit point
                  [0.0, 0.0, 0.0]]) + CENTER   # 7: ends on the centre
    dr = np.array([[-1.0, 0, 0], [0, 0, 0], [-1.0, 0, 0], [-2.0, 0, 0], [-1.0, 0, 0], [np.nan, 0, 0], [-np.inf, 0, 0], [-2 * R, 0, 0]])
    v = np.tile([-C, 0.0, 0.0], (len(r), 1))
    photon = np.array([1, 1, 1, 0, 1, 1, 1, 1], dtype=bool)
    o = light._surface_bounce(r, dr, v, photon, np.arange(len(r)), R, CENTER, 1.0, "specular", C, SEED, 1)
    assert o["hit"].tolist() == [True, False, False, False, False, False, False, True]
    assert o["t"][0] == 0.0 and np.array_equal(o["x"][0], [R, 0, 0]) and np.array_equal(o["nrm"][0], [1.0, 0, 0])
    assert np.array_equal(o["v"][0], [C, 0, 0]) and np.array_equal(o["dr"][0], [1.0, 0, 0]) and np.array_equal(o["r"][0], CENTER + [R + 1.0, 0, 0])
    assert o["t"][7] == 0.5 and np.array_equal(o["r"][7], CENTER + [2 * R, 0, 0])          # back out the way it came
    same = lambda a, b: np.array_equal(a, b, equal_nan=True)                                                     # noqa: E731
    for k in range(1, 7):
        assert same(o["r"][k], r[k]) and same(o["dr"][k], dr[k]) and same(o["v"][k], v[k]), k
    # the normal's z of either sign, and exactly -1 (the frame's pole): finite directions
    r = np.array([[0, 0, R - 1.0], [0, 0, -(R - 1.0)], [0.5, 0.5, -(R - 1.0)]]) + CENTER
    dr = np.array([[0, 0, -2.0], [0, 0, 2.0], [0, 0, 2.0]])
    o = light._surface_bounce(r, dr, np.zeros((3, 3)), np.ones(3, bool), np.arange(3), R, CENTER, 1.0, "lambertian", C, SEED, 1)
    assert o["hit"].all() and np.all(np.isfinite(o["v"])) and np.all((o["v"] * o["nrm"]).sum(axis=1) > 0)


def test_hits_are_the_inward_crossings_of_a_shell_of_the_same_radius():
    r, dr, v = cloud(N, seed=3)
    r[5], dr[7] = np.nan, np.nan
    photon = np.arange(N) % 7 != 0
    counts, _, _ = light._shell_tallies(r[photon], dr[photon], np.zeros(photon.sum()), np.ones(photon.sum(), bool), [RADIUS], CENTER)
    o = light._surface_bounce(r, dr, v, photon, IDS, RADIUS, CENTER, 0.5, "lambertian", C, SEED, 1)
    assert int(o["hit"].sum()) == int(counts[1, 0]) == int(o["reflected"].sum() + o["absorbed"].sum()) > 1000


# ------------------------------------------------------------------------------------------------ the step on the host
def photons(n):
    r, dr, v = cloud(n, seed=11)
    out = []
    for k in range(n):
        o = phys.light.PhotonObject(E=phys.Measurement(np.double(1e-19), "J**1"), v=phys.light.c * [1, 0, 0]) if k % 5 else phys.Object()
        o.r, o.dr = phys.Measurement._from_code(r[k], units="m**1"), phys.Measurement._from_code(dr[k], units="m**1")
        if k % 5:
            o.v = np.array(v[k])
        out.append(o)
    return out, r, dr, v


def test_host_resident_objects_get_the_restatement_s_state(tmp_path):
    n = 400
    objs, r, dr, v = photons(n)

    class Sim:                                                         # what the host path asks of a simulation (no device here)
        _residency, _batch, comm, launch_note = "host", None, None, None
        t, seed, objects = 0.25, SEED, objs
    sim = Sim()
    step = phys.light.SurfaceReflectStep(RADIUS, center=CENTER, albedo=0.5, mode="specular", out_fn=str(tmp_path / "ground.csv"))
    step.run(sim)
    photon = np.arange(n) % 5 != 0
    v_all = np.where(photon[:, None], v, 0.0)
    c_code = light._c_h_literals()[0]
    o = light._surface_bounce(r, dr, v_all, photon, np.arange(n), RADIUS, CENTER, 0.5, "specular", c_code, SEED, 1)
    assert (step.reflected, step.absorbed) == (int(o["reflected"].sum()), int(o["absorbed"].sum())) and step.reflected > 20 and step.absorbed > 20
    assert len(step.data) == 1 and list(step.data[0][1:]) == [step.reflected, step.absorbed]
    for k, obj in enumerate(sim.objects):
        assert np.array_equal(np.asarray(obj.r, dtype=np.float64), o["r"][k]) and np.array_equal(np.asarray(obj.dr, dtype=np.float64), o["dr"][k]), k
        if o["hit"][k]:
            assert np.array_equal(np.asarray(obj.v), o["v"][k]) and np.array_equal(np.asarray(obj.dv), o["dv"][k]), k
            assert type(obj) is phys.light.PhotonObject
    assert sim.launch_note is None                                     # the host path says nothing
    for obj in objs:                                                   # the Newton step of the next pass: v*dt, at rest 0
        obj.dr = phys.Measurement._from_code(np.asarray(obj.v, dtype=np.float64) * 1e-9, units="m**1")
        obj.r = phys.Measurement._from_code(np.asarray(obj.r, dtype=np.float64) + np.asarray(obj.dr, dtype=np.float64), units="m**1")
    step.run(sim)                                                      # the next pass draws its own blocks and finds nobody inside
    assert (step.reflected, step.absorbed) == (0, 0) and step._pass == 2 and len(step.data) == 2
    step.terminate(sim)
    lines = open(str(tmp_path / "ground.csv")).read().splitlines()
    assert len(lines) == 2 and lines[0].split(", ")[1:] == [str(int(o["reflected"].sum())), str(int(o["absorbed"].sum()))]
    assert lines[1].split(", ")[1:] == ["0", "0"]


def test_the_step_is_a_plan_item_of_its_own():
    shell = phys.light.ShellCrossingMeasureStep(None, [RADIUS], center=CENTER)
    ground = phys.light.SurfaceReflectStep(RADIUS, center=CENTER)

    class Sim:                                                         # what _build_plan / _multi_eligible ask of a simulation
        fuse, _hip = True, _hip
        steps = {0: phys.UpdateTimeStep(lambda s: np.double(1e-3)), 1: phys.newton.NewtonianKinematicsStep(),
                 2: phys.light.ScatterIsotropicStep(A=1.0, n=1.0), 3: shell, 4: ground}

        def _py_semantics(self):
            return False
    sim = Sim()
    plan = phys.Simulation._build_plan(sim)
    assert [kind for kind, _ in plan] == ["single", "fused", "single", "single"] and plan[-1][1] is ground and plan[-2][1] is shell
    sim._plan = plan
    assert not phys.Simulation._multi_eligible(sim)
    del Sim.steps[3]                                                   # without the tally: still a plan item of its own
    sim._plan = phys.Simulation._build_plan(sim)
    assert [kind for kind, _ in sim._plan] == ["single", "fused", "single"] and not phys.Simulation._multi_eligible(sim)


def test_device_run_notes_the_launch_schedule_and_reduces_the_counts():
    class Dev:
        count = 5
        calls = []

        def surface_reflect(self, *a):
            self.calls.append(a)
            return 3, 2

    class Sim:
        t, seed, launch_note, _dev = 0.5, 99, None, Dev()
        _scattered = False

        def _k_wanted(self):
            return 32

        def _global(self, values):
            return np.asarray(values, dtype=np.int64) * 2          # two ranks with the same counts
    sim, step = Sim(), phys.light.SurfaceReflectStep(RADIUS, center=CENTER, albedo=0.25)
    step._device_run(sim)
    step._device_run(sim)
    assert "SurfaceReflectStep" in sim.launch_note and sim._scattered
    assert (step.reflected, step.absorbed) == (6, 4) and [list(r) for r in step.data] == [[0.5, 6, 4]] * 2
    (a, b) = Dev.calls
    assert a[0] == RADIUS and a[2] == 0.25 and a[3] == "lambertian" and a[4] == light._c_h_literals()[0] and a[5] == 99
    assert (a[6], b[6]) == (1, 2)                                      # the step's own pass counter, not sim._next_launch()
    sim2 = Sim()
    sim2.launch_note = "something else"
    step._device_run(sim2)
    assert sim2.launch_note == "something else"


def test_multi_device_sums_the_shards_counts():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def surface_reflect(self, *a, **kw):
            return self.k, 2 * self.k
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    got = md.surface_reflect(RADIUS, CENTER, 1.0, "specular", C, 1, 1)
    md._pool.shutdown()
    assert got == (111, 222)


# ------------------------------------------------------------------------------------------------ the library
def test_header_defines_the_modes():
    text = open(os.path.join(ROOT, "include", "physicl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"#define\s+PCL_SURFACE_LAMBERTIAN\s+0\b", text) and re.search(r"#define\s+PCL_SURFACE_SPECULAR\s+1\b", text)
    assert re.search(r"#define\s+PCL_ABI_VERSION\s+1\b", text) or "pcl_abi_version" in text


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context, which is refused as well)."""
    build.build_lib()
    lib = _hip.load()
    counts = np.full(2, -7, dtype=np.int64)
    assert lib.pcl_step_surface_reflect(None, 1.0, None, 1.0, 0, C, 1, 1, counts.ctypes.data) == -2
    assert lib.pcl_group_step_surface_reflect(None, 1.0, None, 1.0, 0, C, 1, 1, counts.ctypes.data) != 0
    assert counts.tolist() == [-7, -7]
