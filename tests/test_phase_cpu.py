"""CPU: PhaseFunctionStep -- the constructor's refusals, the numpy restatement of the sweep (light._phase_redirect) on seeded
clouds (the laws' moments within 5 sigma of their exact values), degenerate rows, the host-resident path, the plan the step
makes, ``_device_run`` on stand-ins, the header's constants and the refusals that need no device."""
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import _hip, build, light
from phase_reference import C, SEED, cloud, frame, ulp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000
ALL = np.ones(N, dtype=bool)
IDS = np.arange(N) + 7_000_000_001
SIGMAS = 5.0


def redirect(phase="hg", g=0.0, n_pass=1, seed=SEED, state=None, photon=ALL, ids=IDS, dtype=np.float64):
    v, dv = state if state is not None else cloud(N)
    return (v, dv), light._phase_redirect(v, dv, photon, ids, phase, g, C, seed, n_pass, dtype)


def near(mean, exact, variance, n):
    """Is the mean of n independent draws within SIGMAS standard errors of its exact value?"""
    return abs(mean - exact) <= SIGMAS * np.sqrt(variance / n)


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("kw, word", [
    (dict(phase="mie"), "phase"), (dict(phase=1), "phase"), (dict(phase=None), "phase"),
    (dict(g=1), "g"), (dict(g=-1), "g"), (dict(g=1.5), "g"), (dict(g=np.nan), "g"), (dict(g=np.inf), "g"), (dict(g="x"), "g"),
    (dict(phase="rayleigh", g=1.0), "g")])
def test_constructor_refusals_name_the_argument(kw, word):
    with pytest.raises(ValueError, match=r"\b%s\b" % word):
        phys.light.PhaseFunctionStep(**kw)


def test_constructor_keeps_what_it_was_given():
    s = phys.light.PhaseFunctionStep("hg", 0.85)
    assert (s.phase, s.g, s.out_fn, s.redirected, s.data, s._pass) == ("hg", 0.85, None, 0, [], 0)
    assert s._fuse_role is None and s._device_native
    d = phys.light.PhaseFunctionStep()
    assert (d.phase, d.g) == ("hg", 0.0)
    assert phys.light.PhaseFunctionStep("rayleigh").phase == "rayleigh" and phys.light.PhaseFunctionStep("isotropic", -0.5).g == -0.5
    assert _hip.PHASE_FUNCTIONS == {"isotropic": 0, "hg": 1, "rayleigh": 2}
    assert _hip.SURFACE_MODES == {"lambertian": 0, "specular": 1}      # a table of its own


# ------------------------------------------------------------------------------------------------ the restatement
def moments(o):
    go = o["redirected"]
    return o["mu"][go], int(go.sum())


def check_geometry(v, dv, o):
    """What holds for every law: who is re-directed, |v| = c, mu is the cosine against the old direction, dv = v - v_old, the
    azimuth is uniform, and nobody else is touched."""
    go = o["redirected"]
    assert np.array_equal(go, np.arange(N) % 3 == 0) and np.array_equal(o["scattered"], go)
    old = (v - dv)[go]
    w = o["w"][go]
    # (w = old/|old|, and |old| is c but for the roundings of the cloud: the unit vector, c*, v - old and v - dv, half an ulp each per
    #  component, and two more for the root and the division here)
    assert np.max(np.abs(w - old / C)) <= 8 * ulp(1.0) and np.all(np.isnan(o["w"][~go])) and np.all(np.isnan(o["mu"][~go]))
    assert np.all(np.abs(w[np.flatnonzero(np.arange(N)[go] % 24 == 0)]).max(axis=1) == 1.0)     # exactly on an axis, the pole included
    speed = np.sqrt((o["v"][go] ** 2).sum(axis=1))
    assert np.max(np.abs(speed - C)) <= 8 * ulp(C)
    direction = o["v"][go] / C
    assert np.max(np.abs((direction * w).sum(axis=1) - o["mu"][go])) <= 1e-14
    assert np.array_equal(o["dv"][go], o["v"][go] - old)
    e1, e2 = frame(w)
    mu, n = moments(o)
    for e in (e1, e2):                                                 # s*cos psi and s*sin psi: mean 0, variance (1 - <mu^2>)/2 <= 1/2
        assert near(float((direction * e).sum(axis=1).mean()), 0.0, 0.5, n)
    assert np.array_equal(o["v"][~go], v[~go]) and np.array_equal(o["dv"][~go], dv[~go]) and not o["dv"][~go].any()
    return mu, n


def test_isotropic_is_uniform_on_the_sphere():
    (v, dv), o = redirect("isotropic")
    mu, n = check_geometry(v, dv, o)
    assert n == len(range(0, N, 3)) and np.all(np.abs(mu) <= 1)
    assert near(mu.mean(), 0.0, 1 / 3, n) and near((mu * mu).mean(), 1 / 3, 1 / 5 - 1 / 9, n)
    assert near((mu > 0.5).mean(), 0.25, 0.25 * 0.75, n)


@pytest.mark.parametrize("g", [-0.5, 0.3, 0.85, -1e-17])
def test_henyey_greenstein_has_the_mean_cosine_g(g):
    (v, dv), o = redirect("hg", g)
    mu, n = check_geometry(v, dv, o)
    second = (1 + 2 * g * g) / 3                                       # <mu^2> of the law; <mu> = g
    assert np.all(np.abs(mu) <= 1) and near(mu.mean(), g, second - g * g, n), mu.mean()
    assert near((mu * mu).mean(), second, 1.0, n)                      # (a variance bound: mu^2 lies in [0, 1])
    # the cumulative distribution at mu = 0:  P(mu <= 0) = (1 - g*g)/(2g) * (1/sqrt(1 + g*g) - 1/(1 + g))
    # (with the difference worked out, (1 + g) - sqrt(1 + g*g) = 2g / ((1 + g) + sqrt(1 + g*g)): the line above is 0/0 at a tiny g)
    root = np.sqrt(1 + g * g)
    below = (1 - g) / (root * ((1 + g) + root))
    assert near((mu <= 0).mean(), below, below * (1 - below), n)


def test_rayleigh_has_the_moments_of_three_eighths_one_plus_mu_squared():
    (v, dv), o = redirect("rayleigh")
    mu, n = check_geometry(v, dv, o)
    assert np.all(np.abs(mu) <= 1)
    assert near(mu.mean(), 0.0, 2 / 5, n) and near((mu * mu).mean(), 2 / 5, 9 / 35 - 4 / 25, n), (mu * mu).mean()
    # P(|mu| <= 1/2) = 3/8 * 2 * (1/2 + 1/24) = 13/32
    assert near((np.abs(mu) <= 0.5).mean(), 13 / 32, 13 / 32 * 19 / 32, n)


def test_another_pass_or_seed_gives_other_draws_and_g_zero_is_isotropic():
    _, o = redirect("rayleigh")
    go = o["redirected"]
    _, again = redirect("rayleigh", n_pass=2)
    _, other = redirect("rayleigh", seed=SEED + 1)
    _, same = redirect("rayleigh")
    assert not np.array_equal(again["mu"][go], o["mu"][go]) and not np.array_equal(other["mu"][go], o["mu"][go])
    assert np.array_equal(same["v"], o["v"])
    _, iso = redirect("isotropic")
    _, hg0 = redirect("hg", 0.0)
    _, ign = redirect("isotropic", 0.7)                                # g is looked at by hg alone
    for name in ("v", "dv", "mu"):
        assert np.array_equal(hg0[name], iso[name], equal_nan=True) and np.array_equal(ign[name], iso[name], equal_nan=True), name
    _, hg = redirect("hg", 1e-3)
    # (for small g the law runs the other way through u_a: mu = -1 at u_a = 0.  To first order in g it is 2*u_a - 1.)
    assert not np.array_equal(hg["mu"][go], iso["mu"][go]) and np.max(np.abs(hg["mu"][go] + iso["mu"][go])) < 2e-3


def test_degenerate_rows_are_left_alone_and_not_counted():
    v = np.array([[C, 0, 0],              # 0: NaN in dv, v finite: scattered, but the old velocity cannot be worked with
                  [0, C, 0],              # 1: v == dv: the old velocity is zero
                  [np.inf, 0, 0],         # 2: an infinite v
                  [0, 0, C],              # 3: a plain Object with dv != 0
                  [0, 0, C],              # 4: dv == 0: missed
                  [0, 0, C],              # 5: an ordinary hit, old direction -z
                  [1e200, 0, 0]])         # 6: a finite old velocity whose square is not
    dv = np.array([[np.nan, 0, 0], [0, C, 0], [1.0, 0, 0], [0, 0, 2 * C], [0, 0, 0], [0, 0, 2 * C], [0, 1.0, 0]])
    photon = np.array([1, 1, 1, 0, 1, 1, 1], dtype=bool)
    for phase in ("isotropic", "hg", "rayleigh"):
        o = light._phase_redirect(v, dv, photon, np.arange(len(v)), phase, 0.5, C, SEED, 1)
        assert o["scattered"].tolist() == [True, True, True, False, False, True, True]
        assert o["redirected"].tolist() == [False, False, False, False, False, True, False]
        keep = ~o["redirected"]
        assert np.array_equal(o["v"][keep], v[keep]) and np.array_equal(o["dv"][keep], dv[keep], equal_nan=True)
        assert np.array_equal(o["w"][5], [0.0, 0.0, -1.0]) and np.all(np.isfinite(o["v"][5]))
        assert abs(np.sqrt((o["v"][5] ** 2).sum()) - C) <= 8 * ulp(C) and abs(o["v"][5][2] / C + o["mu"][5]) <= 1e-14


def test_fp32_rows_are_the_fp64_results_rounded_once():
    state = cloud(N, dtype=np.float32)
    for phase, g in (("hg", 0.85), ("rayleigh", 0.0), ("hg", 1e-12), ("hg", -1e-300)):
        _, o64 = redirect(phase, g, state=state)
        _, o32 = redirect(phase, g, state=state, dtype=np.float32)
        assert o64["redirected"].sum() == len(range(0, N, 3))
        for name in ("v", "dv"):
            assert np.array_equal(o32[name], o64[name].astype(np.float32).astype(np.float64)), name


# ------------------------------------------------------------------------------------------------ the step on the host
def photons(n):
    v, dv = cloud(n, seed=11)
    out = []
    for k in range(n):
        o = phys.light.PhotonObject(E=phys.Measurement(np.double(1e-19), "J**1"), v=phys.light.c * [1, 0, 0]) if k % 5 else phys.Object()
        o.v, o.dv = np.array(v[k]), np.array(dv[k])
        out.append(o)
    return out, v, dv


class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed = 0.25, SEED

    def __init__(self, objs, py=False):
        self.objects, self.py = objs, py

    def _py_semantics(self):
        return self.py


def test_host_resident_objects_get_the_restatement_s_state(tmp_path):
    n = 400
    objs, v, dv = photons(n)
    sim = HostSim(objs)
    step = phys.light.PhaseFunctionStep("hg", 0.85, out_fn=str(tmp_path / "phase.csv"))
    step.run(sim)
    photon = np.arange(n) % 5 != 0
    o = light._phase_redirect(v, dv, photon, np.arange(n), "hg", 0.85, light._c_h_literals()[0], SEED, 1)
    assert step.redirected == int(o["redirected"].sum()) == int(((np.arange(n) % 3 == 0) & photon).sum()) > 100
    assert len(step.data) == 1 and list(step.data[0]) == [0.25, step.redirected]
    for k, obj in enumerate(sim.objects):
        assert np.array_equal(np.asarray(obj.v, dtype=np.float64), o["v"][k]) and np.array_equal(np.asarray(obj.dv, dtype=np.float64), o["dv"][k]), k
        assert type(obj) is (phys.light.PhotonObject if photon[k] else phys.Object)
    assert sim.launch_note is None                                     # the host path says nothing
    step.run(sim)                                                      # dv still says "scattered": the same photons, the pass's own draws
    again = light._phase_redirect(o["v"], o["dv"], photon, np.arange(n), "hg", 0.85, light._c_h_literals()[0], SEED, 2)
    assert step._pass == 2 and step.redirected == int(again["redirected"].sum()) and len(step.data) == 2
    assert np.array_equal(np.array([np.asarray(obj.v, dtype=np.float64) for obj in objs]), again["v"])
    step.terminate(sim)
    lines = open(str(tmp_path / "phase.csv")).read().splitlines()
    assert len(lines) == 2 and lines[0].split(", ")[1:] == [str(step.redirected)]


def test_python_semantics_are_refused_with_the_reason():
    objs, _, _ = photons(10)
    step = phys.light.PhaseFunctionStep("rayleigh")
    with pytest.raises(ValueError, match="dv = v_old"):
        step.run(HostSim(objs, py=True))
    with pytest.raises(ValueError, match="cl_on"):
        step._device_run(HostSim(objs, py=True))
    assert step._pass == 0 and step.data == []


def test_the_step_is_a_plan_item_of_its_own():
    redirector = phys.light.PhaseFunctionStep("hg", 0.85)

    class Sim:                                                         # what _build_plan / _multi_eligible ask of a simulation
        fuse, _hip = True, _hip
        steps = {0: phys.UpdateTimeStep(lambda s: np.double(1e-3)), 1: phys.newton.NewtonianKinematicsStep(),
                 2: phys.light.ScatterIsotropicStep(A=1.0, n=1.0), 3: redirector}

        def _py_semantics(self):
            return False
    sim = Sim()
    plan = phys.Simulation._build_plan(sim)
    assert [kind for kind, _ in plan] == ["single", "fused", "single"] and plan[-1][1] is redirector
    sim._plan = plan
    assert not phys.Simulation._multi_eligible(sim)


def test_device_run_notes_the_launch_schedule_and_reduces_the_count():
    class Dev:
        calls = []

        def phase_redirect(self, *a):
            self.calls.append(a)
            return 7

    class Sim:
        t, seed, launch_note, _dev = 0.5, 99, None, Dev()
        _scattered = False

        def _k_wanted(self):
            return 32

        def _py_semantics(self):
            return False

        def _global(self, values):
            return np.asarray(values, dtype=np.int64) * 2          # two ranks with the same count
    sim, step = Sim(), phys.light.PhaseFunctionStep("hg", 0.85)
    step._device_run(sim)
    step._device_run(sim)
    assert "PhaseFunctionStep" in sim.launch_note and "one launch per light step" in sim.launch_note and sim._scattered
    assert step.redirected == 14 and [list(r) for r in step.data] == [[0.5, 14]] * 2
    (a, b) = Dev.calls
    assert a[:4] == ("hg", 0.85, light._c_h_literals()[0], 99)
    assert (a[4], b[4]) == (1, 2)                                      # the step's own pass counter, not sim._next_launch()
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

        def phase_redirect(self, *a, **kw):
            return self.k
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    got = md.phase_redirect("rayleigh", 0.0, C, 1, 1)
    md._pool.shutdown()
    assert got == 111


# ------------------------------------------------------------------------------------------------ the library
def test_header_defines_the_phase_functions():
    text = open(os.path.join(ROOT, "include", "physicl_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, value in (("PCL_PHASE_ISOTROPIC", 0), ("PCL_PHASE_HG", 1), ("PCL_PHASE_RAYLEIGH", 2)):
        assert re.findall(r"#define\s+%s\s+(\d+)\b" % name, text) == [str(value)], name
        assert _hip.PHASE_FUNCTIONS[name[len("PCL_PHASE_"):].lower()] == value
    for entry in ("pcl_step_phase_redirect", "pcl_group_step_phase_redirect"):
        assert re.search(r"\b%s\s*\(" % entry, text) and entry in _hip.EXPORTS and entry in _hip._PROTOTYPES


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context, which is refused as well)."""
    build.build_lib()
    lib = _hip.load()
    assert hasattr(lib, "pcl_step_phase_redirect") and hasattr(lib, "pcl_group_step_phase_redirect") and lib.pcl_abi_version() == 1
    count = np.full(1, -7, dtype=np.int64)
    for phase, g, c, out in ((1, 0.85, C, count.ctypes.data), (3, 0.0, C, count.ctypes.data), (-1, 0.0, C, count.ctypes.data),
                             (1, 1.0, C, count.ctypes.data), (1, np.nan, C, count.ctypes.data), (2, 0.0, np.inf, count.ctypes.data),
                             (0, 0.0, C, None)):
        assert lib.pcl_step_phase_redirect(None, phase, g, c, 1, 1, out) == -2, (phase, g, c)
        assert lib.pcl_group_step_phase_redirect(None, phase, g, c, 1, 1, out) != 0, (phase, g, c)
    assert count.tolist() == [-7]
