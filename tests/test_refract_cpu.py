"""CPU: RefractiveSurfaceStep (light.RefractiveSurfaceStep, light._refract_surface, pcl_step_refract_surface) -- the constructor, the
numpy restatement against a plain loop on a scene that holds every case, the closed forms of Snell and Fresnel, the statistics of
the draw, the agreement with a shell tally of the same radius, the host-resident path, the header, the bindings, the build table
and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
from physicl_amd import _hip, build, light, tally
from refract_reference import (BAD_CALLS, BAD_STEPS, BUBBLE, C, CENTER, COUNTS, GLASS, GLASS_PLAIN, N_IN, N_OUT, RADIUS, SEED, abi_args,
                               refract, refract_surface_loop, same_answer, scene)
from writer_reference import same_bits

ENTRIES = ("pcl_step_refract_surface", "pcl_group_step_refract_surface")
N = 3000
EPS = float(np.spacing(1.0))


# ------------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("kw, word", BAD_STEPS)
def test_constructor_refusals_name_the_argument(kw, word):
    a = dict(radius=1.0, n_inside=1.5)
    a.update(kw)
    with pytest.raises(ValueError, match=word):
        phys.light.RefractiveSurfaceStep(**a)
    assert "pcl_step_refract_surface" in light._check_refractive.__doc__


def test_constructor_keeps_what_it_was_given_and_the_class_is_where_the_ground_is():
    step = phys.light.RefractiveSurfaceStep(2.5, 4.0 / 3.0, 1.25, CENTER, fresnel=0, out_fn="rows.csv")
    assert (step.radius, step.n_inside, step.n_outside, step.fresnel, step.out_fn) == (2.5, 4.0 / 3.0, 1.25, False, "rows.csv")
    assert step.center.tolist() == CENTER.tolist() and (step._pass, step.data) == (0, [])
    assert [getattr(step, name) for name in COUNTS] == [0] * 6
    plain = phys.light.RefractiveSurfaceStep(1.0, 1.5)
    assert (plain.n_outside, plain.fresnel, plain.out_fn) == (1.0, True, None) and plain.center.tolist() == [0.0, 0.0, 0.0]
    assert plain._writes == ("r", "dr", "v", "dv") and plain._fuse_role is None
    import phys.light as short
    assert short.RefractiveSurfaceStep is light.RefractiveSurfaceStep is phys.light.RefractiveSurfaceStep
    cls = light.RefractiveSurfaceStep
    assert issubclass(cls, tally.WriterStep) and cls.__mro__[1] is tally.WriterStep and not set(vars(cls)) & {"run", "_device_run", "_reduce"}
    assert "one launch per light step" in cls._NOTE and "RefractiveSurfaceStep" in cls._NOTE
    for module in (phys.light, short, light):                          # re-exported wherever the ground is
        assert hasattr(module, "SurfaceReflectStep") and hasattr(module, "RefractiveSurfaceStep")


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cfg", [GLASS, GLASS_PLAIN, BUBBLE], ids=["glass", "glass_plain", "bubble"])
def test_the_restatement_is_the_loop_bit_for_bit(cfg, dtype):
    state = scene(N, dtype)
    for n_pass in (1, 2):
        ref, loop = (refract(fn, state, cfg, n_pass, dtype) for fn in (light._refract_surface, refract_surface_loop))
        assert same_answer(ref, loop), n_pass
    counts = dict(zip(COUNTS, ref["counts"].tolist()))
    assert counts["in_refracted"] > 0 and counts["out_refracted"] > 0 and sum(ref["counts"][:5]) == ref["crossed"].sum()
    if cfg is GLASS:                                                   # both directions, all three outcomes
        assert min(counts[k] for k in COUNTS[:5]) > 0 and counts["out_total"] > N // 20
    if cfg is GLASS_PLAIN:                                             # nothing is drawn: nobody is reflected but beyond the critical angle
        assert counts["in_reflected"] == counts["out_reflected"] == 0 < counts["out_total"] and not ref["reflected"].any()
    if cfg is BUBBLE:                                                  # total on the way in: counted as reflected; none on the way out
        assert counts["out_total"] == 0 and (ref["total"] & ref["inward"]).sum() > 0
        assert counts["in_reflected"] == ((ref["total"] | ref["reflected"]) & ref["inward"]).sum()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_scene_holds_every_case(dtype):
    state = scene(N, dtype)
    ref = refract(light._refract_surface, state, GLASS, dtype=dtype)
    i = np.arange(N)
    hit, photon = ref["crossed"], state["photon"]
    bad = (i % 34 == 8) | (i % 38 == 10) | (i % 58 == 14)             # a NaN in r, a NaN in dr, an infinite dr
    on_before, on_after, on_after_out, still = (i % 62 == 16) & ~bad, (i % 66 == 18) & ~bad, (i % 70 == 20) & ~bad, (i % 74 == 22) & ~bad
    on_before &= ~((i % 66 == 18) | (i % 70 == 20) | (i % 74 == 22))  # (the scene writes them in this order: the later one stays)
    on_after &= ~((i % 70 == 20) | (i % 74 == 22))
    on_after_out &= ~(i % 74 == 22)
    assert not hit[~photon].any() and not hit[bad].any() and (bad & photon).sum() > 100
    assert (on_before & photon).sum() > 0 and ref["inward"][on_before & photon].all() and (ref["t"][on_before & photon] == 0.0).all()
    assert (on_after & photon).sum() > 0 and ref["outward"][on_after & photon].all() and (ref["t"][on_after & photon] == 1.0).all()
    assert (on_after_out & photon).sum() > 0 and not hit[on_after_out].any()
    assert (still & photon).sum() > 0 and not hit[still].any()        # a == 0
    nan_v = (i % 46 == 12) & hit
    assert nan_v.sum() > 0 and np.isnan(ref["dv"][nan_v]).any(axis=1).all() and np.isfinite(ref["v"][nan_v]).all()
    plain = hit & ~nan_v
    assert 0.25 * N < ref["inward"].sum() < 0.4 * N and 0.2 * N < ref["outward"].sum() < 0.4 * N and (~hit).sum() > 0.3 * N
    # who does not cross keeps every bit and is not written; who crosses flies on at c, its dv the change of v
    for f in ("r", "v", "dr"):
        assert same_bits(ref[f][~hit], state[f][~hit]), f
    assert np.isnan(ref["dv"][~hit]).all()
    T = dtype
    assert same_bits(ref["dv"][plain], (ref["dir"][plain] * C - state["v"][plain]).astype(T).astype(np.float64))
    assert same_bits(ref["v"][plain], (C * ref["dir"][plain]).astype(T).astype(np.float64))
    # the masks: one outcome each
    assert np.array_equal(ref["refracted"] | ref["reflected"] | ref["total"], hit)
    assert not (ref["refracted"] & (ref["reflected"] | ref["total"])).any() and not (ref["reflected"] & ref["total"]).any()
    assert not ref["total"][ref["inward"]].any()                       # n_inside > n_outside: total on the way out only
    # the block is the one the header names, the draw its first uniform
    k = int(np.flatnonzero(ref["reflected"])[0])
    u = light._philox_block([state["id"][k]], SEED, 1, 21)[0][0]
    assert u < ref["F"][k] and light._REFRACT_WORD == 21
    k = int(np.flatnonzero(ref["refracted"] & (ref["F"] > 0.2))[0])
    assert not light._philox_block([state["id"][k]], SEED, 1, 21)[0][0] < ref["F"][k]


def test_the_draws_follow_the_id_the_pass_and_the_seed():
    state = scene(N, nan_v=False)
    one = refract(light._refract_surface, state, GLASS)
    for other in (refract(light._refract_surface, state, GLASS, n_pass=2), refract(light._refract_surface, state, GLASS, seed=SEED + 1),
                  refract(light._refract_surface, state, GLASS, ids=state["id"] + 1)):
        assert np.array_equal(other["crossed"], one["crossed"]) and np.array_equal(other["total"], one["total"])
        assert same_bits(other["F"], one["F"]) and not np.array_equal(other["reflected"], one["reflected"])
    perm = np.random.RandomState(3).permutation(N)
    moved = refract(light._refract_surface, {k: a[perm] for k, a in state.items()}, GLASS)
    assert all(same_bits(moved[f], one[f][perm]) for f in ("r", "v", "dr", "dv"))                   # a photon is its id, wherever it stands
    plain = refract(light._refract_surface, state, GLASS_PLAIN, n_pass=2)
    assert same_bits(plain["r"], refract(light._refract_surface, state, GLASS_PLAIN, n_pass=9, seed=1)["r"])   # nothing is drawn


# ------------------------------------------------------------------------------------------------ closed forms
def rays(theta, n1, n2, outward=False, n=None):
    """Photons that meet the unit sphere about the origin at the angle(s) ``theta`` to the normal, coming from the medium n1 into n2:
    the restatement's answer (fresnel=False) and the angles."""
    theta = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    rng = np.random.RandomState(11)
    k = len(theta)
    x = rng.normal(size=(k, 3))
    x /= np.sqrt((x * x).sum(axis=1))[:, None]
    tang = np.cross(x, rng.normal(size=(k, 3)))
    tang /= np.sqrt((tang * tang).sum(axis=1))[:, None]
    sign = 1.0 if outward else -1.0
    way = sign * np.cos(theta)[:, None] * x + np.sin(theta)[:, None] * tang
    length = 1e-3                                                      # half of it on either side: shorter than any chord asked for
    r, dr = x + 0.5 * length * way, length * way
    n_in, n_out = (n1, n2) if outward else (n2, n1)
    ref = light._refract_surface(r, dr, C * way, np.ones(k, dtype=bool), np.arange(k), 1.0, (0.0, 0.0, 0.0), n_in, n_out, False, C, 1, 1)
    assert ref["crossed"].all() and (ref["outward"] if outward else ref["inward"]).all()
    return ref, theta


@pytest.mark.parametrize("n1, n2", [(1.0, 1.5), (1.5, 1.0), (1.0, 4.0 / 3.0), (1.33, 2.42)])
def test_normal_incidence_is_the_textbook_reflectance(n1, n2):
    for outward in (False, True):
        ref, _ = rays(np.zeros(20), n1, n2, outward)
        want = ((n1 - n2) / (n1 + n2)) ** 2
        # ci is 1 within a few ulp (a unit vector's length), and F's slope in ci is gentle there: a few ulp of F, and 8 are allowed
        assert np.max(np.abs(ref["F"] - want)) <= 8 * np.spacing(want), (n1, n2, outward)


@pytest.mark.parametrize("n1, n2", [(1.0, 1.5), (1.5, 1.0), (1.0, 4.0 / 3.0)])
def test_brewster_s_angle_has_no_parallel_reflection(n1, n2):
    ref, _ = rays(np.full(20, np.arctan2(n2, n1)), n1, n2, outward=n1 > n2)
    # rp = (ci - eta*ct) / (ci + eta*ct): numerator and denominator are of order 1, each term good to a few ulp
    assert np.max(np.abs(ref["rp"])) <= 16 * EPS and np.min(np.abs(ref["rs"])) > 0.1


def test_equal_indices_are_no_interface():
    state = scene(N, nan_v=False)
    for n in (1.0, 1.5, 4.0 / 3.0):
        for fresnel in (True, False):
            ref = refract(light._refract_surface, state, dict(GLASS, n_inside=n, n_outside=n, fresnel=fresnel))
            hit = ref["crossed"]
            assert hit.sum() > N // 2 and (ref["F"][hit] == 0.0).all() and (ref["dir"][hit] == ref["mh"][hit]).all()
            assert not ref["reflected"].any() and not ref["total"].any() and ref["refracted"][hit].all()
            assert ref["counts"][[1, 3, 4]].tolist() == [0, 0, 0]


def test_beyond_the_critical_angle_every_crossing_is_total_and_none_draws():
    n1, n2 = 1.5, 1.0
    crit = np.arcsin(n2 / n1)
    theta = np.linspace(crit + 1e-6, np.pi / 2 - 1e-3, 400)
    ref, _ = rays(theta, n1, n2, outward=True)
    assert ref["total"].all() and not ref["refracted"].any() and not ref["reflected"].any() and np.isnan(ref["F"]).all()
    below, _ = rays(np.linspace(0.0, crit - 1e-6, 400), n1, n2, outward=True)
    assert not below["total"].any() and below["refracted"].all()
    # the reflection is a mirror's: the tangential part stays, the normal part turns
    d, mh, nrm = ref["dir"], ref["mh"], ref["N"]
    assert np.max(np.abs((d * nrm).sum(axis=1) + (mh * nrm).sum(axis=1))) <= 8 * EPS
    # and none draws: another seed, another pass, the same bits, with fresnel=True as well
    state = scene(N, nan_v=False)
    state["dr"][~(np.arange(N) % 3 == 1)] = 0.0                        # only the outward crossers move
    a = refract(light._refract_surface, state, GLASS, n_pass=1, seed=1)
    b = refract(light._refract_surface, state, GLASS, n_pass=2, seed=2)
    tot = a["total"]
    assert tot.sum() > 100 and np.array_equal(tot, b["total"]) and all(same_bits(a[f][tot], b[f][tot]) for f in ("r", "v", "dr", "dv"))


@pytest.mark.parametrize("n1, n2, outward", [(1.0, 1.5, False), (1.5, 1.0, True), (1.0, 4.0 / 3.0, False), (4.0 / 3.0, 1.0, True)])
def test_snell_unit_length_and_reversibility(n1, n2, outward):
    # The angles.  A unit vector's components carry half an ulp of 1 each, so a sine made of them is good to a few 1e-16 ABSOLUTE:
    # 1e-14 relative can be asked from sin(theta) = 0.1 on.  On the thin side the angle goes up to 1.45 (83 degrees): the way back
    # from there amplifies an error by 1 / cos(1.45) = 8, and further out the bound would measure that, not the rule.
    thin_top = 1.45
    lo, top = (0.1, thin_top) if n1 < n2 else (np.arcsin(n2 / n1 * np.sin(0.1)), np.arcsin(n2 / n1 * np.sin(thin_top)))
    ref, theta = rays(np.linspace(lo, top, 500), n1, n2, outward)
    d, mh, nrm = ref["dir"], ref["mh"], ref["N"]
    assert ref["refracted"].all()
    length = np.sqrt((d * d).sum(axis=1))
    assert np.max(np.abs(length - 1.0)) <= 4 * EPS                     # |dir| within 4 ulp of 1
    sin_i = np.sqrt((np.cross(mh, nrm) ** 2).sum(axis=1))
    sin_t = np.sqrt((np.cross(d, nrm) ** 2).sum(axis=1))
    assert np.max(np.abs(n1 * sin_i - n2 * sin_t) / (n1 * sin_i)) <= 1e-14              # Snell
    assert np.max(np.abs(sin_i - np.sin(theta)) / np.sin(theta)) <= 1e-12               # (the rays are the ones asked for)
    assert ((d * nrm).sum(axis=1) < 0).all() and np.max(np.abs((np.cross(d, mh) * nrm).sum(axis=1))) <= 4 * EPS   # onward, in the plane
    # sent back through the hit point, the refracted ray refracts onto -mh
    x, length = ref["x"], 1e-3
    back = -d
    r, dr = x + 0.5 * length * back, length * back
    n_in, n_out = (n1, n2) if outward else (n2, n1)
    rev = light._refract_surface(r, dr, C * back, np.ones(len(x), dtype=bool), np.arange(len(x)), 1.0, (0.0, 0.0, 0.0), n_in, n_out, False,
                                 C, 1, 1)
    assert rev["crossed"].all() and (rev["inward"] if outward else rev["outward"]).all() and rev["refracted"].all()
    print("snell %.3g, back onto -mh %.3g" % (np.max(np.abs(n1 * sin_i - n2 * sin_t) / (n1 * sin_i)), np.max(np.abs(rev["dir"] + mh))))
    assert np.max(np.abs(rev["dir"] + mh)) <= 1e-14


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("theta_deg, n1, n2, outward", [(60.0, 1.0, 1.5, False), (35.0, 1.5, 1.0, True)])
def test_the_reflected_share_is_fresnel_s(theta_deg, n1, n2, outward):
    n = 200_000
    theta = np.radians(theta_deg)
    x = np.array([0.0, 0.0, 1.0])
    way = (1.0 if outward else -1.0) * np.cos(theta) * x + np.sin(theta) * np.array([1.0, 0.0, 0.0])
    length = 0.01
    r, dr = np.tile(x + 0.5 * length * way, (n, 1)), np.tile(length * way, (n, 1))
    n_in, n_out = (n1, n2) if outward else (n2, n1)
    ref = light._refract_surface(r, dr, np.tile(C * way, (n, 1)), np.ones(n, dtype=bool), np.arange(n) + 12345, 1.0, (0.0, 0.0, 0.0), n_in,
                                 n_out, True, C, SEED, 3)
    F = ref["F"][0]
    ci, ct = np.cos(theta), np.sqrt(1.0 - (n1 / n2 * np.sin(theta)) ** 2)
    want = 0.5 * (((n1 * ci - n2 * ct) / (n1 * ci + n2 * ct)) ** 2 + ((n1 * ct - n2 * ci) / (n1 * ct + n2 * ci)) ** 2)
    assert ref["crossed"].all() and (ref["F"] == F).all() and abs(F - want) <= 1e-13 and 0.02 < F < 0.5
    got = int(ref["counts"][3 if outward else 1])
    sigma = np.sqrt(n * F * (1.0 - F))                                 # binomial: the bound is derived, not measured
    print("reflected %d of %d, N*F = %.1f, sigma = %.1f: %.2f sigma" % (got, n, n * F, sigma, (got - n * F) / sigma))
    assert abs(got - n * F) <= 5.0 * sigma and got == ref["reflected"].sum()
    assert ref["counts"][2 if outward else 0] == n - got and ref["counts"].sum() == n


# ------------------------------------------------------------------------------------------------ the shell of the same radius
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cfg", [GLASS, BUBBLE], ids=["glass", "bubble"])
def test_a_shell_of_the_same_radius_counts_the_same_crossings(cfg, dtype):
    state = scene(N, dtype, nan_v=False)
    finite = np.isfinite(state["dr"]).all(axis=1) & np.isfinite(state["r"]).all(axis=1)
    state = {k: a[finite] for k, a in state.items()}                   # every q_prev finite
    photon = np.ones(len(state["r"]), dtype=bool)                      # (a shell counts plain Objects, too)
    ref = refract(light._refract_surface, state, cfg, dtype=dtype, photon=photon)
    counts, _, _ = light._shell_tallies(state["r"], state["dr"], np.ones(len(photon)), photon, [RADIUS], CENTER)
    c = dict(zip(COUNTS, ref["counts"].tolist()))
    assert counts[1][0] == c["in_refracted"] + c["in_reflected"] > 0
    assert counts[0][0] == c["out_refracted"] + c["out_reflected"] + c["out_total"] > 0


# ------------------------------------------------------------------------------------------------ the step on the host
class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed = 0.25, SEED

    def __init__(self, objs, py=False):
        self.objects, self.py = objs, py

    def _py_semantics(self):
        return self.py


def objects(state):
    out = []
    for k in range(len(state["photon"])):
        if state["photon"][k]:
            o = phys.light.PhotonObject(E=phys.Measurement(np.double(1e-19), "J**1"), v=phys.light.c * [1, 0, 0])
        else:
            o = phys.Object()
        o.r = phys.Measurement(np.array(state["r"][k]), "m**1")
        o.v, o.dv = np.array(state["v"][k]), np.array(state["dv"][k])
        o.dr = phys.Measurement(np.array(state["dr"][k]), "m**1")
        out.append(o)
    return out


@pytest.mark.parametrize("py", [False, True])
def test_host_resident_objects_get_the_restatement_s_state(tmp_path, py):
    n = 900
    state = scene(n, nan_v=False)
    objs = objects(state)
    sim = HostSim(objs, py=py)                                         # the step reads no dv rule: cl_on=False is not refused
    r0, v0, dr0, dv0 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    step = phys.light.RefractiveSurfaceStep(RADIUS, N_IN, N_OUT, CENTER, out_fn=str(tmp_path / "refract.csv"))
    step.run(sim)
    c_code = light._c_h_literals()[0]
    ref = light._refract_surface(r0, dr0, v0, state["photon"], np.arange(n), RADIUS, CENTER, N_IN, N_OUT, True, c_code, SEED, 1)
    hit = ref["crossed"]
    assert [getattr(step, name) for name in COUNTS] == ref["counts"].tolist() and min(ref["counts"][:5]) > 0
    assert len(step.data) == 1 and list(step.data[0]) == [0.25] + ref["counts"].tolist() and sim.launch_note is None
    r1, v1, dr1, dv1 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    assert same_bits(r1, ref["r"]) and same_bits(v1, ref["v"]) and same_bits(dr1, ref["dr"])
    assert same_bits(dv1[hit], ref["dv"][hit]) and same_bits(dv1[~hit], dv0[~hit])
    for k, obj in enumerate(objs):
        assert type(obj) is (phys.light.PhotonObject if state["photon"][k] else phys.Object)
    step.run(sim)                                                      # a second pass: the counter moves
    again = light._refract_surface(ref["r"], ref["dr"], ref["v"], state["photon"], np.arange(n), RADIUS, CENTER, N_IN, N_OUT, True, c_code,
                                   SEED, 2)
    assert step._pass == 2 and len(step.data) == 2 and list(step.data[1][1:]) == again["counts"].tolist()
    step.terminate(sim)
    lines = open(str(tmp_path / "refract.csv")).read().splitlines()
    assert len(lines) == 2 and [float(x) for x in lines[1].split(",")] == [0.25] + again["counts"].tolist()


def test_the_step_is_a_plan_item_of_its_own():
    import physicl.newton
    step = phys.light.RefractiveSurfaceStep(1.0, 1.5)

    class Sim:                                                         # what _build_plan / _multi_eligible ask of a simulation
        fuse, _hip = True, _hip
        steps = {0: phys.UpdateTimeStep(lambda s: np.double(1e-3)), 1: phys.newton.NewtonianKinematicsStep(),
                 2: phys.light.ScatterIsotropicStep(A=1.0, n=1.0), 3: phys.light.ShellCrossingMeasureStep(None, [1.0]), 4: step}

        def _py_semantics(self):
            return False
    sim = Sim()
    plan = phys.Simulation._build_plan(sim)
    assert plan[-1] == ("single", step) or (plan[-1][0] == "single" and plan[-1][1] is step)
    sim._plan = plan
    assert not phys.Simulation._multi_eligible(sim)


def test_device_run_notes_the_launch_schedule_and_reduces_the_row():
    class Dev:
        count, calls = 1000, []

        def refract_surface(self, *a):
            self.calls.append(a)
            return np.array([5, 4, 3, 2, 1, 0], dtype=np.int64)

    class Sim:
        t, seed, launch_note, _dev, _scattered, chunks = 0.5, 99, None, Dev(), False, []

        def _k_wanted(self):
            return 32

        def _py_semantics(self):
            return True                                                # not refused: the step needs no dv rule

        def _global(self, values):
            self.chunks.append(len(values))
            return np.asarray(values, dtype=np.int64) * 2               # two ranks with the same tallies
    sim = Sim()
    step = phys.light.RefractiveSurfaceStep(2.0, 1.5, 1.25, CENTER, fresnel=False)
    step._device_run(sim)
    step._device_run(sim)
    assert "RefractiveSurfaceStep" in sim.launch_note and "one launch per light step" in sim.launch_note and sim._scattered
    assert [getattr(step, name) for name in COUNTS] == [10, 8, 6, 4, 2, 0]
    assert len(step.data) == 2 and list(step.data[1]) == [0.5, 10, 8, 6, 4, 2, 0]
    assert sim.chunks == [1 + 6] * 2                                    # one collective per pass: N and the six counts
    a, b = Dev.calls
    assert a[:3] == (2.0, 1.5, 1.25) and a[3].tolist() == CENTER.tolist() and a[4] is False and a[5] == light._c_h_literals()[0]
    assert (a[6], a[7], b[7]) == (99, 1, 2)


def test_multi_device_sums_the_shards_counts():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def refract_surface(self, *a, **kw):
            return self.k * np.arange(6, dtype=np.int64)
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    got = md.refract_surface(1.0, 1.5)
    md._pool.shutdown()
    assert got.tolist() == [0, 111, 222, 333, 444, 555]


def test_binding_marshals_the_call():
    def entry(handle, radius, ce, n_in, n_out, fresnel, c, seed, n_pass, counts):
        center = None if ce is None else np.ctypeslib.as_array(ctypes.cast(ce, ctypes.POINTER(ctypes.c_double)), (3,)).tolist()
        seen.append((handle, radius, center, n_in, n_out, fresnel, c, seed, n_pass))
        np.ctypeslib.as_array(ctypes.cast(counts, ctypes.POINTER(ctypes.c_int64)), (6,))[:] = np.arange(6) + 100
        return 0
    seen = []
    got = _hip._refract(entry, "h", 2.0, CENTER, 1.5, 1.25, True, C, -1, 2 ** 32 + 3)
    assert got.tolist() == [100, 101, 102, 103, 104, 105] and got.dtype == np.int64
    assert seen[0] == ("h", 2.0, CENTER.tolist(), 1.5, 1.25, 1, C, 2 ** 64 - 1, 3)
    _hip._refract(entry, "h", 2.0, None, 1.5, 1.0, 0, C, 1, 1)
    assert seen[1][2] is None and seen[1][5] == 0


# ------------------------------------------------------------------------------------------------ the library
def surface_unit():
    (unit,) = [u for u in build.ADDONS if os.path.basename(u["src"]) == "pcl_surface.hip"]
    return unit


def test_header_prototypes_and_the_build_table():
    text = open(build.ABI_HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and len(_hip._PROTOTYPES[entry]) == 10
    assert "(id_lo, id_hi, pass, 21)" in text                          # the arithmetic is written out, the counter word with it
    flat = " ".join(text.split()).replace("* ", "")
    assert "word 21 is used by nothing else" in flat and "0-5 and 8-20 are taken" in flat
    for line in ("k = 1 - (eta*eta)*(1 - ci*ci)", "rs = (ec - ct) / (ec + ct)", "rp = (ci - ect) / (ci + ect)", "F = (rs*rs + rp*rp)*0.5",
                 "dir = eta*mh + (ec - ct)*N", "dir = mh + (2*ci)*N", "t = (0 - cq) / (sq + b)", "t = (sq - b) / a", "t = cq / (sq - b)"):
        assert line in flat, line
    assert hasattr(_hip.Device, "refract_surface") and hasattr(_hip.DeviceGroup, "refract_surface")
    from physicl_amd.multidev import MultiDevice
    assert hasattr(MultiDevice, "refract_surface")
    # the table: the unit of the writer sweeps holds this one, described as every sweep is (tests/test_build_cpu.py checks it as one)
    assert dict(entries=ENTRIES, kernel="k_refract_surface", count=2) in surface_unit()["sweeps"]


def test_the_counter_word_is_a_named_constant_used_nowhere_else():
    src = open(os.path.join(build.CSRC, "pcl_surface.hip")).read()
    assert re.findall(r"\b(kRefract\w+) = (\d+)", src) == [("kRefractDraw", "21")]
    assert len(re.findall(r"pcl_philox4x32_10\([^;]*?, kRefractDraw, ", src)) == 1
    assert len(re.findall(r"\bkRefractDraw\b", src)) == 2              # the constant and its one call
    for f in sorted(os.listdir(build.CSRC)):
        if f.endswith((".hip", ".h", ".inc")):
            text = open(os.path.join(build.CSRC, f)).read()
            words = [int(w) for w in re.findall(r"pcl_philox4x32_10\([^;]*?, (\d+)u, ", text)]
            words += [int(w) for w in re.findall(r"\bk\w+ = (\d+)[,;]", text) if f != "pcl_surface.hip"]
            assert 21 not in words, f
    named = dict(re.findall(r"\b(k[A-Z]\w+) = (\d+)", src))
    assert [k for k, w in named.items() if w == "21"] == ["kRefractDraw"]


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context and a NULL group, refused as well); the counts stay as
    they were."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in BAD_CALLS:
        keep, args, counts = abi_args(**kw)
        assert lib.pcl_step_refract_surface(None, *args) == -2, kw
        assert lib.pcl_group_step_refract_surface(None, *args) == -2, kw
        assert counts is None or (counts == -7).all(), kw
    keep, args, counts = abi_args()                                    # a good call without a context is refused, too
    assert lib.pcl_step_refract_surface(None, *args) == -2 and lib.pcl_group_step_refract_surface(None, *args) != 0
    assert (counts == -7).all()
