"""CPU: LayeredScatterStep (light.LayeredScatterStep, light._scatter_layered, pcl_step_scatter_layered) -- the numpy restatement
against a plain loop on states that hold every case, the contracts of the two miss modes, the independence of the draws, Beer-Lambert
and isotropy on the restatement, the composition with the phase and absorption steps on host-resident objects, the refusals, the
bindings, the header, the build table and the refusals of the library that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import _hip, build, light, tally
from scatter_layered_reference import (BAD_CALLS, C, CENTER, SEED, abi_args, assert_every_outcome, layout, planted, same_answer,
                                       scatter_layered_loop, tables)
from path_absorb_reference import R_PLANTS
from writer_reference import same_bits

ENTRIES = ("pcl_step_scatter_layered", "pcl_group_step_scatter_layered")
N = 600


def scene(n, dtype=np.float64):
    """The layout, who is a photon (every seventh a plain Object) and explicit ids that are not consecutive."""
    state = layout(n, dtype)
    state["photon"] = np.arange(n) % 7 != 3
    state["id"] = 7_000_000_001 + 3 * np.random.RandomState(5).permutation(n).astype(np.int64)
    return state


def sweep(fn, state, cfg, first, n_pass=1, dtype=np.float64, seed=SEED, ids=None):
    p, edges, E_edges = cfg
    return fn(state["r"], state["v"], state["dv"], state["E"], state["photon"], state["id"] if ids is None else ids, p, edges, CENTER, E_edges,
              first, C, seed, n_pass, dtype)


# ------------------------------------------------------------------------------------------------ the rule
SHAPES = [(L, B) for L in (0, 1, 3, 64) for B in (0, 1, 1024) if max(L, 1) * max(B, 1) <= 4096]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("L, B", SHAPES)
def test_the_restatement_is_the_loop_bit_for_bit(L, B, first, dtype):
    state = scene(N, dtype)
    for p in ("mixed", 0.0, 1.0) if (L, B) in ((3, 1024), (0, 0)) else ("mixed",):
        cfg = tables(L, B, p)
        ref, loop = (sweep(fn, state, cfg, first, 2, dtype) for fn in (light._scatter_layered, scatter_layered_loop))
        assert same_answer(ref, loop), p
        if p == "mixed":
            counts = assert_every_outcome(ref, state["v"], state["photon"], cfg[1], cfg[2], (L, B, first, dtype))
            print(L, B, first, dtype.__name__, counts)
        elif p == 0.0:
            assert ref["exposed"].any() and not ref["scattered"].any()
        else:
            assert ref["exposed"].any() and np.array_equal(ref["scattered"], ref["exposed"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_planted_slots_are_found_where_they_were_planted(dtype):
    state = scene(N, dtype)
    cfg = tables(3, 3)
    ref = sweep(light._scatter_layered, state, cfg, False, dtype=dtype)
    moving, _, want_band = planted(N)
    i = np.arange(N)
    want_layer = np.full(N, -2)                                        # three layers: 2.0 opens the second, 3.0 closes the third
    for mod, radius, _ in R_PLANTS:                                     # (a later line wins, as in the layout)
        want_layer[i % mod == 0] = {1.0: 0, 2.0: 1, 3.0: 2}.get(radius, -1)
    photon = state["photon"]
    go = moving & photon
    assert not ref["exposed"][~go].any() and (ref["layer"][~go] == -1).all()               # at rest, -0.0, plain Objects
    known = go & (want_layer != -2)
    assert known.sum() > 100 and np.array_equal(ref["layer"][known], want_layer[known])
    has = go & (ref["layer"] >= 0) & (want_band != -2)
    assert has.sum() > 100 and np.array_equal(ref["band"][has], want_band[has])
    assert go[i % 13 == 0].sum() > 10                                   # a NaN in v0 moves
    nan_v = go & (i % 13 == 0) & ref["scattered"]
    assert nan_v.any() and np.isnan(ref["dv"][nan_v]).any() and np.isfinite(ref["v"][nan_v]).all()       # v' is drawn, dv = v' - NaN


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_contracts_of_a_hit_and_of_the_two_misses(dtype):
    state = scene(N, dtype)
    cfg = tables(3, 3)
    photon = state["photon"]
    for first in (False, True):
        ref = sweep(light._scatter_layered, state, cfg, first, 3, dtype)
        hit = ref["scattered"]
        assert ref["scattered_by_cell"].sum() == hit.sum() <= ref["exposed"].sum() and 0 < hit.sum() < ref["exposed"].sum()
        assert not ref["scattered_by_cell"][cfg[0] == 0.0].any()
        for f in ("v", "dv"):                                          # plain Objects are untouched in either mode
            assert same_bits(ref[f][~photon], state[f][~photon]), f
        assert same_bits(ref["v"][~hit], state["v"][~hit])
        if first:                                                      # every photon that did not scatter: dv = 0, at rest or not
            assert np.array_equal(ref["written"], photon) and same_bits(ref["dv"][photon & ~hit], np.zeros(((photon & ~hit).sum(), 3)))
        else:                                                          # rows that are not scattered are the inputs' bits, dv included
            assert np.array_equal(ref["written"], hit) and same_bits(ref["dv"][~hit], state["dv"][~hit])
        ok = hit & np.isfinite(state["v"]).all(axis=1)
        speed = np.sqrt((ref["v"][ok] ** 2).sum(axis=1))
        eps = np.finfo(dtype).eps
        assert np.max(np.abs(speed / C - 1.0)) <= 8 * eps               # |v'| == c to rounding
        back = ref["v"][ok] - ref["dv"][ok]                            # v' - dv reproduces v_old to one rounding of a value up to 2c
        assert np.max(np.abs(back - state["v"][ok])) <= 2.0 * C * eps
        if dtype is np.float32:
            for f in ("v", "dv"):
                assert same_bits(ref[f][hit].astype(np.float32).astype(np.float64), ref[f][hit]), f
    a, b = (sweep(light._scatter_layered, state, cfg, first, 3, dtype) for first in (False, True))
    assert np.array_equal(a["scattered"], b["scattered"]) and same_bits(a["v"], b["v"])     # the mode changes the misses only


def test_the_draws_follow_the_id_the_pass_and_the_seed():
    state = scene(N)
    cfg = tables(3, 3)
    one = sweep(light._scatter_layered, state, cfg, True)
    for other in (sweep(light._scatter_layered, state, cfg, True, n_pass=2), sweep(light._scatter_layered, state, cfg, True, seed=SEED + 1),
                  sweep(light._scatter_layered, state, cfg, True, ids=state["id"] + 1)):
        assert np.array_equal(other["exposed"], one["exposed"]) and not np.array_equal(other["scattered"], one["scattered"])
    k = int(np.flatnonzero(one["scattered"] & (cfg[0][one["layer"], one["band"]] < 1.0))[0])
    assert light._philox_block([state["id"][k]], SEED, 1, 23)[0][0] < cfg[0][one["layer"][k], one["band"][k]]
    assert light._LAYERED_SCATTER_WORDS == (23, 24)
    u_a = light._philox_block([state["id"][k]], SEED, 1, 24)[0][0]
    assert abs(one["v"][k, 0] / C - (1.0 - 2.0 * u_a)) <= 4 * np.finfo(np.float64).eps      # about (1, 0, 0): the x component is c * mu


def test_the_other_steps_draw_what_they_drew():
    """With the same seed, the path absorption, the phase function and the re-emission give the same results behind a first=False pass
    with p = 0; and the words 23 and 24 stand nowhere else in csrc/."""
    state = scene(N)
    ids, photon = state["id"], state["photon"]
    clear = sweep(light._scatter_layered, state, tables(3, 3, 0.0), False, 1)
    assert same_bits(clear["v"], state["v"]) and same_bits(clear["dv"], state["dv"]) and not clear["written"].any()
    p, edges, E_edges = tables(3, 3)
    for v, dv in ((state["v"], state["dv"]), (clear["v"], clear["dv"])):
        a = light._absorb_path(state["r"], v, dv, state["E"], photon, ids, p, edges, CENTER, E_edges, SEED, 1)
        b = light._phase_redirect(v, dv, photon, ids, "hg", 0.85, C, SEED, 1)
        c = light._reemit_parked(state["r"], v, state["E"], photon, ids, 0.5, "isotropic", None, edges, CENTER, C, SEED, 1)
        got = [a["v"], a["dv"], a["absorbed"], b["v"], b["dv"], b["redirected"], c["v"], c["reemitted"]]
        if v is state["v"]:
            want = got
    assert all(same_bits(x, y) for x, y in zip(got, want)) and want[2].any() and want[5].any() and want[7].any()
    for f in sorted(os.listdir(build.CSRC)):
        if f.endswith((".hip", ".h", ".inc")):
            text = open(os.path.join(build.CSRC, f)).read()
            words = [int(w) for w in re.findall(r"pcl_philox4x32_10\([^;]*?, (\d+)u, ", text)]
            words += [int(w) for k, w in re.findall(r"\b(k[A-Z]\w+) = (\d+)", text) if not k.startswith("kLayeredScatter")]
            assert 23 not in words and 24 not in words, f


def test_the_counter_words_are_named_constants_used_once():
    src = open(os.path.join(build.CSRC, "pcl_surface.hip")).read()
    assert re.findall(r"\b(kLayeredScatter\w+) = (\d+)", src) == [("kLayeredScatterDraw", "23"), ("kLayeredScatterDir", "24")]
    for name in ("kLayeredScatterDraw", "kLayeredScatterDir"):
        assert len(re.findall(r"pcl_philox4x32_10\([^;]*?, %s, " % name, src)) == 1 and len(re.findall(r"\b%s\b" % name, src)) == 2
    body = src[src.index("void __launch_bounds__(kBlock) k_scatter_layered"):src.index("struct lscatter_spec")]
    assert sorted(re.findall(r"pcl_philox4x32_10\([^;]*?, (\w+), a\.k0", body)) == ["kLayeredScatterDir", "kLayeredScatterDraw"]
    assert "__dsub_rn(vk, vo)" in body and "flush_cells, written out" in body


# ------------------------------------------------------------------------------------------------ physics, on the restatement
@pytest.mark.parametrize("tau", [0.5, 2.0])
def test_beer_lambert_and_isotropy(tau):
    """2^16 photons in a beam along +x through one layer of thickness D with k*D = tau, c*dt = D/64, 64 passes of Newton and this step.
    The fraction never scattered is exp(-tau) within 5 standard deviations of the binomial, sqrt(q(1-q)/N); the mean of mu over all
    hits is 0 within 5/sqrt(3*hits) -- mu uniform on [-1, 1] has the variance 1/3.  Derived, not tuned."""
    n, D, passes = 1 << 16, 64.0, 64
    dt = (D / passes) / C
    p = light._path_probability(np.array([[tau / D]]), C, dt)
    assert p.shape == (1, 1) and p[0, 0] == -np.expm1(-(tau / D) * (C * dt))
    r = np.zeros((n, 3))
    v = np.tile([C, 0.0, 0.0], (n, 1))
    dv, ids, photon = np.zeros((n, 3)), np.arange(n), np.ones(n, dtype=bool)
    never = np.ones(n, dtype=bool)
    mu = []
    for k in range(1, passes + 1):
        r = r + v * dt                                                  # Newton; the layer holds every photon wherever it goes
        out = light._scatter_layered(r, v, dv, None, photon, ids, p, None, (0, 0, 0), None, True, C, SEED, k)
        assert out["exposed"].all()
        mu.append(out["v"][out["scattered"], 0] / C)
        never &= ~out["scattered"]
        v, dv = out["v"], out["dv"]
    q = np.exp(-tau)
    got, sigma = never.mean(), np.sqrt(q * (1.0 - q) / n)
    mu = np.concatenate(mu)
    print("tau %g: never scattered %.5f, exp(-tau) %.5f, %.2f sigma; mean mu %.5f over %d hits, bound %.5f"
          % (tau, got, q, (got - q) / sigma, mu.mean(), len(mu), 5.0 / np.sqrt(3.0 * len(mu))))
    assert abs(got - q) <= 5.0 * sigma
    assert abs(mu.mean()) <= 5.0 / np.sqrt(3.0 * len(mu))


# ------------------------------------------------------------------------------------------------ the step on the host
class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed = 0.25, SEED

    def __init__(self, objs, py=False, steps=None, dt=0.5 / C):
        self.objects, self.py, self.steps, self.dt = objs, py, steps or {}, np.double(dt)

    def _py_semantics(self):
        return self.py


def objects(state):
    out = []
    for k in range(len(state["photon"])):
        if state["photon"][k]:
            o = phys.light.PhotonObject(E=np.double(state["E"][k]), v=phys.light.c * [1, 0, 0])
        else:
            o = phys.Object()
        o.r = phys.Measurement(np.array(state["r"][k]), "m**1")
        o.v, o.dv = np.array(state["v"][k]), np.array(state["dv"][k])
        o.dr = phys.Measurement(np.array(state["dr"][k]), "m**1")
        out.append(o)
    return out


def make(first=None, **kw):
    k, edges, E_edges = tables(3, 3)
    return phys.light.LayeredScatterStep(k, edges, CENTER, E_edges, first=first, **kw)


def test_constructor_keeps_what_it_was_given():
    step = make(out_fn="rows.csv")
    k, edges, E_edges = tables(3, 3)
    assert step.k.tolist() == k.tolist() and step.edges.tolist() == edges.tolist() and step.E_edges.tolist() == E_edges.tolist()
    assert (step.first, step._pass, step.data, step.out_fn, step.exposed, step.scattered) == (None, 0, [], "rows.csv", 0, 0)
    assert step.scattered_by_cell.shape == (3, 3) and step.scattered_by_cell.dtype == np.int64 and step._writes == ("v", "dv")
    assert phys.light.LayeredScatterStep(0.5).k.shape == (1, 1) and make(first=True).first is True and make(first=False).first is False
    import phys.light as short
    assert short.LayeredScatterStep is light.LayeredScatterStep is phys.light.LayeredScatterStep
    cls = light.LayeredScatterStep
    assert issubclass(cls, tally.WriterStep) and cls.__mro__[1] is tally.WriterStep and not set(vars(cls)) & {"run", "_device_run", "_reduce"}
    assert "one launch per light step" in cls._NOTE and "LayeredScatterStep" in cls._NOTE and cls._NOTE != light.PathAbsorptionStep._NOTE
    for text in ("v - dv", "omega0", "two scatterings", "reads as a miss", "term cache"):
        assert text in cls.__doc__, text
    assert (_hip.SCATTER_LAYERED_MAX_LAYERS, _hip.SCATTER_LAYERED_MAX_BANDS, _hip.SCATTER_LAYERED_MAX_CELLS) == \
        (_hip.PATH_ABSORB_MAX_LAYERS, _hip.PATH_ABSORB_MAX_BANDS, _hip.PATH_ABSORB_MAX_CELLS) == (64, 1024, 4096)


@pytest.mark.parametrize("kw, word", [
    (dict(k="x"), "k must be a number"), (dict(k=[0.1, 0.2]), "k must have the shape"), (dict(k=-1.0), "finite and not negative"),
    (dict(k=np.nan), "finite and not negative"), (dict(k=[0.1, 0.2], edges=[1.0, 3.0, 2.0]), "edges"),
    (dict(k=[0.1, 0.2], edges=[-1.0, 2.0, 3.0]), "edges"), (dict(k=[0.1, 0.2], E_edges=[1.0, np.nan, 3.0]), "E_edges"),
    (dict(k=np.zeros(65), edges=np.arange(66.0)), "edges"), (dict(k=np.zeros(1025), E_edges=np.arange(1026.0)), "E_edges"),
    (dict(k=np.zeros((64, 65)), edges=np.arange(65.0), E_edges=np.arange(66.0)), "4160 cells"),
    (dict(k=0.5, center=[0, np.nan, 0]), "center"), (dict(k=0.5, first=1), "first must be None, True or False"),
    (dict(k=0.5, first="yes"), "first must be None, True or False")])
def test_constructor_refusals_are_the_path_absorption_s(kw, word):
    with pytest.raises(ValueError, match=word) as mine:
        phys.light.LayeredScatterStep(**kw)
    if "first" not in kw:                                              # the same check, the same message
        with pytest.raises(ValueError) as theirs:
            phys.light.PathAbsorptionStep(**kw)
        assert str(mine.value) == str(theirs.value)


@pytest.mark.parametrize("py", [False, True])
def test_host_resident_objects_get_the_restatement_s_state(tmp_path, py):
    state = scene(400)
    objs = objects(state)
    n = len(objs)
    E0, photon = tally.photon_energies(objs, phys.light.PhotonObject)
    r0, v0, dr0, dv0 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    step = make(out_fn=str(tmp_path / "cloud.csv"))
    sim = HostSim(objs, py=py, steps={0: phys.newton.NewtonianKinematicsStep(), 1: step})
    step.run(sim)                                                      # first resolves to True: works under cl_on=False as well
    assert step.first is True and step._pass == 1
    k, edges, E_edges = tables(3, 3)
    c_code = light._c_h_literals()[0]
    p = light._path_probability(k, c_code, sim.dt)
    ref = light._scatter_layered(r0, v0, dv0, E0, photon, np.arange(n), p, edges, CENTER, E_edges, True, c_code, SEED, 1)
    assert_every_outcome(ref, v0, photon, edges, E_edges, "host")
    assert (step.exposed, step.scattered) == (int(ref["exposed"].sum()), int(ref["scattered"].sum())) and step.scattered > 0
    assert step.scattered_by_cell.tolist() == ref["scattered_by_cell"].tolist()
    row = list(step.data[0])
    assert row[:3] == [0.25, step.exposed, step.scattered] and row[3].tolist() == ref["scattered_by_cell"].tolist() and sim.launch_note is None
    r1, v1, dr1, dv1 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    assert same_bits(r1, r0) and same_bits(dr1, dr0) and same_bits(v1, ref["v"]) and same_bits(dv1, ref["dv"])
    assert same_bits(tally.photon_energies(objs, phys.light.PhotonObject)[0], E0)
    step.run(sim)
    step.terminate(sim)
    lines = open(str(tmp_path / "cloud.csv")).read().splitlines()
    assert step._pass == 2 and len(lines) == 2 and lines[0].startswith("0.25, %d, %d, [[" % (ref["exposed"].sum(), ref["scattered"].sum()))


def test_first_is_resolved_from_the_step_order():
    scat = phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0))
    for front, want in (([], True), ([phys.newton.NewtonianKinematicsStep()], True), ([scat], False),
                        ([phys.light.ScatterSphericalStep(1, 1)], False), ([make(first=True)], False),
                        ([phys.light.PathAbsorptionStep(0.5)], True)):
        step = make()
        sim = HostSim(objects(scene(64)), steps=dict(enumerate(front + [step, phys.light.PhaseFunctionStep("hg", 0.85)])))
        step.run(sim)
        assert step.first is want and step._pass == 1, front
    given = make(first=True)                                            # what was given stays
    given.run(HostSim(objects(scene(64)), steps={0: scat, 1: given}))
    assert given.first is True


def test_refusals_come_before_the_pass_moves():
    scat = phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0))
    step = make()
    with pytest.raises(ValueError, match="ScatterIsotropicStep behind this LayeredScatterStep"):
        step.run(HostSim(objects(scene(64)), steps={0: step, 1: scat}))
    assert step._pass == 0 and step.data == [] and step.first is None
    step = make()
    with pytest.raises(ValueError, match="ScatterSphericalStep.*LayeredScatterStep"):
        step.run(HostSim(objects(scene(64)), steps={0: step, 1: phys.light.ScatterSphericalStep(1, 1)}))
    for step, steps in ((make(first=False), {}), (make(), {0: scat})):     # first=False, given or resolved, under cl_on=False
        steps[5] = step
        with pytest.raises(ValueError, match=r"LayeredScatterStep\(first=False\) needs cl_on=True.*dv = v_old") as e:
            step.run(HostSim(objects(scene(64)), py=True, steps=steps))
        assert step._pass == 0 and step.data == []
        assert "cannot be read off the store" in str(e.value)           # _dv_rule_refusal's wording

        class Sim(HostSim):                                            # the device path refuses as well, before the sweep
            _residency = "device"
        with pytest.raises(ValueError, match="needs cl_on=True"):
            step._device_run(Sim([], py=True, steps=steps))
        assert step._pass == 0
    step = make()
    with pytest.raises(ValueError, match="dt must be finite"):
        step.run(HostSim(objects(scene(64)), steps={0: step}, dt=-1.0))
    assert step._pass == 0 and step.data == []


def test_a_real_simulation_resolves_and_refuses_on_the_host_path():
    """``_refuse`` reads ``Simulation.steps`` itself, not a stand-in's: host-resident objects, no device."""
    def sim_of(*steps):
        sim = phys.Simulation(cl_on=False, seed=SEED)
        sim.add_objs(objects(scene(64)))
        sim.dt = np.double(0.5 / C)
        for k, s in enumerate(steps):
            sim.add_step(k, s)
        return sim
    scat = phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0))
    step = make()
    with pytest.raises(ValueError, match="behind this LayeredScatterStep"):
        step.run(sim_of(step, scat))
    step = make()
    with pytest.raises(ValueError, match="needs cl_on=True"):
        step.run(sim_of(scat, step))                                    # resolved to False under cl_on=False
    assert step._pass == 0
    step = make()
    step.run(sim_of(phys.newton.NewtonianKinematicsStep(), step))
    assert step.first is True and step._pass == 1 and step.exposed > 0


def test_composition_with_a_phase_function_and_an_absorber():
    """Newton -> LayeredScatterStep -> PhaseFunctionStep("hg", 0.85) -> AbsorptionStep(0.5) on host-resident objects: the phase step
    re-directs exactly the hits, the absorber sees exactly them."""
    n = 512
    rng = np.random.RandomState(11)
    u = rng.normal(size=(n, 3))
    state = dict(r=CENTER + rng.uniform(1.1, 2.9, size=n)[:, None] * u / np.sqrt((u * u).sum(axis=1))[:, None],
                 v=np.tile([C, 0.0, 0.0], (n, 1)), dr=np.zeros((n, 3)), dv=rng.normal(size=(n, 3)), E=rng.uniform(1.1, 2.9, size=n),
                 photon=np.arange(n) % 9 != 4)
    objs = objects(state)
    cloud = phys.light.LayeredScatterStep([0.0, 1.5, 0.7], [1.0, 2.0, 2.5, 3.0], CENTER)
    phase, medium = phys.light.PhaseFunctionStep("hg", 0.85), phys.light.AbsorptionStep(0.5)
    sim = HostSim(objs, steps={0: phys.newton.NewtonianKinematicsStep(), 1: cloud, 2: phase, 3: medium})
    v0 = tally.vec3(objs, "v")
    for s in (cloud, phase, medium):
        s.run(sim)
    assert cloud.first is True and 0 < cloud.scattered < cloud.exposed and cloud.scattered_by_cell[0, 0] == 0
    assert phase.redirected == cloud.scattered and medium.interacted == cloud.scattered and 0 < medium.absorbed < medium.interacted
    v1, dv1 = tally.vec3(objs, "v"), tally.vec3(objs, "dv")
    kept = dv1.any(axis=1) & state["photon"]                           # scattered and not absorbed: turned about the OLD direction, +x
    assert kept.sum() == cloud.scattered - medium.absorbed
    assert np.max(np.abs((v1[kept] - dv1[kept]) - v0[kept])) <= 4.0 * C * np.finfo(np.float64).eps
    assert (v1[kept, 0] / C).mean() > 0.7                              # the forward peak: <mu> = g = 0.85


def test_device_run_notes_the_launch_schedule_and_reduces_the_row():
    class Dev:
        count, calls = 1000, []

        def scatter_layered(self, *a):
            self.calls.append(a)
            return 9, 4, np.array([[1, 0, 1], [0, 2, 0], [0, 0, 0]])

    class Sim:
        t, seed, launch_note, _dev, _scattered, chunks = 0.5, 99, None, Dev(), False, []

        def __init__(self):
            self.steps = {}

        def _k_wanted(self):
            return 32

        def _py_semantics(self):
            return False

        def _dt_code(self):
            return 0.5 / light._c_h_literals()[0]

        def _global(self, values):
            self.chunks.append(len(values))
            return np.asarray(values, dtype=np.int64) * 2               # two ranks with the same tallies
    sim = Sim()
    step = make()
    sim.steps = {0: phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)), 1: step}
    step._device_run(sim)
    step._device_run(sim)
    assert sim.launch_note == step._NOTE and sim._scattered and step.first is False
    assert (step.exposed, step.scattered) == (18, 8) and step.scattered_by_cell.tolist() == [[2, 0, 2], [0, 4, 0], [0, 0, 0]]
    row = list(step.data[1])
    assert len(step.data) == 2 and row[:3] == [0.5, 18, 8] and row[3].tolist() == step.scattered_by_cell.tolist()
    assert sim.chunks == [1 + 2 + 9] * 2                                # one collective per pass
    a, b = Dev.calls
    k, edges, E_edges = tables(3, 3)
    assert same_bits(a[0], -np.expm1(-(k * 0.5))) and a[1].tolist() == edges.tolist() and a[2].tolist() == CENTER.tolist()
    assert a[3].tolist() == E_edges.tolist() and a[4] is False and a[5] == light._c_h_literals()[0] and (a[6], a[7], b[7]) == (99, 1, 2)


def test_multi_device_sums_the_shards_tallies():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def scatter_layered(self, *a, **kw):
            return 3 * self.k, self.k, self.k * np.array([[1, 2], [3, 4]])
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    exposed, scattered, cells = md.scatter_layered([[0.5, 0.5], [0.5, 0.5]], [1.0, 2.0, 3.0], None, [1.0, 2.0, 3.0], True, C, 1, 1)
    md._pool.shutdown()
    assert (int(exposed), int(scattered)) == (333, 111) and np.asarray(cells).tolist() == [[111, 222], [333, 444]]


def test_binding_marshals_the_call():
    def entry(handle, L, B, p, ed, ce, Ee, first, c, seed, n_pass, counts, cells):
        arr = lambda q, k: None if q is None else np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_double)), (k,)).tolist()   # noqa: E731
        rows, cols = max(L, 1), max(B, 1)
        seen.append((handle, L, B, arr(p, rows * cols), arr(ed, L + 1), arr(ce, 3), arr(Ee, B + 1), first, c, seed, n_pass))
        np.ctypeslib.as_array(ctypes.cast(counts, ctypes.POINTER(ctypes.c_int64)), (2,))[:] = [100, 50]
        np.ctypeslib.as_array(ctypes.cast(cells, ctypes.POINTER(ctypes.c_int64)), (rows * cols,))[:] = np.arange(rows * cols)
        return 0
    seen = []
    exposed, scattered, cells = _hip._scatter_layered(entry, "h", [[0.5, 0.25], [0.0, 1.0]], [1.0, 2.0, 3.0], CENTER, [1.0, 1.5, 3.0], False, C, -1,
                                                      2 ** 32 + 3)
    assert (exposed, scattered) == (100, 50) and cells.tolist() == [[0, 1], [2, 3]] and cells.dtype == np.int64
    assert seen[0] == ("h", 2, 2, [0.5, 0.25, 0.0, 1.0], [1.0, 2.0, 3.0], CENTER.tolist(), [1.0, 1.5, 3.0], 0, C, 2 ** 64 - 1, 3)
    _hip._scatter_layered(entry, "h", 0.5, None, None, None, True, C, 1, 1)
    assert seen[1][1:8] == (0, 0, [0.5], None, None, None, 1)
    with pytest.raises(ValueError, match="p holds"):
        _hip._scatter_layered(entry, "h", [0.5, 0.5, 0.5], [1.0, 2.0, 3.0], None, None, True, C, 1, 1)
    assert len(_hip._PROTOTYPES[ENTRIES[0]]) == len(_hip._PROTOTYPES[ENTRIES[1]]) == 13


# ------------------------------------------------------------------------------------------------ the library
def surface_unit():
    (unit,) = [u for u in build.ADDONS if os.path.basename(u["src"]) == "pcl_surface.hip"]
    return unit


def test_header_prototypes_and_the_build_table():
    text = open(build.ABI_HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and len(_hip._PROTOTYPES[entry]) == 13
    for name, value in (("LAYERS", 64), ("BANDS", 1024), ("CELLS", 4096)):
        assert re.search(r"#define PCL_SCATTER_LAYERED_MAX_%s %d\b" % (name, value), code)
        assert re.search(r"#define PCL_PATH_ABSORB_MAX_%s %d\b" % (name, value), code)
    flat = " ".join(text.split()).replace("* ", "")
    assert "words 23 and 24 are used by nothing else" in flat and "0-5 and 8-22 are taken" in flat
    for line in ("(id_lo, id_hi, pass, 23)", "(id_lo, id_hi, pass, 24)", "scattered iff u < p", "w = (1, 0, 0); mu = 1 - 2*u_a",
                 "v_k = c direction_k; dv_k = v_k - v_old_k", "first == 0: the particle is not written at all",
                 "first == 1: dv = 0 for every photon that is not scattered", "the last one closed", "p = -expm1(-k (c*dt))",
                 "16 KiB", "32 KiB", "below 64 KiB of LDS", "first that is neither 0 nor 1", "turns its hits about v - dv"):
        assert line in flat, line                                      # the order is written out
    assert hasattr(_hip.Device, "scatter_layered") and hasattr(_hip.DeviceGroup, "scatter_layered")
    from physicl_amd.multidev import MultiDevice
    assert hasattr(MultiDevice, "scatter_layered")
    # the table: the unit of the writer sweeps holds this one, described as every sweep is (tests/test_build_cpu.py checks it as one)
    assert dict(entries=ENTRIES, kernel="k_scatter_layered", count=2) in surface_unit()["sweeps"]


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context and a NULL group, refused as well); the outputs stay as
    they were."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in BAD_CALLS:
        keep, args, (counts, cells) = abi_args(**kw)
        assert lib.pcl_step_scatter_layered(None, *args) == -2, kw
        assert lib.pcl_group_step_scatter_layered(None, *args) == -2, kw
        assert (counts is None or (counts == -7).all()) and (cells is None or (cells == -7).all()), kw
    keep, args, (counts, cells) = abi_args()                           # a good call without a context is refused, too
    assert lib.pcl_step_scatter_layered(None, *args) == -2 and lib.pcl_group_step_scatter_layered(None, *args) != 0
    assert (counts == -7).all() and (cells == -7).all()
