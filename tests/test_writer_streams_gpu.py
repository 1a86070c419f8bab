"""GPU: the Philox streams of the writer sweeps (tests/test_writer_streams_cpu.py holds the block and the counter rule).

* Full-width keys.  The ten writer sweeps that draw, and ``apply_source``, through their ``Device`` calls with seeds that use the
  upper half of the key and pass counters that use the top bit of their word, fp64 and fp32, N = 2049 (one tile and a ragged wave):
  each on its own reference file's scene in the configuration where every outcome is present, against its numpy restatement by the
  ``check_*`` function of that file -- counts exact, the bounds those functions hold.  For every sweep the restatement's decisions
  under ``seed`` and ``seed + 2**32`` differ, and under ``n_pass`` and ``n_pass + 2**31``: the two sides cannot ignore the bits
  together.
* Pairs.  Two steps of one kind in one pass through ``Simulation``: probes in front of, between and behind them; every run of either
  step replays from the probed state in front of it with its ``check_*`` and its own ``_n_pass``; summed over the passes, the
  binomial and the direction bounds of the CPU file (five standard deviations of the law, nothing measured).  Three gases; one pair
  over two contexts on one GPU.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
import absorb_reference as A
import layered_phase_reference as LP
import path_absorb_reference as PA
import phase_reference as PH
import recycle_reference as RC
import reemit_reference as RE
import refract_reference as RF
import scatter_layered_reference as SL
import spectral_surface_reference as SP
import surface_reference as SU
import writer_reference as W
from physicl_amd import light

pytestmark = pytest.mark.gpu

C = W.C
ID_BASE = W.ID_BASE
N = 2049
WIDE = [(2**64 - 1, 2**32 - 1), (2**32, 2**31), (0x5EED5A7F + (0xC0FFEE << 40), 2**31 - 1)]
FIELDS = ("r", "v", "dr", "dv")


@pytest.fixture(scope="module")
def dev():
    from physicl_amd import _hip
    d = _hip.Device(0)
    yield d
    d.close()


def np_type(dtype):
    return np.float32 if dtype == "f32" else np.float64


def put(dev, dtype, state):
    up = {f: state[f] for f in FIELDS + ("E",)}
    up["id_base"] = ID_BASE
    dev.store_alloc(len(state["E"]), dtype)
    dev.upload_state(up)
    return W.snapshot(dev)


# Each sweep: ``scene(T)`` -- r, v, dr, dv, E of its reference file's scene --, ``run(dev, before, seed, n_pass, what)`` -- the Device
# call and the reference file's check, which returns the restatement's dict --, ``again(b, before, T, seed, n_pass)`` -- the
# restatement alone on the widened state -- and the key of its dict that holds what the draws decide.
def _rng_rows(n, seed=3):
    rng = np.random.RandomState(seed)
    return rng.normal(size=(n, 3)), 1.0 + rng.uniform(size=n) * 2.0


def scene_surface(T):
    r, dr, v = SU.cloud(N, seed=1 + N, dtype=T)
    dv, E = _rng_rows(N)
    return dict(r=r, v=v, dr=dr, dv=dv, E=E)


def scene_phase(T):
    v, dv = PH.cloud(N, seed=1 + N, dtype=T)
    rows, E = _rng_rows(N)
    return dict(r=rows, v=v, dr=rows[::-1].copy(), dv=dv, E=E)


def scene_absorb(T):
    s = A.cloud(N, seed=1, dtype=T)
    return dict(r=s["r"], v=s["v"], dr=_rng_rows(N)[0], dv=s["dv"], E=s["E"])


def scene_layered(T):
    r, v, dv = LP.cloud(N, seed=1 + N, dtype=T)
    dr, E = _rng_rows(N)
    return dict(r=r, v=v, dr=dr, dv=dv, E=E)


GLASS = RF.GLASS
GROUND = SP.config(3)
MIX = LP.cases()["mixture"]
LAMP = RC.source("cone", "disc")
CLOUD_P, CLOUD_EDGES, CLOUD_E_EDGES = SL.tables(3, 3)
OMEGA0 = (0.5, 1.0, 0.2)

def _surface_run(d, b, s, n, what):
    counts = d.surface_reflect(SU.RADIUS, SU.CENTER, 0.5, "lambertian", C, s, n)
    return W.check_surface(b, W.snapshot(d), counts, SU.RADIUS, SU.CENTER, 0.5, "lambertian", C, s, n, SP.W_MAX, what)


def _phase_run(d, b, s, n, what):
    count = d.phase_redirect("hg", 0.85, C, s, n)
    return W.check_phase(b, W.snapshot(d), count, "hg", 0.85, C, s, n, what)


def _absorb_run(d, b, s, n, what):
    answer = d.absorb_scattered(OMEGA0, A.EDGES, A.CENTER, A.E_BINS, s, n)
    return W.check_absorb(b, W.snapshot(d), answer, OMEGA0, A.EDGES, A.CENTER, A.E_BINS, s, n, what)


def _layered_run(d, b, s, n, what):
    laws, weights, edges = MIX
    checked, _, cum, edges_c, center = light._check_layered_phase(laws, weights, edges, A.CENTER)
    answer = d.phase_layered(checked, cum, edges_c, center, C, s, n)
    return LP.check_layered(b, W.snapshot(d), answer, laws, weights, edges, A.CENTER, C, s, n, what)


def _recycle_run(d, b, s, n, what):
    counts = d.recycle_spent(LAMP, C, True, RC.TOP, RC.CENTER, (RC.GRID, RC.CDF), s, n)
    return RC.check_recycle(b, W.snapshot(d), counts, LAMP, RC.TOP, RC.CENTER, True, (RC.GRID, RC.CDF), s, n, what)


def _path_run(d, b, s, n, what):
    answer = d.absorb_path(PA.P_CELLS, PA.EDGES, PA.CENTER, PA.E_EDGES, s, n)
    return PA.check_path_absorb(b, W.snapshot(d), answer, PA.P_CELLS, PA.EDGES, PA.CENTER, PA.E_EDGES, s, n, what)


def _reemit_run(d, b, s, n, what):
    cfg = RE.LAYERED
    answer = d.reemit_parked(C, cfg["eta"], cfg["angular"], cfg["tables"], cfg["edges"], cfg["center"], s, n)
    return RE.check_reemit(b, W.snapshot(d), answer, cfg, s, n, what)


def _refract_run(d, b, s, n, what):
    counts = d.refract_surface(GLASS["radius"], GLASS["n_inside"], GLASS["n_outside"], GLASS["center"], GLASS["fresnel"], C, s, n)
    return RF.check_refract(b, W.snapshot(d), counts, GLASS, s, n, what)


def _spectral_run(d, b, s, n, what):
    answer = d.ground_spectral(GROUND["radius"], GROUND["E_edges"], GROUND["albedo"], GROUND["specular"], GROUND["center"], C, s, n)
    return SP.check_spectral(b, W.snapshot(d), answer, GROUND, s, n, what)


def _cloud_run(d, b, s, n, what):
    answer = d.scatter_layered(CLOUD_P, CLOUD_EDGES, SL.CENTER, CLOUD_E_EDGES, True, C, s, n)
    return SL.check_scatter_layered(b, W.snapshot(d), answer, CLOUD_P, CLOUD_EDGES, SL.CENTER, CLOUD_E_EDGES, True, C, s, n, what)


def _E(b):
    return np.asarray(b["E"]).astype(np.float64)


SWEEPS = {
    "surface": (scene_surface, _surface_run, "reflected",
                lambda w, b, T, s, n: light._surface_bounce(w["r"], w["dr"], w["v"], W.photons(b), b["id"], SU.RADIUS, SU.CENTER, 0.5, "lambertian", C, s, n, T)),
    "phase": (scene_phase, _phase_run, "v",
              lambda w, b, T, s, n: light._phase_redirect(w["v"], w["dv"], W.photons(b), b["id"], "hg", 0.85, C, s, n, T)),
    "absorb": (scene_absorb, _absorb_run, "absorbed",
               lambda w, b, T, s, n: light._absorb_scattered(w["r"], w["v"], w["dv"], _E(b), W.photons(b), b["id"], OMEGA0, A.EDGES, A.CENTER, A.E_BINS, s, n, T)),
    "layered phase": (scene_layered, _layered_run, "v",
                      lambda w, b, T, s, n: light._layered_phase_redirect(w["r"], w["v"], w["dv"], W.photons(b), b["id"], MIX[0], MIX[1], MIX[2], A.CENTER, C, s, n, T)),
    "recycle": (lambda T: RC.layout(N, T), _recycle_run, "v",
                lambda w, b, T, s, n: light._recycle_spent(w["r"], w["v"], _E(b), W.photons(b), b["id"], LAMP, RC.TOP, RC.CENTER, True, (RC.GRID, RC.CDF), C, s, n, T)),
    "path absorb": (lambda T: PA.layout(N, T), _path_run, "absorbed",
                    lambda w, b, T, s, n: light._absorb_path(w["r"], w["v"], w["dv"], _E(b), W.photons(b), b["id"], PA.P_CELLS, PA.EDGES, PA.CENTER, PA.E_EDGES, s, n, T)),
    "reemit": (lambda T: RE.scene(N, T), _reemit_run, "reemitted",
               lambda w, b, T, s, n: light._reemit_parked(w["r"], w["v"], _E(b), W.photons(b), b["id"], RE.ETA, RE.ANGULAR, RE.TABLES, RE.EDGES, RE.CENTER, C, s, n, T)),
    "refract": (lambda T: dict(RF.scene(N, T, nan_v=False), E=np.ones(N)), _refract_run, "v",
                lambda w, b, T, s, n: light._refract_surface(w["r"], w["dr"], w["v"], W.photons(b), b["id"], GLASS["radius"], GLASS["center"], GLASS["n_inside"],
                                                             GLASS["n_outside"], GLASS["fresnel"], C, s, n, T)),
    "spectral ground": (lambda T: SP.scene(N, T), _spectral_run, "reflected",
                        lambda w, b, T, s, n: light._spectral_bounce(w["r"], w["dr"], w["v"], _E(b), W.photons(b), b["id"], GROUND["radius"], GROUND["center"],
                                                                     GROUND["albedo"], GROUND["specular"], GROUND["E_edges"], C, s, n, T)),
    "layered scatter": (lambda T: SL.layout(N, T), _cloud_run, "scattered",
                        lambda w, b, T, s, n: light._scatter_layered(w["r"], w["v"], w["dv"], _E(b), W.photons(b), b["id"], CLOUD_P, CLOUD_EDGES, SL.CENTER,
                                                                     CLOUD_E_EDGES, True, C, s, n, T)),
}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SWEEPS))
def test_a_sweep_at_full_width_keys_and_pass_counters(dev, name, dtype):
    scene, run, key, again = SWEEPS[name]
    T = np_type(dtype)
    state = scene(T)
    for seed, n_pass in WIDE:
        before = put(dev, dtype, state)
        ref = run(dev, before, seed, n_pass, "%s %s seed %#x pass %#x" % (name, dtype, seed, n_pass))
        decided = np.asarray(ref[key])
        assert decided.any() and (decided.dtype != bool or not decided.all()), (name, key)      # the draws had something to decide
        w = W.wide(before)
        base = np.asarray(again(w, before, T, seed, n_pass)[key])
        assert W.same_bits(base, decided)
        hi_key = np.asarray(again(w, before, T, (seed + 2**32) % 2**64, n_pass)[key])
        hi_pass = np.asarray(again(w, before, T, seed, (n_pass + 2**31) % 2**32)[key])
        assert not W.same_bits(hi_key, base) and not W.same_bits(hi_pass, base) and not W.same_bits(hi_key, hi_pass), (name, seed, n_pass)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_source_at_full_width_keys(dev, dtype, monkeypatch):
    """``apply_source`` takes a seed and no pass: test_gpu_source's check, which reads that module's seed, under the three seeds."""
    import test_gpu_source as S
    from source_reference import source_state
    src = light.PhotonSource(origin=S.GEOMETRY["oblique_far"][0], direction=S.GEOMETRY["oblique_far"][1], angular="cone", half_angle=0.3,
                             spatial="gaussian", radius=S.GEOMETRY["oblique_far"][2])
    ids = np.arange(N, dtype=np.uint64) + np.uint64(ID_BASE)
    for seed, _ in WIDE:
        dev.store_alloc(N, dtype)
        dev.fill_photons(N, ID_BASE, C, 1.0, 3.0, seed)
        dev.apply_source(src, C, seed)
        monkeypatch.setattr(S, "SEED", seed)
        S.check_source(dev, src, ID_BASE, "cone", "gaussian", "oblique_far", dtype)
        base, other = source_state(src, ids, seed, C), source_state(src, ids, (seed + 2**32) % 2**64, C)
        assert not (base["v"] == other["v"]).all(axis=1).any() and not (base["r"] == other["r"]).all(axis=1).any()


# ------------------------------------------------------------------------------------------------ pairs through Simulation
N_SIM, PASSES = 16385, 6
STEP = 0.25
DT = STEP / C
STATE = ("r", "v", "dr", "dv", "E", "id")
K_HALF, K_QUARTER = -np.log(0.5) / STEP, -np.log(0.25) / STEP          # p = 0.5 and p = 0.75 per move
ORIGIN = (0.0, 0.0, 0.0)


class Look(phys.DeviceStep):
    """The store as it stands, pass by pass (tests/test_gpu_writer_atmosphere_pass.py's probe)."""
    _fuse_role = None

    def __init__(self):
        self.states = []

    def _device_run(self, sim):
        self.states.append({f: sim.download(f) for f in STATE})


class Run:
    pass


def simulate(steps, devices=None, seed=7, front=()):
    """``steps`` behind a time step, a Newton step and ``front`` (a scatter step, right behind Newton), a probe in front of each of them
    and one behind the last."""
    sim = phys.Simulation(cl_on=True, rng="philox", seed=seed, devices=devices, exit=lambda s: len(s.ts) >= PASSES)
    src = phys.light.PhotonSource(origin=ORIGIN, direction=(1, -2, 0.5), angular="isotropic", spatial="disc", radius=3.0)
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=seed, source=src))
    run = Run()
    run.steps, run.looks = steps, [Look() for _ in range(len(steps) + 1)]
    order = [phys.UpdateTimeStep(lambda s: np.double(DT)), phys.newton.NewtonianKinematicsStep()] + list(front)
    for look, step in zip(run.looks, steps):
        order += [look, step]
    order.append(run.looks[-1])
    for k, s in enumerate(order):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    run.final = {f: sim.download(f) for f in STATE}
    run.seed, run.note = sim.seed, sim.launch_note
    sim.close(download=False)
    assert all(len(look.states) == PASSES for look in run.looks) and all(s._pass == PASSES == len(s.data) for s in steps)
    assert "one launch per light step" in run.note
    return run


def five_sigma(n, p):
    return 5.0 * np.sqrt(n * p * (1.0 - p))


def moving(state):
    return np.asarray(state["v"]).any(axis=1)


def check_binomial(what, n, k, p):
    print("%s: n = %d, k = %d, n p = %.1f, bound %.1f" % (what, n, k, n * p, five_sigma(n, p)))
    assert n > N_SIM // 8 and abs(k - n * p) <= five_sigma(n, p), what


def check_directions(what, pairs):
    """``pairs``: per pass (v of the first hit, v of the second) of the photons both steps hit."""
    v1, v2 = (np.concatenate([p[k] for p in pairs]) for k in (0, 1))
    n = len(v1)
    corr, bound = float(np.mean((v1[:, 0] / C) * (v2[:, 0] / C))), 5.0 / (3.0 * np.sqrt(n))
    print("%s: hit by both %d, mean(mu1 mu2) = %.4f (bound %.4f)" % (what, n, corr, bound))
    assert n > N_SIM // 8 and not (v1 == v2).all(axis=1).any() and abs(corr) <= bound, what


def gases(members):
    """Overlapping layers about the source, bands that differ and overlap; p = 0.5 in every cell of the first, 0.75 in the others."""
    tables = [((2, 2), [0.0, 1.2, 2.6], [1.0, 2.0, 2.6]), ((2, 2), [0.6, 2.0, 3.4], [1.4, 2.2, 3.0]), ((1, 2), [0.3, 3.2], [1.2, 2.0, 2.8])]
    return [phys.light.PathAbsorptionStep(np.full(shape, K_HALF if j == 0 else K_QUARTER), edges, ORIGIN, E_edges)
            for j, (shape, edges, E_edges) in enumerate(tables[:members])]


def check_gases(run):
    members = len(run.steps)
    assert [s._family for s in run.steps] == [(members, j) for j in range(members)]
    n = [0] * members
    k = [0] * members
    for p in range(PASSES):
        exposed_before = np.zeros(0, dtype=bool)
        for j, gas in enumerate(run.steps):
            before, after = run.looks[j].states[p], run.looks[j + 1].states[p]
            n_pass = p * members + j + 1
            prob = light._path_probability(gas.k, light._c_h_literals()[0], DT)
            row = gas.data[p]
            ref = PA.check_path_absorb(before, after, (row[1], row[2], row[3]), prob, gas.edges, gas.center, gas.E_edges, run.seed, n_pass,
                                       "gas %d pass %d" % (j + 1, p + 1))
            if j == 0:
                exposed_before = ref["exposed"]
            else:                                                      # exposed to this gas and to one in front of it, which missed
                both = ref["exposed"] & exposed_before
                n[j], k[j] = n[j] + int(both.sum()), k[j] + int(ref["absorbed"][both].sum())
                exposed_before = exposed_before | ref["exposed"]
            if j == 0:
                n[0], k[0] = n[0] + int(ref["exposed"].sum()), k[0] + int(ref["absorbed"].sum())
    check_binomial("gas 1", n[0], k[0], 0.5)
    for j in range(1, members):
        check_binomial("gas %d, exposed to a gas in front of it too" % (j + 1), n[j], k[j], 0.75)


@pytest.fixture(scope="module")
def two_gases():
    return simulate(gases(2))


def test_two_gases_in_one_pass(two_gases):
    check_gases(two_gases)


def test_three_gases_in_one_pass():
    check_gases(simulate(gases(3)))


def test_two_gases_over_two_contexts_give_the_unsharded_run(two_gases):
    both = simulate(gases(2), devices=[0, 0])
    for mine, theirs in zip(both.steps, two_gases.steps):
        assert [[np.asarray(x).tolist() for x in row] for row in mine.data] == [[np.asarray(x).tolist() for x in row] for row in theirs.data]
        assert mine._n_pass == theirs._n_pass and mine._family == theirs._family
    got, want = (np.argsort(r.final["id"], kind="stable") for r in (both, two_gases))
    for f in STATE:
        assert W.same_bits(both.final[f][got], two_gases.final[f][want]), f


def test_two_absorbers_in_one_pass():
    """Behind a scatter step that hits about half: omega0 = 0.5, then 0.25 (absorbed with 1 - omega0)."""
    a, b = phys.light.AbsorptionStep(0.5), phys.light.AbsorptionStep(0.25)
    run = simulate([a, b], front=[phys.light.ScatterIsotropicStep(A=np.double(0.5 / STEP), n=np.double(1.0))])   # A*n*|dr| = 0.5
    n, k = [0, 0], [0, 0]
    for p in range(PASSES):
        for j, (step, omega0) in enumerate(((a, 0.5), (b, 0.25))):
            before, after = run.looks[j].states[p], run.looks[j + 1].states[p]
            row = step.data[p]
            ref = W.check_absorb(before, after, (row[1], row[2], row[3], None), (omega0,), None, step.center, None, run.seed, 2 * p + j + 1,
                                 "absorber %d pass %d" % (j + 1, p + 1))
            n[j], k[j] = n[j] + int(ref["interacted"].sum()), k[j] + int(ref["absorbed"].sum())
    check_binomial("absorber 1", n[0], k[0], 0.5)
    check_binomial("absorber 2, those the first let go on", n[1], k[1], 0.75)


def test_two_clouds_in_one_pass():
    a, b = phys.light.LayeredScatterStep(K_HALF), phys.light.LayeredScatterStep(K_HALF)
    run = simulate([a, b])
    assert (a.first, b.first) == (True, False)
    n, k, pairs = [0, 0, 0], [0, 0, 0], []
    for p in range(PASSES):
        refs = []
        for j, (step, first) in enumerate(((a, True), (b, False))):
            before, after = run.looks[j].states[p], run.looks[j + 1].states[p]
            row = step.data[p]
            prob = light._path_probability(step.k, light._c_h_literals()[0], DT)
            refs.append(SL.check_scatter_layered(before, after, (row[1], row[2], row[3]), prob, None, step.center, None, first, light._c_h_literals()[0],
                                                 run.seed, 2 * p + j + 1, "cloud %d pass %d" % (j + 1, p + 1)))
        hit1, hit2 = refs[0]["scattered"], refs[1]["scattered"]
        assert refs[0]["exposed"].all() and refs[1]["exposed"].all()
        for j, (who, hit) in enumerate(((np.ones(N_SIM, bool), hit1), (~hit1, hit2), (hit1, hit2))):
            n[j], k[j] = n[j] + int(who.sum()), k[j] + int(hit[who].sum())
        both = hit1 & hit2
        pairs.append((run.looks[1].states[p]["v"][both], run.looks[2].states[p]["v"][both]))
    check_binomial("cloud 1", n[0], k[0], 0.5)
    check_binomial("cloud 2, whom cloud 1 missed", n[1], k[1], 0.5)
    check_binomial("cloud 2, whom cloud 1 hit", n[2], k[2], 0.5)
    check_directions("clouds", pairs)


def test_two_reemitters_in_one_pass():
    """Everybody parked in front of either: a black gas (p == 1) behind each re-emitter parks everybody again."""
    a, b = phys.light.ReemissionStep(eta=0.5), phys.light.ReemissionStep(eta=0.5)
    parks = [phys.light.PathAbsorptionStep(1e3 / STEP) for _ in range(3)]
    run = simulate([parks[0], a, parks[1], b, parks[2]])
    cfg = dict(eta=a.eta, angular=a.angular, tables=None, edges=None, center=a.center)
    n, k, pairs = [0, 0, 0], [0, 0, 0], []
    for p in range(PASSES):
        refs = []
        for j, (step, at) in enumerate(((a, 1), (b, 3))):
            before, after = run.looks[at].states[p], run.looks[at + 1].states[p]
            row = step.data[p]
            assert not moving(before).any()
            refs.append(RE.check_reemit(before, after, (row[1], row[2], row[3]), cfg, run.seed, 2 * p + j + 1, "re-emitter %d pass %d" % (j + 1, p + 1),
                                        c=light._c_h_literals()[0]))
        go1, go2 = refs[0]["reemitted"], refs[1]["reemitted"]
        for j, (who, hit) in enumerate(((np.ones(N_SIM, bool), go1), (~go1, go2), (go1, go2))):
            n[j], k[j] = n[j] + int(who.sum()), k[j] + int(hit[who].sum())
        both = go1 & go2
        pairs.append((run.looks[2].states[p]["v"][both], run.looks[4].states[p]["v"][both]))
    assert [s._n_pass for s in parks] == [3 * PASSES - 2, 3 * PASSES - 1, 3 * PASSES]
    check_binomial("re-emitter 1", n[0], k[0], 0.5)
    check_binomial("re-emitter 2, whom 1 left parked", n[1], k[1], 0.5)
    check_binomial("re-emitter 2, whom 1 re-emitted", n[2], k[2], 0.5)
    check_directions("re-emitters", pairs)
