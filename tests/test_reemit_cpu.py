"""CPU: ReemissionStep (light.ReemissionStep, light._reemit_parked, pcl_step_reemit_parked) -- the constructor, the numpy
restatement against a plain loop on a scene that holds every case, the directions, the host-resident path, the header, the
bindings, the build table and the refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
from physicl_amd import _hip, build, light, tally
from reemit_reference import (ANGULAR, BAD_CALLS, C, CDF_A, CDF_B, CENTER, EDGES, ETA, EVERYWHERE, EVERYWHERE_UP, GRID_A, GRID_B,
                              ID_BASE, LAYERED, SEED, TABLES, abi_args, reemit_parked_loop, same_answer, scene)
from writer_reference import DIR_ULP, same_bits, ulp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pcl_step_reemit_parked", "pcl_group_step_reemit_parked")
N = 3000


def reemit(fn, state, cfg, n_pass=1, dtype=np.float64, seed=SEED, **kw):
    a = dict(photon=state["photon"], ids=state["id"])
    a.update(kw)
    return fn(state["r"], state["v"], state["E"], a["photon"], a["ids"], cfg["eta"], cfg["angular"], cfg["tables"], cfg["edges"],
              cfg["center"], C, seed, n_pass, dtype)


# ------------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("kw, word", [
    (dict(edges=[1.0]), "edges"), (dict(edges=[2.0, 1.0]), "edges"), (dict(edges=[-1.0, 1.0]), "edges"), (dict(edges=[0.0, np.nan]), "edges"),
    (dict(edges=[0.0, 1e200]), "edges"), (dict(edges=np.arange(66.0)), "edges"), (dict(edges="far"), "edges"),
    (dict(center=(0, 0)), "center"), (dict(center=(0, np.nan, 0)), "center"),
    (dict(eta=1.5), "eta"), (dict(eta=-0.1), "eta"), (dict(eta=np.nan), "eta"), (dict(eta="often"), "eta"), (dict(eta=[0.5, 0.5]), "eta"),
    (dict(edges=[0.0, 1.0, 2.0], eta=[0.5, 0.5, 0.5]), "eta"), (dict(edges=[0.0, 1.0, 2.0], eta=[0.5, 1.5]), "eta"),
    (dict(angular="specular"), "angular"), (dict(angular=3), "angular"), (dict(angular=["isotropic", "lambertian"]), "angular"),
    (dict(edges=[0.0, 1.0, 2.0], angular=["isotropic", "beam"]), "angular"),
    (dict(spectra=5), "spectra"), (dict(spectra=([1.0, 2.0], [0.5, 1.0, 1.0])), "spectra"), (dict(spectra=[([], [])]), "spectra"),
    (dict(spectra=(np.ones(1025), np.linspace(0, 1, 1025))), "spectra"), (dict(spectra=([1.0, 2.0], [0.5, 0.9])), "cdf"),
    (dict(spectra=([1.0, 2.0], [0.7, 0.5])), "cdf"), (dict(spectra=([1.0, 2.0], [np.nan, 1.0])), "cdf"),
    (dict(spectra=([1.0, np.inf], [0.5, 1.0])), "grid"), (dict(spectra=[(["a", "b"], [0.5, 1.0])]), "spectra"),
    (dict(spectra=phys.light.generate_photons_bulk(10, min=1.0, max=2.0)), "spectra"),
    (dict(edges=[0.0, 1.0, 2.0], spectra=[None]), "spectra"), (dict(edges=[0.0, 1.0, 2.0], spectra=[None, ([1.0], [0.5])]), r"spectra\[1\]"),
    (dict(edges=[0.0, 1.0, 2.0, 3.0], spectra=[(np.ones(1024), np.linspace(0, 1, 1024))] * 3), "2048"),
])
def test_constructor_refusals_name_the_argument(kw, word):
    with pytest.raises(ValueError, match=word):
        phys.light.ReemissionStep(**kw)
    assert light._check_reemission.__doc__ and "pcl_step_reemit_parked" in light._check_reemission.__doc__


def test_constructor_keeps_what_it_was_given():
    step = phys.light.ReemissionStep(TABLES, EDGES, CENTER, ETA, ANGULAR)
    assert step.edges.tolist() == EDGES.tolist() and step.center.tolist() == CENTER.tolist() and step.eta.tolist() == ETA.tolist()
    assert step.angular == ANGULAR and step.spectra[1] is None and same_bits(step.spectra[0][0], GRID_A) and same_bits(step.spectra[3][1], CDF_B)
    assert (step.parked, step.reemitted, step._pass, step.data) == (0, 0, 0, []) and step.by_layer.tolist() == [0, 0, 0, 0]
    assert step._writes == ("r", "dr", "v", "dv", "E")
    plain = phys.light.ReemissionStep()
    assert plain.edges is None and plain.spectra == [None] and plain.eta.tolist() == [1.0] and plain.angular == ("isotropic",)
    assert "E" not in plain._writes                                    # no table: E is not written, the term cache is kept
    assert "E" not in phys.light.ReemissionStep([None, None], [0.0, 1.0, 2.0])._writes
    one = phys.light.ReemissionStep((GRID_B, CDF_B), EDGES, eta=0.25, angular="lambertian")                 # one value for every layer
    assert one.eta.tolist() == [0.25] * 4 and one.angular == ("lambertian",) * 4 and all(same_bits(t[0], GRID_B) for t in one.spectra)
    batch = phys.light.generate_photons_bulk(10, min=1e-19, max=5e-19, T=5800.0, bins=200)
    cdf, grid = batch.table
    taken = phys.light.ReemissionStep([batch, None], [0.0, 1.0, 2.0]).spectra
    assert same_bits(taken[0][0], np.asarray(grid, dtype=np.float64)) and same_bits(taken[0][1], np.asarray(cdf, dtype=np.float64)) and taken[1] is None
    big = phys.light.ReemissionStep([(np.ones(1024), np.linspace(0, 1, 1024))] * 2, [0.0, 1.0, 2.0])         # the limits themselves
    assert sum(len(t[1]) for t in big.spectra) == 2048 == _hip.REEMIT_MAX_TOTAL_BINS
    import phys.light as short
    assert short.ReemissionStep is light.ReemissionStep is phys.light.ReemissionStep and issubclass(light.ReemissionStep, tally.WriterStep)


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("cfg", [LAYERED, EVERYWHERE, EVERYWHERE_UP], ids=["layered", "everywhere", "everywhere_up"])
def test_the_restatement_is_the_loop_bit_for_bit(cfg, dtype):
    state = scene(N, dtype)
    for n_pass in (1, 2):
        ref, loop = (reemit(fn, state, cfg, n_pass, dtype) for fn in (light._reemit_parked, reemit_parked_loop))
        assert same_answer(ref, loop), n_pass
    everybody = cfg is EVERYWHERE                                      # eta 1, isotropic: whoever is parked is re-emitted
    assert 0 < ref["reemitted"].sum() < N and (ref["reemitted"].sum() == ref["parked"].sum()) == everybody


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_scene_holds_every_case(dtype):
    state = scene(N, dtype)
    ref = reemit(light._reemit_parked, state, LAYERED, dtype=dtype)
    i = np.arange(N)
    photon, parked, go, layer = state["photon"], ref["parked"], ref["reemitted"], ref["layer"]
    rest = (i % 2 == 0) & (i % 13 != 0) & photon                       # -0.0 is at rest, a NaN moves, a plain Object is never parked
    rest &= i % 26 != 1
    where = np.zeros(N, dtype=np.int64)                                # the special positions, in the order the scene writes them
    for tag, (m, k) in enumerate(((10, 0), (14, 2), (18, 4), (22, 6)), 1):
        where[i % m == k] = tag
    where[i % 34 == 8] = 5                                             # a NaN in r
    at = lambda tag: rest & (where == tag)                             # noqa: E731
    assert all(at(tag).sum() > 0 for tag in range(1, 6))
    assert not parked[~rest].any() and parked[at(1) & (i % 6 == 0)].all() and (at(1) & (i % 6 == 0)).sum() > 0 and not parked[~photon].any()
    assert (layer[at(1)] == 0).all() and not go[at(1)].any()           # q == 0 in a lambertian layer: parked only
    assert (layer[at(2)] == 1).all()                                   # on the inner edge: the layer above
    assert (layer[at(3)] == 3).all()                                   # the outermost edge is inside
    assert (layer[at(4)] == -1).all() and (layer[at(5)] == -1).all()   # just outside; a NaN
    eta_of = ETA[np.maximum(layer, 0)]
    assert not go[parked & (eta_of == 0.0)].any() and (parked & (layer == 2)).sum() > 0              # eta 0: nobody
    assert go[parked & (layer == 0) & (where != 1)].all()                                          # eta 1: everybody with a vertical
    half = parked & (eta_of == 0.5)
    assert 0.35 < go[half].mean() < 0.65 and half.sum() > 200
    assert ref["by_layer"].tolist() == [int((go & (layer == b)).sum()) for b in range(4)] and ref["by_layer"][2] == 0
    # who is not re-emitted keeps every bit; r is nobody's to write; dr and dv of the re-emitted are +0.0
    assert same_bits(ref["r"], state["r"]) and same_bits(ref["v"][~go], state["v"][~go]) and same_bits(ref["E"][~go], state["E"][~go])
    assert np.isnan(ref["dr"][~go]).all() and same_bits(ref["dr"][go], np.zeros((go.sum(), 3))) and same_bits(ref["dv"][go], np.zeros((go.sum(), 3)))
    # energies: layer 1 has no table and keeps its E; the others' are members of their grid; a bin without mass is never drawn
    assert same_bits(ref["E"][go & (layer == 1)], state["E"][go & (layer == 1)]) and (go & (layer == 1)).sum() > 0
    assert np.isin(ref["E"][go & (layer == 0)], GRID_A[[1, 3, 5]].astype(dtype).astype(np.float64)).all()
    assert np.isin(ref["E"][go & (layer == 3)], GRID_B).all() and (go & (layer == 3)).sum() > 0
    k = int(np.flatnonzero(go & (layer == 0))[0])                      # the blocks are the ones the header names
    u = light._philox_block([state["id"][k]], SEED, 1, 20)[0]
    assert ref["E"][k] == GRID_A[int(np.flatnonzero(CDF_A >= u)[0])]
    assert light._REEMIT_WORDS == (18, 19, 20)


def test_the_draws_follow_the_id_the_pass_and_the_seed():
    state = scene(N)
    one = reemit(light._reemit_parked, state, LAYERED)
    sure = one["reemitted"] & (one["layer"] == 0)                      # eta 1: re-emitted whatever is drawn
    for other in (reemit(light._reemit_parked, state, LAYERED, n_pass=2), reemit(light._reemit_parked, state, LAYERED, seed=SEED + 1),
                  reemit(light._reemit_parked, state, LAYERED, ids=state["id"] + 1)):
        assert np.array_equal(other["parked"], one["parked"]) and other["reemitted"][sure].all()
        assert not (other["v"][sure] == one["v"][sure]).all(axis=1).any()
        assert not np.array_equal(other["reemitted"], one["reemitted"])     # the eta 0.5 layers draw anew
    perm = np.random.RandomState(3).permutation(N)
    moved = reemit(light._reemit_parked, {k: a[perm] for k, a in state.items()}, LAYERED)
    assert same_bits(moved["v"], one["v"][perm]) and same_bits(moved["E"], one["E"][perm])           # a photon is its id, wherever it stands


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_directions(dtype):
    """Lambertian never points below the local horizon; every direction has the length c within the project's direction bound."""
    n = 20000
    rng = np.random.RandomState(2)
    r = (CENTER + rng.uniform(0.5, 3.5, size=n)[:, None] * rng.normal(size=(n, 3))).astype(dtype).astype(np.float64)
    state = {"r": r, "v": np.zeros((n, 3)), "E": np.ones(n), "photon": np.ones(n, dtype=bool), "id": np.arange(n) + ID_BASE}
    v_unit, v_bound = (ulp(C), DIR_ULP) if dtype is np.float64 else (ulp(C, np.float32), DIR_ULP + 0.5)
    for cfg in (EVERYWHERE, dict(EVERYWHERE_UP, eta=1.0)):
        ref = reemit(light._reemit_parked, state, cfg, dtype=dtype)
        assert ref["reemitted"].all()
        v = ref["v"]
        # |v| - c: each component within v_bound units of its exact value, so the length within sqrt(3) times that
        assert np.max(np.abs(np.sqrt((v * v).sum(axis=1)) - C)) <= np.sqrt(3.0) * v_bound * v_unit
        d = r - CENTER
        cos = (v * d).sum(axis=1) / (C * np.sqrt((d * d).sum(axis=1)))
        if cfg["angular"] == "lambertian":
            assert ((v * d).sum(axis=1) >= 0.0).all()
            assert abs(cos.mean() - 2.0 / 3.0) < 5.0 * np.sqrt(1.0 / 18.0 / n)       # cosine-weighted: E[mu] = 2/3, Var = 1/18
        else:
            assert abs((v[:, 0] / C).mean()) < 5.0 * np.sqrt(1.0 / 3.0 / n) and (cos < 0).sum() > 0.4 * n      # uniform on the sphere


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
    for k in range(len(state["E"])):
        if state["photon"][k]:
            o = phys.light.PhotonObject(E=phys.Measurement(np.double(state["E"][k]), "J**1"), v=phys.light.c * [1, 0, 0])
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
    state = scene(n)
    objs = objects(state)
    photon = state["photon"]
    sim = HostSim(objs, py=py)                                         # the step reads no dv rule: cl_on=False is not refused
    r0, v0, dr0, dv0 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    E0 = tally.photon_energies(objs, phys.light.PhotonObject)[0]
    step = phys.light.ReemissionStep(TABLES, EDGES, CENTER, ETA, ANGULAR, out_fn=str(tmp_path / "reemit.csv"))
    step.run(sim)
    c_code = light._c_h_literals()[0]
    ref = light._reemit_parked(r0, v0, E0, photon, np.arange(n), ETA, ANGULAR, TABLES, EDGES, CENTER, c_code, SEED, 1)
    go = ref["reemitted"]
    assert step.parked == int(ref["parked"].sum()) > step.reemitted == int(go.sum()) > 0 and step.by_layer.tolist() == ref["by_layer"].tolist()
    assert len(step.data) == 1 and list(step.data[0][:3]) == [0.25, step.parked, step.reemitted] and sim.launch_note is None
    assert step.data[0][3].tolist() == ref["by_layer"].tolist()
    r1, v1, dr1, dv1 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    E1 = tally.photon_energies(objs, phys.light.PhotonObject)[0]
    assert same_bits(r1, r0) and same_bits(v1, ref["v"])
    assert same_bits(dr1[go], np.zeros((go.sum(), 3))) and same_bits(dv1[go], np.zeros((go.sum(), 3)))
    assert same_bits(dr1[~go], dr0[~go]) and same_bits(dv1[~go], dv0[~go])
    assert same_bits(E1[photon], ref["E"][photon]) and not same_bits(E1[photon], E0[photon])
    for k, obj in enumerate(objs):
        assert type(obj) is (phys.light.PhotonObject if photon[k] else phys.Object)
    step.run(sim)                                                      # a second pass: who stayed parked draws again
    again = light._reemit_parked(r0, ref["v"], ref["E"], photon, np.arange(n), ETA, ANGULAR, TABLES, EDGES, CENTER, c_code, SEED, 2)
    assert step._pass == 2 and len(step.data) == 2 and step.parked == int(again["parked"].sum()) == int((ref["parked"] & ~go).sum())
    assert 0 < step.reemitted == int(again["reemitted"].sum())
    step.terminate(sim)
    lines = open(str(tmp_path / "reemit.csv")).read().splitlines()
    assert lines == ["0.25, %d, %d, %s" % (row[1], row[2], row[3].tolist()) for row in step.data]
    # without a table E is not written back at all
    objs = objects(state)
    phys.light.ReemissionStep(edges=EDGES, center=CENTER).run(HostSim(objs))
    assert same_bits(tally.photon_energies(objs, phys.light.PhotonObject)[0], E0)


def test_the_step_is_a_plan_item_of_its_own():
    import physicl.newton
    step = phys.light.ReemissionStep()

    class Sim:                                                         # what _build_plan / _multi_eligible ask of a simulation
        fuse, _hip = True, _hip
        steps = {0: phys.UpdateTimeStep(lambda s: np.double(1e-3)), 1: phys.newton.NewtonianKinematicsStep(),
                 2: phys.light.ScatterIsotropicStep(A=1.0, n=1.0), 3: phys.light.PathAbsorptionStep(1.0), 4: step}

        def _py_semantics(self):
            return False
    sim = Sim()
    plan = phys.Simulation._build_plan(sim)
    assert [kind for kind, _ in plan] == ["single", "fused", "single", "single"] and plan[3][1] is step
    sim._plan = plan
    assert not phys.Simulation._multi_eligible(sim)


def test_device_run_notes_the_launch_schedule_and_reduces_the_row():
    class Dev:
        count, calls = 1000, []

        def reemit_parked(self, *a):
            self.calls.append(a)
            return 70, 6, np.array([1, 2, 0, 3])

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
    step = phys.light.ReemissionStep(TABLES, EDGES, CENTER, ETA, ANGULAR)
    step._device_run(sim)
    step._device_run(sim)
    assert "ReemissionStep" in sim.launch_note and "one launch per light step" in sim.launch_note and sim._scattered
    assert (step.parked, step.reemitted) == (140, 12) and step.by_layer.tolist() == [2, 4, 0, 6] and step.by_layer.dtype == np.int64
    assert len(step.data) == 2 and list(step.data[1][:3]) == [0.5, 140, 12] and step.data[1][3].tolist() == [2, 4, 0, 6]
    assert sim.chunks == [1 + 2 + 4] * 2                                # one collective per pass: N and the 2 + L' counts
    a, b = Dev.calls
    assert a[0] == light._c_h_literals()[0] and a[1].tolist() == ETA.tolist() and a[2] == ANGULAR and a[3] is step.spectra
    assert a[4].tolist() == EDGES.tolist() and a[5].tolist() == CENTER.tolist() and (a[6], a[7], b[7]) == (99, 1, 2)


def test_multi_device_sums_the_shards_tallies():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def reemit_parked(self, *a, **kw):
            return 10 * self.k, self.k, np.array([self.k, 0, 2 * self.k])
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    parked, go, by_layer = md.reemit_parked(None)
    md._pool.shutdown()
    assert (parked, go, by_layer.tolist()) == (1110, 111, [111, 0, 222])


def test_binding_marshals_the_layers_tables():
    class FakeLib:
        def __init__(self):
            self.calls = []

    def entry(handle, L, ed, ce, et, lam, off, cdf, grid, c, seed, n_pass, counts):
        rows = max(L, 1)
        rd = lambda p, n, t: None if p is None else np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(t)), (n,)).tolist()      # noqa: E731
        offs = rd(off, rows + 1, ctypes.c_int)
        seen.append((L, rd(ed, L + 1, ctypes.c_double), rd(ce, 3, ctypes.c_double), rd(et, rows, ctypes.c_double), rd(lam, rows, ctypes.c_int),
                     offs, rd(cdf, offs[-1], ctypes.c_double), rd(grid, offs[-1], ctypes.c_double), c, seed, n_pass))
        np.ctypeslib.as_array(ctypes.cast(counts, ctypes.POINTER(ctypes.c_int64)), (2 + rows,))[:] = np.arange(2 + rows) + 100
        return 0
    seen = []
    got = _hip._reemit(entry, None, ETA, ANGULAR, TABLES, EDGES, CENTER, C, SEED, 3)
    assert got[:2] == (100, 101) and got[2].tolist() == [102, 103, 104, 105] and got[2].dtype == np.int64
    assert seen[0] == (4, EDGES.tolist(), CENTER.tolist(), ETA.tolist(), [1, 0, 0, 1], [0, 6, 6, 9, 12], np.concatenate([CDF_A, CDF_B, CDF_B]).tolist(),
                       np.concatenate([GRID_A, GRID_B, GRID_B]).tolist(), C, SEED, 3)
    got = _hip._reemit(entry, None, 1.0, "isotropic", None, None, None, C, 1, 2)
    assert seen[1][:8] == (0, None, None, [1.0], [0], [0, 0], None, None) and got[2].tolist() == [102]
    with pytest.raises(ValueError):
        _hip._reemit(entry, None, [1.0, 0.5], "isotropic", None, None, None, C, 1, 2)


# ------------------------------------------------------------------------------------------------ the library
def test_header_limits_prototypes_and_the_build_table():
    text = open(build.ABI_HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and len(_hip._PROTOTYPES[entry]) == 13
    for name, value in (("PCL_REEMIT_MAX_LAYERS", _hip.REEMIT_MAX_LAYERS), ("PCL_REEMIT_MAX_BINS", _hip.REEMIT_MAX_BINS),
                        ("PCL_REEMIT_MAX_TOTAL_BINS", _hip.REEMIT_MAX_TOTAL_BINS)):
        assert re.findall(r"#define\s+%s\s+(\d+)\b" % name, code) == [str(value)], name
    assert (_hip.REEMIT_MAX_LAYERS, _hip.REEMIT_MAX_BINS, _hip.REEMIT_MAX_TOTAL_BINS) == (64, 1024, 2048)
    assert (64 + 65 + 2 * 2048 + 65) * 8 + (2 + 64) * 4 < 64 * 1024    # the largest call's tables and cells fit the LDS a launch may ask for
    for word in (18, 19, 20):
        assert "(id_lo, id_hi, pass, %d)" % word in text                # the arithmetic is written out, the counter words with it
    flat = " ".join(text.split()).replace("* ", "")
    assert "words 18, 19 and 20 are used by nothing else" in flat and "0-5 and 8-17 are taken" in flat
    assert hasattr(_hip.Device, "reemit_parked") and hasattr(_hip.DeviceGroup, "reemit_parked")
    # the table: the unit of the writer sweeps holds this one, described as every sweep is (tests/test_build_cpu.py checks it as one)
    (unit,) = [u for u in build.ADDONS if os.path.basename(u["src"]) == "pcl_surface.hip"]
    assert dict(entries=ENTRIES, kernel="k_reemit_parked", count=2) in unit["sweeps"]


def test_the_counter_words_are_named_constants_used_nowhere_else():
    src = open(os.path.join(build.CSRC, "pcl_surface.hip")).read()
    names = dict(re.findall(r"\b(kReemit\w+) = (\d+)", src))
    assert names == {"kReemitDraw": "18", "kReemitDir": "19", "kReemitEnergy": "20"}
    for name in names:
        assert len(re.findall(r"pcl_philox4x32_10\([^;]*?, %s, " % name, src)) == 1, name
    taken = []
    for f in sorted(os.listdir(build.CSRC)):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(build.CSRC, f)).read()
            taken += [int(w) for w in re.findall(r"pcl_philox4x32_10\(.*?, (\d+)u, ", text)]
            taken += [int(w) for name, w in re.findall(r"\b(k\w+Word) = (\d+)", text)]
    assert not set(taken) & {18, 19, 20} and max(taken) == 17


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context, which is refused as well); the outputs stay as they
    were."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in [{}] + BAD_CALLS:
        keep, args, counts = abi_args(**kw)
        assert lib.pcl_step_reemit_parked(None, *args) == -2, kw
        assert lib.pcl_group_step_reemit_parked(None, *args) != 0, kw
        assert counts is None or (counts == -7).all(), kw
