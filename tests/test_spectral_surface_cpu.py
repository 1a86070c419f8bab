"""CPU: SpectralSurfaceStep (light.SpectralSurfaceStep, light._spectral_bounce, pcl_step_ground_spectral) -- the constructor, the numpy
restatement against a plain loop on a scene that holds every case, the grey ground as the one-band case, the statistics of the
draws, the host-resident path, the header, the bindings, the build table and the refusals that
need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
from physicl_amd import _hip, build, light, tally
from spectral_surface_reference import (BAD_CALLS, BAD_STEPS, C, CENTER, COUNTS, RADIUS, SEED, abi_args, assert_every_outcome, bounce, config,
                                        edges_of, scene, same_answer, spectral_bounce_loop, tables_of)
from writer_reference import same_bits

ENTRIES = ("pcl_step_ground_spectral", "pcl_group_step_ground_spectral")
N = 600


# ------------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("kw, word", BAD_STEPS)
def test_constructor_refusals_name_the_argument(kw, word):
    a = dict(radius=1.0, albedo=[0.5, 0.5, 0.5], E_edges=[1.0, 2.0, 3.0, 4.0])
    a.update(kw)
    with pytest.raises(ValueError, match=word):
        phys.light.SpectralSurfaceStep(**a)
    assert "pcl_step_ground_spectral" in light._check_spectral_surface.__doc__


def test_constructor_keeps_what_it_was_given_and_the_class_is_where_the_ground_is():
    step = phys.light.SpectralSurfaceStep(2.5, [0.05, 0.5], [1.0, 2.0, 3.0], CENTER, specular=[0.0, 1.0], out_fn="rows.csv")
    assert (step.radius, step.out_fn, step._pass, step.data) == (2.5, "rows.csv", 0, [])
    assert step.albedo.tolist() == [0.05, 0.5] and step.specular.tolist() == [0.0, 1.0] and step.E_edges.tolist() == [1.0, 2.0, 3.0]
    assert step.center.tolist() == CENTER.tolist() and [getattr(step, name) for name in COUNTS] == [0] * 4
    assert step.reflected_by_band.tolist() == step.absorbed_by_band.tolist() == [0, 0] and step.reflected_by_band.dtype == np.int64
    plain = phys.light.SpectralSurfaceStep(1.0, [1.0], [0.0, 1.0])
    assert plain.specular.tolist() == [0.0] and plain.center.tolist() == [0.0, 0.0, 0.0] and plain.out_fn is None
    assert phys.light.SpectralSurfaceStep(1.0, [1.0, 0.0], [0.0, 1.0, 2.0], specular=0.25).specular.tolist() == [0.25, 0.25]
    full = phys.light.SpectralSurfaceStep(1.0, np.full(1024, 0.5), np.arange(1025.0))      # PCL_SPECTRAL_MAX_BANDS
    assert len(full.albedo) == _hip.SPECTRAL_MAX_BANDS == 1024
    assert plain._writes == ("r", "dr", "v", "dv") and plain._fuse_role is None
    import phys.light as short
    assert short.SpectralSurfaceStep is light.SpectralSurfaceStep is phys.light.SpectralSurfaceStep
    cls = light.SpectralSurfaceStep
    assert issubclass(cls, tally.WriterStep) and cls.__mro__[1] is tally.WriterStep and not set(vars(cls)) & {"run", "_device_run", "_reduce"}
    assert "one launch per light step" in cls._NOTE and "SpectralSurfaceStep" in cls._NOTE
    assert "term cache" in cls.__doc__                                 # what asking for E costs a wavelength-dependent scatter step


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("B", [1, 3])
def test_the_restatement_is_the_loop_bit_for_bit(B, dtype):
    state = scene(N, dtype, B=B)
    cfg = config(B)
    for n_pass in (1, 2):
        ref, loop = (bounce(fn, state, cfg, n_pass, dtype) for fn in (light._spectral_bounce, spectral_bounce_loop))
        assert same_answer(ref, loop), n_pass
    share = assert_every_outcome(ref, (B, dtype))
    print(B, dtype.__name__, share)
    assert ref["reflected_by_band"].sum() == ref["reflected"].sum() and ref["absorbed_by_band"].sum() == (ref["absorbed"] & ~ref["out_of_band"]).sum()
    if dtype is np.float32:                                            # what is written is a float32 value, rounded once
        hit = ref["hit"]
        for f in ("r", "v", "dr", "dv"):
            assert same_bits(ref[f][hit].astype(np.float32).astype(np.float64), ref[f][hit]), f
        wide = bounce(light._spectral_bounce, state, cfg, 2, np.float64)
        assert not same_bits(wide["r"][hit], ref["r"][hit])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_scene_holds_every_case(dtype):
    state = scene(N, dtype, B=3)
    cfg = config(3)                                                    # albedo (0.05, 1, 0.5), specular (1, 0.5, 0)
    ref = bounce(light._spectral_bounce, state, cfg, dtype=dtype)
    i = np.arange(N)
    hit, photon, band = ref["hit"], state["photon"], ref["band"]
    bad = (i % 34 == 14) | (i % 38 == 16) | (i % 58 == 18)             # a NaN in r, a NaN in dr, an infinite dr
    assert not hit[~photon].any() and not hit[bad].any() and (bad & photon & (i % 2 == 0)).sum() > 10
    assert np.array_equal(hit, (i % 2 == 0) & photon & ~bad)           # the cloud's even slots
    for mod, want in ((2, 0), (4, 1), (6, 2)):                         # on the first edge, on an inner edge, on the last (closed) edge
        at = hit & (i % 26 == mod)
        assert at.sum() > 5 and (band[at] == want).all(), mod
    for mod in (8, 10, 12):                                            # one step outside on either side, and NaN
        at = hit & (i % 26 == mod)
        assert at.sum() > 5 and ref["out_of_band"][at].all() and ref["absorbed"][at].all() and (band[at] == -1).all(), mod
    assert (band[~hit] == -1).all() and np.array_equal(ref["out_of_band"], hit & (band < 0))
    # the outcomes: one each; the tables' exact values decide without a draw
    refl, gone, mirrored = ref["reflected"], ref["absorbed"], ref["mirrored"]
    assert np.array_equal(refl | gone, hit) and not (refl & gone).any() and not (mirrored & ~refl).any()
    assert refl[hit & (band == 1)].all()                               # albedo 1: everybody is reflected
    assert mirrored[refl & (band == 0)].all() and not mirrored[band == 2].any()            # specular 1 and 0
    assert 0 < mirrored[refl & (band == 1)].sum() < (refl & (band == 1)).sum()             # specular 0.5: drawn
    assert 0 < refl[band == 2].sum() < (band == 2).sum() and 0 < refl[band == 0].sum() < 0.3 * (band == 0).sum()
    assert ref["reflected_by_band"].tolist() == [(refl & (band == k)).sum() for k in range(3)]
    assert ref["absorbed_by_band"].tolist() == [(gone & (band == k)).sum() for k in range(3)]
    # parked: on the sphere, at rest;  who is not hit keeps every bit
    x = ref["r"][gone] - CENTER
    assert np.max(np.abs(np.sqrt((x * x).sum(axis=1)) - RADIUS)) < 1e-5 and not ref["v"][gone].any()
    assert same_bits(ref["dv"][gone], (0.0 - state["v"][gone]))
    for f in ("r", "v", "dr"):
        assert same_bits(ref[f][~hit], state[f][~hit]), f
    # the blocks are the ones the header names
    k = int(np.flatnonzero(mirrored & (band == 1))[0])
    assert light._philox_block([state["id"][k]], SEED, 1, 22)[0][0] < 0.5 and light._SPECTRAL_MIRROR_WORD == 22
    k = int(np.flatnonzero(refl & ~mirrored & (band == 1))[0])
    assert not light._philox_block([state["id"][k]], SEED, 1, 22)[0][0] < 0.5
    k = int(np.flatnonzero(gone & (band == 2))[0])
    assert not light._philox_block([state["id"][k]], SEED, 1, 9)[0][0] < 0.5


def test_the_draws_follow_the_id_the_pass_and_the_seed():
    state = scene(N)
    cfg = config(3)
    one = bounce(light._spectral_bounce, state, cfg)
    for other in (bounce(light._spectral_bounce, state, cfg, n_pass=2), bounce(light._spectral_bounce, state, cfg, seed=SEED + 1),
                  bounce(light._spectral_bounce, state, cfg, ids=state["id"] + 1)):
        assert np.array_equal(other["hit"], one["hit"]) and np.array_equal(other["band"], one["band"])
        assert not np.array_equal(other["reflected"], one["reflected"]) and not np.array_equal(other["mirrored"], one["mirrored"])
    perm = np.random.RandomState(3).permutation(N)
    moved = bounce(light._spectral_bounce, {k: a[perm] for k, a in state.items()}, cfg)
    assert all(same_bits(moved[f], one[f][perm]) for f in ("r", "v", "dr", "dv"))                  # a photon is its id, wherever it stands
    black = config(3, albedo=np.zeros(3))                              # nothing is reflected: the other draws are never looked at
    assert same_bits(bounce(light._spectral_bounce, state, black, 2)["r"], bounce(light._spectral_bounce, state, black, 9, seed=1)["r"])
    mirror = config(3, albedo=np.ones(3), specular=np.ones(3))         # nothing is drawn at all
    assert same_bits(bounce(light._spectral_bounce, state, mirror, 2)["v"], bounce(light._spectral_bounce, state, mirror, 9, seed=1)["v"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("albedo", [1.0, 0.0, 0.4])
@pytest.mark.parametrize("specular, mode", [(0.0, "lambertian"), (1.0, "specular")])
def test_one_band_that_holds_every_energy_is_the_grey_ground(specular, mode, albedo, dtype):
    state = scene(N, dtype, special=False)
    cfg = dict(radius=RADIUS, center=CENTER, E_edges=[0.5, 3.5], albedo=[albedo], specular=[specular])
    new = bounce(light._spectral_bounce, state, cfg, 3, dtype)
    old = light._surface_bounce(state["r"], state["dr"], state["v"], state["photon"], state["id"], RADIUS, CENTER, albedo, mode, C, SEED, 3, dtype)
    assert set(old) <= set(new) and old["hit"].sum() == N // 2
    for k in old:                                                      # every returned array
        assert same_bits(new[k], old[k]), k
    assert not new["out_of_band"].any() and np.array_equal(new["mirrored"], new["reflected"] & (mode == "specular"))
    assert (new["band"][new["hit"]] == 0).all()


def test_the_shared_arithmetic_has_not_moved_the_grey_ground():
    """``_surface_bounce`` now runs on ``_ground_hits`` / ``_ground_bounce``: a digest of its results, taken before the split."""
    import hashlib
    state = scene(N, special=True)
    h = hashlib.sha256()
    for mode, albedo, dtype in (("lambertian", 0.5, np.float64), ("specular", 0.3, np.float32), ("lambertian", 1.0, np.float32)):
        out = light._surface_bounce(state["r"], state["dr"], state["v"], state["photon"], state["id"], RADIUS, CENTER, albedo, mode, C, SEED, 2, dtype)
        for k in sorted(out):
            h.update(np.ascontiguousarray(out[k]).tobytes())
    assert h.hexdigest()[:16] == GREY_DIGEST


GREY_DIGEST = "fb5bfeec579d8764"


@pytest.mark.parametrize("specular", [0.25, 0.7])
def test_the_reflected_and_the_mirrored_shares_are_the_tables(specular):
    n, albedo = 200_000, 0.35
    state = scene(n, special=False)
    ref = bounce(light._spectral_bounce, state, dict(radius=RADIUS, center=CENTER, E_edges=[0.5, 3.5], albedo=[albedo], specular=[specular]))
    hit, refl, mirrored = int(ref["hit"].sum()), int(ref["reflected"].sum()), int(ref["mirrored"].sum())
    for got, trials, p in ((refl, hit, albedo), (mirrored, refl, specular)):     # binomial: the bound is derived, not measured
        sigma = np.sqrt(trials * p * (1.0 - p))
        print("%d of %d, expected %.1f, sigma %.1f: %.2f sigma" % (got, trials, trials * p, sigma, (got - trials * p) / sigma))
        assert abs(got - trials * p) <= 5.0 * sigma
    # the two draws are independent: among the mirrored and among the others the albedo draw has the same distribution
    u9 = light._philox_block(state["id"][ref["reflected"]], SEED, 1, 9)[0]
    m = ref["mirrored"][ref["reflected"]]
    assert abs(u9[m].mean() - u9[~m].mean()) <= 5.0 * albedo / np.sqrt(12.0) * np.sqrt(1.0 / m.sum() + 1.0 / (~m).sum())


# ------------------------------------------------------------------------------------------------ the step on the host
class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed = 0.25, SEED

    def __init__(self, objs, py=False, steps=None):
        self.objects, self.py, self.steps = objs, py, steps or {}

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


@pytest.mark.parametrize("py", [False, True])
def test_host_resident_objects_get_the_restatement_s_state(tmp_path, py):
    state = scene(400)
    finite = np.isfinite(state["r"]).all(axis=1) & np.isfinite(state["dr"]).all(axis=1)   # (a shell counts a move from infinitely far)
    state = {k: a[finite] for k, a in state.items()}
    n = int(finite.sum())
    objs = objects(state)
    E0, photon = tally.photon_energies(objs, phys.light.PhotonObject)
    r0, v0, dr0, dv0 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    cfg = config(3)
    step = phys.light.SpectralSurfaceStep(RADIUS, cfg["albedo"], cfg["E_edges"], CENTER, cfg["specular"], out_fn=str(tmp_path / "ground.csv"))
    shell = phys.light.ShellCrossingMeasureStep(None, [RADIUS], center=CENTER)
    sim = HostSim(objs, py=py, steps={0: shell, 1: step})              # the step reads no dv rule: cl_on=False is not refused
    shell.run(sim)
    step.run(sim)
    c_code = light._c_h_literals()[0]
    ref = light._spectral_bounce(r0, dr0, v0, E0, photon, np.arange(n), RADIUS, CENTER, cfg["albedo"], cfg["specular"], cfg["E_edges"], c_code,
                                 SEED, 1)
    assert_every_outcome(ref, "host")
    hit = ref["hit"]
    counts = [int(ref[k].sum()) for k in COUNTS]
    assert [getattr(step, name) for name in COUNTS] == counts and step.absorbed >= step.out_of_band > 0
    assert step.reflected_by_band.tolist() == ref["reflected_by_band"].tolist() and step.absorbed_by_band.tolist() == ref["absorbed_by_band"].tolist()
    row = list(step.data[0])
    assert len(step.data) == 1 and row[:5] == [0.25] + counts and sim.launch_note is None
    assert row[5].tolist() == ref["reflected_by_band"].tolist() and row[6].tolist() == ref["absorbed_by_band"].tolist()
    # a shell of the same radius in front of the step: every incoming move -- the plain Objects' as well, which the step leaves alone
    came_in = int(list(shell.data[0])[3][0])
    every = light._spectral_bounce(r0, dr0, v0, E0, np.ones(n, dtype=bool), np.arange(n), RADIUS, CENTER, cfg["albedo"], cfg["specular"],
                                   cfg["E_edges"], c_code, SEED, 1)
    objects_in = int((every["hit"] & ~photon).sum())
    assert objects_in > 0 and came_in - objects_in == step.reflected + step.absorbed
    r1, v1, dr1, dv1 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    assert same_bits(r1, ref["r"]) and same_bits(v1, ref["v"]) and same_bits(dr1, ref["dr"])
    assert same_bits(dv1[hit], ref["dv"][hit]) and same_bits(dv1[~hit], dv0[~hit])
    assert same_bits(tally.photon_energies(objs, phys.light.PhotonObject)[0], E0)          # E is read, never written
    step.run(sim)                                                      # a second pass: the counter moves
    assert step._pass == 2 and len(step.data) == 2
    step.terminate(sim)
    lines = open(str(tmp_path / "ground.csv")).read().splitlines()
    assert len(lines) == 2 and lines[0].startswith("0.25, %d, %d, %d, %d, [" % tuple(counts))


def test_a_simulation_holds_one_ground():
    state = scene(64)
    cfg = config(3)
    make = lambda: phys.light.SpectralSurfaceStep(RADIUS, cfg["albedo"], cfg["E_edges"], CENTER, cfg["specular"])      # noqa: E731
    for other, name in ((phys.light.SurfaceReflectStep(RADIUS, center=CENTER), "SurfaceReflectStep"), (make(), "SpectralSurfaceStep")):
        step = make()
        sim = HostSim(objects(state), steps={3: other, 4: step})
        with pytest.raises(ValueError, match="one ground.*%s" % name):
            step.run(sim)
        assert step._pass == 0 and step.data == []                     # refused before anything moved

        class Sim(HostSim):                                            # the device path refuses as well, before the sweep
            _residency = "device"
        with pytest.raises(ValueError, match="one ground"):
            step._device_run(Sim([], steps={3: other, 4: step}))
    alone = make()
    alone.run(HostSim(objects(state), steps={1: phys.light.RefractiveSurfaceStep(2 * RADIUS, 1.33), 4: alone}))     # an ocean is no ground
    assert alone._pass == 1


def test_a_real_simulation_with_two_grounds_is_refused_on_the_host_path():
    """``_refuse`` reads ``Simulation.steps`` itself, not a stand-in's: host-resident objects, no device."""
    cfg = config(3)
    for other in (phys.light.SurfaceReflectStep(RADIUS, center=CENTER),
                  phys.light.SpectralSurfaceStep(RADIUS, cfg["albedo"], cfg["E_edges"], CENTER)):
        sim = phys.Simulation(cl_on=False, seed=SEED)
        sim.add_objs(objects(scene(64)))
        step = phys.light.SpectralSurfaceStep(RADIUS, cfg["albedo"], cfg["E_edges"], CENTER, cfg["specular"])
        sim.add_step(3, other)
        sim.add_step(4, step)
        assert step in sim.steps.values() and other in sim.steps.values()
        with pytest.raises(ValueError, match="one ground.*%s" % type(other).__name__):
            step.run(sim)
        assert step._pass == 0 and step.data == []
    sim = phys.Simulation(cl_on=False, seed=SEED)                      # one ground alone runs
    sim.add_objs(objects(scene(64)))
    step = phys.light.SpectralSurfaceStep(RADIUS, cfg["albedo"], cfg["E_edges"], CENTER, cfg["specular"])
    sim.add_step(4, step)
    step.run(sim)
    assert step._pass == 1 and step.reflected + step.absorbed > 0


def test_device_run_notes_the_launch_schedule_and_reduces_the_row():
    class Dev:
        count, calls = 1000, []

        def ground_spectral(self, *a):
            self.calls.append(a)
            return np.array([5, 4, 3, 2], dtype=np.int64), np.array([1, 2, 2]), np.array([0, 1, 1])

    class Sim:
        t, seed, launch_note, _dev, _scattered, chunks, steps = 0.5, 99, None, Dev(), False, [], {}

        def _k_wanted(self):
            return 32

        def _py_semantics(self):
            return True                                                # not refused: the step needs no dv rule

        def _global(self, values):
            self.chunks.append(len(values))
            return np.asarray(values, dtype=np.int64) * 2               # two ranks with the same tallies
    sim = Sim()
    cfg = config(3)
    step = phys.light.SpectralSurfaceStep(2.0, cfg["albedo"], cfg["E_edges"], CENTER, 0.25)
    step._device_run(sim)
    step._device_run(sim)
    assert "SpectralSurfaceStep" in sim.launch_note and "one launch per light step" in sim.launch_note and sim._scattered
    assert [getattr(step, name) for name in COUNTS] == [10, 8, 6, 4]
    assert step.reflected_by_band.tolist() == [2, 4, 4] and step.absorbed_by_band.tolist() == [0, 2, 2]
    row = list(step.data[1])
    assert len(step.data) == 2 and row[:5] == [0.5, 10, 8, 6, 4] and row[5].tolist() == [2, 4, 4] and row[6].tolist() == [0, 2, 2]
    assert sim.chunks == [1 + 4 + 6] * 2                                # one collective per pass: N, the four counts, two rows of three
    a, b = Dev.calls
    assert a[0] == 2.0 and a[1].tolist() == cfg["E_edges"].tolist() and a[2].tolist() == cfg["albedo"].tolist() and a[3].tolist() == [0.25] * 3
    assert a[4].tolist() == CENTER.tolist() and a[5] == light._c_h_literals()[0] and (a[6], a[7], b[7]) == (99, 1, 2)


def test_multi_device_sums_the_shards_tallies():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def ground_spectral(self, *a, **kw):
            return self.k * np.arange(4, dtype=np.int64), self.k * np.array([1, 2, 3]), self.k * np.array([3, 2, 1])
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    counts, refl, gone = md.ground_spectral(1.0, [1.0, 2.0, 3.0, 4.0], [0.5] * 3)
    md._pool.shutdown()
    assert counts.tolist() == [0, 111, 222, 333] and refl.tolist() == [111, 222, 333] and gone.tolist() == [333, 222, 111]


def test_binding_marshals_the_call():
    def entry(handle, radius, ce, B, Ee, al, sp, c, seed, n_pass, counts, bands):
        arr = lambda p, k: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctypes.c_double)), (k,)).tolist()            # noqa: E731
        seen.append((handle, radius, None if ce is None else arr(ce, 3), B, arr(Ee, B + 1), arr(al, B), arr(sp, B), c, seed, n_pass))
        np.ctypeslib.as_array(ctypes.cast(counts, ctypes.POINTER(ctypes.c_int64)), (4,))[:] = np.arange(4) + 100
        np.ctypeslib.as_array(ctypes.cast(bands, ctypes.POINTER(ctypes.c_int64)), (2 * B,))[:] = np.arange(2 * B)
        return 0
    seen = []
    counts, refl, gone = _hip._ground_spectral(entry, "h", 2.0, CENTER, [1.0, 2.0, 3.0], [0.5, 0.25], 0.75, C, -1, 2 ** 32 + 3)
    assert counts.tolist() == [100, 101, 102, 103] and refl.tolist() == [0, 1] and gone.tolist() == [2, 3] and counts.dtype == np.int64
    assert seen[0] == ("h", 2.0, CENTER.tolist(), 2, [1.0, 2.0, 3.0], [0.5, 0.25], [0.75, 0.75], C, 2 ** 64 - 1, 3)
    _hip._ground_spectral(entry, "h", 2.0, None, [1.0, 2.0, 3.0], [0.5, 0.25], [0.0, 1.0], C, 1, 1)
    assert seen[1][2] is None and seen[1][6] == [0.0, 1.0]
    with pytest.raises(ValueError, match="bands"):
        _hip._ground_spectral(entry, "h", 2.0, None, [1.0, 2.0, 3.0], [0.5], 0.0, C, 1, 1)


# ------------------------------------------------------------------------------------------------ the library
def surface_unit():
    (unit,) = [u for u in build.ADDONS if os.path.basename(u["src"]) == "pcl_surface.hip"]
    return unit


def test_header_prototypes_and_the_build_table():
    text = open(build.ABI_HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and len(_hip._PROTOTYPES[entry]) == 12
    assert re.search(r"#define PCL_SPECTRAL_MAX_BANDS 1024\b", code) and _hip.SPECTRAL_MAX_BANDS == 1024
    flat = " ".join(text.split()).replace("* ", "")
    assert "word 22 is used by nothing else" in flat and "0-5 and 8-21 are taken" in flat
    for line in ("(id_lo, id_hi, pass, 22)", "reflected iff u < albedo_b", "mirrored iff u < specular_b", "the last one closed",
                 "r = center + x; v = 0; dr = x - p; dv = 0 - v_old", "dir = mh - (2*dn)*nrm", "mu = sqrt(1 - u_a)",
                 "v = c*dir; dv = v - v_old; dr = w*dir; r = center + (x + dr)", "counted in out_of_band"):
        assert line in flat, line                                      # the order is written out
    assert hasattr(_hip.Device, "ground_spectral") and hasattr(_hip.DeviceGroup, "ground_spectral")
    from physicl_amd.multidev import MultiDevice
    assert hasattr(MultiDevice, "ground_spectral")
    # the table: the unit of the writer sweeps holds this one, described as every sweep is (tests/test_build_cpu.py checks it as one)
    assert dict(entries=ENTRIES, kernel="k_ground_spectral", count=2) in surface_unit()["sweeps"]


def test_the_counter_word_is_a_named_constant_used_once():
    src = open(os.path.join(build.CSRC, "pcl_surface.hip")).read()
    assert re.findall(r"\b(kSpectral\w+) = (\d+)", src) == [("kSpectralMirrorDraw", "22")]
    assert len(re.findall(r"pcl_philox4x32_10\([^;]*?, kSpectralMirrorDraw, ", src)) == 1
    assert len(re.findall(r"\bkSpectralMirrorDraw\b", src)) == 2       # the constant and its one call
    body = src[src.index("void __launch_bounds__(kBlock) k_ground_spectral"):src.index("struct surface_spec")]
    assert sorted(re.findall(r"pcl_philox4x32_10\([^;]*?, (\w+), a\.k0", body)) == ["8u", "9u", "kSpectralMirrorDraw"]
    for f in sorted(os.listdir(build.CSRC)):
        if f.endswith((".hip", ".h", ".inc")):
            text = open(os.path.join(build.CSRC, f)).read()
            words = [int(w) for w in re.findall(r"pcl_philox4x32_10\([^;]*?, (\d+)u, ", text)]
            words += [int(w) for w in re.findall(r"\bk\w+ = (\d+)[,;]", text) if f != "pcl_surface.hip"]
            assert 22 not in words, f
    named = dict(re.findall(r"\b(k[A-Z]\w+) = (\d+)", src))
    assert [k for k, w in named.items() if w == "22"] == ["kSpectralMirrorDraw"]


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context and a NULL group, refused as well); the outputs stay as
    they were."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in BAD_CALLS:
        keep, args, counts, bands = abi_args(**kw)
        assert lib.pcl_step_ground_spectral(None, *args) == -2, kw
        assert lib.pcl_group_step_ground_spectral(None, *args) == -2, kw
        assert (counts is None or (counts == -7).all()) and (bands is None or (bands == -7).all()), kw
    keep, args, counts, bands = abi_args()                             # a good call without a context is refused, too
    assert lib.pcl_step_ground_spectral(None, *args) == -2 and lib.pcl_group_step_ground_spectral(None, *args) != 0
    assert (counts == -7).all() and (bands == -7).all()
    for kw, word in BAD_STEPS:                                         # what the constructor refuses of the tables, the library refuses
        if set(kw) & {"albedo", "specular", "E_edges"} and not any(isinstance(x, str) for x in kw.values()):
            edges = np.atleast_1d(np.asarray(kw.get("E_edges", edges_of(3)), dtype=np.float64))
            B = len(edges) - 1
            tabs = [np.atleast_1d(np.asarray(kw.get(k, tables_of(3)[j]), dtype=np.float64)) for j, k in enumerate(("albedo", "specular"))]
            if B >= 1 and all(len(t) == B for t in tabs):
                keep, args, counts, bands = abi_args(n_bands=B, E_edges=edges, albedo=tabs[0], specular=tabs[1],
                                                     bands=np.full(2 * B + 2, -7, dtype=np.int64))
                assert lib.pcl_step_ground_spectral(None, *args) == -2, kw
