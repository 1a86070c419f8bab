"""GPU: up and down fluxes through planes, as maps (pcl_step_plane_flux, PlaneFluxMapStep).

Every result is an integer, so every comparison is an equality: the counts and every cell of the maps equal the numpy restatement
(``light_grid._plane_flux_maps``) applied to the state that was uploaded (or downloaded) in the store's precision.  At the simulation
level the tallies are checked against a conservation law: per level, up - down of a pass is the change of the population at or above
it over the move, which PositionGridMeasureSteps count independently.
"""
import ctypes

import numpy as np
import pytest

from plane_flux_reference import EDGE_AXIS, EDGE_BANDS, EDGE_EDGES, EDGE_LEVELS, assert_edge_case_tallies, configs, edge_cases, scene

pytestmark = pytest.mark.gpu
C_LIT = 299792458.0
DT = 0.0005
STEP = C_LIT * DT


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


def restated(st, axis, levels, edges, Ee):
    from physicl_amd import light_grid
    return light_grid._plane_flux_maps(*st, axis, levels, edges, Ee)


def uploaded(hip, st, dtype, capacity=None, ids=None):
    r, dr, E, photon = st
    N = len(E)
    dev = hip.Device(0)
    dev.store_alloc(max(capacity or N, 1), dtype)
    dev.upload_state(dict(r=r, dr=dr, E=E))
    if ids is not None:
        dev.upload_ids(ids)
    if not photon.all():
        dev.upload_kind(photon.astype(np.uint8))
    return dev


def check(dev, st, cfg, what):
    axis, levels, edges, Ee = cfg
    want = restated(st, axis, levels, edges, Ee)
    got = dev.plane_flux(axis, levels, edges, Ee)
    for g, w, name in zip(got, want, ("counts", "maps")):
        assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (what, name)
    return got


def test_the_configurations_take_both_forms(hip):
    forms = {name: hip.plane_flux_lds_form(len(lv), len(e[0]) - 1, len(e[1]) - 1, 0 if Ee is None else len(Ee) - 1) for name, (_, lv, e, Ee) in configs().items()}
    assert forms == {"z_1_level_lds": True, "x_16_levels_lds": True, "y_16_levels_bands_global": False, "z_just_above_4096": False,
                     "y_1024_bins_lds": True, "x_bands_lds": True, "z_wide_bins": False}
    assert {cfg[0] for cfg in configs().values()} == {"x", "y", "z"}


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5, 600_011])
def test_tallies_equal_the_restatement(hip, N, dtype):
    """The shells' list of sizes; each of the three axes, 1 and 16 levels, with and without bands; both forms: maps of at most 4096
    cells, one just above, and -- no accepted call fails the byte formula below 4096 cells (tests/test_plane_flux_build_cpu.py) -- the
    LDS form with the longest edge tables."""
    st = scene(N, dtype, spread=0.8 if N < 100_000 else 0.1)             # (the big store: fewer cross, to keep numpy quick)
    dev = uploaded(hip, st, dtype, capacity=5 * 2048 if N == 3 * 2048 + 5 else None)
    try:
        for name, cfg in configs().items():
            counts, maps = check(dev, st, cfg, (N, dtype, name))
            if N >= 2047:
                assert counts.sum() > 0 and maps.sum() > 0, name
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_explicit_ids_and_plain_objects(hip, dtype):
    """A store with ids of its own and plain Objects among the photons: they count and cross, and land in a cell only without bands."""
    N = 50_001
    st = scene(N, dtype, objects=True)
    dev = uploaded(hip, st, dtype, ids=np.arange(N, dtype=np.int64)[::-1] * 3 + 11)
    try:
        cfg = configs()["y_16_levels_bands_global"]
        counts, maps = check(dev, st, cfg, dtype)
        ph = st[3]
        only_photons = restated(tuple(a[ph] for a in st), *cfg)
        assert np.array_equal(maps, only_photons[1]) and np.all(counts >= only_photons[0]) and counts.sum() > only_photons[0].sum()
        bare = check(dev, st, cfg[:3] + (None,), dtype)               # without bands no kind bytes are needed: everybody lands
        assert bare[1].sum() > maps.sum()
        check(dev, st, configs()["x_bands_lds"], dtype)
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_hand_made_edge_cases(hip, dtype):
    st = edge_cases(np.float64 if dtype == "f64" else np.float32)
    dev = uploaded(hip, st, dtype)
    try:
        for bands in (False, True):
            cfg = (EDGE_AXIS, EDGE_LEVELS, EDGE_EDGES, EDGE_BANDS if bands else None)
            assert_edge_case_tallies(*check(dev, st, cfg, (dtype, bands)), bands)
    finally:
        dev.close()


class Source:
    """An isotropic gaussian spot off the origin (what _hip._source reads)."""
    origin, e1, e2, d = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "gaussian", 0.0, 0.5 * STEP


def downloaded(hip, dev):
    r = np.stack([dev.download(hip.R0 + k) for k in range(3)], 1)
    dr = np.stack([dev.download(hip.DR0 + k) for k in range(3)], 1)
    E = dev.download(hip.E)
    return r, dr, E, np.ones(len(E), dtype=bool)


def source_config(axis):
    a = "xyz".index(axis)
    levels = Source.origin[a] + np.array([-1.5, -0.5, 0.5, 1.5]) * STEP
    edges = [Source.origin[k] + np.linspace(-4, 4, n + 1) * STEP for k, n in zip([k for k in range(3) if k != a], (9, 7))]
    return axis, levels, edges, np.linspace(1.1, 2.9, 6)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_after_lazy_fused_steps_and_behind_the_alive_mask_of_a_delete(hip, dtype):
    """The sweep looks at the store first: an implicit dr becomes real, a store behind an alive mask dense.  The twin downloads the
    state (which does the same) and restates it."""
    N = 300_000
    dev = hip.Device(0)
    try:
        dev.store_alloc(N, dtype)
        dev.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        dev.apply_source(Source, C_LIT, 11)
        kw = dict(A=3e-6, n=1.0, flags=0, c=C_LIT, h=0.0, rng_mode=hip.RNG_PHILOX, seed=5)
        for step in (1, 2):
            dev.step_fused(DT, scatter=dict(kw, step=step), planes=None, sync=False, lazy=True)       # dr implicit
        cfg = source_config("y")
        got = dev.plane_flux(*cfg)                                      # looks first: makes dr real
        want = restated(downloaded(hip, dev), *cfg)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[0][0].sum() > 0 and got[0][1].sum() > 0 and got[1].sum() > 0
        out = dev.step_fused_delete(DT, 1e-6, 1.0, seed=5, step=3, planes=None, lazy=True)             # leaves an alive mask
        assert 0 < out["N"] < N
        cfg = source_config("x")
        got = dev.plane_flux(*cfg)                                      # looks first: densifies itself
        st = downloaded(hip, dev)
        assert len(st[2]) == out["N"] == dev.count
        want = restated(st, *cfg)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[0].sum() > 0 and got[1].sum() > 0
    finally:
        dev.close()


def test_empty_store_and_refused_calls(hip):
    dev = hip.Device(0)
    try:
        lib = hip.load()
        lv, ue, ve, Ee = np.array([0.0, 1.0]), np.array([-1.0, 0.0, 1.0]), np.array([-1.0, 1.0]), np.array([1.0, 2.0, 3.0])
        c, m = np.full(4, -1, np.int64), np.full(16, -1, np.int64)
        untouched = lambda: c.tolist() == [-1] * 4 and m.tolist() == [-1] * 16                                  # noqa: E731

        def raw(axis=2, S=2, levels=lv, u_edges=ue, nu=2, v_edges=ve, nv=1, E_edges=Ee, nE=2, counts=c, maps=m):
            p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
            return lib.pcl_step_plane_flux(dev.ctx, axis, S, p(levels), p(u_edges), nu, p(v_edges), nv, p(E_edges), nE, p(counts), p(maps))

        assert raw() == -3 and untouched()                           # PCL_ERR_STATE: no store
        dev.store_alloc(1000)
        dev.set_count(0)
        assert raw() == 0 and c.tolist() == [0] * 4 and m.tolist() == [0] * 16        # empty store: zeros
        c[:], m[:] = -1, -1
        dev.fill_photons(1000, 0, C_LIT, 1.0, 3.0, 1)
        from test_plane_flux_build_cpu import BAD_CALLS
        names = dict(S="S", levels="levels", u_edges="u_edges", nu="nu", v_edges="v_edges", nv="nv", E_edges="E_edges", nE="nE", axis="axis")
        for kw in BAD_CALLS:
            if "counts" in kw or "maps" in kw:
                assert raw(**kw) == -2, kw
                continue
            assert raw(**{names[k]: v for k, v in kw.items()}) == -2 and untouched(), kw      # PCL_ERR_ARG, before anything is written
        with pytest.raises(hip.HipError):
            dev.plane_flux("z", [1.0, 0.0], [[0, 1], [0, 1]])
        assert raw(E_edges=None, nE=0) == 0                          # r = dr = 0: nothing crosses
        assert c.tolist() == [0] * 4 and m.tolist() == [0] * 8 + [-1] * 8
    finally:
        dev.close()


def test_group_and_multidevice_sum_the_shards(hip):
    from physicl_amd.multidev import MultiDevice
    N = 200_003
    cfg = source_config("z")
    one = hip.Device(0)
    try:
        one.store_alloc(N)
        one.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        one.apply_source(Source, C_LIT, 11)
        one.step_newton(DT)
        one.step_newton(DT)
        want = one.plane_flux(*cfg)
        assert all(np.array_equal(g, w) for g, w in zip(want, restated(downloaded(hip, one), *cfg)))
        assert want[0][0].sum() > 0 and want[0][1].sum() > 0 and want[1].sum() > 0
    finally:
        one.close()
    with hip.DeviceGroup([0, 0]) as g:
        g.store_alloc(N)
        g.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        g.apply_source(Source, C_LIT, 11)
        for i in range(2):
            ctx = ctypes.c_void_p()
            hip.check(g.lib.pcl_group_ctx(g.g, i, ctypes.byref(ctx)))
            hip.check(g.lib.pcl_step_newton(ctx, DT))
            hip.check(g.lib.pcl_step_newton(ctx, DT))
        got = g.plane_flux(*cfg)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        out, maps = np.full(4, -1, np.int64), np.full(8, -1, np.int64)
        bad, e = np.array([1.0, 0.0]), np.array([0.0, 1.0, 2.0])
        assert g.lib.pcl_group_step_plane_flux(g.g, 2, 2, bad.ctypes.data, e.ctypes.data, 2, e.ctypes.data, 1, None, 0, out.ctypes.data, maps.ctypes.data) == -2
        assert out.tolist() == [-1] * 4 and maps.tolist() == [-1] * 8  # checked once for the group, before any shard is asked
    md = MultiDevice([0, 0])
    try:
        md.store_alloc(N)
        md.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        md.apply_source(Source, C_LIT, 11)
        md.step_newton(DT)
        md.step_newton(DT)
        got = md.plane_flux(*cfg)
    finally:
        md.close()
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------------ simulation level
N_SIM, PASSES = 4096, 6
SIM_DT = 0.5 / C_LIT                                                   # half a unit per pass
SIM_EDGES = [np.linspace(0.0, 4.0, 9), np.linspace(-2.0, 2.0, 9), np.linspace(-2.0, 2.0, 9)]
SIM_LEVELS = [1.0, 1.75, 3.5]                                          # x is the vertical; the source stands at x = 2, on no level
SLABS = [[-1e9] + SIM_LEVELS + [1e9]]
STATE = ("R0", "R1", "R2", "V0", "V1", "V2", "DR0", "DR1", "DR2", "DV0", "DV1", "DV2", "E")


def run_sim(with_flux):
    import physicl_amd as phys
    from physicl_amd import light, newton
    ix, iy, iz = np.indices((8, 8, 8))
    cloudy = (iy + iz) % 2 == 0                                        # columns along x, cloudy and clear in a checkerboard
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=lambda s: len(s.ts) >= PASSES)
    src = light.PhotonSource(origin=(2.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), angular="isotropic")
    sim.add_objs(light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    field = light.GridScatterStep(np.where(cloudy, 1.2, 0.0), ("x", "y", "z"), SIM_EDGES)
    flux = light.PlaneFluxMapStep(None, "x", SIM_LEVELS, [np.linspace(-2.0, 2.0, 9)] * 2, E_bins=[1.0, 2.0, 3.0], frames=True)
    here = light.PositionGridMeasureStep(None, ("x",), SLABS)          # beside the flux step: where the move ended
    ground = light.SurfaceReflectStep(100.0, center=(-99.75, 0.0, 0.0), albedo=0.5)      # the ground: a large sphere, its top at x = 0.25
    walls = light.BoxBoundaryStep((0.0, -2.0, -2.0), (0.0, 2.0, 2.0), walls=(None, "periodic", "periodic"))
    end = light.PositionGridMeasureStep(None, ("x",), SLABS)           # behind the ground and the walls: where the next move begins
    steps = [phys.UpdateTimeStep(lambda s: np.double(SIM_DT)), newton.NewtonianKinematicsStep(),
             light.ScatterIsotropicStep(A=np.double(0.5), n=np.double(1.0)), field] + ([flux] if with_flux else []) + [here, ground, walls, end]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    dev = sim._dev
    state = {f: dev.download(getattr(sim._hip, f)) for f in STATE}
    state["id"] = dev.download_ids()
    note = sim.launch_note
    sim.close(download=False)
    rows = {name: [list(r) for r in s.data] for name, s in (("field", field), ("here", here), ("ground", ground), ("walls", walls), ("end", end))}
    return flux, rows, state, note


@pytest.fixture(scope="module")
def sim_runs():
    return {"with": run_sim(True), "without": run_sim(False)}


def test_net_flux_is_the_change_of_the_population_at_or_above_each_level(sim_runs):
    flux, rows, state, note = sim_runs["with"]
    assert note is not None and "one launch per light step" in note
    assert len(flux.data) == PASSES and all(len(r) == 6 and r[1] == N_SIM for r in flux.data)
    above = lambda row: np.cumsum(np.asarray(row[2])[::-1])[::-1][1:]   # noqa: E731  (the slabs from a level up: at or above it)
    start, net = np.array([N_SIM, N_SIM, 0]), np.zeros(3, dtype=np.int64)               # everybody starts at x = 2
    for k in range(PASSES):
        net += np.asarray(flux.data[k][2]) - np.asarray(flux.data[k][3])
        assert np.array_equal(start + net, above(rows["here"][k])), k                      # cumsum(up - down): the population at or above
        # the ground's top is at x = 0.25 and a bounce flies half a unit at the most: nobody passes a level behind the flux step
        assert np.array_equal(above(rows["end"][k]), above(rows["here"][k])), k
    total_up, total_down = (np.sum([r[k] for r in flux.data], axis=0) for k in (2, 3))
    print("up %s down %s over %d passes" % (total_up.tolist(), total_down.tolist(), PASSES))
    assert total_up.min() > 0 and total_down.min() > 0 and sum(int(r[1]) + int(r[2]) for r in rows["ground"]) > 0      # the ground was hit
    for r in flux.data:                                                # every photon has an energy in [1, 3] and the map spans the box: all land
        assert r[4].shape == r[5].shape == (3, 2, 8, 8)
        assert np.all(r[4].sum(axis=(1, 2, 3)) <= r[2]) and np.all(r[5].sum(axis=(1, 2, 3)) <= r[3])
    assert np.array_equal(flux.up_map, np.sum([r[4] for r in flux.data], axis=0))          # the exposure is the sum of the frames
    assert np.array_equal(flux.down_map, np.sum([r[5] for r in flux.data], axis=0)) and flux.up_map.sum() > 0 and flux.down_map.sum() > 0
    assert np.array_equal(flux.up, flux.data[-1][2]) and np.array_equal(flux.down, flux.data[-1][3])


def test_the_step_does_not_disturb_the_run(sim_runs):
    (_, rows_a, state_a, _), (flux_b, rows_b, state_b, note_b) = sim_runs["with"], sim_runs["without"]
    assert flux_b.data == [] and note_b is not None                    # (the writers of the pass need every pass as well)
    for f in state_a:
        assert np.array_equal(state_a[f], state_b[f], equal_nan=True) and state_a[f].tobytes() == state_b[f].tobytes(), f
    for name in rows_a:
        assert len(rows_a[name]) == len(rows_b[name]) == PASSES, name
        for a, b in zip(rows_a[name], rows_b[name]):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), name
