"""GPU: binned position grids (pcl_step_position_grid, PositionGridMeasureStep).

Every result is an integer, so every comparison is an equality: the grid equals the numpy restatement
(tests/grid_reference.py) applied to the downloaded ``r``.  Both accumulation forms (workgroup histograms in LDS / 64-bit
atomics on the device grid) are forced on the same inputs through PCL_GRID_LDS_CELLS.  At the simulation level a twin run with
``steps_per_launch=1`` gives the same rows and ends in the same store, while the run itself keeps its K-pass launches.
"""
import ctypes

import numpy as np
import pytest

from grid_reference import position_grid

pytestmark = pytest.mark.gpu
C_LIT = 299792458.0
DT = 0.0005
STEP = C_LIT * DT                      # what an unscattered photon moves per Newton step
ORIGIN = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP)
FORMS = {"lds": "8192", "global": "0"}


class Source:
    """An isotropic gaussian spot off the origin (what _hip._source reads)."""
    origin, e1, e2, d = ORIGIN, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "gaussian", 0.0, 0.5 * STEP


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


def scatter_kw(hip, step, seed=5):
    return dict(A=3e-6, n=1.0, flags=0, c=C_LIT, h=0.0, rng_mode=hip.RNG_PHILOX, seed=seed, step=step)   # hit probability 0.45 per step


def spread(hip, N, dtype, moves=4, seed=11):
    """Photons from an isotropic spot plus a few Newton + scatter steps: a cloud a few steps wide around ORIGIN."""
    dev = hip.Device(0)
    dev.store_alloc(max(N, 1), dtype)
    dev.fill_photons(N, 0, C_LIT, 1.0, 3.0, seed)
    dev.apply_source(Source, C_LIT, seed)
    for k in range(moves):
        dev.step_fused(DT, scatter=scatter_kw(hip, k + 1), planes=None, sync=False, lazy=False)
    return dev


def positions(hip, dev):
    return np.stack([dev.download(hip.R0 + k) for k in range(3)], 1).astype(np.float64)


def edges_for(axis, n_bins, kind):
    """Edges over part of the cloud (some photons fall below and above), uniform or geometric."""
    if axis == "r":
        return np.linspace(0.3 * STEP, 3.2 * STEP, n_bins + 1) if kind == "uniform" else np.geomspace(0.05 * STEP, 4.0 * STEP, n_bins + 1)
    mid = ORIGIN["xyz".index(axis)]
    if kind == "uniform":
        return np.linspace(mid - 2.5 * STEP, mid + 3.0 * STEP, n_bins + 1)
    return mid - 2.0 * STEP + np.geomspace(0.01 * STEP, 5.0 * STEP, n_bins + 1)


CENTER = (ORIGIN[0] + 0.25 * STEP, ORIGIN[1], ORIGIN[2] - 0.125 * STEP)       # off the origin, and off the source
CASES = [(("x",), (1,), "uniform"), (("x",), (50,), "uniform"), (("x",), (1024,), "geometric"),
         (("r",), (1,), "uniform"), (("r",), (50,), "geometric"), (("r",), (1024,), "uniform"),
         (("y", "z"), (50, 50), "uniform"), (("y", "z"), (1024, 1024), "uniform"),                 # 2^20 cells
         (("x", "y", "z"), (1, 1, 1), "uniform"), (("x", "y", "z"), (16, 16, 16), "geometric"), (("x", "y", "z"), (50, 50, 50), "uniform"),
         (("r", "x"), (50, 50), "uniform"), (("r", "x"), (1024, 4), "geometric"), (("z", "r", "y"), (8, 50, 8), "uniform")]


def check(dev, r, axes, edges, center, monkeypatch, what):
    want = position_grid(r, axes, edges, center)
    cells = want.size
    grids = {}
    for form, value in FORMS.items():
        if form == "lds" and cells > 8192:
            continue
        monkeypatch.setenv("PCL_GRID_LDS_CELLS", value)
        grids[form] = dev.position_grid(axes, edges, center)
    monkeypatch.delenv("PCL_GRID_LDS_CELLS")
    grids["default"] = dev.position_grid(axes, edges, center)
    for form, got in grids.items():
        assert got.dtype == np.int64 and got.shape == want.shape, (what, form)
        assert np.array_equal(got, want), (what, form, int(got.sum()), int(want.sum()))
    return want


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", [1, 63, 64, 2047, 2048, 2049, 3 * 2048 + 5, 1_000_000])
def test_grid_equals_the_restatement_on_a_spread_cloud(hip, N, dtype, monkeypatch):
    dev = spread(hip, N, dtype)
    try:
        r = positions(hip, dev)
        hit = 0
        for axes, bins, kind in CASES:
            edges = [edges_for(a, b, kind) for a, b in zip(axes, bins)]
            want = check(dev, r, axes, edges, CENTER, monkeypatch, (N, dtype, axes, bins, kind))
            assert want.sum() <= N
            hit = max(hit, np.count_nonzero(want))
        assert np.array_equal(positions(hip, dev), r)                       # a measurement: nothing moved
        if N >= 2047:
            assert hit > 500                                                # many cells are hit
        whole = dev.position_grid("x", [[-1e30, 1e30]])
        assert whole.tolist() == [N]
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", [1, 63, 64, 2049, 1_000_000])
def test_one_cell_start(hip, N, dtype, monkeypatch):
    """The untouched fill: every photon at the origin, i.e. in one cell (one add per wave)."""
    dev = hip.Device(0)
    try:
        dev.store_alloc(N, dtype)
        dev.fill_photons(N, 0, C_LIT, 1.0, 3.0, 3)
        for form in ("lds", "global"):
            monkeypatch.setenv("PCL_GRID_LDS_CELLS", FORMS[form])
            g = dev.position_grid(("x", "y", "z"), [np.linspace(-1, 1, 17)] * 3)
            assert g[8, 8, 8] == N == g.sum(), form                          # 0 is the edge between bins 7 and 8: the upper one
            g = dev.position_grid(("r", "x"), [[0.0, 1.0, 2.0], [-1.0, 0.0]])
            assert g.tolist() == [[N], [0]], form                            # q = 0 on the first edge, x = 0 on the last: closed
            assert not dev.position_grid(("y", "z"), [np.linspace(0.5, 1, 65)] * 2).any(), form          # a grid that misses it
            assert not dev.position_grid(("r",), [np.linspace(1, 2, 51)], (0.0, 0.0, 0.0)).any(), form
            g = dev.position_grid(("r",), [np.linspace(1, 2, 51)], (1.5, 0.0, 0.0))                       # q = 2.25, on or beside an edge
            assert g.sum() == N and np.array_equal(g, position_grid(np.zeros((N, 3)), ("r",), [np.linspace(1, 2, 51)], (1.5, 0.0, 0.0))), form
        monkeypatch.setenv("PCL_GRID_LDS_CELLS", "0")
        g = dev.position_grid(("y", "z"), [np.linspace(-1, 1, 1025)] * 2)    # 2^20 cells
        assert g[512, 512] == N == g.sum()
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_store_states_lazy_alive_mask_compaction(hip, dtype, monkeypatch):
    N = 300_000
    dev = spread(hip, N, dtype, moves=2)
    axes, bins = ("r", "x"), (50, 50)
    edges = [edges_for(a, b, "uniform") for a, b in zip(axes, bins)]
    try:
        dev.step_fused(DT, scatter=scatter_kw(hip, 3), planes=None, sync=False, lazy=True)     # dr and dv implicit
        g = dev.position_grid(axes, edges, CENTER)                                              # looks first: materialises itself
        assert np.array_equal(g, position_grid(positions(hip, dev), axes, edges, CENTER))
        check(dev, positions(hip, dev), ("x", "y", "z"), [edges_for(a, 16, "uniform") for a in "xyz"], CENTER, monkeypatch, "lazy")
        out = dev.step_fused_delete(DT, 1e-6, 1.0, seed=5, step=4, planes=None, lazy=True)     # leaves an alive mask
        assert 0 < out["N"] < N
        g = dev.position_grid(axes, edges, CENTER)                                              # looks first: densifies itself
        assert dev.count == out["N"]
        r = positions(hip, dev)
        assert len(r) == out["N"] and np.array_equal(g, position_grid(r, axes, edges, CENTER))
        alive, removed = dev.step_scatter_delete(1e-6, 1.0, hip.RNG_PHILOX, 5, 5)               # a compaction
        assert 0 < alive < out["N"]
        check(dev, positions(hip, dev), axes, edges, CENTER, monkeypatch, "compacted")
        assert dev.position_grid("x", [[-1e30, 1e30]]).tolist() == [alive]
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_plain_objects_count_and_values_on_edges(hip, dtype, monkeypatch):
    N = 50_000
    T = np.float64 if dtype == "f64" else np.float32
    rng = np.random.default_rng(4)
    dev = hip.Device(0)
    try:
        dev.store_alloc(N, dtype)
        dev.set_count(N)
        ex, ey, er = np.array([-1.0, -0.5, 0.0, 0.25, 1.5]), np.linspace(-2, 2, 9), np.array([0.0, 0.5, 1.0, 2.0])
        r = rng.normal(size=(3, N)).astype(T)
        r[0, 5::101] = np.tile(ex, N)[:len(r[0, 5::101])]                   # exactly on inner and outer edges
        r[1, 7::103] = 2.0
        r[0, ::97], r[1, 3::89], r[2, 11::83] = np.nan, np.inf, -np.inf
        r[:, 13::211] = 0.0                                                 # q = 0 about the origin
        for k in range(3):
            dev.upload(hip.R0 + k, r[k])
            for f in (hip.V0, hip.DR0, hip.DV0):
                dev.upload(f + k, np.zeros(N))
        dev.upload(hip.E, np.ones(N))
        dev.upload_kind((rng.random(N) < 0.7).astype(np.uint8))             # plain Objects among them: they count
        rr = r.T.astype(np.float64)
        for axes, edges, center in [(("x",), [ex], None), (("x", "y"), [ex, ey], None), (("r",), [er], (0.0, 0.0, 0.0)),
                                    (("r", "y", "x"), [er, ey, ex], (0.5, -0.25, 0.125))]:
            want = check(dev, rr, axes, edges, center if center is not None else (0.0, 0.0, 0.0), monkeypatch, axes)
            assert 0 < want.sum() < N
            if center is None:
                assert np.array_equal(dev.position_grid(axes, edges), want)          # no centre: the origin
        finite = np.all(np.isfinite(rr[:, :2]), axis=1)
        assert np.array_equal(dev.position_grid(("x", "y"), [ex, ey]), np.histogramdd(rr[finite][:, :2], bins=[ex, ey])[0].astype(np.int64))
    finally:
        dev.close()


def test_empty_store_and_refused_calls(hip):
    dev = hip.Device(0)
    try:
        lib = hip.load()
        co, nb = np.array([0, 3], dtype=np.int32), np.array([2, 1], dtype=np.int32)
        ed, ce = np.array([0.0, 1.0, 2.0, 0.0, 5.0]), np.array([0.0, 0.0, 0.0])
        out = np.full(2, -1, np.int64)

        def raw(n_axes=2, coords=co, n_bins=nb, edges=ed, center=ce, grid=out):
            p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
            return lib.pcl_step_position_grid(dev.ctx, n_axes, p(coords), p(n_bins), p(edges), p(center), p(grid))

        assert raw() == -3 and out.tolist() == [-1, -1]               # PCL_ERR_STATE: no store
        dev.store_alloc(1000)
        dev.set_count(0)
        assert raw() == 0 and out.tolist() == [0, 0]                  # empty store: zeros
        dev.fill_photons(1000, 0, C_LIT, 1.0, 3.0, 1)
        out[:] = -1
        i32, f64 = lambda *a: np.array(a, dtype=np.int32), lambda *a: np.array(a, dtype=np.float64)      # noqa: E731
        big = np.arange(1025.0)
        for kw in (dict(coords=None), dict(n_bins=None), dict(edges=None), dict(grid=None), dict(n_axes=0), dict(n_axes=4), dict(n_axes=-1),
                   dict(coords=i32(0, 4)), dict(coords=i32(-1, 3)), dict(coords=i32(0, 0)), dict(coords=i32(3, 3)),
                   dict(n_bins=i32(0, 1)), dict(n_bins=i32(2, 1025)), dict(n_bins=i32(-2, 1)),
                   dict(n_axes=3, coords=i32(0, 1, 2), n_bins=i32(1024, 1024, 2), edges=np.concatenate([big, big, big[:3]])),   # 2^21 cells
                   dict(edges=f64(0, 0, 2, 0, 5)), dict(edges=f64(0, 3, 2, 0, 5)), dict(edges=f64(0, np.nan, 2, 0, 5)), dict(edges=f64(0, 1, np.inf, 0, 5)),
                   dict(edges=f64(0, 1, 2, -1, 5)), dict(edges=f64(0, 1, 2, 0, 1e200)), dict(edges=f64(0, 1, 2, 1e-200, 2e-200)), dict(edges=f64(0, 1, 2, 5, 5)),
                   dict(center=f64(0, np.nan, 0)), dict(center=f64(np.inf, 0, 0))):
            assert raw(**kw) == -2, kw                                # PCL_ERR_ARG
            assert out.tolist() == [-1, -1], kw                       # ... and nothing was written
        with pytest.raises(hip.HipError):
            dev.position_grid(("x",), [[2.0, 1.0]])
        assert raw(center=None) == 0 and out.tolist() == [1000, 0]    # x = 0 in [0, 1), q = 0 in [0, 25]; NULL centre = the origin
        with hip.DeviceGroup([0, 0]) as g:
            out[:] = -1
            p = lambda a: a.ctypes.data                               # noqa: E731
            assert lib.pcl_group_step_position_grid(g.g, 2, p(i32(0, 0)), p(nb), p(ed), p(ce), p(out)) == -2 and out.tolist() == [-1, -1]
            assert lib.pcl_group_step_position_grid(g.g, 2, p(co), p(nb), p(ed), p(ce), p(out)) == -3 and out.tolist() == [-1, -1]
    finally:
        dev.close()


def test_group_and_multidevice_sum_the_shards(hip, monkeypatch):
    from physicl_amd.multidev import MultiDevice
    N = 200_003
    axes = ("x", "y", "z")
    edges = [np.linspace(ORIGIN[k] - 2.5 * STEP, ORIGIN[k] + 2.0 * STEP, 17) for k in range(3)]

    def one_device():
        dev = hip.Device(0)
        try:
            dev.store_alloc(N)
            dev.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
            dev.apply_source(Source, C_LIT, 11)
            dev.step_newton(DT)
            dev.step_newton(DT)
            return dev.position_grid(axes, edges), dev.position_grid(("r",), [np.linspace(0, 4 * STEP, 1025)], ORIGIN), positions(hip, dev)
        finally:
            dev.close()
    want, want_r, r = one_device()
    assert np.array_equal(want, position_grid(r, axes, edges)) and np.count_nonzero(want) > 500 and 0 < want.sum() < N
    for form in ("lds", "global"):
        monkeypatch.setenv("PCL_GRID_LDS_CELLS", FORMS[form])
        with hip.DeviceGroup([0, 0]) as g:
            g.store_alloc(N)
            g.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
            g.apply_source(Source, C_LIT, 11)
            for i in range(2):
                ctx = ctypes.c_void_p()
                hip.check(g.lib.pcl_group_ctx(g.g, i, ctypes.byref(ctx)))
                hip.check(g.lib.pcl_step_newton(ctx, DT))
                hip.check(g.lib.pcl_step_newton(ctx, DT))
            assert np.array_equal(g.position_grid(axes, edges), want), form
            assert np.array_equal(g.position_grid(("r",), [np.linspace(0, 4 * STEP, 1025)], ORIGIN), want_r), form
    md = MultiDevice([0, 0])
    try:
        md.store_alloc(N)
        md.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        md.apply_source(Source, C_LIT, 11)
        md.step_newton(DT)
        md.step_newton(DT)
        assert np.array_equal(md.position_grid(axes, edges), want)
    finally:
        md.close()


# ------------------------------------------------------------------------------------------------ simulation level
def grid_steps(light):
    """Two snapshot steps on different rhythms: an image every ``every`` passes and a radius profile on every other record."""
    image = lambda every: light.PositionGridMeasureStep(None, ("y", "z"), [np.linspace(-30 * STEP, 30 * STEP, 65)] * 2, every=every)      # noqa: E731
    shells = lambda every: light.PositionGridMeasureStep(None, ("r",), [np.linspace(0, 120 * STEP, 101)], center=ORIGIN, every=every,     # noqa: E731
                                                         measure_n=False)
    return image, shells


def run_loop(loop, every, passes, place="last", with_grid=True, **kw):
    import physicl_amd as phys
    from physicl_amd import light, newton
    exit_fn = (lambda s: len(s.objects) == 0) if loop == "delete" else (lambda s: s.t >= DT * (passes - 0.5))
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=exit_fn, **kw)
    sim.add_objs(light.generate_photons_bulk(40_000, min=1.0, max=3.0, seed=3, source=light.PhotonSource(origin=ORIGIN, angular="isotropic")))
    image, shells = grid_steps(light)
    grids = [image(every), shells(2 * every)] if with_grid else []
    steps = [phys.UpdateTimeStep(lambda x: DT), newton.NewtonianKinematicsStep()]
    if loop in ("scatter", "mixed"):
        steps += [light.ScatterIsotropicStep(n=1.0, A=3e-7), light.ScatterSignMeasureStep(None)]
        if place == "middle":
            steps += grids
    if loop == "mixed":
        steps += [newton.NewtonianKinematicsStep()]
    if loop in ("delete", "mixed"):
        steps += [light.ScatterDeleteStep(1.0, 3e-7 if loop == "delete" else 2e-8)]
    if loop == "delete":
        steps += [light.ScatterMeasureStep(None, True, [[ORIGIN[0] + 5 * STEP, np.nan, np.nan]])]
    if place == "last":
        steps += grids
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    dev = sim._dev
    state = {f: dev.download(getattr(sim._hip, f)) for f in ("R0", "R1", "R2", "V0", "V1", "V2", "E")}
    state["id"] = dev.download_ids()
    rows = [[list(r) for r in g.data] for g in grids]
    counters = [np.array(s.data) for s in steps if getattr(s, "_fuse_role", None) == "measure"]
    sim.close(download=False)
    return sim, rows, counters, state


def assert_same_run(a, b):
    (_, rows_a, cnt_a, st_a), (_, rows_b, cnt_b, st_b) = a, b
    assert len(rows_a) == len(rows_b)
    for ga, gb in zip(rows_a, rows_b):
        assert len(ga) == len(gb)
        for ra, rb in zip(ga, gb):
            assert len(ra) == len(rb) and all(np.array_equal(x, y) for x, y in zip(ra, rb))
    for ca, cb in zip(cnt_a, cnt_b):
        assert np.array_equal(ca, cb)
    for f in st_a:
        assert np.array_equal(st_a[f], st_b[f]), f


@pytest.mark.parametrize("every", [8, 32])
@pytest.mark.parametrize("loop", ["scatter", "delete", "mixed"])
def test_k_schedule_is_kept_and_rows_equal_the_one_launch_twin(loop, every):
    passes = 200 if loop == "scatter" else 72
    run = run_loop(loop, every, passes)
    twin = run_loop(loop, every, passes, steps_per_launch=1)
    assert_same_run(run, twin)
    sim, rows, counters, state = run
    n_pass = len(sim.ts)
    assert len(rows[0]) == n_pass // every and len(rows[1]) == n_pass // (2 * every) and n_pass == len(twin[0].ts)
    assert sim.launch_note is None and twin[0].launch_note is None
    for k, row in enumerate(rows[0]):
        t, n, grid = row
        assert t == sim.ts[(k + 1) * every - 1] and grid.shape == (64, 64) and grid.dtype == np.int64 and grid.sum() <= n
    assert all(len(row) == 2 and row[1].shape == (100,) for row in rows[1])
    if loop == "scatter":
        assert n_pass == 200 and dict(sim.schedule) == {"fused_multi": 25 if every == 8 else 7}      # 200 = 6 x 32 + 8: 7 launches, 6 rows
        assert dict(twin[0].schedule) == {"fused": 200} and max(np.count_nonzero(row[2]) for row in rows[0]) > 500
        if n_pass % every == 0:                                      # the last pass recorded: the grid of the final store
            assert np.array_equal(rows[0][-1][2], position_grid(np.stack([state["R0"], state["R1"], state["R2"]], 1), ("y", "z"),
                                                                [np.linspace(-30 * STEP, 30 * STEP, 65)] * 2))
    elif loop == "delete":
        assert len(state["E"]) == 0 and n_pass > 2 * every and set(twin[0].schedule) == {"fused_delete"}
        assert sim.schedule["fused_delete_multi"] >= n_pass // every and sim.schedule["fused_delete_multi"] + sim.schedule["fused_delete"] < n_pass / 4
        assert rows[0][0][1] > 0 and rows[0][0][2].sum() > 0
    else:
        assert n_pass == 72 and dict(sim.schedule) == {"mixed_multi": 9 if every == 8 else 3}       # 72 = 2 x 32 + 8
        assert set(twin[0].schedule) == {"fused", "fused_delete"} and 0 < len(state["E"]) < 40_000


def test_sharded_inside_the_process_and_a_step_before_the_last_light_step():
    base = run_loop("mixed", 8, 40, steps_per_launch=1)
    two = run_loop("mixed", 8, 40, devices=[0, 0])
    assert_same_run(two, base)
    assert dict(two[0].schedule) == {"mixed_multi": 5}
    mid = run_loop("mixed", 8, 40, place="middle")
    twin = run_loop("mixed", 8, 40, place="middle", steps_per_launch=1)
    assert_same_run(mid, twin)
    assert "PositionGridMeasureStep" in mid[0].launch_note and set(mid[0].schedule) == {"fused", "fused_delete"}
    assert len(mid[1][0]) == 5 and mid[1][0][-1][2].sum() > 0
    # the snapshot in the middle saw the store before the delete phase of its pass: never fewer photons than the one at the end
    assert all(m[1] >= b[1] for m, b in zip(mid[1][0], base[1][0])) and any(m[1] > b[1] for m, b in zip(mid[1][0], base[1][0]))


def test_a_run_without_the_step_keeps_its_schedule():
    sim, rows, counters, _ = run_loop("scatter", 8, 200, with_grid=False)
    assert rows == [] and dict(sim.schedule) == {"fused_multi": 7} and sim.launch_note is None and len(counters[0]) == 200
    sim, _, counters, _ = run_loop("mixed", 8, 72, with_grid=False)
    assert dict(sim.schedule) == {"mixed_multi": 3} and sim.launch_note is None          # 32 passes x 2 phases per launch
    sim, _, counters, state = run_loop("delete", 8, 0, with_grid=False)
    assert set(sim.schedule) == {"fused_delete_multi"} and len(state["E"]) == 0
