"""GPU: binned plane-crossing energy spectra (pcl_step_plane_spectra, ScatterMeasureStep(measure_E=True, E_bins=...)).

Every result is an integer, so every comparison is an equality: the histogram of a plane equals
``numpy.histogram(Device.plane_energies(plane), edges)`` -- the list form the reference defines, binned the way its scripts
bin it --, the count equals the plane counter of ``step_counters``.  At the simulation level a twin run with the list form
(same seed) gives the lists, and both runs end in the same state.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
C_LIT = 299792458.0
NAN = float("nan")
DT = 0.0005
STEP = C_LIT * DT                      # what an unscattered photon moves per Newton step


def planes_for(n, after_moves=1):
    """n planes mixing the three axes, one of them repeated, around where the photons are after ``after_moves`` moves."""
    x = STEP * after_moves
    pool = [[x * 0.5, NAN, NAN], [NAN, 0.0, NAN], [NAN, NAN, 0.0], [x, NAN, NAN], [x * 0.5, NAN, NAN], [NAN, STEP * 0.1, NAN],
            [x * 2, NAN, NAN], [NAN, NAN, -STEP * 0.2], [x * 0.9, 1.0, 2.0], [NAN, 0.0, 5.0], [0.0, NAN, NAN], [x * 0.25, NAN, NAN]]
    return np.array(pool[:n], dtype=np.float64)


def edges_for(n_bins, kind, lo=1.0, hi=3.0):
    if kind == "uniform":
        return np.linspace(lo + 0.1, hi - 0.1, n_bins + 1)          # some energies fall below and above
    return np.geomspace(lo * 0.9, hi * 0.95, n_bins + 1)


def expect(dev, planes, edges):
    cnt = dev.step_counters(planes)
    hist = np.stack([np.histogram(dev.plane_energies(pl).astype(np.float64), bins=edges)[0] for pl in planes]).astype(np.int64)
    return cnt[4:], hist


def check(dev, planes, edges, what):
    want_c, want_h = expect(dev, planes, edges)
    counts, hist = dev.plane_spectra(planes, edges)
    assert counts.dtype == np.int64 and hist.dtype == np.int64 and hist.shape == (len(planes), len(edges) - 1)
    assert np.array_equal(counts, want_c), (what, counts, want_c)
    assert np.array_equal(hist, want_h), what
    assert np.all(hist.sum(axis=1) <= counts), what
    return counts, hist


def filled(hip, N, dtype, moves=1, seed=11):
    dev = hip.Device(0)
    dev.store_alloc(max(N, 1), dtype)
    dev.fill_photons(N, 0, C_LIT, 1.0, 3.0, seed)
    for _ in range(moves):
        dev.step_newton(DT)
    return dev


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", [1, 63, 64, 2047, 2048, 2049, 3 * 2048 + 5, 1_000_000])
def test_spectra_equal_histogram_of_the_lists_after_a_newton_step(hip, N, dtype):
    dev = filled(hip, N, dtype)
    try:
        for n_planes, n_bins, kind in [(1, 1, "uniform"), (4, 50, "uniform"), (12, 1024, "log"), (4, 50, "log"), (12, 50, "uniform"),
                                       (1, 1024, "uniform")]:
            counts, _ = check(dev, planes_for(n_planes), edges_for(n_bins, kind), (N, dtype, n_planes, n_bins, kind))
        assert counts[0] == N                      # every photon of the bulk population crosses x = half a step
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_spectra_after_a_lazy_fused_step_and_after_a_delete_behind_the_alive_mask(hip, dtype):
    N = 300_000
    dev = filled(hip, N, dtype, moves=0)
    try:
        dev.step_fused(DT, scatter=dict(A=1e-6, n=1.0, flags=0, c=C_LIT, h=0.0, rng_mode=hip.RNG_PHILOX, seed=5, step=1),
                       planes=None, sync=False, lazy=True)         # dr and dv implicit, v in the other half of its buffer
        check(dev, planes_for(4), edges_for(50, "uniform"), ("lazy fused", dtype))
        dev.step_fused(DT, scatter=dict(A=1e-6, n=1.0, flags=0, c=C_LIT, h=0.0, rng_mode=hip.RNG_PHILOX, seed=5, step=2),
                       planes=None, sync=False, lazy=True)
        check(dev, planes_for(12, 2), edges_for(50, "log"), ("second lazy fused", dtype))
        out = dev.step_fused_delete(DT, 1e-6, 1.0, seed=5, step=3, planes=None, lazy=True)     # leaves an alive mask
        assert 0 < out["N"] < N
        counts, hist = dev.plane_spectra(planes_for(4, 3), edges_for(50, "uniform"))           # looks first: densifies itself
        want_c, want_h = expect(dev, planes_for(4, 3), edges_for(50, "uniform"))
        assert np.array_equal(counts, want_c) and np.array_equal(hist, want_h)
        assert dev.count == out["N"]
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_spectra_with_plain_objects_and_against_the_state(hip, dtype):
    """A kind array with plain Objects: they are counted by the plane counter (as step_counters does) and carry no energy.
    The predicate is restated here on the state in the store's precision (r - dr rounded to it, E widened exactly)."""
    N = 50_000
    T = np.float64 if dtype == "f64" else np.float32
    rng = np.random.default_rng(4)
    dev = hip.Device(0)
    try:
        dev.store_alloc(N, dtype)
        dev.set_count(N)
        r, dr = rng.normal(size=(3, N)).astype(T), (rng.normal(size=(3, N)) * 0.5).astype(T)
        E = rng.uniform(0.5, 3.5, N).astype(T)
        E[::97] = np.nan
        edges = np.array([1.0, 1.5, 2.0, 2.25, 3.0])
        E[5::101] = 1.5
        E[7::103] = 3.0                                                     # exactly on an inner edge / on the last edge
        E[9::107] = 1.0
        kind = (rng.random(N) < 0.7).astype(np.uint8)
        for k in range(3):
            dev.upload(hip.R0 + k, r[k])
            dev.upload(hip.DR0 + k, dr[k])
            dev.upload(hip.V0 + k, np.zeros(N))
            dev.upload(hip.DV0 + k, np.zeros(N))
        dev.upload(hip.E, E)
        dev.upload_kind(kind)
        planes = np.array([[0.1, NAN, NAN], [NAN, -0.2, NAN], [NAN, NAN, 0.0], [NAN, -0.2, NAN]])
        counts, hist = check(dev, planes, edges, "objects")
        for p, (ax, L) in enumerate([(0, 0.1), (1, -0.2), (2, 0.0), (1, -0.2)]):
            x, prev, L = r[ax], (r[ax] - dr[ax]).astype(T), T(L)
            cross = ((prev <= L) & (L <= x)) | ((prev >= L) & (L >= x))
            assert counts[p] == np.count_nonzero(cross)
            assert np.array_equal(hist[p], np.histogram(E[cross & (kind != 0)].astype(np.float64), bins=edges)[0])
        assert hist.sum() < counts.sum()
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_spectra_of_a_stop_exactly_on_the_plane(hip, dtype):
    dev = filled(hip, 5000, dtype)
    try:
        x = dev.download(hip.R0)
        assert np.all(x == x[0])
        planes = np.array([[x[0], NAN, NAN], [0.0, NAN, NAN], [np.nextafter(x[0], x.dtype.type(np.inf)), NAN, NAN]], dtype=np.float64)   # stops on it / starts on it / misses
        counts, hist = check(dev, planes, edges_for(50, "uniform"), "on the plane")
        assert counts.tolist() == [5000, 5000, 0]
    finally:
        dev.close()


def test_empty_store_and_refused_calls(hip):
    dev = hip.Device(0)
    try:
        lib = hip.load()
        pl = np.array([[0.0, NAN, NAN]])
        ed = np.array([1.0, 2.0, 3.0])
        c, hst = np.full(1, -1, np.int64), np.full(2, -1, np.int64)

        def raw(planes=pl, n_planes=1, edges=ed, n_bins=2, counts=c, hist=hst):
            p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
            return lib.pcl_step_plane_spectra(dev.ctx, p(planes), n_planes, p(edges), n_bins, p(counts), p(hist))

        assert raw() == -3                                           # PCL_ERR_STATE: no store
        dev.store_alloc(1000)
        dev.set_count(0)
        assert raw() == 0 and c.tolist() == [0] and hst.tolist() == [0, 0]                    # empty store: zeros
        dev.fill_photons(1000, 0, C_LIT, 1.0, 3.0, 1)
        for kw in (dict(planes=None), dict(edges=None), dict(counts=None), dict(hist=None), dict(n_planes=0), dict(n_planes=13),
                   dict(n_bins=0), dict(n_bins=1025), dict(edges=np.array([1.0, 1.0, 2.0])), dict(edges=np.array([1.0, 3.0, 2.0])),
                   dict(edges=np.array([1.0, NAN, 2.0])), dict(edges=np.array([1.0, 2.0, np.inf])), dict(planes=np.array([[NAN, NAN, NAN]]))):
            assert raw(**kw) == -2, kw                                # PCL_ERR_ARG
        with pytest.raises(hip.HipError):
            dev.plane_spectra(pl, [2.0, 1.0])
        assert raw() == 0 and c.tolist() == [1000]                    # r = dr = 0: every photon sits on the plane x = 0 (light.py:386)
    finally:
        dev.close()


def test_group_and_multidevice_sum_the_shards(hip):
    from physicl_amd.multidev import MultiDevice
    N = 200_003
    planes, edges = planes_for(4), edges_for(50, "uniform")
    one = filled(hip, N, "f64")
    try:
        want = one.plane_spectra(planes, edges)
    finally:
        one.close()
    with hip.DeviceGroup([0, 0]) as g:
        g.store_alloc(N)
        g.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        for i in range(2):
            ctx = ctypes.c_void_p()
            hip.check(g.lib.pcl_group_ctx(g.g, i, ctypes.byref(ctx)))
            hip.check(g.lib.pcl_step_newton(ctx, DT))
        got = g.plane_spectra(planes, edges)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    md = MultiDevice([0, 0])
    try:
        md.store_alloc(N)
        md.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        md.step_newton(DT)
        got = md.plane_spectra(planes, edges)
    finally:
        md.close()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------ simulation level
def planck_steps(phys, light, newton, sim, E_bins):
    """The step list of examples/planck_measure.py (without its trace step)."""
    sim.add_step(0, phys.UpdateTimeStep(lambda x: DT))
    sim.add_step(1, newton.NewtonianKinematicsStep())
    sim.add_step(2, light.ScatterSphericalStep(0.00000000000001, 0.000000000000005, wavelength_dep_scattering=True))
    sim.add_step(3, light.ScatterMeasureStep(None, measure_n=True, measure_locs=[[x * C_LIT * DT * 5, 0, 0] for x in range(1, 5)],
                                             measure_E=True, E_bins=E_bins))


def run_planck(make_objs, E_bins, passes=22, **kw):
    import physicl_amd as phys
    from physicl_amd import light, newton
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=lambda s: s.t >= DT * (passes - 0.5), **kw)
    sim.add_objs(make_objs(phys, light))
    planck_steps(phys, light, newton, sim, E_bins)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    dev = sim._dev
    state = {f: dev.download(getattr(sim._hip, f)) for f in ("R0", "R1", "R2", "V0", "V1", "V2", "E")}
    return sim.steps[3].data, state


def assert_binned_rows(binned, lists, edges):
    assert len(binned) == len(lists) > 0
    crossed = 0
    for rb, rl in zip(binned, lists):
        assert rb[0] == rl[0] and rb[1] == rl[1] and len(rb) == len(rl) == 10
        for p in range(4):
            assert rb[2 + 2 * p] == rl[2 + 2 * p]
            want = np.histogram(np.array(rl[3 + 2 * p], dtype=np.float64), bins=edges)[0]
            assert rb[3 + 2 * p].dtype == np.int64 and np.array_equal(rb[3 + 2 * p], want)
            crossed += rl[2 + 2 * p]
    assert crossed > 0


@pytest.mark.parametrize("kw", [{}, {"devices": [0, 0]}], ids=["one_device", "devices_0_0"])
def test_planck_loop_on_a_photon_batch(kw):
    lo, hi = 2e-19, 8e-19                                       # visible light: the scatter is wavelength dependent
    edges = np.linspace(lo, hi * 0.9, 51)
    make = lambda phys, light: phys.PhotonBatch(40_000, lo, hi, seed=3)      # noqa: E731
    lists, state_l = run_planck(make, None)
    binned, state_b = run_planck(make, edges, **kw)
    assert_binned_rows(binned, lists, edges)
    for f in state_l:                      # the measure does not disturb the run (the wavelength-term cache is rebuilt)
        assert np.array_equal(state_l[f], state_b[f]), f


def test_planck_loop_on_explicit_objects():
    lo, hi = 2e-19, 8e-19
    edges = np.geomspace(lo, hi, 51)

    def make(phys, light):
        np.random.seed(5)
        return light.generate_photons(300, min=lo, max=hi)
    lists, state_l = run_planck(make, None)
    binned, state_b = run_planck(make, edges)
    assert_binned_rows(binned, lists, edges)
    for f in state_l:
        assert np.array_equal(state_l[f], state_b[f]), f
