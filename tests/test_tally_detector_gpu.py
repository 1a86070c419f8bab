"""GPU: the detector's image (pcl_step_detector_image, DetectorMeasureStep).

Every result is an integer, so every comparison is an equality: the two counts and every image cell equal the numpy restatement
(light._detector_image, held against a per-particle loop in tests/test_detector_cpu.py) applied to the state that was uploaded
(or downloaded) in the store's precision.  Before anything is compared the restatement's own answer is held to be worth
comparing with: somebody through, fewer seen, more than one cell lit.
"""
import ctypes

import numpy as np
import pytest

from detector_reference import configs, geometry, scene

pytestmark = pytest.mark.gpu
C_LIT = 299792458.0
DT = 0.0005
STEP = C_LIT * DT
SIZES = [1, 63, 64, 65, 2047, 2048, 2049, 4097]              # around a wave and around a tile of the slab


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


def restated(st, cfg):
    from physicl_amd import light
    return light._detector_image(*st, **cfg)


def uploaded(hip, st, dtype, capacity=None):
    r, dr, E, photon = st
    N = len(E)
    dev = hip.Device(0)
    dev.store_alloc(capacity or max(N, 1), dtype)
    dev.set_count(N)
    for k in range(3):
        dev.upload(hip.R0 + k, r[:, k])
        dev.upload(hip.DR0 + k, dr[:, k])
        dev.upload(hip.V0 + k, np.zeros(N))
        dev.upload(hip.DV0 + k, np.zeros(N))
    dev.upload(hip.E, E)
    if not photon.all():
        dev.upload_kind(photon.astype(np.uint8))
    return dev


def worth_comparing(want, N, cfg):
    """The restatement's answer itself: no case passes on zeros."""
    counts, image = want
    assert image.sum() <= counts[1] <= counts[0] <= N
    if N >= 64:
        assert 0 < counts[1] < counts[0] < N, counts
        assert np.count_nonzero(image) >= min(2, image.size), np.count_nonzero(image)      # (a 1 x 1 image without bands has one cell)


def check(dev, st, cfg, what):
    want = restated(st, cfg)
    worth_comparing(want, len(st[2]), cfg)
    counts, image = dev.detector_image(cfg["position"], cfg["frame"], cfg["radius"], cfg["x_edges"], cfg["y_edges"], cfg["E_edges"])
    assert counts.dtype == image.dtype == np.int64 and counts.shape == (2,) and image.shape == want[1].shape, what
    assert counts.tolist() == want[0].tolist(), what
    assert np.array_equal(image, want[1]), what
    return counts, image


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("aperture", ["aligned", "tilted"])
def test_counts_and_image_equal_the_restatement(hip, aperture, N, dtype):
    """One upload per aperture; every configuration that looks through it: 33 x 17 and 1 x 1, with bands and without."""
    names = [name for name in sorted(configs()) if geometry(name) == aperture]
    st = scene(N, dtype, names[0])
    dev = uploaded(hip, st, dtype)
    try:
        assert len(names) >= 2
        for name in names:
            check(dev, st, configs()[name], (name, N, dtype))
    finally:
        dev.close()


def test_the_planted_cases_on_the_device(hip):
    """The slots that hold the planted cases alone (tests/detector_reference.py says what each is), against the hand-made answer."""
    from detector_reference import planted_answers, planted_state
    for name, bands in (("aligned_33x17_bands", True), ("aligned_33x17", False)):
        cfg = configs()[name]
        for dtype in ("f64", "f32"):
            T = np.float64 if dtype == "f64" else np.float32
            st = planted_state(cfg)
            st = tuple(a.astype(T) for a in st[:3]) + (st[3],)
            dev = uploaded(hip, st, dtype)
            try:
                counts, image = dev.detector_image(cfg["position"], cfg["frame"], cfg["radius"], cfg["x_edges"], cfg["y_edges"], cfg["E_edges"])
            finally:
                dev.close()
            through, seen, cells = planted_answers(bands)
            want = np.zeros_like(image)
            for cell, k in cells.items():
                want[cell] = k
            assert counts.tolist() == [through, seen] and np.array_equal(image, want), (name, dtype)


class Source:
    """An isotropic gaussian spot (what _hip._source reads)."""
    origin, e1, e2, d = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "gaussian", 0.0, 0.5 * STEP


def camera(bands):
    """A camera two moves from the spot, looking back at it past its side."""
    from physicl_amd import light
    position = np.array(Source.origin) + np.array([1.5, 0.75, -0.5]) * STEP
    hx, hy = np.tan(0.5), np.tan(0.35)                                # narrower than the spot and the disc make the pencil: not all are seen
    return dict(position=position, frame=light._detector_frame((-1.5, -0.6, 0.7), (0.1, 0.2, 1.0)), radius=0.8 * STEP,
                x_edges=np.linspace(-hx, hx, 34), y_edges=np.linspace(-hy, hy, 18), E_edges=np.linspace(1.2, 2.8, 6) if bands else None)


def downloaded(hip, dev):
    r = np.stack([dev.download(hip.R0 + k) for k in range(3)], 1)
    dr = np.stack([dev.download(hip.DR0 + k) for k in range(3)], 1)
    E = dev.download(hip.E)
    return r, dr, E, np.ones(len(E), dtype=bool)


def call(dev, cfg):
    return dev.detector_image(cfg["position"], cfg["frame"], cfg["radius"], cfg["x_edges"], cfg["y_edges"], cfg["E_edges"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_behind_a_lazy_fused_step_where_dr_is_implicit(hip, dtype):
    N = 20_001
    dev = hip.Device(0)
    try:
        dev.store_alloc(N, dtype)
        dev.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        dev.apply_source(Source, C_LIT, 11)
        kw = dict(A=3e-6, n=1.0, flags=0, c=C_LIT, h=0.0, rng_mode=hip.RNG_PHILOX, seed=5)
        for step in (1, 2):
            dev.step_fused(DT, scatter=dict(kw, step=step), planes=None, sync=False, lazy=True)       # dr implicit
        for bands in (True, False):
            cfg = camera(bands)
            got = call(dev, cfg)                                       # looks first: makes dr real
            want = restated(downloaded(hip, dev), cfg)
            worth_comparing(want, N, cfg)
            assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1]), bands
    finally:
        dev.close()


def test_group_of_two_contexts_and_multidevice_sum_the_shards(hip):
    from physicl_amd.multidev import MultiDevice
    N = 20_003
    cfg = camera(True)
    one = hip.Device(0)
    try:
        one.store_alloc(N)
        one.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        one.apply_source(Source, C_LIT, 11)
        one.step_newton(DT)
        one.step_newton(DT)
        want = call(one, cfg)
        ref = restated(downloaded(hip, one), cfg)
        worth_comparing(ref, N, cfg)
        assert want[0].tolist() == ref[0].tolist() and np.array_equal(want[1], ref[1])
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
        got = call(g, cfg)
        assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1])
        counts, image = np.full(2, -1, np.int64), np.full(4, -1, np.int64)
        p = np.array([0.0, 0.0, 0.0])
        f, e = np.eye(3).reshape(-1), np.array([-1.0, 0.0, 1.0])
        assert g.lib.pcl_group_step_detector_image(g.g, p.ctypes.data, f.ctypes.data, ctypes.c_double(-1.0), e.ctypes.data, 2, e.ctypes.data, 2,
                                                   None, 0, counts.ctypes.data, image.ctypes.data) == -2
        assert counts.tolist() == [-1] * 2 and image.tolist() == [-1] * 4      # checked once for the group, before any shard is asked
    md = MultiDevice([0, 0])
    try:
        md.store_alloc(N)
        md.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        md.apply_source(Source, C_LIT, 11)
        md.step_newton(DT)
        md.step_newton(DT)
        got = call(md, cfg)
    finally:
        md.close()
    assert got[0].tolist() == want[0].tolist() and np.array_equal(got[1], want[1])


def test_empty_store_no_store_and_refused_calls(hip):
    dev = hip.Device(0)
    try:
        lib = hip.load()
        p, f, e, b = np.array([0.0, 0.0, 0.0]), np.eye(3).reshape(-1), np.array([-1.0, 0.0, 1.0]), np.array([1.0, 2.0, 3.0])
        counts, image = np.full(2, -1, np.int64), np.full(8, -1, np.int64)

        def raw(radius=1.0, nx=2, nE=2, E_edges=b):
            return lib.pcl_step_detector_image(dev.ctx, p.ctypes.data, f.ctypes.data, ctypes.c_double(radius), e.ctypes.data, nx, e.ctypes.data, 2,
                                               None if E_edges is None else E_edges.ctypes.data, nE, counts.ctypes.data, image.ctypes.data)
        untouched = lambda: counts.tolist() == [-1] * 2 and image.tolist() == [-1] * 8          # noqa: E731
        assert raw() == -3 and untouched()                           # PCL_ERR_STATE: no store
        dev.store_alloc(1000)
        dev.set_count(0)
        assert raw() == 0 and counts.tolist() == [0] * 2 and image.tolist() == [0] * 8           # empty store: zeros
        counts[:], image[:] = -1, -1
        dev.fill_photons(1000, 0, C_LIT, 1.0, 3.0, 1)
        for kw in (dict(radius=0.0), dict(nx=0), dict(nE=-1), dict(E_edges=None)):
            assert raw(**kw) == -2 and untouched(), kw               # PCL_ERR_ARG, before anything is written
        assert raw(nE=0, E_edges=None) == 0                          # r = dr = 0: nobody moved, nobody is through
        assert counts.tolist() == [0, 0] and image.tolist() == [0] * 4 + [-1] * 4
        with pytest.raises(hip.HipError):
            dev.detector_image(p, f, 1.0, [1.0, 0.0], e)
    finally:
        dev.close()


# ------------------------------------------------------------------------------------------------ simulation level
N_SIM, PASSES = 4097, 6


def run_sim(devices=None):
    import physicl_amd as phys
    from physicl_amd import light, newton

    class Behind(phys.DeviceStep):
        """The store as it stands behind the camera, pass by pass."""
        _fuse_role = None

        def __init__(self):
            self.states = []

        def _device_run(self, sim):
            self.states.append({f: sim.download(f) for f in ("r", "dr", "E")})
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, devices=devices, exit=lambda s: len(s.ts) >= PASSES)
    sim.add_objs(light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=3, source=light.PhotonSource(origin=(0.0, 0.0, 0.0), angular="isotropic")))
    cam = light.DetectorMeasureStep(None, position=(2.0 * STEP, 0.5 * STEP, -0.25 * STEP), normal=(-1.0, -0.3, 0.2), radius=1.25 * STEP,
                                    pixels=(12, 9), fov=(1.1, 0.9), E_bins=np.linspace(1.0, 3.0, 4), frames=True)
    look = Behind()
    steps = [phys.UpdateTimeStep(lambda x: DT), newton.NewtonianKinematicsStep(), light.ScatterIsotropicStep(n=1.0, A=3e-6), cam, look]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    note = sim.launch_note
    sim.close(download=False)
    return cam, look, note


@pytest.fixture(scope="module")
def sim_run():
    return run_sim()


def test_every_pass_s_row_is_the_restatement_of_the_store_behind_it(sim_run):
    from physicl_amd import light
    cam, look, note = sim_run
    assert len(cam.data) == len(look.states) == PASSES and "DetectorMeasureStep" in note and note.startswith("one launch per light step")
    exposure = np.zeros_like(cam.image)
    for row, st in zip(cam.data, look.states):
        counts, image = light._detector_image(st["r"], st["dr"], st["E"], np.ones(N_SIM, dtype=bool), cam.position, cam.frame, cam.radius,
                                              cam.x_edges, cam.y_edges, cam.E_bins)
        assert len(row) == 5 and row[1] == N_SIM and [row[2], row[3]] == counts.tolist() and np.array_equal(row[4], image)
        exposure += row[4]
    assert np.array_equal(cam.image, exposure) and cam.image.shape == (3, 9, 12) and cam.image.dtype == np.int64
    through, seen = sum(r[2] for r in cam.data), sum(r[3] for r in cam.data)
    assert 0 < cam.image.sum() <= seen <= through and np.count_nonzero(cam.image) >= 2 and (cam.through, cam.seen) == (cam.data[-1][2], cam.data[-1][3])


def test_sharded_inside_the_process_gives_the_same_rows(hip, sim_run):
    n = max(1, hip.device_count())
    cam, _, note = run_sim(devices=[i % n for i in range(2)])
    want = sim_run[0]
    assert len(cam.data) == PASSES and "DetectorMeasureStep" in note and np.array_equal(cam.image, want.image)
    for a, b in zip(cam.data, want.data):
        assert list(a[:4]) == list(b[:4]) and np.array_equal(a[4], b[4])
