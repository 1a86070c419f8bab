"""GPU: spherical-shell crossing tallies (pcl_step_shell_crossings, ShellCrossingMeasureStep).

Every result is an integer, so every comparison is an equality: counts and histograms equal the numpy restatement
(tests/shell_reference.py) applied to the state that was uploaded (or downloaded) in the store's precision.  At the simulation
level the tallies are checked against a conservation law: per shell, cumsum(out - in) over the passes is the change of the
number of particles outside the sphere, which a PositionGridMeasureStep counts independently.
"""
import ctypes

import numpy as np
import pytest

from shell_reference import EDGE_RADII, E_EDGES, MU_EDGES, assert_edge_case_tallies, edge_cases, shell_crossings

pytestmark = pytest.mark.gpu
NAN = float("nan")
CENTER = (0.25, -0.5, 1.0)
RADII16 = [1.5, 0.75, 3.0, 2.0, 0.1, 0.5, 1.0, 1.25, 1.75, 2.25, 2.5, 2.75, 3.5, 4.0, 5.0, 0.25]        # in no order
C_LIT = 299792458.0
DT = 0.0005
STEP = C_LIT * DT


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


_STATES = {}


def state(N, dtype, objects=False):
    """(r, dr, E, photon) in the store's precision, made once per (N, dtype): a cloud around CENTER whose moves cross the
    shells of RADII16 both ways, with dr = 0, NaN coordinates and energies on, beside and outside the edges of E_EDGES."""
    key = (N, dtype, objects)
    if key not in _STATES:
        T = np.float64 if dtype == "f64" else np.float32
        rng = np.random.default_rng(N % 1000 + 7)
        r = (rng.normal(size=(N, 3)) * 1.5 + CENTER).astype(T)
        dr = (rng.normal(size=(N, 3)) * (0.8 if N < 100_000 else 0.05)).astype(T)     # (the big store: a twentieth crosses, to keep numpy quick)
        dr[3::17] = 0
        r[5::41, 1] = NAN
        E = rng.uniform(0.5, 3.5, N).astype(T)
        E[1::29], E[2::31], E[4::37], E[6::43] = 1.0, 2.0, 3.0, NAN
        photon = rng.random(N) < 0.7 if objects else np.ones(N, dtype=bool)
        _STATES[key] = (r, dr, E, photon)
    return _STATES[key]


def uploaded(hip, st, dtype, capacity=None, ids=None):
    r, dr, E, photon = st
    N = len(E)
    dev = hip.Device(0)
    dev.store_alloc(max(capacity or N, 1), dtype)
    dev.set_count(N)
    for k in range(3):
        dev.upload(hip.R0 + k, r[:, k])
        dev.upload(hip.DR0 + k, dr[:, k])
        dev.upload(hip.V0 + k, np.zeros(N))
        dev.upload(hip.DV0 + k, np.zeros(N))
    dev.upload(hip.E, E)
    if ids is not None:
        dev.upload_ids(ids)
    if not photon.all():
        dev.upload_kind(photon.astype(np.uint8))
    return dev


def check(dev, st, radii, center, E_edges, mu_edges, what):
    want = shell_crossings(*st, radii, (0, 0, 0) if center is None else center, E_edges, mu_edges)
    got = dev.shell_crossings(radii, center, E_edges, mu_edges)
    assert got[0].dtype == np.int64 and got[0].shape == (2, len(radii))
    for g, w, name in zip(got, want, ("counts", "E_hist", "mu_hist")):
        assert (g is None) == (w is None), (what, name)
        if g is not None:
            assert g.dtype == np.int64 and g.shape == w.shape and np.array_equal(g, w), (what, name)
    return got


def configs():
    """(radii, centre, E edges, mu edges): counts only; E only; mu only; both; S = 1 and 16; 1024 bins and the 8192-cell limit."""
    e50, m20 = np.linspace(0.8, 3.2, 51), np.linspace(-1, 1, 21)
    out = [(RADII16[:1], CENTER, None, None), (RADII16, CENTER, None, None), (RADII16[:4], None, None, None),
           (RADII16[:4], CENTER, e50, None), (RADII16[:4], CENTER, None, m20), (RADII16[:4], CENTER, e50, m20),
           (RADII16, CENTER, E_EDGES, MU_EDGES), (RADII16, CENTER, np.geomspace(0.9, 3.0, 129), np.linspace(-1, 1, 129))]   # 16 shells x 256: the limit
    out += [(RADII16[:1], CENTER, np.linspace(0.8, 3.2, 1025), np.linspace(-1, 1, 1025)),                 # 1024 bins each
            (RADII16[:4], CENTER, np.geomspace(0.9, 3.0, 1025), None),                                    # 4 x 1024 x 2 = 8192 cells: the limit
            (RADII16[:4], CENTER, None, np.linspace(-0.9, 1, 1025))]
    return out


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 2047, 2048, 2049, 3 * 2048 + 5, 600_011])
def test_tallies_equal_the_restatement(hip, N, dtype):
    st = state(N, dtype)
    dev = uploaded(hip, st, dtype, capacity=5 * 2048 if N == 3 * 2048 + 5 else None)
    try:
        for k, (radii, center, E_edges, mu_edges) in enumerate(configs()):
            counts, E_hist, mu_hist = check(dev, st, radii, center, E_edges, mu_edges, (N, dtype, k))
        if N >= 2047:
            assert counts.sum() > 0 and mu_hist.sum() > 0
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_explicit_ids_and_plain_objects(hip, dtype):
    """A store with ids of its own and plain Objects among the photons: they count, cross and have a direction, and no E."""
    N = 50_001
    st = state(N, dtype, objects=True)
    dev = uploaded(hip, st, dtype, ids=np.arange(N, dtype=np.int64)[::-1] * 3 + 11)
    try:
        counts, E_hist, mu_hist = check(dev, st, RADII16[:4], CENTER, np.linspace(0.8, 3.2, 51), np.linspace(-1, 1, 21), dtype)
        only_photons = shell_crossings(st[0][st[3]], st[1][st[3]], st[2][st[3]], st[3][st[3]], RADII16[:4], CENTER, np.linspace(0.8, 3.2, 51))
        assert np.array_equal(E_hist, only_photons[1]) and np.all(counts > only_photons[0]) and E_hist.sum() < mu_hist.sum()
        check(dev, st, RADII16, CENTER, None, None, dtype)      # counts only: no kind bytes are needed
    finally:
        dev.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_hand_made_edge_cases(hip, dtype):
    st = edge_cases()
    T = np.float64 if dtype == "f64" else np.float32
    st = tuple(a.astype(T) for a in st[:3]) + (st[3],)
    dev = uploaded(hip, st, dtype)
    try:
        assert_edge_case_tallies(*check(dev, st, EDGE_RADII, (0.0, 0.0, 0.0), E_EDGES, MU_EDGES, dtype))
        assert_edge_case_tallies(*check(dev, st, EDGE_RADII, None, E_EDGES, MU_EDGES, dtype))          # no centre: the origin
    finally:
        dev.close()


class Source:
    """An isotropic gaussian spot off the centre (what _hip._source reads)."""
    origin, e1, e2, d = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "gaussian", 0.0, 0.5 * STEP


def downloaded(hip, dev):
    r = np.stack([dev.download(hip.R0 + k) for k in range(3)], 1)
    dr = np.stack([dev.download(hip.DR0 + k) for k in range(3)], 1)
    E = dev.download(hip.E)
    return r, dr, E, np.ones(len(E), dtype=bool)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_after_lazy_fused_steps_and_behind_the_alive_mask_of_a_delete(hip, dtype):
    N = 300_000
    dev = hip.Device(0)
    try:
        dev.store_alloc(N, dtype)
        dev.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        dev.apply_source(Source, C_LIT, 11)
        radii = [0.5 * STEP, 1.0 * STEP, 1.5 * STEP, 2.5 * STEP]
        kw = dict(A=3e-6, n=1.0, flags=0, c=C_LIT, h=0.0, rng_mode=hip.RNG_PHILOX, seed=5)
        for step in (1, 2):
            dev.step_fused(DT, scatter=dict(kw, step=step), planes=None, sync=False, lazy=True)       # dr implicit
        got = dev.shell_crossings(radii, Source.origin, np.linspace(1.1, 2.9, 51), np.linspace(-1, 1, 21))   # looks first: makes dr real
        want = shell_crossings(*downloaded(hip, dev), radii, Source.origin, np.linspace(1.1, 2.9, 51), np.linspace(-1, 1, 21))
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[0][0].sum() > 0 and got[0][1].sum() > 0
        out = dev.step_fused_delete(DT, 1e-6, 1.0, seed=5, step=3, planes=None, lazy=True)             # leaves an alive mask
        assert 0 < out["N"] < N
        got = dev.shell_crossings(radii, Source.origin, np.linspace(1.1, 2.9, 51), np.linspace(-1, 1, 21))   # looks first: densifies itself
        st = downloaded(hip, dev)
        assert len(st[2]) == out["N"] == dev.count
        want = shell_crossings(*st, radii, Source.origin, np.linspace(1.1, 2.9, 51), np.linspace(-1, 1, 21))
        assert all(np.array_equal(g, w) for g, w in zip(got, want)) and got[0].sum() > 0 and got[1].sum() > 0 and got[2].sum() > 0
    finally:
        dev.close()


def test_empty_store_and_refused_calls(hip):
    dev = hip.Device(0)
    try:
        lib = hip.load()
        ra, ce = np.array([1.0, 2.0]), np.array(CENTER)
        ed, mu = np.array([1.0, 2.0, 3.0]), np.array([-1.0, 0.0, 1.0])
        c, eh, mh = np.full(4, -1, np.int64), np.full(8, -1, np.int64), np.full(8, -1, np.int64)
        untouched = lambda: c.tolist() == [-1] * 4 and eh.tolist() == [-1] * 8 and mh.tolist() == [-1] * 8          # noqa: E731

        def raw(n_shells=2, radii=ra, center=ce, E_edges=ed, n_E=2, mu_edges=mu, n_mu=2, counts=c, E_hist=eh, mu_hist=mh):
            p = lambda a: None if a is None else a.ctypes.data      # noqa: E731
            return lib.pcl_step_shell_crossings(dev.ctx, n_shells, p(radii), p(center), p(E_edges), n_E, p(mu_edges), n_mu, p(counts), p(E_hist),
                                                p(mu_hist))

        assert raw() == -3 and untouched()                           # PCL_ERR_STATE: no store
        dev.store_alloc(1000)
        dev.set_count(0)
        assert raw() == 0 and c.tolist() == [0] * 4 and eh.tolist() == [0] * 8 and mh.tolist() == [0] * 8     # empty store: zeros
        c[:], eh[:], mh[:] = -1, -1, -1
        dev.fill_photons(1000, 0, C_LIT, 1.0, 3.0, 1)
        big = np.full(2 * 4 * 1025, -1, np.int64)
        over = dict(n_shells=4, radii=np.array([1.0, 2.0, 3.0, 4.0]), E_edges=np.linspace(1, 3, 1025), n_E=1024, mu_edges=mu, n_mu=1,
                    counts=np.full(8, -1, np.int64), E_hist=big, mu_hist=np.full(8, -1, np.int64))            # 2 x 4 x 1025 cells: one too many bins
        assert raw(**over) == -2 and np.all(big == -1) and np.all(over["counts"] == -1) and np.all(over["mu_hist"] == -1)
        for kw in (dict(radii=None), dict(counts=None), dict(n_shells=0), dict(n_shells=17), dict(radii=np.array([1.0, 0.0])),
                   dict(radii=np.array([1.0, -2.0])), dict(radii=np.array([NAN, 1.0])), dict(radii=np.array([1.0, np.inf])), dict(radii=np.array([1.0, 1e200])),
                   dict(center=np.array([0.0, NAN, 0.0])), dict(E_edges=None), dict(E_hist=None), dict(mu_edges=None), dict(mu_hist=None),
                   dict(n_E=-1), dict(n_mu=-1), dict(n_E=1025), dict(E_edges=np.array([1.0, 1.0, 2.0])), dict(E_edges=np.array([1.0, NAN, 2.0])),
                   dict(E_edges=np.array([1.0, 2.0, np.inf])), dict(mu_edges=np.array([0.0, 1.0, 0.5])), dict(mu_edges=np.array([0.0, 1e-200, 2e-200])),
                   dict(mu_edges=np.array([0.0, 1.0, 1e200]))):
            assert raw(**kw) == -2 and untouched(), kw               # PCL_ERR_ARG, before anything is written
        with pytest.raises(hip.HipError):
            dev.shell_crossings([1.0], E_edges=[2.0, 1.0])
        assert raw(center=None, E_edges=None, n_E=0, E_hist=None, mu_edges=None, n_mu=0, mu_hist=None) == 0      # r = dr = 0: nothing crosses
        assert c.tolist() == [0] * 4 and eh.tolist() == [-1] * 8
    finally:
        dev.close()


def test_group_and_multidevice_sum_the_shards(hip):
    from physicl_amd.multidev import MultiDevice
    N = 200_003
    radii, e, m = [0.5 * STEP, 1.0 * STEP, 1.5 * STEP, 2.5 * STEP], np.linspace(1.1, 2.9, 51), np.linspace(-1, 1, 21)
    one = hip.Device(0)
    try:
        one.store_alloc(N)
        one.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        one.apply_source(Source, C_LIT, 11)
        one.step_newton(DT)
        one.step_newton(DT)
        want = one.shell_crossings(radii, Source.origin, e, m)
        assert all(np.array_equal(g, w) for g, w in zip(want, shell_crossings(*downloaded(hip, one), radii, Source.origin, e, m)))
        assert want[0][0].sum() > 0 and want[1].sum() > 0 and want[2].sum() > 0
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
        got = g.shell_crossings(radii, Source.origin, e, m)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        got = g.shell_crossings(radii, Source.origin)
        assert np.array_equal(got[0], want[0]) and got[1] is None and got[2] is None
        out = np.full(8, -1, np.int64)
        bad = np.array([1.0, -1.0, 2.0, 3.0])
        assert g.lib.pcl_group_step_shell_crossings(g.g, 4, bad.ctypes.data, None, None, 0, None, 0, out.ctypes.data, None, None) == -2
        assert out.tolist() == [-1] * 8                              # checked once for the group, before any shard is asked
    md = MultiDevice([0, 0])
    try:
        md.store_alloc(N)
        md.fill_photons(N, 0, C_LIT, 1.0, 3.0, 11)
        md.apply_source(Source, C_LIT, 11)
        md.step_newton(DT)
        md.step_newton(DT)
        got = md.shell_crossings(radii, Source.origin, e, m)
    finally:
        md.close()
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


# ------------------------------------------------------------------------------------------------ simulation level
SHELLS = [2.0 * STEP, 6.0 * STEP, 0.75 * STEP, 12.0 * STEP]
SIM_CENTER = (1.0 * STEP, 0.0, -0.5 * STEP)                           # the source sits off the spheres' centre
PASSES = 40


def run_sim(with_shells=True, **kw):
    import physicl_amd as phys
    from physicl_amd import light, newton
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=lambda s: s.t >= DT * (PASSES - 0.5), **kw)
    sim.add_objs(light.generate_photons_bulk(20_000, min=1.0, max=3.0, seed=3, source=light.PhotonSource(origin=(0.0, 0.0, 0.0), angular="isotropic")))
    shell = light.ShellCrossingMeasureStep(None, SHELLS, center=SIM_CENTER, E_bins=np.linspace(1.0, 3.0, 11), mu_bins=np.linspace(-1, 1, 9))
    grids = [light.PositionGridMeasureStep(None, ("r",), [[0.0, R]], center=SIM_CENTER) for R in SHELLS]
    steps = [phys.UpdateTimeStep(lambda x: DT), newton.NewtonianKinematicsStep(), light.ScatterIsotropicStep(n=1.0, A=3e-6)]
    steps += ([shell] if with_shells else []) + grids
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    dev = sim._dev
    state = {f: dev.download(getattr(sim._hip, f)) for f in ("R0", "R1", "R2", "V0", "V1", "V2", "DR0", "DR1", "DR2", "E")}
    state["id"] = dev.download_ids()
    note, schedule = sim.launch_note, dict(sim.schedule)
    sim.close(download=False)
    return [list(r) for r in shell.data], [[list(r) for r in g.data] for g in grids], state, note, schedule


@pytest.fixture(scope="module")
def sim_runs():
    return {"with": run_sim(True), "without": run_sim(False)}


def test_cumulated_net_flux_is_the_change_of_the_population_outside(sim_runs):
    rows, grids, state, note, schedule = sim_runs["with"]
    assert len(rows) == PASSES and all(len(r) == 8 and r[1] == 20_000 for r in rows)
    assert "ShellCrossingMeasureStep" in note and set(schedule) == {"fused"} and schedule["fused"] == PASSES     # one launch per light step
    out, inn = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])                                     # [pass, shell]
    for k, R in enumerate(SHELLS):
        inside = np.array([g[2][0] for g in grids[k]])              # the grid's bin [0, R]: q < R*R (nobody sits on the closed edge, below)
        outside = 20_000 - inside
        start = 20_000 if 0.0 + sum(c * c for c in SIM_CENTER) >= R * R else 0                                    # everybody starts at the origin
        assert np.array_equal(start + np.cumsum(out[:, k] - inn[:, k]), outside), k
        assert out[:, k].sum() > 0
    assert inn.sum() > 0                                            # scattered photons come back in
    r = np.stack([state["R0"], state["R1"], state["R2"]], 1) - SIM_CENTER
    q = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    assert not any(np.any(q == R * R) for R in SHELLS)              # (the grid's last bin is closed: the two definitions of "inside" agree off the edge)
    for row in rows:                                                # the histograms stay within the counts; every photon has an energy in [1, 3]
        assert np.array_equal(row[4].sum(axis=1), row[2]) and np.array_equal(row[5].sum(axis=1), row[3])
        assert np.all(row[6].sum(axis=1) <= row[2]) and np.all(row[7].sum(axis=1) <= row[3])
    dr = np.stack([state["DR0"], state["DR1"], state["DR2"]], 1)
    want = shell_crossings(r + SIM_CENTER, dr, state["E"], np.ones(len(q), dtype=bool), SHELLS, SIM_CENTER, np.linspace(1.0, 3.0, 11), np.linspace(-1, 1, 9))
    for got, w in zip(rows[-1][2:], [want[0][0], want[0][1], want[1][0], want[1][1], want[2][0], want[2][1]]):
        assert np.array_equal(got, w)                               # the last row is the tally of the final store


def test_the_step_does_not_disturb_the_run(sim_runs):
    (_, grids_a, state_a, _, _), (rows_b, grids_b, state_b, note_b, schedule_b) = sim_runs["with"], sim_runs["without"]
    assert rows_b == [] and note_b is None and set(schedule_b) == {"fused_multi"}          # without the step: K passes per launch, as before
    for f in state_a:
        assert np.array_equal(state_a[f], state_b[f]), f
    for ga, gb in zip(grids_a, grids_b):
        assert len(ga) == len(gb) == PASSES and all(a[1] == b[1] and np.array_equal(a[2], b[2]) for a, b in zip(ga, gb))


def test_sharded_inside_the_process_gives_the_same_rows(hip, sim_runs):
    n = max(1, hip.device_count())
    rows, grids, state, note, _ = run_sim(True, devices=[i % n for i in range(2)])
    want_rows, want_grids, want_state = sim_runs["with"][:3]
    assert len(rows) == len(want_rows) == PASSES and "ShellCrossingMeasureStep" in note
    for a, b in zip(rows, want_rows):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    for f in state:
        assert np.array_equal(state[f], want_state[f]), f
