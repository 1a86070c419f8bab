"""CPU: ShellCrossingMeasureStep and Device.shell_crossings without a GPU.

* the numpy restatement (tests/shell_reference.py) agrees with a per-particle Python loop written from the header's text, on
  drawn points and on hand-made edge cases; the package's own host-path statement agrees with both;
* the step called on host-resident Python objects (plain Objects among the photons) files the restatement's row;
* the constructor's checks; header constants against ``_hip`` (the unit's build is held in tests/test_build_cpu.py);
* ``MultiDevice.shell_crossings`` sums stand-in shards; what ``Device.shell_crossings`` / ``DeviceGroup.shell_crossings`` put
  over the C ABI and hand back, on a stand-in for the library in the manner of tests/test_binding_marshal_cpu.py.
"""
import os
import re

import numpy as np
import pytest

import physicl_amd as phys
from physicl_amd import _hip, build, light
from shell_reference import EDGE_RADII, E_EDGES, MU_EDGES, assert_edge_case_tallies, edge_cases, shell_crossings, shell_crossings_loop

NAN, INF = float("nan"), float("inf")


def same(a, b):
    return all((x is None and y is None) or (x.dtype == np.int64 and np.array_equal(x, y)) for x, y in zip(a, b)) and len(a) == len(b) == 3


# ------------------------------------------------------------------------------------------------ the restatement
def test_edge_cases_by_hand_and_against_the_loop():
    r, dr, E, ph = edge_cases()
    got = shell_crossings(r, dr, E, ph, EDGE_RADII, (0, 0, 0), E_EDGES, MU_EDGES)
    assert same(got, shell_crossings_loop(r, dr, E, ph, EDGE_RADII, (0, 0, 0), E_EDGES, MU_EDGES))
    assert same(got, light._shell_tallies(r, dr, E, ph, EDGE_RADII, np.zeros(3), E_EDGES, MU_EDGES))
    assert_edge_case_tallies(*got)


@pytest.mark.parametrize("seed,center", [(1, (0.0, 0.0, 0.0)), (2, (0.25, -0.5, 1.0))])
def test_restatement_equals_the_loop_on_drawn_points(seed, center):
    rng = np.random.default_rng(seed)
    n = 400
    r = rng.normal(size=(n, 3)) * 1.5 + center
    dr = rng.normal(size=(n, 3)) * 0.8
    dr[::17] = 0.0
    r[5::41, 1] = NAN
    E = rng.uniform(0.5, 3.5, n)
    E[3::29], E[4::31], E[6::37], E[7::43] = 1.0, 2.0, 3.0, NAN
    ph = rng.random(n) < 0.8
    radii = [1.5, 0.75, 3.0, 2.0]
    mu = np.linspace(-1, 1, 21)
    for E_edges, mu_edges in [(None, None), (E_EDGES, None), (None, mu), (E_EDGES, mu), (E_EDGES, MU_EDGES[2:5])]:
        got = shell_crossings(r, dr, E, ph, radii, center, E_edges, mu_edges)
        assert same(got, shell_crossings_loop(r, dr, E, ph, radii, center, E_edges, mu_edges))
        assert same(got, light._shell_tallies(r, dr, E, ph, radii, np.array(center), E_edges, mu_edges))
    counts, E_hist, mu_hist = shell_crossings(r, dr, E, ph, radii, center, E_EDGES, mu)
    assert counts.min() > 5 and np.all(E_hist.sum(axis=2) <= counts) and np.all(mu_hist.sum(axis=2) <= counts) and 0 < E_hist.sum() < counts.sum()
    assert mu_hist.sum() > 0
    # mu against the plain cosine, away from the edges
    d = r - np.array(center)
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = np.einsum("ij,ij->i", d, dr) / np.sqrt(np.einsum("ij,ij->i", d, d) * np.einsum("ij,ij->i", dr, dr))
        q_now, q_prev = np.einsum("ij,ij->i", d, d), np.einsum("ij,ij->i", d - dr, d - dr)
        out = (q_prev < 1.5 ** 2) & (q_now >= 1.5 ** 2)
    assert np.array_equal(mu_hist[0, 0], np.histogram(cos[out & np.isfinite(cos)], bins=mu)[0])


# ------------------------------------------------------------------------------------------------ constructor
R1 = [1.0]


@pytest.mark.parametrize("kw", [
    dict(radii=[]), dict(radii=np.arange(1.0, 18.0)), dict(radii=[0.0]), dict(radii=[-1.0]), dict(radii=[NAN]), dict(radii=[INF]),
    dict(radii=[1e200]), dict(radii=[[1.0, 2.0]]), dict(radii="ab"), dict(radii=2.0),
    dict(radii=R1, center=(0, NAN, 0)), dict(radii=R1, center=(0, 0)), dict(radii=R1, center="c"),
    dict(radii=R1, E_bins=[1.0]), dict(radii=R1, E_bins=[1.0, 1.0, 2.0]), dict(radii=R1, E_bins=[1.0, 3.0, 2.0]), dict(radii=R1, E_bins=[1.0, NAN]),
    dict(radii=R1, E_bins=[1.0, INF]), dict(radii=R1, E_bins=np.arange(1026.0)), dict(radii=R1, E_bins=[[1.0, 2.0]]), dict(radii=R1, E_bins="ab"),
    dict(radii=R1, mu_bins=[0.5]), dict(radii=R1, mu_bins=[0.5, 0.5]), dict(radii=R1, mu_bins=[1.0, -1.0]), dict(radii=R1, mu_bins=[-1.0, NAN, 1.0]),
    dict(radii=R1, mu_bins=np.linspace(-1, 1, 1026)), dict(radii=R1, mu_bins=[0.0, 1e200]), dict(radii=R1, mu_bins=[0.0, 1e-200, 2e-200]),
    dict(radii=[1.0, 2.0, 3.0, 4.0, 5.0], E_bins=np.arange(1025.0)),                                        # 2 x 5 x 1024 cells
    dict(radii=[1.0, 2.0, 3.0, 4.0], E_bins=np.arange(1025.0), mu_bins=np.linspace(-1, 1, 2))])            # 2 x 4 x 1025
def test_malformed_steps_are_refused_at_construction(kw):
    with pytest.raises(ValueError):
        light.ShellCrossingMeasureStep(None, **kw)


def test_accepted_forms():
    s = light.ShellCrossingMeasureStep(None, [3, 1, 2], center=(6371000, 0, 0), E_bins=np.arange(1025), mu_bins=[-1, 1], measure_n=False)
    assert s.radii.tolist() == [3.0, 1.0, 2.0] and s.radii.dtype == np.float64 and s.center.tolist() == [6371000.0, 0.0, 0.0]
    assert len(s.E_bins) == 1025 and s.mu_bins.tolist() == [-1.0, 1.0] and s._fuse_role is None and s._device_native and s.data == []
    s = light.ShellCrossingMeasureStep(None, np.arange(1.0, 17.0))                                         # 16 shells, counts only
    assert s.E_bins is None and s.mu_bins is None and s.measure_n is True and s.center.tolist() == [0.0, 0.0, 0.0]
    light.ShellCrossingMeasureStep(None, [1.0, 2.0, 3.0, 4.0], E_bins=np.arange(513.0), mu_bins=np.linspace(-1, 1, 513))   # 8192 cells: the most
    m = light.ShellCrossingMeasureStep(None, phys.Measurement(np.array([1.0, 2.0]), "m**1"))
    assert type(m.radii) is np.ndarray and m.radii.tolist() == [1.0, 2.0]                                  # a Measurement: by its stored value
    import physicl.light
    assert physicl.light.ShellCrossingMeasureStep is light.ShellCrossingMeasureStep is phys.light.ShellCrossingMeasureStep


def test_a_loop_with_the_step_is_planned_one_launch_per_light_step():
    from physicl_amd import newton
    sim = phys.Simulation(cl_on=False, rng="philox")
    sim.cl_on, sim._hip = True, _hip                 # (plan as a device run would; no device is opened by planning)
    shell = light.ShellCrossingMeasureStep(None, [1.0])
    steps = [phys.UpdateTimeStep(lambda s: 1.0), newton.NewtonianKinematicsStep(), light.ScatterIsotropicStep(n=1.0, A=1e-9), shell]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim._plan = sim._build_plan()
    assert [k for k, _ in sim._plan] == ["single", "fused", "single"] and sim._plan[-1][1] is shell
    assert sim._multi_eligible() is False

    class Dev:
        count = 7

        def shell_crossings(self, radii, center, E_edges, mu_edges):
            return np.array([[3], [2]], dtype=np.int64), None, None
    sim._dev = Dev()
    assert sim.launch_note is None
    shell._device_run(sim)
    assert "ShellCrossingMeasureStep" in sim.launch_note and sim.launch_note.startswith("one launch per light step")
    (row,) = shell.data
    assert row[1] == 7 and row[2].tolist() == [3] and row[3].tolist() == [2] and len(row) == 4
    sim.launch_note, sim.steps_per_launch = None, 1  # asked for: nothing to say
    shell._device_run(sim)
    assert sim.launch_note is None
    sim._dev = None


# ------------------------------------------------------------------------------------------------ host path
def test_host_path_gives_the_restatement_s_rows(tmp_path):
    rng = np.random.default_rng(8)
    n, n_obj = 300, 20
    r, dr = rng.normal(size=(n, 3)) * 1.5, rng.normal(size=(n, 3)) * 0.8
    E = rng.uniform(0.5, 3.5, n)
    r[:14], dr[:14], E[:14] = edge_cases()[:3]
    sim = phys.Simulation(cl_on=False)               # (cl_on=True opens its device at once)
    objs = [light.PhotonObject(E=E[k], v=light.c * [1, 0, 0]) for k in range(n - n_obj)] + [phys.Object() for _ in range(n_obj)]
    for o, rr, mm in zip(objs, r, dr):
        o.r, o.dr = np.array(rr, dtype=np.float64), np.array(mm, dtype=np.float64)
    sim.add_objs(objs)
    sim.t = 0.25
    ph = np.arange(n) < n - n_obj
    radii, c = [2.0, 5.0, 0.5], (0.1, 0.0, -0.2)
    out = tmp_path / "shells.csv"
    a = light.ShellCrossingMeasureStep(str(out), radii, center=c, E_bins=E_EDGES, mu_bins=MU_EDGES)
    b = light.ShellCrossingMeasureStep(None, radii, measure_n=False)
    a.run(sim)
    b.run(sim)
    assert sim._dev is None                          # nothing was uploaded for a measurement of host-resident objects
    (row,), (rowb,) = a.data, b.data
    counts, E_hist, mu_hist = shell_crossings(r, dr, E, ph, radii, c, E_EDGES, MU_EDGES)
    assert row.dtype == object and len(row) == 8 and row[0] == 0.25 and row[1] == n
    for got, want in zip(row[2:], [counts[0], counts[1], E_hist[0], E_hist[1], mu_hist[0], mu_hist[1]]):
        assert got.dtype == np.int64 and np.array_equal(got, want)
    assert counts.min() > 0 and E_hist.sum() > 0 and mu_hist.sum() > 0 and E_hist.sum() < counts.sum()
    plain = shell_crossings(r, dr, E, ph, radii)[0]
    assert len(rowb) == 3 and rowb[0] == 0.25 and np.array_equal(rowb[1], plain[0]) and np.array_equal(rowb[2], plain[1])
    a.terminate(sim)
    assert out.read_text() == "0.25, %d, %s\n" % (n, ", ".join(str(x.tolist()) for x in row[2:]))
    b.terminate(sim)                                 # no file asked for: nothing written


# ------------------------------------------------------------------------------------------------ binding
class FakeLib:
    """Records the call with the arrays behind its pointers; answers cells 1000, 1001, ... / 2000, ... / 3000, ..."""

    def __init__(self):
        self.calls = []

    def _shells(self, name, handle, S, radii, center, E_edges, nE, mu_edges, nmu, counts, E_hist, mu_hist):
        at = lambda addr, dt, n: np.ctypeslib.as_array((np.ctypeslib.as_ctypes_type(dt) * n).from_address(addr))     # noqa: E731
        opt = lambda addr, n: None if addr is None else at(addr, np.float64, n).tolist()                              # noqa: E731
        self.calls.append((name, handle, S, at(radii, np.float64, S).tolist(), opt(center, 3), opt(E_edges, nE + 1), nE, opt(mu_edges, nmu + 1), nmu,
                           E_hist is None, mu_hist is None))
        at(counts, np.int64, 2 * S)[:] = 1000 + np.arange(2 * S)
        if E_hist is not None:
            at(E_hist, np.int64, 2 * S * nE)[:] = 2000 + np.arange(2 * S * nE)
        if mu_hist is not None:
            at(mu_hist, np.int64, 2 * S * nmu)[:] = 3000 + np.arange(2 * S * nmu)
        return 0

    def pcl_step_shell_crossings(self, *a):
        return self._shells("pcl_step_shell_crossings", *a)

    def pcl_group_step_shell_crossings(self, *a):
        return self._shells("pcl_group_step_shell_crossings", *a)


@pytest.mark.parametrize("cls,handle,entry", [(_hip.Device, "ctx", "pcl_step_shell_crossings"), (_hip.DeviceGroup, "g", "pcl_group_step_shell_crossings")])
def test_shell_crossings_marshalling(cls, handle, entry):
    d = cls.__new__(cls)
    d.lib = FakeLib()
    setattr(d, handle, None)
    counts, E_hist, mu_hist = d.shell_crossings([3, 1, 2], center=(1.5, -2, 0.25), E_edges=[1, 2, 4], mu_edges=[-1, 0, 0.5, 1])
    assert d.lib.calls[0] == (entry, None, 3, [3.0, 1.0, 2.0], [1.5, -2.0, 0.25], [1.0, 2.0, 4.0], 2, [-1.0, 0.0, 0.5, 1.0], 3, False, False)
    assert counts.dtype == np.int64 and counts.tolist() == [[1000, 1001, 1002], [1003, 1004, 1005]]        # [0] outward, [1] inward
    assert E_hist.shape == (2, 3, 2) and E_hist.reshape(-1).tolist() == list(range(2000, 2012))            # C order
    assert mu_hist.shape == (2, 3, 3) and mu_hist.reshape(-1).tolist() == list(range(3000, 3018))
    counts, E_hist, mu_hist = d.shell_crossings([7.0])
    assert d.lib.calls[1][2:] == (1, [7.0], None, None, 0, None, 0, True, True)                             # nothing asked for: NULLs and zeros
    assert counts.tolist() == [[1000], [1001]] and E_hist is None and mu_hist is None
    counts, E_hist, mu_hist = d.shell_crossings([7.0], mu_edges=np.linspace(-1, 1, 3))
    assert d.lib.calls[2][5:] == (None, 0, [-1.0, 0.0, 1.0], 2, True, False) and E_hist is None and mu_hist.shape == (2, 1, 2)


def test_prototypes_constants_and_multidevice_sum():
    assert "pcl_step_shell_crossings" in _hip.EXPORTS and "pcl_group_step_shell_crossings" in _hip.EXPORTS
    assert len(_hip._PROTOTYPES["pcl_step_shell_crossings"]) == 11 == len(_hip._PROTOTYPES["pcl_group_step_shell_crossings"])
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "physicl_hip.h")).read()
    for name, value in (("PCL_SHELL_MAX_SHELLS", _hip.SHELL_MAX_SHELLS), ("PCL_SHELL_MAX_BINS", _hip.SHELL_MAX_BINS),
                        ("PCL_SHELL_MAX_CELLS", _hip.SHELL_MAX_CELLS)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value
    assert (_hip.SHELL_MAX_SHELLS, _hip.SHELL_MAX_BINS, _hip.SHELL_MAX_CELLS) == (16, 1024, 8192)
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def shell_crossings(self, radii, center=None, E_edges=None, mu_edges=None):
            return (np.full((2, 3), self.k, dtype=np.int64), None if E_edges is None else np.full((2, 3, 4), 2 * self.k, dtype=np.int64),
                    None if mu_edges is None else np.full((2, 3, 2), 3 * self.k, dtype=np.int64))
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    counts, E_hist, mu_hist = md.shell_crossings([1, 2, 3], mu_edges=[-1, 0, 1])
    both = md.shell_crossings([1, 2, 3], E_edges=[1, 2, 3, 4, 5], mu_edges=[-1, 0, 1])
    md._pool.shutdown()
    assert counts.dtype == np.int64 and counts.tolist() == [[111] * 3] * 2 and E_hist is None and mu_hist.tolist() == [[[333] * 2] * 3] * 2
    assert both[1].shape == (2, 3, 4) and np.all(both[1] == 222)
