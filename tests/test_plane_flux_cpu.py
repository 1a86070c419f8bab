"""CPU: PlaneFluxMapStep without a device -- the constructor's refusals, the numpy restatement ``light_grid._plane_flux_maps`` against
the per-particle loop (tests/plane_flux_reference.py) and against hand-made edge cases with written-out answers, the rule's bins
against the exact crossing point in rationals, the step on host-resident objects, and the scene of the past-one-trip test."""
from fractions import Fraction

import numpy as np
import pytest

import physicl_amd as phys
from physicl_amd import _hip, light, light_grid, tally
from plane_flux_reference import (AXES, EDGE_AXIS, EDGE_BANDS, EDGE_EDGES, EDGE_LEVELS, E_BANDS, LEVELS16, NAN, INF, assert_edge_case_tallies,
                                  configs, crossers, edge_cases, exact_points, plane_flux_loop, scene)

E2 = [[0.0, 1.0], [0.0, 1.0]]


def same(a, b):
    return all(x.dtype == np.int64 and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("kw, match", [
    (dict(axis="r"), "axis must be one of"), (dict(axis=2), "axis must be one of"), (dict(axis=None), "axis must be one of"),
    (dict(levels=[]), "1 to 16"), (dict(levels=np.arange(17.0)), "1 to 16"), (dict(levels=[[0.0]]), "1 to 16"),
    (dict(levels=[0.0, NAN]), "finite and strictly increasing"), (dict(levels=[0.0, INF]), "finite and strictly increasing"),
    (dict(levels=[1.0, 1.0]), "finite and strictly increasing"), (dict(levels=[1.0, 0.0]), "finite and strictly increasing"),
    (dict(levels="abc"), "sequence of numbers"),
    (dict(edges=[[0.0, 1.0]]), "two sequences"), (dict(edges=[[0.0, 1.0]] * 3), "two sequences"), (dict(edges=5), "two sequences"),
    (dict(edges=[[0.0, 1.0], [1.0]]), "at least two bin edges"), (dict(edges=[[0.0, 0.0], [0.0, 1.0]]), "strictly increasing"),
    (dict(edges=[[0.0, 1.0], [0.0, NAN]]), "strictly increasing"),
    (dict(edges=[np.linspace(0, 1, 1026), [0.0, 1.0]]), "at most 1024"), (dict(edges=[[0.0, 1.0], np.linspace(0, 1, 1026)]), "at most 1024"),
    (dict(E_bins=np.linspace(1, 2, 1026)), "at most 1024"), (dict(E_bins=[1.0, 1.0]), "strictly increasing"), (dict(E_bins=[1.0]), "at least two"),
    (dict(edges=[np.linspace(0, 1, 1025), np.linspace(0, 1, 513)]), r"2 directions x 1 levels x 1 bands x 1024 x 512 bins are 1048576"),   # (accepted: see below)
    (dict(levels=[0.0, 1.0], edges=[np.linspace(0, 1, 1025), np.linspace(0, 1, 513)]), r"2 directions x 2 levels x 1 bands x 1024 x 512 bins are 2097152 map cells, at most 1048576"),
    (dict(edges=[np.linspace(0, 1, 1025), [0.0, 1.0, 2.0]], E_bins=np.linspace(1, 2, 514)), r"x 513 bands x 1024 x 2 bins are 2101248"),
])
def test_the_constructor_refuses(kw, match):
    args = dict(dict(out_fn=None, axis="z", levels=[0.0], edges=E2), **kw)
    if "are 1048576" in match:                                         # exactly 2**20 cells: the limit itself is accepted
        step = light.PlaneFluxMapStep(**args)
        assert step.up_map.size + step.down_map.size == 1 << 20
        return
    with pytest.raises(ValueError, match=match):
        light.PlaneFluxMapStep(**args)
    with pytest.raises(ValueError, match=match):
        light_grid._check_plane_flux(args["axis"], args["levels"], args["edges"], args.get("E_bins"))


def test_accepted_forms():
    step = light.PlaneFluxMapStep(None, "y", np.arange(16.0), [(0, 1, 2), np.linspace(-1, 1, 4)], E_bins=[1, 2, 4], frames=True, measure_n=False)
    assert step.axis == "y" and step.levels.dtype == np.float64 and len(step.levels) == 16 and step.frames and not step.measure_n
    assert [e.tolist() for e in step.edges] == [[0.0, 1.0, 2.0], np.linspace(-1, 1, 4).tolist()] and step.E_bins.tolist() == [1.0, 2.0, 4.0]
    assert step.up_map.shape == step.down_map.shape == (16, 2, 2, 3) and step.up.shape == step.down.shape == (16,)
    assert step._fuse_role is None and "PlaneFluxMapStep" in step._NOTE and step._NOTE.startswith("one launch per light step")
    assert light.PlaneFluxMapStep is light_grid.PlaneFluxMapStep and isinstance(step, tally.TallyStep)
    assert AXES == light_grid._PLANE_AXES == {"x": (0, 1, 2), "y": (1, 0, 2), "z": (2, 0, 1)}


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("bands", [False, True])
def test_hand_made_edge_cases_by_hand_and_against_the_loop(bands):
    st = edge_cases()
    Ee = EDGE_BANDS if bands else None
    got = light_grid._plane_flux_maps(*st, EDGE_AXIS, EDGE_LEVELS, EDGE_EDGES, Ee)
    assert_edge_case_tallies(*got, bands)
    assert same(got, plane_flux_loop(*st, EDGE_AXIS, EDGE_LEVELS, EDGE_EDGES, Ee))
    f32 = edge_cases(np.float32)
    assert_edge_case_tallies(*light_grid._plane_flux_maps(*f32, EDGE_AXIS, EDGE_LEVELS, EDGE_EDGES, Ee), bands)


@pytest.mark.parametrize("name", ["z_1_level_lds", "x_16_levels_lds", "y_16_levels_bands_global", "x_bands_lds"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_restatement_equals_the_loop_on_a_scene(name, dtype):
    axis, levels, edges, Ee = configs()[name]
    st = scene(1500, dtype, objects=True)
    got = light_grid._plane_flux_maps(*st, axis, levels, edges, Ee)
    assert same(got, plane_flux_loop(*st, axis, levels, edges, Ee))
    assert got[0][0].sum() > 0 and got[0][1].sum() > 0 and 0 < got[1].sum() < got[0].sum()
    # several levels in one move: more crossings than crossers
    if len(levels) > 1:
        assert got[0].sum() > crossers(st, axis, levels).sum()


def test_every_change_of_side_is_counted_once():
    st = scene(5000, "f64")
    for axis in "xyz":
        a = AXES[axis][0]
        counts, _ = light_grid._plane_flux_maps(*st, axis, LEVELS16, E2)
        now, prev = st[0][:, a], st[0][:, a] - st[1][:, a]
        now, prev = now[~np.isnan(prev)], prev[~np.isnan(prev)]        # (a NaN crosses nothing and is on no side)
        for s, X in enumerate(LEVELS16):
            assert counts[0][s] - counts[1][s] == int((now >= X).sum()) - int((prev >= X).sum()), (axis, s)


def test_the_rule_s_bin_is_the_bin_of_the_exact_crossing_point():
    """Margin.  With eps = 2**-53 every rounding of the rule is a relative eps: prev = fl(now - m) (an absolute eps |prev| in G), G =
    fl(|X - prev|), p = fl(r_t - dr_t), the two products, their sum, and the edge's product e * D.  To first order the rule compares H
    with e * D with an error of at most eps (3 |p| D + 3 |dr_t| G + |dr_t| |prev| + |e| D): three roundings on each term of H, the
    level's, and the edge's.  Divided by D that is a distance along t; a crossing whose exact point is farther than FOUR times that
    (the factor covers the second-order terms) from every edge must land in the exact point's bin, and one outside the map by more
    than that in no cell.  Nothing is tuned: on this scene far fewer than 1 % of the crossers are that close to an edge."""
    eps = Fraction(1, 2 ** 53)
    axis, levels = "z", [-0.75, 0.0, 0.5]
    edges = [np.linspace(-3, 3, 25), np.linspace(-2.5, 2.5, 12)]
    rng = np.random.default_rng(5)
    n = 3000
    r, dr = rng.normal(size=(n, 3)) * 1.5, rng.normal(size=(n, 3)) * 0.8
    photon, E = np.ones(n, dtype=bool), np.ones(n)
    a, tu, tv = AXES[axis]
    points = exact_points(r, dr, axis, levels)
    want = np.zeros((2, len(levels), 1, 24, 11), dtype=np.int64)
    left_out, clear = set(), []
    for i, d, s, xu, xv in points:
        now, m = float(r[i][a]), float(dr[i][a])
        prev, D = now - m, abs(m)
        G = abs(levels[s] - prev)
        cell, close = [], False
        for t, x, e in ((tu, xu, edges[0]), (tv, xv, edges[1])):
            p = float(r[i][t]) - float(dr[i][t])
            base = 3 * abs(Fraction(p)) * Fraction(D) + 3 * abs(Fraction(float(dr[i][t]))) * Fraction(G) + abs(Fraction(float(dr[i][t]))) * abs(Fraction(prev))
            margins = [4 * eps * (base + abs(Fraction(float(ek))) * Fraction(D)) / Fraction(D) for ek in e]
            close = close or any(abs(x - Fraction(float(ek))) <= mk for ek, mk in zip(e, margins))
            inside = Fraction(float(e[0])) <= x <= Fraction(float(e[-1]))
            cell.append(max(k for k in range(len(e) - 1) if Fraction(float(e[k])) <= x) if inside else None)
        if close:
            left_out.add(i)
        else:
            clear.append((i, d, s, cell))
    crossing = {i for i, *_ in points}
    assert len(crossing) > 1000 and len(left_out) <= 0.01 * len(crossing)            # the cap; the scene stays far below it
    keep = np.array(sorted(crossing - left_out))
    for i, d, s, cell in clear:
        if i not in left_out and None not in cell:
            want[d, s, 0, cell[0], cell[1]] += 1
    got = light_grid._plane_flux_maps(r[keep], dr[keep], E[keep], photon[keep], axis, levels, edges)
    assert np.array_equal(got[1], want) and want.sum() > 1000 and np.count_nonzero(want) > 200
    assert got[0].sum() == sum(1 for i, *_ in points if i not in left_out)


# ------------------------------------------------------------------------------------------------ the step, host-resident
def test_host_path_gives_the_restatement_s_rows(tmp_path):
    n, n_obj = 400, 30
    axis, levels, edges = "z", [-0.5, 0.25, 1.0], [np.linspace(-3, 3, 7), np.linspace(-3, 3, 5)]
    r, dr, E, _ = (np.asarray(x, dtype=np.float64) for x in scene(n, "f64"))
    E = np.where(np.isnan(E), 2.0, E)
    sim = phys.Simulation(cl_on=False)                      # (cl_on=True opens its device at once)
    objs = [light.PhotonObject(E=E[k], v=light.c * [1, 0, 0]) for k in range(n - n_obj)] + [phys.Object() for _ in range(n_obj)]
    for o, rr, mm in zip(objs, r, dr):
        o.r, o.dr = np.array(rr, dtype=np.float64), np.array(mm, dtype=np.float64)
    sim.add_objs(objs)
    sim.t = 0.25
    ph = np.arange(n) < n - n_obj
    out = tmp_path / "flux.csv"
    a = light.PlaneFluxMapStep(str(out), axis, levels, edges, E_bins=E_BANDS, frames=True)
    b = light.PlaneFluxMapStep(None, axis, levels, edges, measure_n=False)
    for _ in range(2):
        a.run(sim)
        b.run(sim)
    assert sim._dev is None                                 # nothing was uploaded for a measurement of host-resident objects
    counts, maps = light_grid._plane_flux_maps(r, dr, E, ph, axis, levels, edges, E_BANDS)
    assert same((counts, maps), plane_flux_loop(r, dr, E, ph, axis, levels, edges, E_BANDS))
    row = a.data[1]
    assert row.dtype == object and len(row) == 6 and list(row[:2]) == [0.25, n]
    assert np.array_equal(row[2], counts[0]) and np.array_equal(row[3], counts[1]) and np.array_equal(row[4], maps[0]) and np.array_equal(row[5], maps[1])
    assert row[4].shape == (3, 3, 6, 4) and 0 < maps.sum() < counts.sum()
    assert np.array_equal(a.up_map, 2 * maps[0]) and np.array_equal(a.down_map, 2 * maps[1])            # exposures: the sum of the frames
    assert np.array_equal(a.up, counts[0]) and np.array_equal(a.down, counts[1])                          # the last pass's counts
    wide = light_grid._plane_flux_maps(r, dr, E, ph, axis, levels, edges)
    assert len(b.data[0]) == 3 and b.data[0][0] == 0.25 and np.array_equal(b.data[0][1], wide[0][0]) and np.array_equal(b.data[0][2], wide[0][1])
    assert np.array_equal(b.up_map, 2 * wide[1][0]) and b.up_map.shape == (3, 1, 6, 4) and wide[1].sum() > maps.sum()
    a.terminate(sim)
    line = "0.25, %d, %s, %s, %s, %s\n" % (n, counts[0].tolist(), counts[1].tolist(), maps[0].tolist(), maps[1].tolist())
    assert out.read_text() == line * 2


class Dev:
    count = 7

    def __init__(self):
        self.calls = []

    def plane_flux(self, axis, levels, edges, E_edges=None):
        self.calls.append((axis, levels, edges, E_edges))
        k = len(self.calls)
        return np.array([[1 * k, 2 * k], [3 * k, 4 * k]], dtype=np.int64), np.arange(2 * 2 * 1 * 1 * 3, dtype=np.int64).reshape(2, 2, 1, 1, 3) * k


class Sim:
    t, launch_note = 0.5, None

    def __init__(self):
        self._dev, self.chunks = Dev(), []

    def _k_wanted(self):
        return 4

    def _global(self, values):
        self.chunks.append(len(values))
        return np.asarray(values, dtype=np.int64) * 2               # two ranks with the same tallies


def test_the_step_on_a_stand_in_device():
    sim = Sim()
    step = light.PlaneFluxMapStep(None, "x", [0.0, 1.0], [[0.0, 1.0], [0.0, 1.0, 2.0, 3.0]], frames=True)
    step._device_run(sim)
    step._device_run(sim)
    assert sim.launch_note == step._NOTE
    assert sim.chunks == [1 + 4 + 12] * 2                  # one collective per pass: N, the counts, the maps
    assert sim._dev.calls[0] == ("x", step.levels, step.edges, None)
    a, b = step.data
    assert list(a[:2]) == [0.5, 14] and a[2].tolist() == [2, 4] and a[3].tolist() == [6, 8] and b[2].tolist() == [4, 8]
    assert a[4].tolist() == [[[[0, 2, 4]]], [[[6, 8, 10]]]] and a[5].tolist() == [[[[12, 14, 16]]], [[[18, 20, 22]]]]
    assert step.up_map.tolist() == (a[4] + b[4]).tolist() and step.down_map.tolist() == (a[5] + b[5]).tolist()
    assert step.up.tolist() == [4, 8] and step.down.tolist() == [12, 16]


def test_a_loop_with_the_step_is_planned_one_launch_per_light_step():
    from physicl_amd import newton
    sim = phys.Simulation(cl_on=False, rng="philox")
    sim.cl_on, sim._hip = True, _hip                        # (plan as a device run would; no device is opened by planning)
    flux = light.PlaneFluxMapStep(None, "z", [0.0], E2)
    steps = [phys.UpdateTimeStep(lambda s: 1.0), newton.NewtonianKinematicsStep(), light.ScatterIsotropicStep(n=1.0, A=1e-9), flux]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim._plan = sim._build_plan()
    assert [k for k, _ in sim._plan] == ["single", "fused", "single"] and sim._plan[-1][1] is flux
    assert sim._multi_eligible() is False


def test_multidevice_sums_the_shards():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def plane_flux(self, axis, levels, edges, E_edges=None):
            return np.full((2, 2), self.k, dtype=np.int64), np.full((2, 2, 1 if E_edges is None else 2, 1, 3), 2 * self.k, dtype=np.int64)
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    counts, maps = md.plane_flux("z", [0.0, 1.0], [[0, 1], [0, 1, 2, 3]])
    banded = md.plane_flux("z", [0.0, 1.0], [[0, 1], [0, 1, 2, 3]], [1.0, 2.0, 3.0])
    md._pool.shutdown()
    assert counts.dtype == np.int64 and np.all(counts == 111) and maps.shape == (2, 2, 1, 1, 3) and np.all(maps == 222)
    assert banded[1].shape == (2, 2, 2, 1, 3) and np.all(banded[1] == 222)


# ------------------------------------------------------------------------------------------------ the past-one-trip scene
def test_the_trip_scene_meets_has_work_s_floor_by_the_restatement_alone():
    """tests/test_plane_flux_trips_gpu.py's population and levels, at the sizes a 256-CU device gives: the restatement's mask of
    crossers meets test_writer_trips_gpu.has_work's conditions (a)-(c) with its default floor, without a device."""
    from test_plane_flux_trips_gpu import TRIP_AXIS, TRIP_LEVELS, state_of
    from test_writer_trips_gpu import has_work, slots
    cap = 256 * 8 * 256
    for size, dtype in (("N2", "f64"), ("N2", "f32"), ("N3", "f64")):
        st = state_of(slots(cap, size), dtype)
        fraction = has_work(crossers(st, TRIP_AXIS, TRIP_LEVELS), cap, "plane flux %s %s" % (size, dtype))
        assert 0.1 <= fraction <= 0.9
