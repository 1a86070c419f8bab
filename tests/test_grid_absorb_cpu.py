"""CPU: GridAbsorptionStep (physicl_amd/light_grid.py) -- the constructor's refusals, the numpy restatement of pcl_step_absorb_grid
against an independent per-particle loop on Python integers and floats (tests/grid_absorb_reference.py), the binomial law of the two
draws, the step on host-resident objects, and what the step hands the device.  Nothing has a tolerance but the binomial bounds, which
are the law's own."""
import math

import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import light, light_grid, tally
from grid_absorb_reference import (C, CENTER, E_EDGES, ID_BASE, SEED, TABLES, WORDS, assert_every_outcome, grid_absorb_loop, grid_edges,
                                   philox, scene, tables)
from scatter_layered_reference import same_answer
from test_layered_phase_cpu import HostSim, objects
from writer_reference import same_bits

X2 = dict(axes=("x",), edges=[[0.0, 1.0, 2.0]])


# ------------------------------------------------------------------------------------------------ the class and its refusals
def test_the_class_is_a_writer_step_of_its_own_stream_and_is_exported():
    import physicl_amd.light as short
    step = phys.light.GridAbsorptionStep(k=0.5, **X2)
    assert short.GridAbsorptionStep is light.GridAbsorptionStep is light_grid.GridAbsorptionStep is phys.light.GridAbsorptionStep
    assert light_grid.GridAbsorptionStep.__bases__ == (tally.WriterStep,) and tally.writer_family(step) == "absorb_grid"
    assert vars(light_grid.GridAbsorptionStep)["_STREAM"] == "absorb_grid" and light_grid._GRID_ABSORB_WORDS == WORDS == (27, 28)
    assert "GridAbsorptionStep" in step._NOTE and step._NOTE.startswith("one launch per light step: ")
    assert step.terminate.__func__ is tally.TallyStep.terminate
    assert step.k.tolist() == [0.5, 0.5] and step.omega0 is None and step.absorbed_by_cell.tolist() == [0, 0]
    both = phys.light.GridAbsorptionStep(("x", "y"), [[0, 1, 2], [0, 1]], k=np.ones((2, 1, 3)), omega0=0.25, E_edges=E_EDGES)
    assert both.k.shape == both.omega0.shape == both.absorbed_by_cell.shape == (2, 1, 3) and both.absorbed_by_cell.dtype == np.int64
    assert (both.exposed, both.interacted, both.absorbed_path, both.absorbed_hit, both.absorbed) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("kw, words", [
    (dict(X2), "k and omega0 are both None"),
    (dict(X2, k=[1.0, 2.0, 3.0]), "k must be one number or have the shape (2,)"),
    (dict(X2, omega0=[[0.5, 0.5]]), "omega0 must be one number or have the shape (2,)"),
    (dict(X2, k=[1.0, 2.0], E_edges=E_EDGES), "k must be one number or have the shape (2, 3) -- the grid's cells by bands of E_edges"),
    (dict(X2, k="ab"), "k must be a number"), (dict(X2, omega0=["a", 1]), "omega0 must be a number"),
    (dict(X2, k=-1.0), "k must be finite and not negative"), (dict(X2, k=[0.0, np.nan]), "k must be finite and not negative"),
    (dict(X2, k=np.inf), "k must be finite and not negative"),
    (dict(X2, omega0=1.5), "omega0 must lie in [0, 1]"), (dict(X2, omega0=[0.5, -0.1]), "omega0 must lie in [0, 1]"),
    (dict(X2, omega0=np.nan), "omega0 must lie in [0, 1]"), (dict(X2, k=1.0, omega0=[0.5, 2.0]), "omega0 must lie in [0, 1]"),
    (dict(axes=("x", "y", "z"), edges=[np.arange(1025.0), np.arange(1025.0), [0.0, 1.0, 2.0]], k=1.0), "the grid has 2097152 cells, at most 1048576"),
    (dict(axes=("x", "y"), edges=[np.arange(1025.0), np.arange(513.0)], omega0=1.0, E_edges=E_EDGES), "omega0: 1024 x 512 x 3 are 1572864 cells"),
    (dict(X2, k=1.0, axes=("x", "x"), edges=[[0, 1]] * 2), "axes"), (dict(X2, k=1.0, axes=("w",)), "axes"), (dict(X2, k=1.0, axes=()), "axes"),
    (dict(X2, k=1.0, axes=("x", "y")), "edges"), (dict(X2, k=1.0, edges=[[0.0, 2.0, 1.0]]), "axis 'x'"),
    (dict(X2, k=1.0, edges=[np.arange(1026.0)]), "axis 'x'"), (dict(k=1.0, axes=("r",), edges=[[-1.0, 1.0, 2.0]]), "axis 'r'"),
    (dict(X2, k=1.0, center=(0, 0)), "center"), (dict(X2, k=1.0, center=(0, np.nan, 0)), "center"),
    (dict(X2, k=1.0, E_edges=[1.0]), "E_edges"), (dict(X2, k=1.0, E_edges=[1.0, 3.0, 2.0]), "E_edges must be finite and strictly increasing"),
    (dict(X2, k=1.0, E_edges=np.arange(1026.0)), "E_edges describes 1025 bins, at most 1024")])
def test_constructor_refusals_name_the_argument(kw, words):
    with pytest.raises(ValueError) as e:
        phys.light.GridAbsorptionStep(**kw)
    assert words in str(e.value), str(e.value)


def test_the_grid_is_refused_in_the_position_grid_s_words():
    for kw in (dict(axes=("x", "x"), edges=[[0, 1]] * 2), dict(axes=("w",), edges=[[0, 1]]), dict(axes=("x",), edges=[[0.0, 2.0, 1.0]]),
               dict(axes=("x",), edges=[[0.0, 1.0]], center=(0, np.inf, 0))):
        said = []
        for make in (lambda: phys.light.PositionGridMeasureStep(None, kw["axes"], kw["edges"], center=kw.get("center", (0, 0, 0))),
                     lambda: phys.light.GridAbsorptionStep(k=1.0, **kw)):
            with pytest.raises(ValueError) as e:
                make()
            said.append(str(e.value))
        assert said[0] == said[1], kw


# ------------------------------------------------------------------------------------------------ the restatement against the loop
GRIDS = {"one cell": (("x",), (1,), False), "x 3": (("x",), (3,), False), "r": (("r",), (4,), False), "4x4x4x3": (("x", "y", "z"), (4, 4, 4), True),
         "z,r x3": (("z", "r"), (3, 4), True)}
N = 2600


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("which", TABLES)
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_the_restatement_is_the_plain_loop_bit_for_bit(grid, which, dtype):
    axes, bins, bands = GRIDS[grid]
    edges = grid_edges(axes, bins)
    E_edges = E_EDGES if bands else None
    p, om = tables(tuple(bins) + ((3,) if bands else ()), which)
    if grid == "one cell":                                             # one value each: neither 0 nor 1, so that every outcome occurs
        p, om = (None if t is None else np.full(t.shape, x) for t, x in ((p, 0.25), (om, 0.5)))
    s = scene(N, axes, edges, dtype)
    photon = np.arange(N) % 7 != 3
    ids = ID_BASE + 3 * np.random.RandomState(5).permutation(N).astype(np.int64)            # above 2^32, not consecutive
    args = (s["r"], s["v"], s["dv"], s["E"], photon, ids, p, om, axes, edges, CENTER, E_edges, SEED)
    for n_pass in (1, 2 ** 32 - 1):
        got, ref = light_grid._grid_absorb(*args, n_pass, dtype), grid_absorb_loop(*args, n_pass, dtype)
        assert same_answer(got, ref), (grid, which, n_pass)
    counts = assert_every_outcome(ref, s["v"], s["dv"], photon, which, (grid, which))
    print(grid, which, counts)
    gone = ref["absorbed"]
    assert same_bits(ref["v"][~gone], s["v"][~gone]) and same_bits(ref["dv"][~gone], s["dv"][~gone]) and not ref["v"][gone].any()
    assert ref["absorbed_by_cell"].shape == tuple(bins) + ((3,) if bands else ()) and ref["absorbed_by_cell"].sum() == gone.sum()
    if which == "k":
        assert not ref["interacted"].any() and not ref["absorbed_hit"].any()
    if p is not None:
        assert not ref["absorbed_by_cell"][(p == 0.0) & (True if om is None else om == 1.0)].any()


def test_edges_and_bands_are_binned_as_the_position_grid_bins_them():
    edges = [[0.0, 1.0, 2.0]]
    x = np.array([0.0, 1.0, 2.0, np.nextafter(0.0, -1), np.nextafter(2.0, 3), np.nextafter(1.0, 0), np.nan])
    E = np.array([1.0, 1.5, 3.0, 2.0, 2.0, np.nextafter(1.0, 0), np.nan, np.nextafter(3.0, 4)])
    n = len(x) * len(E)
    r = np.zeros((n, 3))
    r[:, 0] = np.repeat(x, len(E))
    v = np.tile([C, 0.0, 0.0], (n, 1))
    got = light_grid._grid_absorb(r, v, np.zeros((n, 3)), np.tile(E, len(x)), np.ones(n, dtype=bool), np.arange(n), np.ones((2, 3)), None,
                                  ("x",), edges, (0, 0, 0), E_EDGES, SEED, 1)
    cell_x = np.repeat([0, 1, 1, -1, -1, 0, -1], len(E))
    band = np.tile([0, 1, 2, 2, 2, -1, -1, -1], len(x))
    want = np.where((cell_x >= 0) & (band >= 0), cell_x * 3 + band, -1)
    assert got["cell"].tolist() == want.tolist() and got["absorbed"].tolist() == (want >= 0).tolist()      # p = 1 absorbs every exposed photon
    assert got["absorbed_by_cell"].tolist() == np.bincount(want[want >= 0], minlength=6).reshape(2, 3).tolist()


# ------------------------------------------------------------------------------------------------ the binomial law
N_LAW = 20000
LAW_SEED = 20261021                               # chosen here, on the CPU: the integer Philox alone meets the bounds below (checked first)
P1, P2, OM = 0.25, 0.4, 0.7


def within(k, n, p):
    return abs(k - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))


def test_the_draws_follow_the_binomial_law_and_two_steps_draw_independently():
    ids = ID_BASE + np.arange(N_LAW)
    # the integer Philox alone, first: word 27 under two pass counters (two steps of one pass), word 28
    u1, u2, uh = (np.array([philox(int(i), LAW_SEED, n_pass, word)[0] for i in ids]) for n_pass, word in ((1, WORDS[0]), (2, WORDS[0]), (1, WORDS[1])))
    a1, a2 = u1 < P1, u2 < P2
    assert within(a1.sum(), N_LAW, P1) and within(a2.sum(), N_LAW, P2) and within((a1 & a2).sum(), N_LAW, P1 * P2)
    survivors = int((~a1).sum())
    assert within((~a1 & ~(uh < OM)).sum(), survivors, 1.0 - OM)
    # the restatement: one cell, everybody moving and scattered
    r, v = np.full((N_LAW, 3), 0.5), np.tile([C, 0.0, 0.0], (N_LAW, 1))
    dv = np.tile([0.0, 1.0, 0.0], (N_LAW, 1))
    run = lambda p, om, n_pass: light_grid._grid_absorb(r, v, dv, None, np.ones(N_LAW, dtype=bool), ids, p, om, ("x",), [[0.0, 1.0]],  # noqa: E731
                                                        (0, 0, 0), None, LAW_SEED, n_pass)
    first, second = run([P1], [OM], 1), run([P2], None, 2)
    assert first["exposed"].all() and first["interacted"].all() and not second["interacted"].any()
    assert np.array_equal(first["absorbed_path"], a1) and np.array_equal(second["absorbed_path"], a2)
    assert np.array_equal(first["absorbed_hit"], ~a1 & ~(uh < OM))
    n_path, n_hit = int(first["absorbed_path"].sum()), int(first["absorbed_hit"].sum())
    print("along the path %d of %d (p = %g); at the interaction %d of %d survivors (1 - omega0 = %g); both steps %d (p1 p2 = %g)"
          % (n_path, N_LAW, P1, n_hit, survivors, 1 - OM, (a1 & a2).sum(), P1 * P2))
    assert within(n_path, N_LAW, P1) and within(n_hit, N_LAW - n_path, 1.0 - OM)
    assert within(int(second["absorbed_path"].sum()), N_LAW, P2)
    assert within(int((first["absorbed_path"] & second["absorbed_path"]).sum()), N_LAW, P1 * P2)      # independent
    assert first["absorbed_by_cell"].tolist() == [n_path + n_hit]


def test_certain_tables_draw_nothing_and_decide_everything():
    n = 500
    r, v, dv = np.full((n, 3), 0.5), np.tile([C, 0.0, 0.0], (n, 1)), np.tile([0.0, 1.0, 0.0], (n, 1))
    dv[::2] = 0.0
    run = lambda p, om: light_grid._grid_absorb(r, v, dv, None, np.ones(n, dtype=bool), np.arange(n), p, om, ("x",), [[0.0, 1.0]],  # noqa: E731
                                                (0, 0, 0), None, SEED, 1)
    assert not run([0.0], [1.0])["absorbed"].any() and run([1.0], [0.0])["absorbed_path"].all()
    got = run([0.0], [0.0])
    assert got["absorbed_hit"].tolist() == got["interacted"].tolist() == (np.arange(n) % 2 == 1).tolist() and not got["absorbed_path"].any()


# ------------------------------------------------------------------------------------------------ the step on the host
HOST = dict(axes=("x", "y", "z"), edges=[np.linspace(CENTER[k] - 3.0, CENTER[k] + 3.0, 4) for k in range(3)], center=CENTER)
HOST_K = np.where(np.arange(27).reshape(3, 3, 3) % 3 == 0, 0.0, 0.6)
HOST_OM = np.where(np.arange(27).reshape(3, 3, 3) % 4 == 0, 1.0, 0.5)
DT = 0.5 / C


class Sim(HostSim):
    dt = np.double(DT)


@pytest.mark.parametrize("which", TABLES)
def test_host_resident_objects_get_the_restatement_s_state(tmp_path, which):
    n = 900
    objs, v, dv = objects(n)
    photon = np.arange(n) % 5 != 0
    k, om = (HOST_K if which != "omega0" else None), (HOST_OM if which != "k" else None)
    step = phys.light.GridAbsorptionStep(k=k, omega0=om, out_fn=str(tmp_path / "heat.csv"), **HOST)
    sim = Sim(objs, steps={0: step})
    r_code = tally.vec3(objs, "r")
    step.run(sim)
    p = None if k is None else light._path_probability(k, light._c_h_literals()[0], DT)
    ref = light_grid._grid_absorb(r_code, v, dv, None, photon, np.arange(n), p, om, HOST["axes"], HOST["edges"], CENTER, None, SEED, 1)
    want = [int(ref[f].sum()) for f in ("exposed", "interacted", "absorbed_path", "absorbed_hit")]
    assert [step.exposed, step.interacted, step.absorbed_path, step.absorbed_hit] == want and step.absorbed == want[2] + want[3] > 0
    assert step.absorbed_by_cell.tolist() == ref["absorbed_by_cell"].tolist() and step.absorbed_by_cell.shape == (3, 3, 3)
    assert (want[1] > 0) == (which != "k") and (want[2] > 0) == (which != "omega0") and (want[3] > 0) == (which != "k")
    row = step.data[0]
    assert len(step.data) == 1 and len(row) == 6 and list(row[:5]) == [0.25] + want and row[5].tolist() == step.absorbed_by_cell.tolist()
    for i, obj in enumerate(sim.objects):
        assert same_bits(np.asarray(obj.v, dtype=np.float64), ref["v"][i]) and same_bits(np.asarray(obj.dv, dtype=np.float64), ref["dv"][i]), i
        if not photon[i]:
            assert same_bits(np.asarray(obj.v), v[i]) and same_bits(np.asarray(obj.dv), dv[i])       # plain Objects are untouched
    assert same_bits(tally.vec3(objs, "r"), r_code) and sim.launch_note is None
    step.run(sim)
    assert step._pass == 2 and step._n_pass == 2 and len(step.data) == 2
    step.terminate(sim)
    lines = open(str(tmp_path / "heat.csv")).read().splitlines()
    assert len(lines) == 2 and lines[0].startswith("0.25, %d, %d, %d, %d, [[[" % tuple(want))


def test_python_semantics_are_refused_with_omega0_and_work_with_k_alone():
    objs, _, _ = objects(40)
    for kw in (dict(omega0=0.5), dict(k=1.0, omega0=0.5)):
        step = phys.light.GridAbsorptionStep(**HOST, **kw)
        with pytest.raises(ValueError, match="dv = v_old") as e:
            step.run(Sim(objs, py=True))
        assert "GridAbsorptionStep" in str(e.value) and "cl_on=True" in str(e.value)
        with pytest.raises(ValueError, match="cl_on"):
            step._device_run(Sim(objs, py=True))
        assert step._pass == 0 and step.data == []
    step = phys.light.GridAbsorptionStep(k=50.0, **HOST)
    step.run(Sim(objs, py=True))
    assert step._pass == 1 and step.exposed > 0 and step.interacted == 0 and step.absorbed == step.absorbed_path == step.absorbed_by_cell.sum()


def test_two_steps_of_a_pass_interleave_their_counters_and_a_bad_dt_is_refused():
    objs, _, _ = objects(30)
    a, b = phys.light.GridAbsorptionStep(k=1.0, **HOST), phys.light.GridAbsorptionStep(omega0=0.5, **HOST)
    other = phys.light.PathAbsorptionStep(1.0)                          # another family: does not count
    sim = Sim(objs, steps={0: a, 1: other, 2: b})
    for run in (1, 2):
        a.run(sim)
        b.run(sim)
        assert (a._n_pass, b._n_pass) == (2 * run - 1, 2 * run)
    bad = Sim(objs, steps={0: a})
    bad.dt = np.double(-1.0)
    with pytest.raises(ValueError, match="dt must be finite and not negative"):
        a.run(bad)
    assert a._pass == 2
    b.run(bad)                                                         # omega0 alone reads no dt
    assert b._pass == 3


def test_device_run_hands_the_sweep_its_arguments_and_records_the_global_row():
    """With a stand-in device: what ``absorb_grid`` is handed, the launch note, the one collective and the row."""
    class Dev:
        count = 7

        def absorb_grid(self, *a):
            self.args = a
            return np.array([9, 5, 2, 1]), np.arange(27).reshape(3, 3, 3)

    class DevSim(Sim):
        _residency = "device"
        _dev = Dev()

        def _k_wanted(self):
            return 8

        def _dt_code(self):
            return DT

        def _global(self, flat):
            self.flat = list(flat)
            return [2 * x for x in flat]                                 # two ranks with the same shard
    step = phys.light.GridAbsorptionStep(k=HOST_K, omega0=HOST_OM, **HOST)
    sim = DevSim([], steps={0: step})
    step._device_run(sim)
    p, om, axes, edges, center, E_edges, seed, n_pass = sim._dev.args
    assert same_bits(p, light._path_probability(HOST_K, light._c_h_literals()[0], DT)) and om is step.omega0 and axes == ("x", "y", "z")
    assert len(edges) == 3 and center.tolist() == CENTER.tolist() and E_edges is None and (seed, n_pass) == (SEED, 1)
    assert sim.flat == [7, 9, 5, 2, 1] + list(range(27)) and sim.launch_note == step._NOTE and sim._scattered is True
    assert (step.exposed, step.interacted, step.absorbed_path, step.absorbed_hit, step.absorbed) == (18, 10, 4, 2, 6)
    assert step.absorbed_by_cell.tolist() == (2 * np.arange(27).reshape(3, 3, 3)).tolist() and step.absorbed_by_cell.dtype == np.int64
    alone = phys.light.GridAbsorptionStep(omega0=HOST_OM, **HOST)
    alone._device_run(DevSim([], steps={0: alone}))
    assert sim._dev.args[0] is None and sim._dev.args[1] is alone.omega0
