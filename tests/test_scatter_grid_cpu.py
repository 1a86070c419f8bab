"""CPU: GridScatterStep (light.GridScatterStep, light._scatter_grid, pcl_step_scatter_grid) -- the refusals, the numpy restatement
against a plain loop on Python integers and floats on the edge scene, the radius grid against the scattering by layer, the position
grid behind its refactoring, the step on host-resident objects, the statistics of the draw, the counter words, the bindings, the
collective of a large row, the header, the build table and the refusals of the library that need no device."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest

import grid_reference
import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import _hip, build, light, tally
from scatter_grid_reference import (BAD_CALLS, C, CENTER, E_EDGES, SEED, abi_args, assert_every_outcome, grid_edges, philox, probabilities,
                                    same_answer, scatter_grid_loop, scene)
from writer_reference import same_bits

ENTRIES = ("pcl_step_scatter_grid", "pcl_group_step_scatter_grid")
N = 2049
GRIDS = [(("x", "y", "z"), (4, 4, 4)), (("z", "r"), (3, 4)), (("r",), (4,))]


def planted(n, axes, edges, dtype):
    state = scene(n, axes, edges, dtype)
    state["photon"] = np.arange(n) % 7 != 3
    state["id"] = 7_000_000_001 + 3 * np.random.RandomState(5).permutation(n).astype(np.int64)
    return state


def sweep(fn, state, p, axes, edges, E_edges, first, n_pass=1, dtype=np.float64, seed=SEED):
    return fn(state["r"], state["v"], state["dv"], state["E"], state["photon"], state["id"], p, axes, edges, CENTER, E_edges, first, C, seed,
              n_pass, dtype)


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("first", [True, False])
@pytest.mark.parametrize("bands", [False, True])
@pytest.mark.parametrize("axes, bins", GRIDS)
def test_the_restatement_is_the_loop_bit_for_bit(axes, bins, bands, first, dtype):
    edges = grid_edges(axes, bins)
    E_edges = E_EDGES if bands else None
    state = planted(N, axes, edges, dtype)
    shape = tuple(bins) + ((3,) if bands else ())
    for kind in ("mixed", 0.0, 1.0) if first else ("mixed",):
        p = probabilities(shape, kind)
        ref, loop = (sweep(fn, state, p, axes, edges, E_edges, first, 2, dtype) for fn in (light._scatter_grid, scatter_grid_loop))
        assert same_answer(ref, loop), kind
        assert ref["scattered_by_cell"].shape == shape and ref["scattered_by_cell"].sum() == ref["scattered"].sum()
        if kind == "mixed":
            print(axes, bands, first, dtype.__name__, assert_every_outcome(ref, state["v"], state["photon"], E_edges, (axes, bands)))
            assert not ref["scattered_by_cell"][p == 0.0].any()
        elif kind == 0.0:
            assert ref["exposed"].any() and not ref["scattered"].any()
        else:
            assert ref["exposed"].any() and np.array_equal(ref["scattered"], ref["exposed"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_planted_slots_are_found_where_they_were_planted(dtype):
    """On the first edge: bin 0; on an inner edge: the bin it opens; on the last edge: the last bin (closed); one ``dtype`` value
    outside either end, a NaN: no cell.  By the scene's own arithmetic on the slot numbers."""
    for axes, bins in GRIDS:
        edges = grid_edges(axes, bins)
        state = scene(N, axes, edges, dtype)
        state["photon"], state["id"] = np.ones(N, dtype=bool), np.arange(N)
        state["v"][:] = [C, 0.0, 0.0]                                   # everybody moves: exposure is the cell alone
        ref = sweep(light._scatter_grid, state, np.zeros(bins), axes, edges, None, False, dtype=dtype)
        strides = [int(np.prod(bins[a + 1:])) for a in range(len(axes))]
        seen = set()
        for k in range(0, N, 3):
            a, which = (k // 3) % len(axes), (k // (3 * len(axes))) % 5
            if np.isnan(state["r"][k]).any():
                assert ref["cell"][k] == -1
                continue
            if which >= 3:
                assert ref["cell"][k] == -1, (axes, k, which)
            elif ref["cell"][k] >= 0:                                   # (another axis's random coordinate may stand outside)
                want = [0, (bins[a] + 1) // 2, bins[a] - 1][which]
                assert (ref["cell"][k] // strides[a]) % bins[a] == want, (axes, k, which)
                seen.add((a, which))
        assert seen == {(a, w) for a in range(len(axes)) for w in range(3)}, axes
        assert (ref["cell"][np.isnan(state["r"]).any(axis=1)] == -1).all()


def test_a_radius_grid_exposes_the_layers_photons():
    """axes=("r",) with the same edges, seed and n_pass exposes the photons light._scatter_layered exposes, into the same cells; the
    hits differ: the counter words do."""
    edges = grid_edges(("r",), (4,))
    for E_edges in (None, E_EDGES):
        state = planted(N, ("r",), edges, np.float64)
        p = probabilities((4,) + ((3,) if E_edges is not None else ()))
        mine = sweep(light._scatter_grid, state, p, ("r",), edges, E_edges, True, 3)
        theirs = light._scatter_layered(state["r"], state["v"], state["dv"], state["E"], state["photon"], state["id"], p, edges[0], CENTER,
                                        E_edges, True, C, SEED, 3)
        assert np.array_equal(mine["exposed"], theirs["exposed"]) and mine["exposed"].sum() > 500
        cols = p.shape[1] if p.ndim == 2 else 1
        their_cell = np.where(theirs["exposed"], theirs["layer"] * cols + theirs["band"], -1)
        assert np.array_equal(mine["cell"], their_cell)
        assert not np.array_equal(mine["scattered"], theirs["scattered"]) and mine["scattered"].any() and theirs["scattered"].any()


def test_the_position_grid_is_what_it_was():
    """light._grid_of_positions, whose per-particle cell now comes from the helper the scattering shares, against
    tests/grid_reference.py on the edge scene: bit for bit, dtype included."""
    for dtype in (np.float64, np.float32):
        for axes, bins in GRIDS + [(("y", "x"), (5, 3)), (("r", "x", "z"), (2, 3, 5))]:
            edges = grid_edges(axes, bins)
            r = scene(N, axes, edges, dtype)["r"]
            got = light._grid_of_positions(r, axes, edges, CENTER)
            want = grid_reference.position_grid(r, axes, edges, CENTER)
            assert same_bits(got, np.asarray(want, dtype=np.int64)) and got.shape == tuple(bins) and 0 < got.sum() < N
    ok, cell = light._cell_of_positions(np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [9.0, 0.0, 0.0]]), ("x",), [np.array([-1.0, 0.0, 1.0])],
                                        CENTER)
    assert ok.tolist() == [True, False, False] and cell[0] == 1


def test_the_draws_follow_the_id_the_pass_and_the_seed_at_full_width():
    axes, bins = GRIDS[0]
    edges = grid_edges(axes, bins)
    state = planted(N, axes, edges, np.float64)
    p = probabilities(bins)
    one = sweep(light._scatter_grid, state, p, axes, edges, None, True)
    for kw in (dict(n_pass=2), dict(seed=SEED + 1)):
        other = sweep(light._scatter_grid, state, p, axes, edges, None, True, **kw)
        assert np.array_equal(other["exposed"], one["exposed"]) and not np.array_equal(other["scattered"], one["scattered"])
    for seed, n_pass in ((2 ** 64 - 1, 2 ** 32 - 1), (2 ** 32, 2 ** 31)):
        ref, loop = (sweep(fn, state, p, axes, edges, None, True, n_pass, seed=seed) for fn in (light._scatter_grid, scatter_grid_loop))
        assert same_answer(ref, loop) and ref["scattered"].any()
    assert light._GRID_SCATTER_WORDS == (25, 26)
    k = int(np.flatnonzero(one["scattered"] & (p.reshape(-1)[one["cell"]] < 1.0))[0])
    assert philox(int(state["id"][k]), SEED, 1, 25)[0] < p.reshape(-1)[one["cell"][k]]
    u_a = philox(int(state["id"][k]), SEED, 1, 26)[0]
    assert abs(one["v"][k, 0] / C - (1.0 - 2.0 * u_a)) <= 4 * np.finfo(np.float64).eps      # about (1, 0, 0): the x component is c * mu


# ------------------------------------------------------------------------------------------------ statistics
STAT_N, STAT_SEED = 16385, 20261020


def test_half_of_the_exposed_photons_of_a_half_cell_scatter():
    """N = 16 385 photons, the even ones in a cell with p = 0.5, the odd ones in a cell with p = 0: k hits of n exposed to p = 0.5 with
    |k - n p| <= 5 sqrt(n p (1 - p)).  The seed is first shown to satisfy that with the integer Philox alone."""
    n = (STAT_N + 1) // 2
    bound = 5.0 * np.sqrt(n * 0.25)
    k_int = sum(philox(i, STAT_SEED, 1, 25)[0] < 0.5 for i in range(0, STAT_N, 2))
    assert abs(k_int - n * 0.5) <= bound, (k_int, n)
    r = np.zeros((STAT_N, 3))
    r[:, 0] = np.where(np.arange(STAT_N) % 2 == 0, -0.5, 0.5)
    v = np.tile([0.0, C, 0.0], (STAT_N, 1))
    out = light._scatter_grid(r, v, np.zeros((STAT_N, 3)), None, np.ones(STAT_N, dtype=bool), np.arange(STAT_N), [0.5, 0.0], ("x",),
                              [np.array([-1.0, 0.0, 1.0])], (0, 0, 0), None, True, C, STAT_SEED, 1)
    assert out["exposed"].all() and out["scattered_by_cell"].tolist() == [k_int, 0] and int(out["scattered"].sum()) == k_int
    assert not out["scattered"][1::2].any()
    print("k = %d of n = %d, |k - n/2| = %.1f, bound %.1f" % (k_int, n, abs(k_int - n * 0.5), bound))


# ------------------------------------------------------------------------------------------------ the step on the host
class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed = 0.25, SEED

    def __init__(self, objs, py=False, steps=None, dt=0.5 / C):
        self.objects, self.py, self.steps, self.dt = objs, py, steps or {}, np.double(dt)

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


AXES, BINS = GRIDS[0]
EDGES = grid_edges(AXES, BINS)
K = probabilities(BINS + (3,)) * 4.0


def some_objects(n=64):
    return objects(planted(n, AXES, EDGES, np.float64))


def make(first=None, **kw):
    return phys.light.GridScatterStep(K, AXES, EDGES, CENTER, E_EDGES, first=first, **kw)


def layered(first=None):
    return phys.light.LayeredScatterStep(0.5, first=first)


def test_constructor_keeps_what_it_was_given():
    step = make(out_fn="rows.csv")
    assert same_bits(step.k, K) and step.axes == AXES and [e.tolist() for e in step.edges] == [e.tolist() for e in EDGES]
    assert step.E_edges.tolist() == E_EDGES.tolist() and step.center.tolist() == CENTER.tolist()
    assert (step.first, step._pass, step.data, step.out_fn, step.exposed, step.scattered) == (None, 0, [], "rows.csv", 0, 0)
    assert step.scattered_by_cell.shape == (4, 4, 4, 3) and step.scattered_by_cell.dtype == np.int64 and step._writes == ("v", "dv")
    one = phys.light.GridScatterStep(0.5, AXES, EDGES)                   # one number is broadcast
    assert one.k.shape == (4, 4, 4) and (one.k == 0.5).all() and one.E_edges is None and one.center.tolist() == [0, 0, 0]
    assert phys.light.GridScatterStep(0.5, AXES, EDGES, E_edges=E_EDGES).k.shape == (4, 4, 4, 3)
    assert make(first=True).first is True and make(first=False).first is False
    import phys.light as short
    assert short.GridScatterStep is light.GridScatterStep is phys.light.GridScatterStep
    cls = light.GridScatterStep
    assert issubclass(cls, tally.WriterStep) and not set(vars(cls)) & {"run", "_device_run", "_reduce"}
    # a writer family of its own, though the class derives from the sibling for the rules they share
    assert tally.writer_family(step) == cls._STREAM != tally.writer_family(layered()) and "_STREAM" in vars(cls)
    assert tally.writer_family(layered()) == light.LayeredScatterStep._STREAM and issubclass(cls, light.LayeredScatterStep)

    class Plume(cls):                                                   # a subclass draws from the grid step's words
        pass
    assert tally.writer_family(Plume(0.5, AXES, EDGES)) == cls._STREAM
    assert "one launch per light step" in cls._NOTE and "GridScatterStep" in cls._NOTE and cls._NOTE != light.LayeredScatterStep._NOTE
    assert cls.terminate is tally.TallyStep.terminate
    assert (_hip.SCATTER_GRID_MAX_BANDS, _hip.SCATTER_GRID_MAX_CELLS) == (1024, 2 ** 20) and _hip.SCATTER_GRID_MAX_CELLS == _hip.GRID_MAX_CELLS


@pytest.mark.parametrize("kw, word", [
    (dict(axes=5), "axes must be a sequence of names"), (dict(axes=()), "one to three axes"), (dict(axes="xyzr"), "one to three axes"),
    (dict(axes=("x", "x")), "distinct names"), (dict(axes=("x", "w")), "distinct names"), (dict(edges=5), "edges must be one 1-D sequence"),
    (dict(edges=[[0, 1]]), "one sequence of bin edges per axis: 2 axes, 1 sequences"), (dict(edges=[[0, 1], [1, 0]]), "axis 'y'"),
    (dict(edges=[[0, 1], np.arange(1026.0)]), "axis 'y' describes 1025 bins"), (dict(axes=("x", "r"), edges=[[0, 1], [-1, 1]]), "radius edges"),
    (dict(center=[0, np.nan, 0]), "center")])
def test_geometry_refusals_are_the_position_grid_s(kw, word):
    args = dict(axes=("x", "y"), edges=[[0.0, 1.0], [0.0, 1.0]], center=(0, 0, 0))
    args.update(kw)
    with pytest.raises(ValueError, match=word) as mine:
        phys.light.GridScatterStep(0.5, **args)
    with pytest.raises(ValueError) as theirs:                           # the same check, the same message
        phys.light.PositionGridMeasureStep(None, **args)
    assert str(mine.value) == str(theirs.value)


@pytest.mark.parametrize("kw, word", [
    (dict(k="x"), "k must be a number"), (dict(k=[0.1, 0.2]), r"k must be one number or have the shape \(2, 3\)"),
    (dict(k=np.zeros((2, 3)), E_edges=[1.0, 2.0]), r"shape \(2, 3, 1\)"), (dict(k=-1.0), "finite and not negative"),
    (dict(k=np.nan), "finite and not negative"), (dict(k=np.inf), "finite and not negative"),
    (dict(k=0.5, E_edges=[1.0, np.nan, 3.0]), "E_edges"), (dict(k=0.5, E_edges=np.arange(1026.0)), "E_edges describes 1025 bins"),
    (dict(k=0.5, edges=[np.arange(1025.0), np.arange(1025.0)]), "1048576 cells"),          # (the position grid's own limit is met first)
    (dict(k=0.5, edges=[np.arange(1025.0), np.arange(513.0)], E_edges=[1.0, 2.0, 3.0, 4.0]), "1024 x 512 x 3 are 1572864 cells, at most 1048576"),
    (dict(k=0.5, first=1), "first must be None, True or False"), (dict(k=0.5, first="yes"), "first must be None, True or False")])
def test_constructor_refusals(kw, word):
    args = dict(k=0.5, axes=("x", "y"), edges=[[0.0, 1.0, 2.0], [0.0, 1.0, 2.0, 3.0]])
    args.update(kw)
    if "1048576 cells" in word and "x" not in word:                     # exactly 2^20 cells are supported
        step = phys.light.GridScatterStep(**dict(args, edges=[np.arange(1025.0), np.arange(1025.0)]))
        assert step.k.shape == (1024, 1024)
        args["edges"] = [np.arange(1025.0), np.arange(1025.0), [0.0, 1.0, 2.0]]
        args["axes"] = ("x", "y", "z")
        word = "2097152 cells"
    with pytest.raises(ValueError, match=word):
        phys.light.GridScatterStep(**args)


@pytest.mark.parametrize("py", [False, True])
def test_host_resident_objects_get_the_restatement_s_state(tmp_path, py):
    state = planted(400, AXES, EDGES, np.float64)
    objs = objects(state)
    n = len(objs)
    E0, photon = tally.photon_energies(objs, phys.light.PhotonObject)
    r0, v0, dr0, dv0 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    step = make(out_fn=str(tmp_path / "field.csv"))
    sim = HostSim(objs, py=py, steps={0: phys.newton.NewtonianKinematicsStep(), 1: step})
    step.run(sim)                                                      # first resolves to True: works under cl_on=False as well
    assert step.first is True and step._pass == 1 == step._n_pass
    c_code = light._c_h_literals()[0]
    p = light._path_probability(K, c_code, sim.dt)
    assert same_bits(p, -np.expm1(-(K * (np.float64(c_code) * np.float64(sim.dt)))))
    ref = scatter_grid_loop(r0, v0, dv0, E0, photon, np.arange(n), p, AXES, EDGES, CENTER, E_EDGES, True, c_code, SEED, 1)
    assert_every_outcome(ref, v0, photon, E_EDGES, "host")
    assert (step.exposed, step.scattered) == (int(ref["exposed"].sum()), int(ref["scattered"].sum())) and step.scattered > 0
    assert same_bits(step.scattered_by_cell, ref["scattered_by_cell"])
    row = list(step.data[0])
    assert row[:3] == [0.25, step.exposed, step.scattered] and same_bits(row[3], ref["scattered_by_cell"]) and sim.launch_note is None
    r1, v1, dr1, dv1 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    assert same_bits(r1, r0) and same_bits(dr1, dr0) and same_bits(v1, ref["v"]) and same_bits(dv1, ref["dv"])
    assert same_bits(tally.photon_energies(objs, phys.light.PhotonObject)[0], E0)
    step.run(sim)
    step.terminate(sim)
    lines = open(str(tmp_path / "field.csv")).read().splitlines()
    assert step._pass == 2 and len(lines) == 2 and lines[0].startswith("0.25, %d, %d, [[[[" % (ref["exposed"].sum(), ref["scattered"].sum()))


def test_first_is_resolved_from_the_step_order():
    scat = phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0))
    for front, want in (([], True), ([phys.newton.NewtonianKinematicsStep()], True), ([scat], False),
                        ([phys.light.ScatterSphericalStep(1, 1)], False), ([layered(first=True)], False), ([make(first=True)], False),
                        ([phys.light.PathAbsorptionStep(0.5)], True)):
        step = make()
        sim = HostSim(some_objects(), steps=dict(enumerate(front + [step, phys.light.PhaseFunctionStep("hg", 0.85)])))
        step.run(sim)
        assert step.first is want and step._pass == 1, front
    given = make(first=True)                                            # what was given stays
    given.run(HostSim(some_objects(), steps={0: scat, 1: given}))
    assert given.first is True


def test_a_cloud_deck_behind_a_cloud_field_keeps_the_field_s_marks():
    field, deck = make(), layered()
    objs = some_objects(256)
    sim = HostSim(objs, steps={0: phys.newton.NewtonianKinematicsStep(), 1: field, 2: deck})
    field.run(sim)
    marks = tally.vec3(objs, "dv").copy()
    deck.run(sim)
    assert field.first is True and deck.first is False and field.scattered > 0
    after = tally.vec3(objs, "dv")
    hit_by_deck = (after != marks).any(axis=1)
    kept = marks.any(axis=1) & ~hit_by_deck
    assert kept.any() and same_bits(after[kept], marks[kept])
    alone = layered()                                                   # and without a field in front nothing has changed
    alone.run(HostSim(some_objects(), steps={0: alone}))
    assert alone.first is True
    two = [make(), make()]                                              # two fields interleave their counters (tally.WriterStep)
    sim = HostSim(some_objects(), steps=dict(enumerate(two)))
    for _ in range(2):
        for s in two:
            s.run(sim)
    assert [s._n_pass for s in two] == [3, 4] and [s.first for s in two] == [True, False]
    assert (field._n_pass, deck._n_pass) == (1, 1)                      # a field and a deck: families of their own, no interleaving


def test_refusals_come_before_the_pass_moves():
    scat = phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0))
    step = make()
    with pytest.raises(ValueError, match="ScatterIsotropicStep behind this GridScatterStep") as e:
        step.run(HostSim(some_objects(), steps={0: step, 1: scat}))
    assert step._pass == 0 and step.data == [] and step.first is None
    twin = layered()                                                    # worded as LayeredScatterStep's message
    with pytest.raises(ValueError) as theirs:
        twin.run(HostSim(some_objects(), steps={0: twin, 1: scat}))
    assert str(e.value) == str(theirs.value).replace("LayeredScatterStep", "GridScatterStep")
    for step, steps in ((make(first=False), {}), (make(), {0: scat})):     # first=False, given or resolved, under cl_on=False
        steps[5] = step
        with pytest.raises(ValueError, match=r"GridScatterStep\(first=False\) needs cl_on=True.*dv = v_old") as e:
            step.run(HostSim(some_objects(), py=True, steps=steps))
        assert step._pass == 0 and step.data == [] and "cannot be read off the store" in str(e.value)

        class Sim(HostSim):                                            # the device path refuses as well, before the sweep
            _residency = "device"
        with pytest.raises(ValueError, match="needs cl_on=True"):
            step._device_run(Sim([], py=True, steps=steps))
        assert step._pass == 0
    step = make()
    with pytest.raises(ValueError, match="dt must be finite"):
        step.run(HostSim(some_objects(), steps={0: step}, dt=-1.0))
    assert step._pass == 0 and step.data == []


def test_a_real_simulation_resolves_and_refuses_on_the_host_path():
    """``_refuse`` reads ``Simulation.steps`` itself, not a stand-in's: host-resident objects, no device."""
    def sim_of(*steps):
        sim = phys.Simulation(cl_on=False, seed=SEED)
        sim.add_objs(some_objects())
        sim.dt = np.double(0.5 / C)
        for k, s in enumerate(steps):
            sim.add_step(k, s)
        return sim
    scat = phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0))
    step = make()
    with pytest.raises(ValueError, match="behind this GridScatterStep"):
        step.run(sim_of(step, scat))
    step = make()
    with pytest.raises(ValueError, match="needs cl_on=True"):
        step.run(sim_of(scat, step))                                    # resolved to False under cl_on=False
    assert step._pass == 0
    step, deck = make(), layered()
    sim = sim_of(phys.newton.NewtonianKinematicsStep(), step, deck)
    step.run(sim)
    assert step.first is True and step._pass == 1 and step.exposed > 0
    with pytest.raises(ValueError, match=r"LayeredScatterStep\(first=False\) needs cl_on=True"):
        deck.run(sim)                                                   # resolved to False by the field in front of it


# ------------------------------------------------------------------------------------------------ the device path, with stand-ins
def test_device_run_reduces_a_row_of_2_to_the_20_cells_in_chunks():
    shape = (128, 128, 64)
    cells = (np.arange(2 ** 20, dtype=np.int64) % 5).reshape(shape)

    class Dev:
        count, calls = 1000, []

        def scatter_grid(self, *a):
            self.calls.append(a)
            return 9, 4, cells

    class Sim:
        t, seed, launch_note, _dev, _scattered = 0.5, 99, None, Dev(), False

        def __init__(self):
            self.steps, self.chunks = {}, []

        def _k_wanted(self):
            return 32

        def _py_semantics(self):
            return False

        def _dt_code(self):
            return 0.5 / light._c_h_literals()[0]

        def _global(self, values):
            self.chunks.append(len(values))
            return np.asarray(values, dtype=np.int64) * 2               # two ranks with the same tallies
    sim = Sim()
    axes, edges = ("x", "y", "z"), grid_edges(("x", "y", "z"), shape)
    step = phys.light.GridScatterStep(2.0, axes, edges, CENTER)
    sim.steps = {0: phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)), 1: step}
    step._device_run(sim)
    assert sim.launch_note == step._NOTE and sim._scattered and step.first is False
    assert (step.exposed, step.scattered) == (18, 8) and same_bits(step.scattered_by_cell, 2 * cells)
    payload = 1 + 2 + 2 ** 20                                          # N, the two counts, the cells: 512 whole chunks and one of 3
    assert sim.chunks == [tally.ALLREDUCE_CHUNK] * 512 + [3] and sum(sim.chunks) == payload
    (a,) = Dev.calls
    assert same_bits(a[0], np.full(shape, -np.expm1(-(2.0 * 0.5)))) and a[1] == axes and a[3].tolist() == CENTER.tolist()
    assert a[4] is None and a[5] is False and a[6] == light._c_h_literals()[0] and (a[7], a[8]) == (99, 1)


def test_multi_device_sums_the_shards_tallies():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def scatter_grid(self, *a, **kw):
            return 3 * self.k, self.k, self.k * np.array([[1, 2], [3, 4]])
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    exposed, scattered, cells = md.scatter_grid(np.full((2, 2), 0.5), ("x", "y"), [[0, 1, 2], [0, 1, 2]], None, None, True, C, 1, 1)
    md._pool.shutdown()
    assert (int(exposed), int(scattered)) == (333, 111) and np.asarray(cells).tolist() == [[111, 222], [333, 444]]


def test_binding_marshals_the_call():
    def entry(handle, n_axes, coords, n_bins, ed, ce, B, Ee, p, first, c, seed, n_pass, counts, cells):
        dbl = lambda q, k: None if q is None else np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_double)), (k,)).tolist()   # noqa: E731
        i32 = lambda q, k: np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_int32)), (k,)).tolist()                          # noqa: E731
        bins = i32(n_bins, n_axes)
        n_p = int(np.prod(bins)) * max(B, 1)
        seen.append((handle, n_axes, i32(coords, n_axes), bins, dbl(ed, sum(bins) + n_axes), dbl(ce, 3), B, dbl(Ee, B + 1), dbl(p, n_p), first,
                     c, seed, n_pass))
        np.ctypeslib.as_array(ctypes.cast(counts, ctypes.POINTER(ctypes.c_int64)), (2,))[:] = [100, 50]
        np.ctypeslib.as_array(ctypes.cast(cells, ctypes.POINTER(ctypes.c_int64)), (n_p,))[:] = np.arange(n_p)
        return 0
    seen = []
    exposed, scattered, cells = _hip._scatter_grid(entry, "h", [0.5, 0.25], ("z", "r"), [[0.0, 1.0], [1.0, 2.0]], CENTER,
                                                   [1.0, 1.5, 3.0], False, C, -1, 2 ** 32 + 3)
    assert (exposed, scattered) == (100, 50) and cells.tolist() == [[[0, 1]]] and cells.dtype == np.int64
    exposed, scattered, cells = _hip._scatter_grid(entry, "h", np.arange(6) / 8.0, ("x", "y"), [[0.0, 1.0, 2.0], [0.0, 1.0, 2.0, 3.0]], None, None,
                                                   True, C, 1, 1)
    assert cells.tolist() == [[0, 1, 2], [3, 4, 5]]
    assert seen[0] == ("h", 2, [2, 3], [1, 1], [0.0, 1.0, 1.0, 2.0], CENTER.tolist(), 2, [1.0, 1.5, 3.0], [0.5, 0.25], 0, C, 2 ** 64 - 1, 3)
    assert seen[1][1:10] == (2, [0, 1], [2, 3], [0.0, 1.0, 2.0, 0.0, 1.0, 2.0, 3.0], None, 0, None, (np.arange(6) / 8.0).tolist(), 1)
    with pytest.raises(ValueError, match="p holds 3 values"):
        _hip._scatter_grid(entry, "h", [0.5, 0.5, 0.5], ("x",), [[0.0, 1.0, 2.0]], None, None, True, C, 1, 1)
    with pytest.raises(ValueError, match="one sequence of edges per axis"):
        _hip._scatter_grid(entry, "h", [0.5], ("x", "y"), [[0.0, 1.0]], None, None, True, C, 1, 1)
    assert len(_hip._PROTOTYPES[ENTRIES[0]]) == len(_hip._PROTOTYPES[ENTRIES[1]]) == 15


# ------------------------------------------------------------------------------------------------ the counter words
def test_the_counter_words_are_named_constants_used_once_and_nowhere_else():
    src = open(os.path.join(build.CSRC, "pcl_surface.hip")).read()
    assert re.findall(r"\b(kGridScatterD\w+) = (\d+), (kGridScatterD\w+) = (\d+)", src) == [("kGridScatterDraw", "25", "kGridScatterDir", "26")]
    for name in ("kGridScatterDraw", "kGridScatterDir"):
        assert len(re.findall(r"pcl_philox4x32_10\([^;]*?, %s, " % name, src)) == 1 and len(re.findall(r"\b%s\b" % name, src)) == 2
    body = src[src.index("void __launch_bounds__(kBlock) k_scatter_grid"):src.index("struct gscatter_spec")]
    assert sorted(re.findall(r"pcl_philox4x32_10\([^;]*?, (\w+), a\.k0", body)) == ["kGridScatterDir", "kGridScatterDraw"]
    assert "__dsub_rn(vk, vo)" in body and "flush_cells, written out" in body and "flush_cells(" not in body
    assert body.index("if (!hit) continue;") > body.rindex("__ballot(") and "asm" not in body
    for f in sorted(os.listdir(build.CSRC)):                            # no other kernel draws from 25 or 26, by literal or by constant
        if f.endswith((".hip", ".h", ".inc")):
            text = open(os.path.join(build.CSRC, f)).read()
            words = [int(w) for w in re.findall(r"pcl_philox4x32_10\([^;]*?, (\d+)u, ", text)]
            words += [int(w) for k, w in re.findall(r"\b(k[A-Z]\w+) = (\d+)", text) if not k.startswith("kGridScatterD")]
            assert 25 not in words and 26 not in words, f
    tree = ast.parse(open(light.__file__).read())
    calls = [n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "id", "") == "_philox_block"]
    literal = [n.args[3].value for n in calls if isinstance(n.args[3], ast.Constant)]
    assert calls and 25 not in literal and 26 not in literal
    holders = [n for n in ast.walk(tree) if isinstance(n, ast.Assign) and isinstance(n.value, ast.Tuple)
               and [getattr(e, "value", None) for e in n.value.elts] == [25, 26]]
    assert [h.targets[0].id for h in holders] == ["_GRID_SCATTER_WORDS"]


# ------------------------------------------------------------------------------------------------ the library
def surface_unit():
    (unit,) = [u for u in build.ADDONS if os.path.basename(u["src"]) == "pcl_surface.hip"]
    return unit


def test_header_prototypes_and_the_build_table():
    text = open(build.ABI_HEADER).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and len(_hip._PROTOTYPES[entry]) == 15
    assert re.search(r"#define PCL_SCATTER_GRID_MAX_CELLS \(1 << 20\)", code) and re.search(r"#define PCL_GRID_MAX_CELLS \(1 << 20\)", code)
    assert re.search(r"#define PCL_SCATTER_GRID_MAX_BANDS 1024\b", code)
    src = open(os.path.join(build.CSRC, "pcl_surface.hip")).read()
    assert "static_assert(PCL_SCATTER_GRID_MAX_CELLS == PCL_GRID_MAX_CELLS" in src
    flat = " ".join(text.split()).replace("* ", "")
    assert "words 25 and 26 are used by nothing else" in flat and "0-5 and 8-26 are taken" in flat
    for line in ("(id_lo, id_hi, pass, 25)", "(id_lo, id_hi, pass, 26)", "scattered iff u < p", "w = (1, 0, 0); mu = 1 - 2*u_a",
                 "first == 0: the particle is not written at all", "first == 1: dv = 0 for every photon that is not scattered",
                 "the last one closed", "p = -expm1(-k (c*dt))", "q = ((x-cx)*(x-cx) + (y-cy)*(y-cy)) + (z-cz)*(z-cz)", "row-major",
                 "8 MB up and 8 MB down per call", "64 KiB", "nothing is cached between calls"):
        assert line in flat, line                                      # the rule and its cost are written out
    assert hasattr(_hip.Device, "scatter_grid") and hasattr(_hip.DeviceGroup, "scatter_grid")
    from physicl_amd.multidev import MultiDevice
    assert hasattr(MultiDevice, "scatter_grid")
    # the table: the unit of the writer sweeps holds this one, described as every sweep is (tests/test_build_cpu.py checks it as one)
    assert dict(entries=ENTRIES, kernel="k_scatter_grid", count=4) in surface_unit()["sweeps"]
    assert build.csrc_sha() == "b54e0443ee3f400f"                       # the tuned core has not moved


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context and a NULL group, refused as well); the outputs stay as
    they were."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in BAD_CALLS:
        keep, args, (counts, cells) = abi_args(**kw)
        assert lib.pcl_step_scatter_grid(None, *args) == -2, kw
        assert lib.pcl_group_step_scatter_grid(None, *args) == -2, kw
        assert (counts is None or (counts == -7).all()) and (cells is None or (cells == -7).all()), kw
    keep, args, (counts, cells) = abi_args()                           # a good call without a context is refused, too
    assert lib.pcl_step_scatter_grid(None, *args) == -2 and lib.pcl_group_step_scatter_grid(None, *args) != 0
    assert (counts == -7).all() and (cells == -7).all()


# ------------------------------------------------------------------------------------------------ past the first trip
@pytest.mark.parametrize("size", ["N2", "N3"])
def test_the_run_cases_send_waves_from_cell_to_cell_between_trips(size):
    """tests/test_scatter_grid_trips_gpu.py's patterns, by their own arithmetic and without a device (256 CUs): a wave stands in one
    cell per trip, and over the waves the runs end, wait through a clear cell and are taken up again."""
    from test_scatter_grid_trips_gpu import PATTERNS, pattern, sequences, stride_of
    from test_writer_trips_gpu import slots
    cap = 256 * 8 * 256
    n = slots(cap, size)
    stride = stride_of(n, 256)
    trips = {"N2": 2, "N3": 3}[size]
    assert stride % 64 == 0 and (trips - 1) * stride < n <= trips * stride
    found = {}
    for name in PATTERNS:
        where, rest = pattern(name, n, cap, stride)
        waves = where[:n // 64 * 64].reshape(-1, 64)
        assert (waves == waves[:, :1]).all(), name                      # every wave in one cell, in every trip
        found[name], t = sequences(where, stride)
        assert t == trips and rest.any() == (name == "per_wave")
    assert found["one_cell"] == {"A" * trips} and found["by_trip"] == {"AZA"[:trips]}
    assert len(found["below_and_above_cap"]) >= 2 and any("AB" in q for q in found["below_and_above_cap"])
    assert {"AB", "AZ", "ZA", "BA", "AA"} <= {q[:2] for q in found["per_wave"]}
    if trips == 3:
        assert {"AZA", "ABA", "AAB", "ZAB"} <= found["per_wave"]
