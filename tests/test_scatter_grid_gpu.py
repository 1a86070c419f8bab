"""GPU: GridScatterStep (pcl_step_scatter_grid, light.GridScatterStep).

* ``Device.scatter_grid`` against the plain loop of tests/scatter_grid_reference.py (Python integers and floats, no light.py) on the
  edge scene, uploaded explicitly and downloaded before and after the call, N = 2049 (a tile and a slot, a ragged last wave), fp64 and
  fp32 stores, ``first`` 0 and 1: the LDS form (4 x 4 x 4 cells; 2 x 2 x 2 cells by 3 bands; a z-by-radius grid), the global form
  forced by size (17 x 16 x 16 = 4352 cells, just above the switch at 4096) and 128 x 128 x 64 cells with k zero outside five of
  them.  Who is exposed, who is hit, every cell, the rows that are not written and the dv = 0 rows have no tolerance; v and dv of the
  hit rows have the bound tests/writer_reference.py derives for a direction made by frame / polar / turned.
* every photon in one cell with p = 1, both forms: the wave-wide add of a run of hits; p = 0 everywhere; a mixed store with plain
  Objects and ids that are not consecutive; seeds and passes at full width; the refusals; an empty store; a device group.
* through ``Simulation``: 6 passes of Newton, ScatterIsotropicStep, GridScatterStep (``first`` resolved to False), LayeredPhaseStep
  and a PositionGridMeasureStep on the same axes and edges, every pass replayed from the probed state in front of the step -- at
  N = 16 385 with light._scatter_grid, the numpy restatement, which tests/test_scatter_grid_cpu.py holds bit for bit to the loop.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
import writer_reference as W
from physicl_amd import light
from scatter_grid_reference import (BAD_CALLS, C, CENTER, E_EDGES, ID_BASE, SEED, abi_args, assert_every_outcome, check_scatter_grid,
                                    grid_edges, probabilities, scatter_grid_loop, scene)
from writer_reference import same_bits

pytestmark = pytest.mark.gpu

N = 2049
FIELDS = ("r", "v", "dr", "dv")
XYZ = ("x", "y", "z")
# name -> (axes, bins, bands): the first three take the LDS form, the last the global one
GRIDS = {"lds 4x4x4": (XYZ, (4, 4, 4), False), "lds 2x2x2x3": (XYZ, (2, 2, 2), True), "lds z,r": (("z", "r"), (3, 4), True),
         "global 17x16x16": (XYZ, (17, 16, 16), False)}


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


def upload(dev, state, dtype, ids=None, kind=None):
    state = dict(state, id_base=ID_BASE)
    if ids is not None:
        state["id"] = ids
    if kind is not None:
        state["kind"] = kind
    dev.store_alloc(len(state["E"]), dtype)
    dev.upload_state(state)
    return W.snapshot(dev)


def np_type(dtype):
    return np.float32 if dtype == "f32" else np.float64


def check_call(dev, before, p, axes, edges, E_edges, first, seed, n_pass, what, every=True):
    answer = dev.scatter_grid(p, axes, edges, CENTER, E_edges, first, C, seed, n_pass)
    after = W.snapshot(dev)
    ref = check_scatter_grid(before, after, answer, p, axes, edges, CENTER, E_edges, first, C, seed, n_pass, what, restate=scatter_grid_loop)
    if every:
        assert_every_outcome(ref, W.wide(before)["v"], W.photons(before), E_edges, what)
    return answer, after, ref


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_every_particle_against_the_plain_loop(dev, grid, dtype, first):
    axes, bins, bands = GRIDS[grid]
    edges = grid_edges(axes, bins)
    E_edges = E_EDGES if bands else None
    p = probabilities(tuple(bins) + ((3,) if bands else ()))
    before = upload(dev, scene(N, axes, edges, np_type(dtype)), dtype)
    answer, after, ref = check_call(dev, before, p, axes, edges, E_edges, first, SEED, 1, "%s %s first=%d" % (grid, dtype, first))
    assert dev.is_uniform() and answer[2].shape == p.shape and not answer[2][p == 0.0].any() and 0 < answer[1] < answer[0] < N
    check_call(dev, after, p, axes, edges, E_edges, first, SEED, 2, "%s %s first=%d, second pass" % (grid, dtype, first))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_field_of_2_to_the_20_cells_with_k_zero_outside_a_handful(dev, dtype):
    bins = (128, 128, 64)
    edges = grid_edges(XYZ, bins)
    spots = np.array([[0.01, 0.01, 0.01], [-1.99, -1.99, -1.99], [1.99, 1.99, 1.99], [0.51, -0.77, 1.3], [-1.2, 0.4, -0.6]])
    state = scene(N, XYZ, edges, np_type(dtype))
    odd = np.arange(N) % 2 == 1
    state["r"][odd] = spots[(np.arange(N)[odd] // 2) % 5].astype(np_type(dtype)).astype(np.float64)
    cells = tuple(np.array([np.searchsorted(e, s, side="right") - 1 for e, s in zip(edges, spots.T)]))
    p = np.zeros(bins)
    p[cells] = [1.0, 0.5, 0.5, 0.25, 0.75]
    assert len(set(zip(*cells))) == 5
    before = upload(dev, state, dtype)
    for first in (1, 0):
        answer, before, ref = check_call(dev, before, p, XYZ, edges, None, first, SEED, 3 + first, "128x128x64 %s first=%d" % (dtype, first))
        got = np.asarray(answer[2])
        assert got.shape == bins and int(got.sum()) == int(got[cells].sum()) == answer[1] and (got[cells] > 0).all()
        assert answer[0] > N // 2 and got[cells][0] >= 150            # the p = 1 cell: every moving photon that stands in it


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("form", ["lds 4x4x4", "global 17x16x16"])
def test_every_photon_in_one_cell_with_p_one(dev, form, dtype):
    """What every bulk run starts from: whole waves hit in one cell -- one add of the wave's count (one trip at this size; the run
    carried from trip to trip is held by tests/test_scatter_grid_trips_gpu.py)."""
    axes, bins, _ = GRIDS[form]
    edges = grid_edges(axes, bins)
    rng = np.random.RandomState(2)
    u = rng.normal(size=(N, 3))
    state = {"r": np.tile([0.3, -0.6, 1.1], (N, 1)), "v": C * u / np.sqrt((u * u).sum(axis=1))[:, None], "dr": np.zeros((N, 3)),
             "dv": rng.normal(size=(N, 3)), "E": np.full(N, 2.0)}
    state = {k: a.astype(np_type(dtype)).astype(np.float64) for k, a in state.items()}
    before = upload(dev, state, dtype)
    for first in (1, 0):
        answer, before, ref = check_call(dev, before, np.ones(bins), axes, edges, None, first, SEED, 5 + first,
                                         "one cell %s %s first=%d" % (form, dtype, first), every=False)
        got = np.asarray(answer[2])
        assert answer[:2] == (N, N) and got.max() == N == got.sum() and ref["scattered"].all()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("form", ["lds 2x2x2x3", "global 17x16x16"])
def test_clear_cells_write_nothing_but_the_first_scatterer_s_zeros(dev, form, dtype):
    axes, bins, bands = GRIDS[form]
    edges = grid_edges(axes, bins)
    E_edges = E_EDGES if bands else None
    p = np.zeros(tuple(bins) + ((3,) if bands else ()))
    before = upload(dev, scene(N, axes, edges, np_type(dtype)), dtype)
    answer, after, ref = check_call(dev, before, p, axes, edges, E_edges, 0, SEED, 1, "clear %s %s first=0" % (form, dtype), every=False)
    assert answer[0] > 0 and answer[1] == 0 and not np.asarray(answer[2]).any()
    W.assert_same_state(after, before, "p = 0, first = 0: nothing is written")
    answer, last, ref = check_call(dev, after, p, axes, edges, E_edges, 1, SEED, 2, "clear %s %s first=1" % (form, dtype), every=False)
    assert answer[1] == 0 and ref["written"].all()
    a, b = W.wide(last), W.wide(after)
    assert not a["dv"].any() and all(same_bits(a[f], b[f]) for f in ("r", "v", "dr")) and same_bits(last["E"], after["E"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("form", ["lds 2x2x2x3", "global 17x16x16"])
def test_plain_objects_and_ids_of_their_own(dev, hip, form, dtype):
    axes, bins, bands = GRIDS[form]
    edges = grid_edges(axes, bins)
    E_edges = E_EDGES if bands else None
    p = probabilities(tuple(bins) + ((3,) if bands else ()))
    ids = ID_BASE + 3 * np.random.RandomState(5).permutation(N).astype(np.int64)            # explicit, not consecutive
    kind = np.where(np.arange(N) % 4 == 1, hip.KIND_OBJECT, hip.KIND_PHOTON).astype(np.uint8)
    state = scene(N, axes, edges, np_type(dtype))
    for use_kind in (None, kind):                                      # the ids alone, then with plain Objects among the photons
        before = upload(dev, state, dtype, ids=ids, kind=use_kind)
        assert not dev.is_uniform()
        for first in (1, 0):
            what = "%s %s ids%s first=%d" % (form, dtype, "" if use_kind is None else " and Objects", first)
            answer, after, ref = check_call(dev, before, p, axes, edges, E_edges, first, SEED, 8 + first, what)
            if use_kind is not None:
                obj = kind == hip.KIND_OBJECT
                b, a = W.wide(before), W.wide(after)
                assert not ref["written"][obj].any() and all(same_bits(a[f][obj], b[f][obj]) for f in FIELDS)
            before = after
    plain = upload(dev, state, dtype)                                  # the same photons under other ids draw other numbers
    other = dev.scatter_grid(p, axes, edges, CENTER, E_edges, 0, C, SEED, 9)
    assert other[0] > answer[0] and other[1] != answer[1]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("seed, n_pass", [(2 ** 64 - 1, 2 ** 32 - 1), (2 ** 32, 2 ** 31)])
def test_seeds_and_passes_at_full_width(dev, seed, n_pass, dtype):
    for form in ("lds 4x4x4", "global 17x16x16"):
        axes, bins, _ = GRIDS[form]
        edges = grid_edges(axes, bins)
        before = upload(dev, scene(N, axes, edges, np_type(dtype)), dtype)
        check_call(dev, before, probabilities(bins), axes, edges, None, 1, seed, n_pass, "%s %s seed %#x pass %#x" % (form, dtype, seed, n_pass))


def test_refused_calls_and_an_empty_store(dev, hip):
    axes, bins = XYZ, (2, 2, 2)
    edges = grid_edges(axes, bins)
    before = upload(dev, scene(300, axes, edges, np.float64), "f64")
    for kw in BAD_CALLS:
        keep, args, (counts, cells) = abi_args(**kw)
        assert dev.lib.pcl_step_scatter_grid(dev.ctx, *args) == -2, kw
        assert (counts is None or (counts == -7).all()) and (cells is None or (cells == -7).all()), kw
    W.assert_same_state(W.snapshot(dev), before, "a refused call writes nothing")
    with pytest.raises(ValueError, match="p holds"):
        dev.scatter_grid([0.5, 0.5], axes, edges, CENTER, None, True, C, SEED, 1)
    keep, good, (counts, cells) = abi_args()
    assert dev.lib.pcl_step_scatter_grid(dev.ctx, *good) == 0
    p = probabilities((2, 2, 2, 3))
    ref = check_scatter_grid(before, W.snapshot(dev), (counts[0], counts[1], cells[:24].reshape(2, 2, 2, 3)), p, axes, edges, CENTER, E_EDGES, 1, C,
                             1, 1, "by hand", restate=scatter_grid_loop)
    assert ref["scattered"].any() and (counts[2:] == -7).all() and (cells[24:] == -7).all()  # two counts and 24 cells, no more
    dev.set_count(0, 0)
    empty = dev.scatter_grid(p, axes, edges, CENTER, E_EDGES, True, C, SEED, 1)
    assert empty[:2] == (0, 0) and empty[2].shape == (2, 2, 2, 3) and not empty[2].any()
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.scatter_grid(0.5, ("x",), [[0.0, 1.0]], None, None, True, C, SEED, 1)
    assert e.value.code == -3
    bare.close()


@pytest.mark.parametrize("form", ["lds 4x4x4", "global 17x16x16"])
def test_device_group_gives_the_unsharded_store(dev, hip, form):
    n = 3 * 2048 + 77
    axes, bins, _ = GRIDS[form]
    edges = grid_edges(axes, bins)
    p = probabilities(bins)
    before = upload(dev, scene(n, axes, edges, np.float64), "f64")
    whole = dev.scatter_grid(p, axes, edges, CENTER, None, 1, C, SEED, 4)
    with hip.DeviceGroup([0, 0]) as g:
        g.store_alloc(n)
        g.fill_photons(n, ID_BASE, C, 1.0, 2.0, SEED)
        for i in range(2):                                             # the shards' rows through their own contexts
            lo, hi = g.shard(n, i)
            ctx = hip.c_void_p()
            hip.check(g.lib.pcl_group_ctx(g.g, i, hip.byref(ctx)))
            for f, name in ((f, name) for name in FIELDS for f in hip.FIELD_GROUPS[name]):
                col = np.ascontiguousarray(before[name][f - hip.FIELD_GROUPS[name][0]][lo:hi])
                hip.check(g.lib.pcl_store_upload(ctx, f, col.ctypes.data, 0, hi - lo))
            col = np.ascontiguousarray(before["E"][lo:hi])
            hip.check(g.lib.pcl_store_upload(ctx, hip.E, col.ctypes.data, 0, hi - lo))
        got = g.scatter_grid(p, axes, edges, CENTER, None, 1, C, SEED, 4)
        assert got[:2] == whole[:2] and np.array_equal(got[2], whole[2]) and 0 < whole[1] < whole[0]
        for f in range(hip.E + 1):
            assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            g.scatter_grid(np.full(bins, 1.5), axes, edges, CENTER, None, 1, C, SEED, 4)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 16385, 6
STEP = 0.5                             # length of a move: A*n*|dr| = 0.25, a quarter of the photons scatter in the clear air per pass
DT = STEP / C
SIM_BINS = (8, 8, 8)
SIM_EDGES = [np.linspace(0.0, 4.0, 9), np.linspace(-2.0, 2.0, 9), np.linspace(-2.0, 2.0, 9)]
ix, iy, iz = np.indices(SIM_BINS)
FIELD_K = np.where((ix + iy) % 2 == 0, 1.2, 0.0)                       # columns along z, cloudy and clear in a checkerboard
STATE = ("r", "v", "dr", "dv", "E", "id")


class Look(phys.DeviceStep):
    """The store as it stands, pass by pass, and the pass counter the step in front was handed."""
    _fuse_role = None

    def __init__(self, watch=None):
        self.states, self.n_pass, self.watch = [], [], watch

    def _device_run(self, sim):
        self.states.append({f: sim.download(f) for f in STATE})
        self.n_pass.append(None if self.watch is None else self.watch._n_pass)


def test_a_cloud_field_behind_the_clear_air_replays_from_the_probed_states():
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=lambda s: len(s.ts) >= PASSES)
    src = phys.light.PhotonSource(origin=(2.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), angular="isotropic")
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    field = phys.light.GridScatterStep(FIELD_K, XYZ, SIM_EDGES)
    phase = phys.light.LayeredPhaseStep([("hg", 0.85)])
    where = phys.light.PositionGridMeasureStep(None, XYZ, SIM_EDGES)
    looks = [Look(), Look(field)]
    steps = [phys.UpdateTimeStep(lambda s: np.double(DT)), phys.newton.NewtonianKinematicsStep(),
             phys.light.ScatterIsotropicStep(A=np.double(0.5), n=np.double(1.0)), looks[0], field, looks[1], phase, where]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    seed, note = sim.seed, sim.launch_note
    sim.close(download=False)
    c_lit = light._c_h_literals()[0]
    p = light._path_probability(FIELD_K, c_lit, DT)
    assert field.first is False and field._pass == PASSES == len(field.data) == len(where.data) and note == field._NOTE
    total = np.zeros(SIM_BINS, dtype=np.int64)
    for k in range(PASSES):
        s0, s1 = (look.states[k] for look in looks)
        row, n_pass = field.data[k], looks[1].n_pass[k]
        what = "pass %d" % (k + 1)
        assert n_pass == k + 1, what
        ref = check_scatter_grid(s0, s1, (row[1], row[2], row[3]), p, XYZ, SIM_EDGES, np.zeros(3), None, False, c_lit, seed, n_pass, what)
        marked = W.wide(s0)["dv"].any(axis=1) & ~ref["scattered"]       # the clear air's hits survive where the field did not hit
        assert marked.any() and same_bits(W.wide(s1)["dv"][marked], W.wide(s0)["dv"][marked]), what
        grid = np.asarray(where.data[k][2])
        assert grid.shape == SIM_BINS and not np.asarray(row[3])[grid == 0].any() and not np.asarray(row[3])[FIELD_K == 0.0].any(), what
        assert int(grid.sum()) >= int(row[1]) >= int(row[2]) > 0, what  # exposed: the moving photons with a cell
        total += np.asarray(row[3])
    print("scattered by column over %d passes: %s" % (PASSES, total.sum(axis=2).tolist()))
    assert (total.sum(axis=2)[(ix + iy)[:, :, 0] % 2 == 0] > 0).sum() >= 8
