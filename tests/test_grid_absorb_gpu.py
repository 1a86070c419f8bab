"""GPU: GridAbsorptionStep (pcl_step_absorb_grid, light_grid.GridAbsorptionStep).  Nothing has a tolerance.

* ``Device.absorb_grid`` slot by slot against the numpy restatement (light_grid._grid_absorb, which tests/test_grid_absorb_cpu.py holds
  bit for bit to a loop on Python integers) on the state downloaded before and after the call: stores of 1, 63, 64, 65, 2047, 2049
  and 4173 slots (the last spans tiles, has a ragged last wave and a last tile that is not full), fp64 and fp32, explicit scrambled
  ids above 2^32 and plain Objects among the photons; one cell, three bins of x, a radius axis, 4 x 4 x 4 cells by three bands,
  16 x 16 x 16 cells -- the LDS form with one table, the global form with two -- and 17 x 16 x 16, the global form always; with k
  alone, omega0 alone and both; tables of zeros, of ones and mixed.
* two cross-checks against older kernels, bit for bit: p = 1 on a radius axis is ``Device.absorb_path`` with p = 1 on the same layers,
  omega0 = 0 on a radius axis is ``Device.absorb_scattered`` with omega0 = 0 there.
* the refusals, an empty store, a store without ids to stage, a device group and ``MultiDevice``.
* through ``Simulation``: 4 096 photons over 6 passes of Newton, ScatterIsotropicStep, GridScatterStep, GridPhaseStep, two
  GridAbsorptionSteps (both tables; k alone) and BoxBoundaryStep, every pass replayed from the probed state in front of the step.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
import writer_reference as W
from physicl_amd import light, light_grid
from grid_absorb_reference import (BAD_CALLS, C, CENTER, E_EDGES, ID_BASE, SEED, TABLES, abi_args, assert_every_outcome, check_grid_absorb,
                                   grid_edges, scene, tables)
from writer_reference import same_bits

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 2047, 2049, 4173)
XYZ = ("x", "y", "z")
# name -> (axes, bins, bands)
GRIDS = {"one cell": (("x",), (1,), False), "x 3": (("x",), (3,), False), "r": (("r",), (4,), False), "4x4x4x3": (XYZ, (4, 4, 4), True),
         "16x16x16": (XYZ, (16, 16, 16), False), "17x16x16": (XYZ, (17, 16, 16), False)}


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


def np_type(dtype):
    return np.float32 if dtype == "f32" else np.float64


def upload(dev, state, dtype, ids=None, kind=None):
    state = dict(state, id_base=ID_BASE)
    if ids is not None:
        state["id"] = ids
    if kind is not None:
        state["kind"] = kind
    dev.store_alloc(len(state["E"]), dtype)
    dev.upload_state(state)
    return W.snapshot(dev)


def mixed_store(dev, hip, n, axes, edges, dtype):
    """The edge scene under explicit scrambled ids above 2^32, every fourth slot a plain Object."""
    ids = ID_BASE + 3 * np.random.RandomState(5).permutation(n).astype(np.int64)
    kind = np.where(np.arange(n) % 4 == 1, hip.KIND_OBJECT, hip.KIND_PHOTON).astype(np.uint8)
    return upload(dev, scene(n, axes, edges, np_type(dtype)), dtype, ids=ids, kind=kind)


def lds_form(hip, bins, bands, which):
    cells = int(np.prod(bins)) * (3 if bands else 1)
    return hip.absorb_grid_lds_form(2 if which == "both" else 1, sum(b + 1 for b in bins) + (4 if bands else 0), cells)


def check_call(dev, before, p, om, axes, edges, E_edges, seed, n_pass, what):
    answer = dev.absorb_grid(p, om, axes, edges, CENTER, E_edges, seed, n_pass)
    after = W.snapshot(dev)
    return answer, after, check_grid_absorb(before, after, answer, p, om, axes, edges, CENTER, E_edges, seed, n_pass, what)


def fixed(grid, p, om):
    """One cell has one value per table: neither 0 nor 1, so that the cell shows every outcome."""
    if grid != "one cell":
        return p, om
    return tuple(None if t is None else np.full(t.shape, x) for t, x in ((p, 0.25), (om, 0.5)))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_every_slot_against_the_restatement(dev, hip, grid, dtype):
    axes, bins, bands = GRIDS[grid]
    edges = grid_edges(axes, bins)
    E_edges = E_EDGES if bands else None
    shape = tuple(bins) + ((3,) if bands else ())
    forms = {which: lds_form(hip, bins, bands, which) for which in TABLES}
    assert forms == {"16x16x16": dict(k=True, omega0=True, both=False), "17x16x16": dict(k=False, omega0=False, both=False)}.get(
        grid, dict(k=True, omega0=True, both=True)), forms
    for n in SIZES:
        for which in TABLES:
            p, om = fixed(grid, *tables(shape, which))
            before = mixed_store(dev, hip, n, axes, edges, dtype)
            assert not dev.is_uniform() or n == 1
            what = "%s %s n=%d %s" % (grid, dtype, n, which)
            answer, after, ref = check_call(dev, before, p, om, axes, edges, E_edges, SEED, 1, what)
            obj = ~W.photons(before)
            assert not ref["exposed"][obj].any() and all(same_bits(W.wide(after)[f][obj], W.wide(before)[f][obj]) for f in W.FIELDS), what
            if n >= 2047:
                b = W.wide(before)
                assert_every_outcome(ref, b["v"], b["dv"], W.photons(before), which, what)
                check_call(dev, after, p, om, axes, edges, E_edges, SEED, 2, what + ", second pass")
            elif n >= 63 and not bands:
                assert ref["exposed"].any(), what


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("grid", ["4x4x4x3", "16x16x16", "17x16x16"])
def test_tables_of_zeros_and_of_ones(dev, hip, grid, dtype):
    axes, bins, bands = GRIDS[grid]
    edges = grid_edges(axes, bins)
    E_edges = E_EDGES if bands else None
    shape = tuple(bins) + ((3,) if bands else ())
    zeros, ones = np.zeros(shape), np.ones(shape)
    n = 4173
    for which, p, om in (("k", zeros, None), ("omega0", None, ones), ("both", zeros, ones)):       # transparent and conservative
        before = mixed_store(dev, hip, n, axes, edges, dtype)
        what = "%s %s nothing absorbs, %s" % (grid, dtype, which)
        answer, after, ref = check_call(dev, before, p, om, axes, edges, E_edges, SEED, 1, what)
        assert ref["exposed"].sum() > 100 and not ref["absorbed"].any() and not np.asarray(answer[1]).any(), what
        assert ref["interacted"].any() == (which != "k"), what
        W.assert_same_state(after, before, what + ": nothing is written")
    for which, p, om in (("k", ones, None), ("omega0", None, zeros), ("both", ones, zeros), ("both", zeros, zeros)):      # black
        before = mixed_store(dev, hip, n, axes, edges, dtype)
        what = "%s %s everything absorbs, %s" % (grid, dtype, which)
        answer, after, ref = check_call(dev, before, p, om, axes, edges, E_edges, SEED, 1, what)
        want = ref["exposed"] if p is ones else ref["interacted"]
        assert want.sum() > 100 and np.array_equal(ref["absorbed"], want) and int(np.asarray(answer[1]).sum()) == int(want.sum()), what
        assert not ref["absorbed_hit"].any() if p is ones else not ref["absorbed_path"].any(), what


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("form", ["16x16x16", "17x16x16"])
def test_every_photon_in_one_cell(dev, hip, form, dtype):
    """What every bulk run starts from: whole waves absorbed in one cell -- one add of the wave's count -- in both forms."""
    axes, bins, _ = GRIDS[form]
    edges = grid_edges(axes, bins)
    n = 4173
    rng = np.random.RandomState(2)
    u = rng.normal(size=(n, 3))
    state = {"r": np.tile([0.3, -0.6, 1.1], (n, 1)), "v": C * u / np.sqrt((u * u).sum(axis=1))[:, None], "dr": np.zeros((n, 3)),
             "dv": rng.normal(size=(n, 3)), "E": np.full(n, 2.0)}
    state = {k: a.astype(np_type(dtype)).astype(np.float64) for k, a in state.items()}
    for which, p, om in (("k", np.ones(bins), None), ("both", np.full(bins, 0.5), np.zeros(bins))):
        before = upload(dev, state, dtype)
        assert dev.is_uniform() and lds_form(hip, bins, False, which) == (form == "16x16x16" and which == "k")
        answer, after, ref = check_call(dev, before, p, om, axes, edges, None, SEED, 5, "one cell %s %s %s" % (form, dtype, which))
        got = np.asarray(answer[1])
        assert ref["absorbed"].all() and got.max() == n == got.sum() and int(answer[0][0]) == n, which
        assert (int(answer[0][2]), int(answer[0][3])) == ((n, 0) if which == "k" else (int(ref["absorbed_path"].sum()), int(ref["absorbed_hit"].sum())))
        assert which == "k" or 0 < int(answer[0][2]) < n


# ------------------------------------------------------------------------------------------------ the older kernels
def radial_state(n, dtype):
    """The edge scene about a radius axis without NaN positions, every photon at rest with dv = 0: both kernels of a pair see the same
    photons (the older at-the-interaction sweep looks at dv alone and counts a photon in no layer as interacting)."""
    edges = [np.array([0.0, 0.5, 1.5, 64.0])]
    s = scene(n, ("r",), edges, np_type(dtype))
    s["r"] = np.where(np.isnan(s["r"]), 0.25, s["r"])
    s["r"][((s["r"] - CENTER) ** 2).sum(axis=1) > 60.0 ** 2] = CENTER + [1.0, 0.0, 0.0]      # (the slots planted on and beyond the last edge)
    rest = (s["v"] == 0).all(axis=1)
    s["dv"][rest] = 0.0
    assert rest.any() and (s["dv"][~rest] == 0).all(axis=1).any() and ((s["r"] - CENTER) ** 2).sum(axis=1).max() < 60.0 ** 2
    return s, edges


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_p_one_on_a_radius_axis_is_the_path_absorption_by_layer(dev, dtype):
    n = 4173
    state, edges = radial_state(n, dtype)
    p = light._path_probability(np.full(3, 1e30), C, 0.5 / C)          # k so large that p == 1.0
    assert (p == 1.0).all()
    before = upload(dev, state, dtype)
    exposed, absorbed, cells = dev.absorb_path(p, edges[0], CENTER, None, SEED, 1)
    older = W.snapshot(dev)
    assert upload(dev, state, dtype)["count"] == before["count"]      # the same state again, for the new sweep
    answer, after, ref = check_call(dev, before, p, None, ("r",), edges, None, SEED, 1, "p = 1 on r, %s" % dtype)
    W.assert_same_state(after, older, "p = 1: the store absorb_path leaves")
    assert [int(x) for x in answer[0]] == [exposed, 0, absorbed, 0] and exposed == absorbed > n // 2
    assert np.asarray(answer[1]).tolist() == np.asarray(cells).reshape(-1).tolist() and min(np.asarray(answer[1])) > 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_omega0_zero_on_a_radius_axis_is_the_absorption_at_the_interaction_by_layer(dev, dtype):
    n = 4173
    state, edges = radial_state(n, dtype)
    om = np.zeros(3)
    before = upload(dev, state, dtype)
    interacted, absorbed, by_layer, _ = dev.absorb_scattered(om, edges[0], CENTER, None, SEED, 1)
    older = W.snapshot(dev)
    assert upload(dev, state, dtype)["count"] == before["count"]
    answer, after, ref = check_call(dev, before, None, om, ("r",), edges, None, SEED, 1, "omega0 = 0 on r, %s" % dtype)
    W.assert_same_state(after, older, "omega0 = 0: the store absorb_scattered leaves")
    assert [int(x) for x in answer[0]][1:] == [interacted, 0, absorbed] and interacted == absorbed > n // 3 and int(answer[0][0]) > interacted
    assert np.asarray(answer[1]).tolist() == np.asarray(by_layer).tolist() and min(np.asarray(answer[1])) > 0


# ------------------------------------------------------------------------------------------------ refusals, the empty store, groups
def test_refused_calls_an_empty_store_and_a_uniform_store(dev, hip):
    axes, bins = XYZ, (2, 2, 2)
    edges = grid_edges(axes, bins)
    before = upload(dev, scene(300, axes, edges, np.float64), "f64")
    for kw in BAD_CALLS:
        keep, args, (counts, cells) = abi_args(**kw)
        assert dev.lib.pcl_step_absorb_grid(dev.ctx, *args) == -2, kw
        assert (counts is None or (counts == -7).all()) and (cells is None or (cells == -7).all()), kw
    W.assert_same_state(W.snapshot(dev), before, "a refused call writes nothing")
    with pytest.raises(ValueError, match="p holds"):
        dev.absorb_grid([0.5, 0.5], None, axes, edges, CENTER, None, SEED, 1)
    keep, good, (counts, cells) = abi_args()
    assert dev.is_uniform() and dev.lib.pcl_step_absorb_grid(dev.ctx, *good) == 0
    p, om = tables((2, 2, 2, 3), "both")
    ref = check_grid_absorb(before, W.snapshot(dev), (counts[:4], cells[:24].reshape(2, 2, 2, 3)), p, om, axes, edges, CENTER, E_EDGES, 1, 1, "by hand")
    assert ref["absorbed"].any() and (counts[4:] == -7).all() and (cells[24:] == -7).all()   # four counts and 24 cells, no more
    dev.set_count(0, 0)
    empty = dev.absorb_grid(p, om, axes, edges, CENTER, E_EDGES, SEED, 1)
    assert not empty[0].any() and empty[1].shape == (2, 2, 2, 3) and not empty[1].any()
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.absorb_grid(0.5, None, ("x",), [[0.0, 1.0]], None, None, SEED, 1)
    assert e.value.code == -3
    bare.close()


@pytest.mark.parametrize("form, which", [("4x4x4x3", "both"), ("16x16x16", "k"), ("16x16x16", "both")])
def test_device_group_and_multidevice_give_the_unsharded_store(dev, hip, form, which):
    from physicl_amd.multidev import MultiDevice
    n = 3 * 2048 + 77
    axes, bins, bands = GRIDS[form]
    edges = grid_edges(axes, bins)
    E_edges = E_EDGES if bands else None
    p, om = tables(tuple(bins) + ((3,) if bands else ()), which)
    before = upload(dev, scene(n, axes, edges, np.float64), "f64")
    whole = dev.absorb_grid(p, om, axes, edges, CENTER, E_edges, SEED, 4)
    assert 0 < whole[0][2] + whole[0][3] < whole[0][0]
    with hip.DeviceGroup([0, 0]) as g:
        g.store_alloc(n)
        g.fill_photons(n, ID_BASE, C, 1.0, 2.0, SEED)
        for i in range(2):                                             # the shards' rows through their own contexts
            lo, hi = g.shard(n, i)
            ctx = hip.c_void_p()
            hip.check(g.lib.pcl_group_ctx(g.g, i, hip.byref(ctx)))
            for f, name in ((f, name) for name in W.FIELDS for f in hip.FIELD_GROUPS[name]):
                col = np.ascontiguousarray(before[name][f - hip.FIELD_GROUPS[name][0]][lo:hi])
                hip.check(g.lib.pcl_store_upload(ctx, f, col.ctypes.data, 0, hi - lo))
            col = np.ascontiguousarray(before["E"][lo:hi])
            hip.check(g.lib.pcl_store_upload(ctx, hip.E, col.ctypes.data, 0, hi - lo))
        got = g.absorb_grid(p, om, axes, edges, CENTER, E_edges, SEED, 4)
        assert got[0].tolist() == whole[0].tolist() and np.array_equal(got[1], whole[1])
        for f in range(hip.E + 1):
            assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            g.absorb_grid(np.full(p.shape if p is not None else om.shape, 1.5), None, axes, edges, CENTER, E_edges, SEED, 4)
        assert e.value.code == -2

    class Shard:                                                       # MultiDevice's sum over shards, each a device of its own store
        def __init__(self, lo, hi):
            self.dev = hip.Device(0)
            part = {f: ([np.asarray(row)[lo:hi] for row in before[f]] if f in W.FIELDS else np.asarray(before[f])[lo:hi])
                    for f in before if f != "count"}
            W.upload_plain(self.dev, part, hi - lo, "f64")

        def absorb_grid(self, *a, **kw):
            return self.dev.absorb_grid(*a, **kw)

    from concurrent.futures import ThreadPoolExecutor
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(0, n // 2), Shard(n // 2, n)], ThreadPoolExecutor(max_workers=2)
    counts, cells = md.absorb_grid(p, om, axes, edges, CENTER, E_edges, SEED, 4)
    md._pool.shutdown()
    assert np.asarray(counts).tolist() == whole[0].tolist() and np.array_equal(np.asarray(cells), whole[1])
    parts = [W.snapshot(s.dev) for s in md.shards]
    for s in md.shards:
        s.dev.close()
    after = W.wide(W.snapshot(dev))
    for f in ("v", "dv"):
        assert same_bits(np.concatenate([W.wide(q)[f] for q in parts]), after[f]), f


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 4096, 6
STEP = 0.5
DT = STEP / C
SIM_BINS = (8, 8, 8)
SIM_EDGES = [np.linspace(0.0, 4.0, 9), np.linspace(-2.0, 2.0, 9), np.linspace(-2.0, 2.0, 9)]
ix, iy, iz = np.indices(SIM_BINS)
CLOUDY = (ix + iy) % 2 == 0                                            # columns along z, cloudy and clear in a checkerboard
FIELD_K = np.where(CLOUDY, 1.2, 0.0)
OMEGA0 = np.where(CLOUDY, 0.9, 1.0)                                    # the droplets absorb a tenth of their interactions
VAPOUR = np.where((ix == 5) & (iy == 3), 0.8, 0.0)                     # a column of water vapour: k along the path
STATE = ("r", "v", "dr", "dv", "E", "id")


class Look(phys.DeviceStep):
    """The store as it stands, pass by pass, and the pass counter the step in front was handed."""
    _fuse_role = None

    def __init__(self, watch=None):
        self.states, self.n_pass, self.watch = [], [], watch

    def _device_run(self, sim):
        self.states.append({f: sim.download(f) for f in STATE})
        self.n_pass.append(None if self.watch is None else self.watch._n_pass)


def test_a_cloud_field_that_absorbs_replays_from_the_probed_states():
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=lambda s: len(s.ts) >= PASSES)
    src = phys.light.PhotonSource(origin=(2.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), angular="isotropic")
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    field = phys.light.GridScatterStep(FIELD_K, XYZ, SIM_EDGES)
    phase = phys.light.GridPhaseStep(["rayleigh", ("hg", 0.85)], [[1, 0], [0.1, 0.9]], XYZ, SIM_EDGES, mixture=CLOUDY.astype(np.int64), outside=0)
    heat = phys.light.GridAbsorptionStep(XYZ, SIM_EDGES, k=VAPOUR, omega0=OMEGA0)
    again = phys.light.GridAbsorptionStep(XYZ, SIM_EDGES, k=0.05)
    walls = phys.light.BoxBoundaryStep((0.0, -2.0, -2.0), (4.0, 2.0, 2.0), "periodic")
    looks = [Look(), Look(heat), Look(again)]
    steps = [phys.UpdateTimeStep(lambda s: np.double(DT)), phys.newton.NewtonianKinematicsStep(),
             phys.light.ScatterIsotropicStep(A=np.double(0.5), n=np.double(1.0)), field, phase, looks[0], heat, looks[1], again, looks[2], walls]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    seed, note = sim.seed, sim.launch_note
    sim.close(download=False)
    c_lit = light._c_h_literals()[0]
    assert note is not None and "one launch per light step" in note
    assert heat._pass == again._pass == PASSES == len(heat.data) == len(again.data) and heat._family == (2, 0) and again._family == (2, 1)
    total = np.zeros(SIM_BINS, dtype=np.int64)
    for k in range(PASSES):
        s0, s1, s2 = (look.states[k] for look in looks)
        what = "pass %d" % (k + 1)
        assert (looks[1].n_pass[k], looks[2].n_pass[k]) == (2 * k + 1, 2 * k + 2), what      # interleaved counters
        for step, before, after, n_pass in ((heat, s0, s1, 2 * k + 1), (again, s1, s2, 2 * k + 2)):
            row = step.data[k]
            p = light._path_probability(step.k, c_lit, DT)
            ref = check_grid_absorb(before, after, (row[1:5], row[5]), p, step.omega0, XYZ, SIM_EDGES, np.zeros(3), None, seed, n_pass,
                                    "%s, %s" % (what, "both tables" if step is heat else "k alone"))
            assert ref["absorbed"].any() or k > 3, what
        row = heat.data[k]
        assert row[2] > 0 and row[1] >= row[2] and row[3] + row[4] == np.asarray(row[5]).sum(), what
        assert not np.asarray(row[5])[~CLOUDY & (VAPOUR == 0.0)].any(), what             # clear air outside the column absorbs nothing
        total += np.asarray(row[5])
    print("absorbed by column over %d passes: %s" % (PASSES, total.sum(axis=2).tolist()))
    assert total[CLOUDY].sum() > 0 and total.sum() == sum(int(r[3] + r[4]) for r in heat.data)
    assert heat.absorbed == heat.absorbed_path + heat.absorbed_hit == int(heat.absorbed_by_cell.sum())
