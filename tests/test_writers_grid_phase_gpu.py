"""GPU: GridPhaseStep (pcl_step_phase_grid, light_grid.GridPhaseStep).

* ``Device.phase_grid`` slot by slot against the numpy restatement (light_grid._grid_phase_redirect) on the state downloaded before and
  after the call, under layered_phase_reference.check_layered's conditions (grid_phase_reference.check_grid), in f64 and f32, on the
  scenes of grid_phase_reference.scenes(): 4 x 4 x 4 cells over x, y, z with three mixtures and cells that are left alone, a radius
  axis, z with a radius, the 17 x 16 x 16 field of tests/test_scatter_grid_gpu_dist.py (a map of several kilobytes), ``outside`` as a
  row and as None, a tabulated law;
* the two equivalences on the device: the same state on a twin, swept by ``phase_layered`` (a radius axis, the layers as mixtures)
  and by ``phase_redirect`` (one cell, one law, outside = 0): every field bit for bit, the tallies equal;
* the cosine left in the store against exact arithmetic, tests/test_writers_direction_exact_gpu.py's method and bounds, for every law
  of layered_phase_reference.SINGLE and a table: the kernel takes the closed-form laws from a helper of pcl_rules.h, a third
  statement of the Henyey-Greenstein inverse;
* the store states of tests/test_gpu_writer_store_states.py: behind an alive mask (S2), scrambled explicit ids above 2^32 and plain
  Objects among the photons (S5), on twin devices in f64 and f32;
* the ABI by hand: every refusal of grid_phase_reference.BAD_CALLS leaves store and output untouched; one call at the largest LDS
  size the header's bound accepts; an empty store; no store;
* through ``Simulation``: a PhotonBatch with a ScatterIsotropicStep, a GridScatterStep and the step behind them -- the rows are the
  restatement's pass by pass on downloads, and two contexts on one GPU give the same rows; ``sim.launch_note`` names the step
  where it is the pass's first writer step (behind a GridScatterStep the note is that step's, as for every writer step)."""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
import test_writers_direction_exact_gpu as X
import writer_reference as W
from physicl_amd import light, light_grid
from absorb_reference import CENTER, EDGES
from grid_phase_reference import BAD_CALLS, abi_args, args_of, call, check_grid, lds_limit_args, scenes, state_of
from layered_phase_reference import C, MIX_LAWS, MIX_WEIGHTS, SEED, SINGLE, as_phase
from test_gpu_writer_store_states import test_a_writer_sweep_on_twin_devices as twin_devices

pytestmark = pytest.mark.gpu

SCENES = scenes()
N = 4097                                                               # two tiles and a slot; the exact-arithmetic store holds 549


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def devs(hip):
    made = [hip.Device(0), hip.Device(0)]
    yield made
    for d in made:
        d.close()


@pytest.fixture(scope="module")
def dev(devs):
    return devs[0]


def upload(dev, n, dtype, state):
    dev.store_alloc(n, dtype)
    dev.upload_state(state)
    return W.snapshot(dev)


# ------------------------------------------------------------------------------------------------ slot by slot
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name", list(SCENES))
def test_every_slot_against_the_numpy_restatement(dev, name, dtype):
    scene, n_pass = SCENES[name], 2 + list(SCENES).index(name)
    before = upload(dev, N, dtype, state_of(N, dtype))
    answer = call(dev, scene, n_pass)
    ref = check_grid(before, W.snapshot(dev), answer, scene, C, SEED, n_pass, "%s %s" % (name, dtype))
    scattered, redirected, by_mixture, by_law = answer
    assert by_mixture.dtype == np.int64 and scattered == (N + 2) // 3 and dev.count == N      # every third slot was scattered
    assert 0 < redirected < scattered or scene["outside"] is not None and -1 not in scene["mixture"]
    assert by_mixture.min() > 0 and by_law.min() > 0                   # every mixture and every law has work
    nan = np.isnan(W.wide(before)["r"]).any(axis=1) & ref["scattered"]
    assert nan.sum() > 10 and ref["redirected"][nan].all() == (scene["outside"] is not None)
    if name == "field 17x16x16":
        assert scene["mixture"].size == 4352 and redirected == scattered


# ------------------------------------------------------------------------------------------------ the two equivalences
def fields_equal(a, b, what):
    for f in W.FIELDS:
        for k in range(3):
            assert W.same_bits(a[f][k], b[f][k]), (what, f, k)
    assert W.same_bits(a["E"], b["E"]) and np.array_equal(a["id"], b["id"]), what


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_radius_axis_with_its_layers_as_mixtures_is_phase_layered_bit_for_bit(devs, dtype):
    dev, twin = devs
    state = state_of(N, dtype)
    upload(dev, N, dtype, state)
    upload(twin, N, dtype, state)
    laws, _, cum, edges, center = light._check_layered_phase(MIX_LAWS, MIX_WEIGHTS, EDGES, CENTER)
    got = dev.phase_grid(laws, cum, ("r",), [edges], center, np.arange(3), None, C, SEED, 4)
    want = twin.phase_layered(laws, cum, edges, center, C, SEED, 4)
    assert got[:2] == want[:2] and got[2].tolist() == want[2].tolist() and got[3].tolist() == want[3].tolist()
    assert 0 < got[1] < got[0] and min(got[2]) > 0 and min(got[3]) > 0
    fields_equal(dev.download_state(), twin.download_state(), dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("law", SINGLE, ids=[law if isinstance(law, str) else "%s %g" % law for law in SINGLE])
def test_one_cell_one_law_and_outside_zero_is_phase_redirect_bit_for_bit(devs, law, dtype):
    dev, twin = devs
    state = state_of(N, dtype)
    upload(dev, N, dtype, state)
    upload(twin, N, dtype, state)
    checked, _, cum, _, _ = light._check_layered_phase([law], None, None, CENTER)
    n_pass = 5 + SINGLE.index(law)
    got = dev.phase_grid(checked, cum, ("x", "y"), [[0.0, 1.0], [0.0, 1.0]], None, None, 0, C, SEED, n_pass)
    phase, g = as_phase(law)
    assert twin.phase_redirect(phase, g, C, SEED, n_pass) == got[0] == got[1] == got[3][0] == (N + 2) // 3
    assert 0 < got[2][0] == got[1]                                     # (hardly anybody stands in the one cell: the rest through ``outside``)
    fields_equal(dev.download_state(), twin.download_state(), (law, dtype))


# ------------------------------------------------------------------------------------------------ exact arithmetic
EXACT = {(law if isinstance(law, str) else "%s %g" % law): ([law], None) for law in SINGLE}
EXACT["a table"] = ([X.TABLE3], None)
EXACT["three laws, two mixtures"] = ([("hg", -1e-17), X.TABLE17, "rayleigh"], [[0.5, 0.3, 0.2], [0.0, 0.6, 0.4]])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("deck", list(EXACT))
def test_phase_grid_leaves_the_exact_cosine(dev, deck, dtype):
    """The population of tests/test_writers_direction_exact_gpu.py stands at 0.5, 1.5, 2.5 and 3.5 from its CENTER, a fifth off either
    way: a radius axis with the edges 1, 2, 3 puts mixture 0 (or the only one) in [1, 2) and the last in [2, 3]; inside 1 and beyond 3
    a photon is left alone.  Nobody stands within 0.3 of an edge: no rounding decides a cell."""
    laws, weights = EXACT[deck]
    K = 1 if weights is None else len(weights)
    scene = dict(laws=laws, weights=weights, axes=("r",), edges=[X.EDGES], mixture=np.array([0, K - 1]), outside=None, center=X.CENTER)
    checked, cum = args_of(scene)[:2]
    state = X.population(dtype)
    scattered = X.scattered_photons(state)
    rad = np.sqrt(((state["r"] - X.CENTER) ** 2).sum(axis=1))
    layer = np.where((rad < X.EDGES[0]) | (rad > X.EDGES[-1]), -1, np.searchsorted(X.EDGES, rad) - 1)
    mixture = np.where(layer < 0, -1, scene["mixture"][np.maximum(layer, 0)])
    go = scattered & (mixture >= 0)
    n_pass = 60 + list(EXACT).index(deck)
    u_s = light._philox_block(state["id"], SEED, n_pass, 13)[0]
    pick = (cum[np.maximum(mixture, 0)] <= u_s[:, None]).sum(axis=1)  # the first law with u_s < C[m][j]
    got = X.sweep_and_compare(dev, dtype, lambda: call(dev, scene, n_pass), checked, pick, go, n_pass, "phase_grid, " + deck)
    assert got[:2] == (scattered.sum(), go.sum()) and 0 < go.sum() < scattered.sum()
    assert got[2].tolist() == np.bincount(mixture[go], minlength=K).tolist() and got[3].tolist() == np.bincount(pick[go], minlength=len(laws)).tolist()
    assert min(got[2]) > 50 and (len(laws) == 1 or min(got[3]) > 30)   # every mixture and every law of it is used


# ------------------------------------------------------------------------------------------------ the store states
class GridPhase:
    name = "grid phase"

    def scene(self, state):
        """4 x 4 x 4 cells of a move's width about the source, three mixtures, every fourth cell left alone; beyond them: row 0."""
        origin = np.asarray(W.Source.origin)
        ix, iy, iz = np.indices((4, 4, 4))
        return dict(laws=MIX_LAWS, weights=MIX_WEIGHTS, axes=("x", "y", "z"), edges=[origin[k] + np.linspace(-2.0, 2.0, 5) * W.STEP for k in range(3)],
                    mixture=(ix + 2 * iy + 3 * iz) % 4 - 1, outside=0, center=(0, 0, 0))

    def call(self, dev, state):
        scattered, redirected, by_mixture, by_law = call(dev, self.scene(state), W.N_PASS, W.SEED)
        return scattered, redirected, by_mixture.tolist(), by_law.tolist()

    def check(self, before, after, answer, state, what):
        scattered, redirected, by_mixture, by_law = answer
        assert min(by_mixture) > 0 and min(by_law) > 0 and 0 < redirected < scattered, what      # every mixture and law has work; some are left alone
        ref = check_grid(before, after, answer, self.scene(state), W.C, W.SEED, W.N_PASS, what)
        if state == "S5":
            assert not ref["scattered"][::7].any() and np.asarray(before["id"]).min() > 2 ** 32 and (np.diff(before["id"]) < 0).any(), what


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", ["S2", "S5"])
def test_the_sweep_on_the_store_the_hot_path_left(hip, devs, state, dtype):
    """S2: behind an alive mask; S5: every 7th particle a plain Object, explicit ids in scrambled order.  Twin devices: one meets the
    store as the hot path left it, the other a dense, real store; answers and stores equal, also behind what the loop does next."""
    twin_devices(hip, devs, GridPhase(), state, dtype)


# ------------------------------------------------------------------------------------------------ the ABI, by hand
def test_refused_calls_leave_store_and_output_untouched(dev, hip):
    before = upload(dev, 300, "f64", state_of(300, "f64"))
    for kw in BAD_CALLS:
        keep, args, counts = abi_args(**kw)
        assert dev.lib.pcl_step_phase_grid(dev.ctx, *args) == -2, {k: np.shape(v) for k, v in kw.items()}
        assert counts is None or (counts == -7).all(), kw
    after = W.snapshot(dev)
    W.assert_same_state(before, after, "behind the refused calls")
    keep, good, counts = abi_args()
    assert dev.lib.pcl_step_phase_grid(dev.ctx, *good) == 0 and counts[0] == 100 and counts[2:5].sum() == counts[5:8].sum() == counts[1] > 0
    assert (counts[8:] == -7).all()                                    # 2 + K + M values are written, no more
    g = hip.DeviceGroup([0, 0])
    try:
        keep, args, counts = abi_args(map=[0, 1, 3, 255, 2, 0])
        assert g.lib.pcl_group_step_phase_grid(g.g, *args) == -2 and (counts == -7).all()       # before the group is looked at: it has no store
    finally:
        g.close()
    laws, cum = args_of(SCENES["r"])[:2]
    dev.set_count(0, 0)
    scattered, redirected, by_mixture, by_law = dev.phase_grid(laws, cum, ("r",), [EDGES], CENTER, np.arange(3), None, C, SEED, 1)
    assert (scattered, redirected, by_mixture.tolist(), by_law.tolist()) == (0, 0, [0, 0, 0], [0, 0])
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.phase_grid(laws, cum, ("r",), [EDGES], CENTER, np.arange(3), None, C, SEED, 1)
    assert e.value.code == -3
    bare.close()


def test_one_call_at_the_largest_lds_size_the_bound_accepts(dev, hip):
    """Three laws, two of them tables, 64 mixtures and 2050 edges: the bytes are the header's formula, a table node short of 64 KiB.
    The grid is 1024 x 1024 cells: the map is the whole MiB.  Every slot against the restatement."""
    kw, lds = lds_limit_args(over=False)
    assert 65536 - 24 < lds <= 65536
    bins = kw["T"][1]
    mu, F = np.asarray(kw["mu"]), np.asarray(kw["F"])
    tables = [("table", mu[:1025], np.diff(F[:1025]) / np.diff(mu[:1025])), ("table", mu[1025:], np.diff(F[1025:]) / np.diff(mu[1025:]))]
    scene = dict(laws=(tables[0], tables[1], "rayleigh"), weights=np.tile([0.4, 0.4, 0.2], (64, 1)), axes=("x", "y"),
                 edges=[kw["edges"][:1025], kw["edges"][1025:]], mixture=kw["map"].reshape(1024, 1024).astype(np.int64), outside=0, center=CENTER)
    laws, cum, axes, edges, center, mixture, outside = args_of(scene)
    assert len(laws[1][2]) == bins + 1 and hip.phase_grid_lds_bytes(64, 3, 2050, 1025 + bins + 1) == lds
    assert hip.phase_grid_lds_bytes(64, 3, 2050, 1025 + bins + 2) > hip.PHASE_GRID_LDS_BYTES == 65536
    before = upload(dev, N, "f64", state_of(N, "f64"))
    answer = call(dev, scene, 9)
    check_grid(before, W.snapshot(dev), answer, scene, C, SEED, 9, "the largest LDS size")
    assert answer[1] == answer[0] == (N + 2) // 3 and np.count_nonzero(answer[2]) > 32 and answer[3].min() > 100


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 4097, 4
STEP = 0.5                             # length of a move: A*n*|dr| = 0.5, about half of the photons scatter per pass in the clear air
DT = STEP / C
FIELD_EDGES = [np.linspace(-2.0, 2.0, 5)] * 3
CLOUDY = (np.indices((4, 4, 4)).sum(axis=0) % 2 == 0)
SIM_SCENE = dict(laws=("rayleigh", ("hg", 0.85)), weights=[[1, 0], [0.1, 0.9]], axes=("x", "y", "z"), edges=FIELD_EDGES,
                 mixture=CLOUDY.astype(np.int64), outside=0, center=(0, 0, 0))


class Before(phys.DeviceStep):
    """In front of the step: the state the step will meet, downloaded (the store is dense and real behind it on every run alike)."""
    _fuse_role = None

    def __init__(self):
        self.states = []

    def _device_run(self, sim):
        self.states.append({f: sim.download(f) for f in ("r", "v", "dv", "id")})


def field_sim(devices=None, look=True, cloud=True, passes=PASSES):
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, devices=devices, exit=lambda s: len(s.ts) >= passes)
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=phys.light.PhotonSource(angular="isotropic")))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
    if cloud:
        sim.add_step(3, phys.light.GridScatterStep(np.where(CLOUDY, 3.0, 0.0), ("x", "y", "z"), FIELD_EDGES))
    seen = Before() if look else None
    if look:
        sim.add_step(4, seen)
    step = phys.light.GridPhaseStep(**SIM_SCENE)
    sim.add_step(5, step)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    return sim, step, seen


def rows_of(step):
    return [[int(row[1]), int(row[2])] + row[3].tolist() + row[4].tolist() for row in step.data]


def test_the_rows_are_the_restatement_s_pass_by_pass_and_two_contexts_give_them_too():
    sim, step, seen = field_sim()
    assert len(step.data) == PASSES == len(seen.states) and step._pass == PASSES and step._n_pass == PASSES
    for n_pass, (st, row) in enumerate(zip(seen.states, rows_of(step)), start=1):
        ref = light_grid._grid_phase_redirect(st["r"], st["v"], st["dv"], np.ones(N_SIM, dtype=bool), st["id"], c=light._c_h_literals()[0],
                                              seed=7, n_pass=n_pass, **SIM_SCENE)
        assert row == [int(ref["scattered"].sum()), int(ref["redirected"].sum())] + ref["by_mixture"].tolist() + ref["by_law"].tolist(), n_pass
        assert row[0] == row[1] > N_SIM // 3 and min(row[2:]) > 0      # outside = 0: everybody scattered is re-directed; both mixtures, both laws
    assert sim.schedule["fused"] == PASSES and not sim.schedule["fused_multi"]                      # one launch per light step
    assert "one launch per light step" in sim.launch_note and "GridScatterStep" in sim.launch_note      # the pass's first writer step says it
    one = (rows_of(step), np.argsort(sim.download("id")), sim.download("r"), sim.download("v"))
    sim.close(download=False)
    sim, step, _ = field_sim(devices=[0, 0])
    order = np.argsort(sim.download("id"))
    assert rows_of(step) == one[0]
    assert np.array_equal(sim.download("r")[order], one[2][one[1]]) and np.array_equal(sim.download("v")[order], one[3][one[1]])
    sim.close(download=False)


def test_the_launch_note_names_the_step_where_it_is_the_pass_s_first_writer():
    sim, step, _ = field_sim(look=False, cloud=False, passes=2)
    assert "one launch per light step" in sim.launch_note and "GridPhaseStep" in sim.launch_note
    assert sim.schedule["fused"] == 2 and not sim.schedule["fused_multi"] and [row[0] for row in rows_of(step)] == [row[1] for row in rows_of(step)]
    sim.close(download=False)


def test_a_second_phase_step_is_refused_at_the_first_run():
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=lambda s: len(s.ts) >= 1)
    sim.add_objs(phys.light.generate_photons_bulk(257, min=1.0, max=3.0, seed=7, source=phys.light.PhotonSource(angular="isotropic")))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
    step = phys.light.GridPhaseStep(**SIM_SCENE)
    sim.add_step(3, step)
    sim.add_step(4, phys.light.PhaseFunctionStep("rayleigh"))
    sim._to_device()
    with pytest.raises(ValueError, match="one phase step"):
        step.run(sim)
    assert step._pass == 0 and step.data == []
    sim.close(download=False)
