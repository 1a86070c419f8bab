"""GPU: PathAbsorptionStep (pcl_step_absorb_path, light.PathAbsorptionStep).

* ``Device.absorb_path`` against the numpy restatement (light._absorb_path) on a state that is uploaded explicitly
  (tests/path_absorb_reference.py: ``layout``, with its planted slots: at rest, -0.0, NaN, on the first, inner and last radius, on
  band edges, outside), downloaded before and after the call: N at the wave, workgroup and tile edges and one size at which a
  workgroup takes more than one trip, fp64 and fp32 stores; with layers and bands, layers only, bands only and neither.  Nothing has
  a tolerance: the tallies, v and dv are the restatement's, every other field is bit-identical.
* a store with explicit ids in scrambled order and plain Objects; two passes; the refusals; an empty store; a device group.
* through ``Simulation``: one pass shared with an ``AbsorptionStep`` against a twin without the new step (the other steps draw what
  they drew), and 20 passes of the recycling atmosphere, every writer replayed with its numpy restatement from the probed state in
  front of it.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
import writer_reference as W
from path_absorb_reference import BAD_CALLS, C, CENTER, E_EDGES, EDGES, ID_BASE, P_CELLS, SEED, abi_args, check_path_absorb, configs, \
    layout, planted
from physicl_amd import light
from recycle_reference import check_recycle
from writer_reference import same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]
FIELDS = ("r", "v", "dr", "dv")


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


def upload(dev, n, dtype, ids=None, kind=None):
    state = dict(layout(n, np.float32 if dtype == "f32" else np.float64), id_base=ID_BASE)
    if ids is not None:
        state["id"] = ids
    if kind is not None:
        state["kind"] = kind
    dev.store_alloc(n, dtype)
    dev.upload_state(state)
    return W.snapshot(dev)


def check_call(dev, n, dtype, config, n_pass, ids=None, kind=None, before=None):
    p, edges, E_edges = configs()[config]
    before = upload(dev, n, dtype, ids, kind) if before is None else before
    answer = dev.absorb_path(p, edges, CENTER, E_edges, SEED, n_pass)
    after = W.snapshot(dev)
    what = "path absorb n=%d %s %s pass %d%s" % (n, dtype, config, n_pass, " ids" if ids is not None else "")
    ref = check_path_absorb(before, after, answer, p, edges, CENTER, E_edges, SEED, n_pass, what)
    return answer, before, after, ref


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_particle_against_the_numpy_restatement(dev, n, dtype):
    for n_pass, config in ((1, "both"), (2, "neither")):
        answer, _, _, ref = check_call(dev, n, dtype, config, n_pass)
        assert dev.is_uniform()
        if n >= 255:
            assert 0 < answer[1] < answer[0] < n
    moving, want_layer, want_band = planted(n)                         # the planted slots were found where they were planted
    assert not ref["exposed"][~moving].any() and ref["exposed"][moving].all()              # (no layers, no bands: every moving photon)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_workgroup_takes_more_than_one_trip(dev, dtype):
    n = dev.info()["compute_units"] * 8 * 256 + 77                     # just above the grid's cap of resident workgroups
    answer, _, _, _ = check_call(dev, n, dtype, "both", 3)
    assert answer[0] > n // 4 and answer[1] > n // 10 and (np.asarray(answer[2]) > 0).sum() == 5 and answer[2][0, 0] == 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("config", ["both", "layers", "bands", "neither"])
def test_layers_and_bands_in_every_combination(dev, config, dtype):
    n = 3 * 2048 + 77
    answer, _, _, ref = check_call(dev, n, dtype, config, 4)
    moving, want_layer, want_band = planted(n)
    i = np.arange(n)
    p, edges, E_edges = configs()[config]
    assert np.asarray(answer[2]).shape == (1 if edges is None else 2, 1 if E_edges is None else 3)
    assert not ref["exposed"][~moving].any()                           # at rest and -0.0: skipped
    if edges is not None:                                              # on the first, inner and last radius; NaN; outside
        assert ((ref["layer"] == want_layer) | (want_layer == -2) | ~moving).all()
        for mod, b in ((5, 0), (7, 1), (23, 1), (11, -1), (17, -1), (19, -1)):
            assert (moving & (want_layer == b) & (i % mod == 0)).any(), mod
    if E_edges is not None:                                            # on a band edge, the last and the first; NaN; outside
        has_layer = ref["layer"] >= 0
        assert ((ref["band"] == want_band) | (want_band == -2) | ~has_layer).all()
        for mod, rest, e in ((4, 1, 1), (9, 2, 2), (16, 9, 0), (10, 3, -1), (14, 5, -1), (15, 7, -1)):
            assert (has_layer & (want_band == e) & (i % mod == rest)).any(), mod
    assert 0 < answer[1] < answer[0] < moving.sum() + (config == "neither")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_transparent_and_a_black_gas(dev, dtype):
    n = 2049
    before = upload(dev, n, dtype)
    clear = dev.absorb_path(np.zeros((2, 3)), EDGES, CENTER, E_EDGES, SEED, 1)
    assert clear[0] > n // 4 and clear[1] == 0 and not clear[2].any()
    W.assert_same_state(W.snapshot(dev), before, "p = 0 writes nothing")
    black = dev.absorb_path(np.ones((2, 3)), EDGES, CENTER, E_EDGES, SEED, 1)
    after = W.snapshot(dev)
    assert black[0] == black[1] == clear[0] == black[2].sum()
    check_path_absorb(before, after, black, np.ones((2, 3)), EDGES, CENTER, E_EDGES, SEED, 1, "p = 1 %s" % dtype)
    assert dev.absorb_path(np.ones((2, 3)), EDGES, CENTER, E_EDGES, SEED, 2)[:2] == (0, 0)    # everybody exposed is at rest now


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_store_that_is_not_uniform(dev, hip, dtype):
    n = 2049
    ids = ID_BASE + 3 * np.random.RandomState(5).permutation(n).astype(np.int64)            # explicit, not consecutive
    kind = np.where(np.arange(n) % 4 == 1, hip.KIND_OBJECT, hip.KIND_PHOTON).astype(np.uint8)
    answer, before, after, ref = check_call(dev, n, dtype, "both", 6, ids=ids, kind=kind)
    assert not dev.is_uniform() and answer[1] > 0
    obj = kind == hip.KIND_OBJECT
    b, a = W.wide(before), W.wide(after)
    for f in FIELDS:                                                   # moving Objects are untouched
        assert same_bits(a[f][obj], b[f][obj]), f
    assert not ref["exposed"][obj].any() and (planted(n)[0] & obj).any()
    # the draws follow the ids: the same photons with ids in store order are absorbed differently
    plain = light._absorb_path(b["r"], b["v"], b["dv"], np.asarray(before["E"], dtype=np.float64), ~obj, ID_BASE + np.arange(n), P_CELLS,
                               EDGES, CENTER, E_EDGES, SEED, 6)
    assert np.array_equal(plain["exposed"], ref["exposed"]) and not np.array_equal(plain["absorbed"], ref["absorbed"])


def test_two_passes_draw_twice(dev):
    n = 2049
    first, before, after, ref1 = check_call(dev, n, "f64", "layers", 1)
    second, _, _, ref2 = check_call(dev, n, "f64", "layers", 2, before=after)               # on what the first pass left
    assert second[0] == first[0] - first[1] and second[1] > 0 and not ref2["exposed"][ref1["absorbed"]].any()
    other, _, _, ref3 = check_call(dev, n, "f64", "layers", 2)                               # the same state, another pass: other draws
    assert other[0] == first[0] and not np.array_equal(ref3["absorbed"], ref1["absorbed"])


def test_refused_calls_and_an_empty_store(dev, hip):
    before = upload(dev, 300, "f64")
    for kw in BAD_CALLS:
        keep, args, (counts, cells) = abi_args(**kw)
        assert dev.lib.pcl_step_absorb_path(dev.ctx, *args) == -2, kw
        assert (counts is None or (counts == -7).all()) and (cells is None or (cells == -7).all()), kw
    W.assert_same_state(W.snapshot(dev), before, "a refused call writes nothing")
    with pytest.raises(ValueError, match="p holds"):
        dev.absorb_path([0.5, 0.5, 0.5], EDGES, CENTER, None, SEED, 1)
    keep, good, (counts, cells) = abi_args()
    assert dev.lib.pcl_step_absorb_path(dev.ctx, *good) == 0
    ref = check_path_absorb(before, W.snapshot(dev), (counts[0], counts[1], cells[:6].reshape(2, 3)), P_CELLS, EDGES, CENTER, E_EDGES, 1, 1, "by hand")
    assert ref["absorbed"].any() and (counts[2:] == -7).all() and (cells[6:] == -7).all()   # two counts and six cells, no more
    dev.set_count(0, 0)
    empty = dev.absorb_path(P_CELLS, EDGES, CENTER, E_EDGES, SEED, 1)
    assert empty[:2] == (0, 0) and empty[2].tolist() == [[0] * 3] * 2
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.absorb_path(0.5, None, None, None, SEED, 1)
    assert e.value.code == -3
    bare.close()


def test_device_group_gives_the_unsharded_store(dev, hip):
    n = 3 * 2048 + 77
    before = upload(dev, n, "f64")
    whole = dev.absorb_path(P_CELLS, EDGES, CENTER, E_EDGES, SEED, 4)
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
        got = g.absorb_path(P_CELLS, EDGES, CENTER, E_EDGES, SEED, 4)
        assert got[:2] == whole[:2] and got[2].tolist() == whole[2].tolist() and whole[1] > 0
        for f in range(hip.E + 1):
            assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            g.absorb_path(np.full((2, 3), 1.5), EDGES, CENTER, E_EDGES, SEED, 4)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 4096, 20
STEP = 0.5                             # length of a move: A*n*|dr| = 0.5, about half of the photons interact per pass
DT = STEP / C
GROUND, TOP_SIM = 1.0, 4.0
SRC_SIM = dict(origin=(2.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), angular="isotropic")
GAS_EDGES = np.array([1.0, 2.5, 4.0])
GAS_BANDS = np.array([1.0, 2.0, 3.0])
GAS_K = np.array([[0.4, 0.0], [0.1, 0.8]])            # per unit length: tau = k * STEP; the lower layer is clear in the upper band
STATE = ("r", "v", "dr", "dv", "E", "id")


class Look(phys.DeviceStep):
    """The store as it stands, pass by pass."""
    _fuse_role = None

    def __init__(self):
        self.states = []

    def _device_run(self, sim):
        self.states.append({f: sim.download(f) for f in STATE})


def run(sim):
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    return sim


def shared_pass(gas):
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=lambda s: len(s.ts) >= 1)
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=phys.light.PhotonSource(**SRC_SIM)))
    looks = [Look(), Look()]
    medium = phys.light.AbsorptionStep(omega0=0.5)
    steps = [phys.UpdateTimeStep(lambda s: np.double(DT)), phys.newton.NewtonianKinematicsStep(),
             phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)), looks[0]] + ([gas] if gas is not None else []) + [looks[1], medium]
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    run(sim)
    final = {f: sim.download(f) for f in STATE}
    seed, note = sim.seed, sim.launch_note
    sim.close(download=False)
    return looks, medium, final, seed, note


def test_a_pass_shared_with_an_absorption_step_leaves_its_draws_alone():
    gas = phys.light.PathAbsorptionStep(0.6)                           # grey: p = 1 - exp(-0.3)
    looks, medium, final, seed, note = shared_pass(gas)
    twin_looks, twin_medium, twin_final, _, _ = shared_pass(None)
    s0, s1 = looks[0].states[0], looks[1].states[0]
    p = light._path_probability(gas.k, light._c_h_literals()[0], DT)
    ref = check_path_absorb(s0, s1, (gas.exposed, gas.absorbed, gas.absorbed_by_cell), p, None, gas.center, None, seed, 1, "shared pass")
    for f in STATE:                                                    # in front of the new step the two runs are one
        assert same_bits(s0[f], twin_looks[0].states[0][f]) and same_bits(s0[f], twin_looks[1].states[0][f]), f
    gone = ref["absorbed"]
    assert gas.exposed == N_SIM and 0 < gas.absorbed == gone.sum() < N_SIM and "PathAbsorptionStep" in note
    p1 = p.item()
    sigma = np.sqrt(N_SIM * p1 * (1.0 - p1))                           # Beer-Lambert over one move, binomial
    assert p1 == -np.expm1(-0.6 * (light._c_h_literals()[0] * DT)) and abs(gas.absorbed - N_SIM * p1) <= 5.0 * sigma
    for f in STATE:                                                    # who the gas left alone ends the pass as in the twin: same draws
        assert same_bits(final[f][~gone], twin_final[f][~gone]), f
    assert not final["v"][gone].any() and not final["dv"][gone].any() and same_bits(final["r"][gone], twin_final["r"][gone])
    twin_hit = twin_final["dv"].any(axis=1) | ~twin_final["v"].any(axis=1)                   # the twin's interacting photons
    twin_gone = ~twin_final["v"].any(axis=1)
    assert twin_medium.interacted == int(twin_hit.sum()) and twin_medium.absorbed == int(twin_gone.sum()) > 0
    assert medium.interacted == int((twin_hit & ~gone).sum()) and medium.absorbed == int((twin_gone & ~gone).sum()) > 0


def atmosphere(passes, devices=None, probes=True):
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, devices=devices, exit=lambda s: len(s.ts) >= passes)
    src = phys.light.PhotonSource(**SRC_SIM)
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    gas = phys.light.PathAbsorptionStep(GAS_K, GAS_EDGES, (0, 0, 0), GAS_BANDS)
    floor = phys.light.SurfaceReflectStep(GROUND, albedo=0.5)
    lamp = phys.light.RecycleStep(src, top=TOP_SIM)
    looks = [Look() for _ in range(4)] if probes else [None] * 4
    steps = [phys.UpdateTimeStep(lambda s: np.double(DT)), phys.newton.NewtonianKinematicsStep(),
             phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)), looks[0], gas, looks[1], floor, looks[2], lamp, looks[3]]
    for k, s in enumerate(x for x in steps if x is not None):
        sim.add_step(k, s)
    run(sim)
    final = {f: sim.download(f) for f in STATE}
    out = dict(gas=gas, floor=floor, lamp=lamp, looks=looks, final=final, seed=sim.seed, note=sim.launch_note, schedule=dict(sim.schedule),
               n_objects=len(sim.objects))
    sim.close(download=False)
    return out


def rows_of(out):
    return {name: [[np.asarray(x).tolist() for x in row] for row in out[name].data] for name in ("gas", "floor", "lamp")}


@pytest.fixture(scope="module")
def steady():
    return atmosphere(PASSES)


def test_the_recycling_atmosphere_replays_from_the_probed_states(steady):
    c_lit = light._c_h_literals()[0]
    gas, floor, lamp = steady["gas"], steady["floor"], steady["lamp"]
    p = light._path_probability(GAS_K, c_lit, DT)
    assert p[0, 1] == 0.0 and same_bits(p, -np.expm1(-(GAS_K * (c_lit * DT))))
    assert len(gas.data) == len(floor.data) == len(lamp.data) == PASSES == gas._pass
    cells = np.zeros((2, 2), dtype=np.int64)
    rate = []
    for k in range(PASSES):
        s0, s1, s2, s3 = (look.states[k] for look in steady["looks"])
        what = "pass %d" % (k + 1)
        row = gas.data[k]
        ref = check_path_absorb(s0, s1, (row[1], row[2], row[3]), p, GAS_EDGES, np.zeros(3), GAS_BANDS, steady["seed"], k + 1, what + " gas")
        ref_g = W.check_surface(s1, s2, (floor.data[k][1], floor.data[k][2]), GROUND, np.zeros(3), 0.5, "lambertian", c_lit, steady["seed"], k + 1,
                                1.001 * STEP, what + " ground")
        ref_l = check_recycle(s2, s3, (lamp.data[k][1], lamp.data[k][2]), lamp.source, TOP_SIM, np.zeros(3), True, None, steady["seed"], k + 1,
                              what + " lamp")
        assert len(s3["id"]) == N_SIM and same_bits(s0["id"], s3["id"]), what
        # whoever is at rest behind the ground was absorbed in this pass, by the gas or by the ground: the lamp takes them all
        assert int(lamp.data[k][1]) == int(row[2]) + int(floor.data[k][2]) == int(ref_l["at_rest"].sum()), what
        assert not ref_g["hit"][ref["absorbed"]].any(), what            # a photon the gas has parked does not reach the ground
        assert s3["v"].any(axis=1).all(), what                          # behind the lamp everybody moves
        assert int(row[1]) <= N_SIM and np.asarray(row[3])[0, 1] == 0, what
        cells += np.asarray(row[3])
        rate.append(int(lamp.data[k][1]) + int(lamp.data[k][2]))
    print("absorbed by cell over %d passes: %s; emission rate per pass: %s" % (PASSES, cells.tolist(), rate))
    assert cells[0, 0] > 0 and cells[1, 0] > 0 and cells[1, 1] > 0 and min(rate) > 0
    assert "one launch per light step" in steady["note"] and steady["schedule"]["fused"] == PASSES and not steady["schedule"].get("fused_multi")
    assert steady["n_objects"] == N_SIM
    for f in STATE:                                                    # nothing moves behind the last probe
        assert same_bits(steady["final"][f], steady["looks"][3].states[-1][f]), f


def test_the_probes_do_not_disturb_the_run(steady):
    bare = atmosphere(PASSES, probes=False)
    assert rows_of(bare) == rows_of(steady) and bare["note"] == steady["note"]
    for f in STATE:
        assert same_bits(bare["final"][f], steady["final"][f]), f


def test_two_contexts_on_one_gpu_give_the_unsharded_run(steady):
    both = atmosphere(PASSES, devices=[0, 0], probes=False)
    assert rows_of(both) == rows_of(steady) and both["n_objects"] == N_SIM
    a, b = np.argsort(both["final"]["id"], kind="stable"), np.argsort(steady["final"]["id"], kind="stable")
    for f in STATE:
        assert same_bits(both["final"][f][a], steady["final"][f][b]), f
