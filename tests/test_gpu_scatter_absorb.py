"""GPU: AbsorptionStep (pcl_step_absorb_scattered, light.AbsorptionStep).

* ``Device.absorb_scattered`` against the numpy restatement (light._absorb_scattered) applied to the state downloaded before the
  call: N at the wave, workgroup and tile edges, fp64 and fp32 stores; one omega0 everywhere, three layers (conservative, grey,
  black) with and without energy bins, 64 layers; a uniform store and a store with explicit ids in scrambled order and every 7th
  particle a plain Object (the path that stages ids and kinds).  The state is made on the device: an isotropic point source, one
  Newton step, one scatter step that hits about half.  The sweep has no sin, cos, exp or division: all 13 fields, ids and kinds
  are compared bit for bit and every tally cell for equality -- there is no tolerance anywhere in this file.
* a photon draws by its id wherever it stands, refused calls leave the store alone, an empty store answers zeros, two contexts
  on one GPU give the unsharded call's store and tallies.
* through ``Simulation``, before and behind a PhaseFunctionStep: the counts add up pass by pass, absorbed photons stay where they
  were absorbed, the scatter step draws what it draws without the step, ``launch_note`` names the step.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import light
from absorb_reference import C, SEED, same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]
GROUPS = ("r", "v", "dr", "dv")
ID_BASE = 7_000_000_001
H_LIT = 6.62607015e-34
STEP = 0.5                                 # length of the Newton move
DT = STEP / C
# the photons stand on the sphere of radius STEP about the origin: about CENTER their distances reach from 0.4 to 1.6 STEP
CENTER = np.array([0.6 * STEP, 0.0, 0.0])
EDGES3 = np.array([0.5, 0.8, 1.1, 1.4]) * STEP
EDGES64 = np.linspace(0.45, 1.55, 65) * STEP
OMEGA64 = np.linspace(0.0, 1.0, 64)        # layer 0 black, layer 63 conservative
E_BINS = np.linspace(1.25, 2.75, 9)        # the fill's energies reach from 1 to 3: some fall outside
CASES = {"scalar": (0.5, None, None), "layers3": ((1.0, 0.5, 0.0), EDGES3, None), "layers3_E": ((1.0, 0.5, 0.0), EDGES3, E_BINS),
         "layers64": (OMEGA64, EDGES64, None)}


class Isotropic:                           # a point source at the origin (what Device.apply_source reads)
    origin, e1, e2, d = (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "point", 0.0, 0.0


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


def snapshot(dev):
    s = dev.download_state()
    s["kind"] = dev.download_kind()
    return s


_made = {}


def scattered_state(dev, hip, n, dtype):
    """The store after a source, one Newton step and a scatter step with about half hit, made on the device once per (n, dtype)
    and kept on the host: every case starts from an upload of it."""
    if (n, dtype) not in _made:
        dev.store_alloc(n, dtype)
        dev.fill_photons(n, ID_BASE, C, 1.0, 3.0, SEED)
        dev.apply_source(Isotropic, C, SEED)
        dev.step_newton(DT)
        hits = dev.step_scatter_isotropic(0.5 / STEP, 1.0, 0, C, H_LIT, None, hip.RNG_PHILOX, SEED, 1)   # pcoll = A*n*|dr| = 0.5
        s = snapshot(dev)
        assert hits == int(np.stack(s["dv"], 1).any(axis=1).sum()) and (n < 64 or n // 4 < hits < 3 * n // 4)
        _made[(n, dtype)] = s
    return _made[(n, dtype)]


def upload(dev, state, dtype, ids=None, kind=None):
    n = len(state["E"])
    dev.store_alloc(n, dtype)
    up = {g: np.stack(state[g], 1) for g in GROUPS}
    up.update(E=state["E"], id_base=ID_BASE)
    if ids is not None:
        up["id"] = ids
    if kind is not None:
        up["kind"] = kind
    dev.upload_state(up)
    return snapshot(dev)


def expect(before, case, n_pass, hip):
    """(the restatement's answer, the state the store must hold after the call) from the downloaded state ``before``."""
    omega0, edges, E_bins = CASES[case] if isinstance(case, str) else case
    wide = {g: np.stack(before[g], 1).astype(np.float64) for g in GROUPS}
    np_dtype = before["E"].dtype.type
    ref = light._absorb_scattered(wide["r"], wide["v"], wide["dv"], before["E"].astype(np.float64), before["kind"] != hip.KIND_OBJECT,
                                  before["id"], omega0, edges, CENTER, E_bins, SEED, n_pass, np_dtype)
    want = dict(before)
    for g in ("v", "dv"):
        want[g] = [ref[g][:, k].astype(np_dtype) for k in range(3)]
    return ref, want


def same_state(after, want):
    for g in GROUPS:
        for k in range(3):
            assert same_bits(after[g][k], want[g][k]), (g, k)
    assert same_bits(after["E"], want["E"]) and same_bits(after["id"], want["id"]) and same_bits(after["kind"], want["kind"])


def check_call(dev, hip, before, case, n_pass):
    omega0, edges, E_bins = CASES[case]
    ref, want = expect(before, case, n_pass, hip)
    interacted, absorbed, by_layer, E_hist = dev.absorb_scattered(omega0, edges, CENTER, E_bins, SEED, n_pass)
    same_state(snapshot(dev), want)
    assert dev.count == len(before["E"])
    assert (interacted, absorbed) == (int(ref["interacted"].sum()), int(ref["absorbed"].sum())), case
    assert by_layer.dtype == np.int64 and by_layer.tolist() == ref["absorbed_by_layer"].tolist(), case
    assert (E_hist is None) == (E_bins is None)
    if E_bins is not None:
        assert E_hist.dtype == np.int64 and E_hist.tolist() == ref["E_hist"].tolist(), case
    return ref


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_particle_and_every_tally_cell_against_the_numpy_restatement(dev, hip, n, dtype):
    state = scattered_state(dev, hip, n, dtype)
    ids = ID_BASE + np.random.RandomState(5).permutation(n).astype(np.int64)
    kind = np.where(np.arange(n) % 7 == 0, hip.KIND_OBJECT, hip.KIND_PHOTON).astype(np.uint8)
    seen = 0
    for k, case in enumerate(CASES):
        before = upload(dev, state, dtype)
        assert dev.is_uniform()
        ref = check_call(dev, hip, before, case, 1 + k)
        seen += int(ref["absorbed"].sum())
        before = upload(dev, state, dtype, ids=ids, kind=kind)          # the path that downloads ids and kinds and stages them
        assert not dev.is_uniform()
        ref = check_call(dev, hip, before, case, 1 + k)
        assert not ref["interacted"][::7].any()                         # plain Objects, dv != 0 or not
    assert n < 256 or seen > n // 8                                     # the cases do absorb


def test_layers_hold_what_the_cloud_puts_there(dev, hip):
    """The population the parity test runs on does reach every branch: each of the three layers, the hole, the outside, bins and
    energies outside the bins."""
    n = 4097
    before = upload(dev, scattered_state(dev, hip, n, "f64"), "f64")
    ref, _ = expect(before, ((0.0, 0.0, 0.0), EDGES3, E_BINS), 1, hip)
    lay = ref["layer"][ref["interacted"]]
    assert all((lay == b).sum() > 100 for b in (-1, 0, 1, 2)) and ref["absorbed"].sum() == (lay >= 0).sum()
    assert 0 < ref["E_hist"].sum() < ref["absorbed"].sum() and (ref["E_hist"] > 0).all()
    ref64, _ = expect(before, "layers64", 1, hip)
    assert len(np.unique(ref64["layer"])) == 65


def test_a_photon_is_its_id_s_photon_wherever_it_stands(dev, hip):
    n = 2049
    state = scattered_state(dev, hip, n, "f64")
    before = upload(dev, state, "f64", ids=ID_BASE + np.arange(n, dtype=np.int64))      # ids that are id[0] + index: nothing is staged
    check_call(dev, hip, before, "scalar", 3)
    plain = upload(dev, state, "f64")
    dev.absorb_scattered(0.5, None, None, None, SEED, 9)
    v_plain = np.stack(dev.download_state()["v"], 1)
    order = np.random.RandomState(6).permutation(n)
    moved = {g: [a[order] for a in plain[g]] for g in GROUPS}
    moved.update(E=plain["E"][order])
    upload(dev, moved, "f64", ids=plain["id"][order])
    dev.absorb_scattered(0.5, None, None, None, SEED, 9)
    assert same_bits(np.stack(dev.download_state()["v"], 1), v_plain[order])
    upload(dev, state, "f64")
    dev.absorb_scattered(0.5, None, None, None, SEED, 10)               # another pass: other draws
    assert not np.array_equal(np.stack(dev.download_state()["v"], 1), v_plain)


def test_refused_calls_leave_the_store_untouched_and_an_empty_store_answers_zeros(dev, hip):
    before = upload(dev, scattered_state(dev, hip, 257, "f64"), "f64")
    good = dict(omega0=(1.0, 0.5, 0.0), edges=EDGES3, center=CENTER, E_edges=E_BINS, seed=SEED, n_pass=1)
    bad = [dict(omega0=(1.0, 1.5, 0.0)), dict(omega0=(1.0, np.nan, 0.0)), dict(omega0=(-0.5, 0.5, 0.0)), dict(omega0=1.5, edges=None),
           dict(edges=EDGES3[::-1]), dict(edges=(-1.0, 0.4, 0.5, 0.6)), dict(edges=(0.1, 0.4, 0.5, np.inf)), dict(edges=(0.1, 0.4, 0.5, 1e200)),
           dict(center=(0.0, np.nan, 0.0)), dict(E_edges=E_BINS[::-1]), dict(E_edges=(1.0, np.nan)), dict(E_edges=np.arange(1026.0)),
           dict(omega0=[0.5] * 65, edges=np.arange(66.0)), dict(omega0=[0.5] * 64, edges=np.arange(65.0), E_edges=np.arange(193.0))]
    for kw in bad:
        with pytest.raises(hip.HipError) as e:
            dev.absorb_scattered(**dict(good, **kw))
        assert e.value.code == -2, kw
    om = np.array([0.5])
    assert dev.lib.pcl_step_absorb_scattered(dev.ctx, 0, om.ctypes.data, None, None, 0, None, 1, 1, None, None) == -2
    same_state(snapshot(dev), before)
    dev.set_count(0, 0)
    interacted, absorbed, by_layer, E_hist = dev.absorb_scattered(**good)
    assert (interacted, absorbed, by_layer.tolist()) == (0, 0, [0, 0, 0]) and E_hist.shape == (3, 8) and not E_hist.any()
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.absorb_scattered(0.5)
    assert e.value.code == -3
    bare.close()


def test_device_group_gives_the_unsharded_store_and_tallies(dev, hip):
    n = 3 * 2048 + 77
    before = upload(dev, scattered_state(dev, hip, n, "f64"), "f64")
    omega0, edges, E_bins = CASES["layers3_E"]
    whole = dev.absorb_scattered(omega0, edges, CENTER, E_bins, SEED, 4)
    assert whole[1] > n // 16
    with hip.DeviceGroup([0, 0]) as g:
        g.store_alloc(n)
        g.fill_photons(n, ID_BASE, C, 1.0, 2.0, SEED)
        for i in range(2):                                             # the shards' rows through their own contexts
            lo, hi = g.shard(n, i)
            ctx = hip.c_void_p()
            hip.check(g.lib.pcl_group_ctx(g.g, i, hip.byref(ctx)))
            cols = [(f, before[name][f - hip.FIELD_GROUPS[name][0]]) for name in GROUPS for f in hip.FIELD_GROUPS[name]] + [(hip.E, before["E"])]
            for f, col in cols:
                col = np.ascontiguousarray(col[lo:hi])
                hip.check(g.lib.pcl_store_upload(ctx, f, col.ctypes.data, 0, hi - lo))
        got = g.absorb_scattered(omega0, edges, CENTER, E_bins, SEED, 4)
        assert got[:2] == whole[:2] and got[2].tolist() == whole[2].tolist() and got[3].tolist() == whole[3].tolist()
        for f in range(hip.E + 1):
            assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            g.absorb_scattered((1.0, 1.5, 0.0), edges, CENTER, E_bins, SEED, 4)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES, OMEGA = 4097, 6, 0.8


class Probe(phys.DeviceStep):
    """Behind the steps under test: the scatter step's hit count of this pass, and who is at rest where."""
    _fuse_role = None

    def __init__(self):
        self.hits, self.rest, self.r = [], [], []

    def _device_run(self, sim):
        self.hits.append(sim.hits)
        self.rest.append(~sim.download("v").any(axis=1))
        self.r.append(sim.download("r"))


def absorb_sim(order=("absorb", "phase"), passes=PASSES, devices=None):
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, devices=devices, exit=lambda s: len(s.ts) >= passes)
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=phys.light.PhotonSource(angular="isotropic")))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
    made = {"absorb": phys.light.AbsorptionStep(OMEGA), "phase": phys.light.PhaseFunctionStep("hg", 0.85), "probe": Probe()}
    for k, name in enumerate(tuple(order) + ("probe",)):
        sim.add_step(3 + k, made[name])
    return sim, made


def run(sim):
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    return sim


@pytest.mark.parametrize("order", [("absorb", "phase"), ("phase", "absorb")])
def test_the_counts_add_up_and_absorbed_photons_stay_where_they_were_absorbed(order):
    sim, made = absorb_sim(order)
    run(sim)
    step, phase, look = made["absorb"], made["phase"], made["probe"]
    rows = [[int(x) for x in row[1:3]] + [row[3].tolist()] for row in step.data]
    assert len(rows) == PASSES == step._pass and [r[0] for r in rows] == look.hits       # interacted: the scatter step's hit count
    assert all(r[2] == [r[1]] for r in rows) and len(step.data[0]) == 4                  # one layer: everything in it
    redirected = [int(row[1]) for row in phase.data]
    if order[0] == "absorb":
        assert redirected == [r[0] - r[1] for r in rows]               # an absorbed photon did not scatter, for the phase function
    else:
        assert redirected == [r[0] for r in rows]
    total = 0
    for p in range(PASSES):                                            # at rest: exactly the photons absorbed so far
        total += rows[p][1]
        assert int(look.rest[p].sum()) == total
        assert p == 0 or not (look.rest[p - 1] & ~look.rest[p]).any()
    assert total > N_SIM // 4 and sum(r[0] for r in rows) > total * 3   # omega0 = 0.8: about a fifth of the interactions
    first = np.argmax(np.stack(look.rest), axis=0)                      # the pass that absorbed each photon at rest at the end
    gone = look.rest[-1]
    r_then = np.stack(look.r)[first, np.arange(N_SIM)]
    assert same_bits(look.r[-1][gone], r_then[gone]) and same_bits(sim.download("r")[gone], r_then[gone])
    assert not sim.download("v")[gone].any() and not sim.download("dv")[gone].any()
    assert np.abs(np.sqrt((sim.download("v")[~gone] ** 2).sum(axis=1)) - C).max() <= 8 * np.spacing(C)
    assert sim.schedule["fused"] == PASSES and not sim.schedule["fused_multi"]          # one launch per light step
    assert "one launch per light step" in sim.launch_note and ("AbsorptionStep" if order[0] == "absorb" else "PhaseFunctionStep") in sim.launch_note
    assert len(sim.objects) == N_SIM
    sim.close(download=False)


def test_launch_note_names_the_step_and_the_scatter_step_draws_what_it_draws_without_it():
    out = []
    for order in (("absorb",), ()):
        sim, made = absorb_sim(order, passes=1)
        run(sim)
        out.append((sim.hits, sim.download("dv").any(axis=1), sim.download("r"), ~sim.download("v").any(axis=1)))
        if order:
            assert made["absorb"].interacted == sim.hits and made["absorb"].absorbed == int(out[0][3].sum()) > N_SIM // 20
            assert "one launch per light step" in sim.launch_note and "AbsorptionStep" in sim.launch_note
        sim.close(download=False)
    (hits_a, dv_a, r_a, rest_a), (hits_b, dv_b, r_b, rest_b) = out
    assert hits_a == hits_b > N_SIM // 3 and same_bits(r_a, r_b) and not rest_b.any()
    assert np.array_equal(dv_a | rest_a, dv_b) and not (dv_a & rest_a).any()            # the same photons were hit; the absorbed ones carry dv = 0


def test_two_contexts_on_one_gpu_give_the_unsharded_run():
    out = []
    for devices in (None, [0, 0]):
        sim, made = absorb_sim(passes=4, devices=devices)
        run(sim)
        order = np.argsort(sim.download("id"))
        out.append((sim.download("r")[order], sim.download("v")[order], [[int(x) for x in row[1:3]] + row[3].tolist() for row in made["absorb"].data]))
        sim.close(download=False)
    assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and min(r[1] for r in out[0][2]) > N_SIM // 40
