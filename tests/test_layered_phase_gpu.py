"""GPU: LayeredPhaseStep (pcl_step_phase_layered, light.LayeredPhaseStep).

* ``Device.phase_layered`` against the numpy restatement (light._layered_phase_redirect) on the state downloaded before and after
  the call: N at the wave, workgroup and tile edges, fp64 and fp32 stores, a uniform store and a store with explicit ids in
  scrambled order and every 7th particle a plain Object; each single law, the three-layer mixture, a 64-bin table in one layer and
  a table plus Rayleigh over two layers.  All tallies are exact; rows that are not re-directed, and r, dr, E and ids of all rows,
  are bit-identical; re-directed rows lie within the bounds tests/writer_reference.py derives for the phase function's v and dv
  (everything up to sin / cos is the restatement's bit for bit, a table's mu included: a search and one multiply-add).
* every single-law case: a twin device running ``Device.phase_redirect`` with the same seed and pass ends with the same store
  bit for bit and the same count.
* an empty store, every PCL_ERR_ARG refusal through the ABI, two contexts on one GPU, and the step through ``Simulation``.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import light
from absorb_reference import CENTER
from layered_phase_reference import BAD_CALLS, C, SEED, abi_args, as_phase, cases, cloud, hg_table, table_moments
from writer_reference import DIR_ULP, same_bits, ulp

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]
FIELDS = ("r", "v", "dr", "dv")
ID_BASE = 7_000_000_001
CASES = cases()


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


def state_of(n, dtype, ids=None, kind=None, seed=1):
    r, v, dv = cloud(n, seed=seed + n, dtype=np.float32 if dtype == "f32" else np.float64)
    rng = np.random.RandomState(n)
    state = {"r": r, "v": v, "dr": rng.normal(size=(n, 3)), "dv": dv, "E": 1.0 + rng.uniform(size=n), "id_base": ID_BASE}
    if ids is not None:
        state["id"] = ids
    if kind is not None:
        state["kind"] = kind
    return state


def upload(dev, n, dtype, state):
    dev.store_alloc(n, dtype)
    dev.upload_state(state)
    return dev.download_state()


def arrays(s):
    return {f: np.stack(s[f], 1).astype(np.float64) for f in FIELDS}


def check_call(devs, n, dtype, name, n_pass, ids=None, kind=None):
    dev, twin = devs
    laws, weights, edges = CASES[name]
    state = state_of(n, dtype, ids, kind)
    before = upload(dev, n, dtype, state)
    b = arrays(before)
    np_dtype = np.float32 if dtype == "f32" else np.float64
    photon = np.ones(n, dtype=bool) if kind is None else kind != 0
    ref = light._layered_phase_redirect(b["r"], b["v"], b["dv"], photon, before["id"], laws, weights, edges, CENTER, C, SEED, n_pass, np_dtype)
    checked, _, cum, edges_c, center = light._check_layered_phase(laws, weights, edges, CENTER)
    scattered, redirected, by_layer, by_law = dev.phase_layered(checked, cum, edges_c, center, C, SEED, n_pass)
    after = dev.download_state()
    a = arrays(after)
    go = ref["redirected"]
    what = (n, dtype, name, ids is not None)
    assert scattered == int(ref["scattered"].sum()) == int(((np.arange(n) % 3 == 0) & photon).sum()), what
    assert redirected == int(go.sum()) and by_layer.tolist() == ref["by_layer"].tolist() and by_law.tolist() == ref["by_law"].tolist(), what
    assert by_layer.dtype == np.int64 and by_layer.sum() == by_law.sum() == redirected, what
    assert same_bits(after["E"], before["E"]) and np.array_equal(after["id"], before["id"]) and dev.count == n
    for f in FIELDS:                                                   # not re-directed: bit-identical; r and dr: everybody
        assert same_bits(a[f][~go], b[f][~go]), (what, f)
    assert same_bits(a["r"], b["r"]) and same_bits(a["dr"], b["dr"]), what
    if go.any():
        v_unit, v_bound = (ulp(C), DIR_ULP) if dtype == "f64" else (ulp(C, np.float32), DIR_ULP + 0.5)
        v_err = np.max(np.abs(a["v"][go] - ref["v"][go])) / v_unit
        dv_err = np.max(np.abs(a["dv"][go] - ref["dv"][go])) / v_unit
        print("layered n=%d %s %s: v %.3g ulp(c) (bound %g), dv %.3g ulp(c) (bound %g)" % (n, dtype, name, v_err, v_bound, dv_err, v_bound + 1))
        assert v_err <= v_bound, what
        assert dv_err <= v_bound + 1.0, what                           # dv = v - v_old: one more rounding, of a value up to 2c
    if edges is None and len(laws) == 1 and laws[0][0] != "table":     # the phase function's own sweep on a twin: the same store
        upload(twin, n, dtype, state)
        phase, g = as_phase(laws[0])
        assert twin.phase_redirect(phase, g, C, SEED, n_pass) == redirected == scattered, what
        other = twin.download_state()
        for f in FIELDS:
            for k in range(3):
                assert same_bits(after[f][k], other[f][k]), (what, f, k)
        assert same_bits(after["E"], other["E"]) and np.array_equal(after["id"], other["id"]), what
    return scattered, redirected


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_particle_against_the_numpy_restatement(devs, hip, n, dtype):
    ids = ID_BASE + np.random.RandomState(5).permutation(n).astype(np.int64)
    kind = np.where(np.arange(n) % 7 == 0, hip.KIND_OBJECT, hip.KIND_PHOTON).astype(np.uint8)
    for k, name in enumerate(CASES):
        scattered, redirected = check_call(devs, n, dtype, name, 1 + k)
        assert devs[0].is_uniform() and scattered == (n + 2) // 3      # every third slot was scattered
        assert redirected == scattered or CASES[name][2] is not None
        # the path that downloads ids and kinds and stages them behind the tables
        check_call(devs, n, dtype, name, 1 + k, ids=ids, kind=kind)
        assert not devs[0].is_uniform()


def test_layers_leave_some_photons_alone_and_every_law_is_used(devs):
    for name in ("mixture", "table", "table+rayleigh"):
        scattered, redirected = check_call(devs, 4097, "f64", name, 3)
        assert 0 < redirected < scattered, name
    laws, weights, edges = CASES["mixture"]
    upload(devs[0], 4097, "f64", state_of(4097, "f64"))
    checked, _, cum, edges_c, center = light._check_layered_phase(laws, weights, edges, CENTER)
    _, _, by_layer, by_law = devs[0].phase_layered(checked, cum, edges_c, center, C, SEED, 3)
    assert by_layer.min() > 0 and by_law.min() > 0


def test_the_limits_fit_the_workgroup(dev):
    """Eight laws, 2048 bins in two tables and 64 layers: the largest tables a call can have (about 54 KiB of LDS)."""
    n = 4097
    table = ("table", np.linspace(-1, 1, 1025), 1.0 + np.arange(1024.0) % 7)
    laws = [table, ("hg", 0.5), table, "rayleigh", "isotropic", ("hg", -0.3), ("hg", 0.9), "rayleigh"]
    weights = 1.0 + (np.arange(64 * 8).reshape(64, 8) % 5)
    edges = np.linspace(0.0, 5.0, 65)
    before = upload(dev, n, "f64", state_of(n, "f64"))
    b = arrays(before)
    ref = light._layered_phase_redirect(b["r"], b["v"], b["dv"], np.ones(n, dtype=bool), before["id"], laws, weights, edges, CENTER, C, SEED, 2)
    checked, _, cum, edges_c, center = light._check_layered_phase(laws, weights, edges, CENTER)
    scattered, redirected, by_layer, by_law = dev.phase_layered(checked, cum, edges_c, center, C, SEED, 2)
    assert (scattered, redirected) == (int(ref["scattered"].sum()), int(ref["redirected"].sum())) and redirected > 1000
    assert by_layer.tolist() == ref["by_layer"].tolist() and by_law.tolist() == ref["by_law"].tolist() and by_law.min() > 0
    a = arrays(dev.download_state())
    go = ref["redirected"]
    assert same_bits(a["v"][~go], b["v"][~go]) and np.max(np.abs(a["v"][go] - ref["v"][go])) <= DIR_ULP * ulp(C)


def test_refused_calls_and_an_empty_store(dev, hip):
    before = upload(dev, 300, "f64", state_of(300, "f64"))
    keep, good, counts = abi_args()
    for kw in BAD_CALLS:
        keep, args, counts = abi_args(**kw)
        assert dev.lib.pcl_step_phase_layered(dev.ctx, *args) == -2, kw
        assert counts is None or (counts == -7).all(), kw
    after = dev.download_state()
    for f in FIELDS:
        for k in range(3):
            assert same_bits(after[f][k], before[f][k]), f
    keep, good, counts = abi_args()
    assert dev.lib.pcl_step_phase_layered(dev.ctx, *good) == 0 and counts[0] == 100 and counts[2:5].sum() == counts[5:8].sum() == counts[1] > 0
    assert (counts[8:] == -7).all()                                    # 2 + L' + M values are written, no more
    laws, _, cum, _, _ = light._check_layered_phase(["rayleigh"], None, None, CENTER)
    dev.set_count(0, 0)
    scattered, redirected, by_layer, by_law = dev.phase_layered(laws, cum, None, None, C, SEED, 1)
    assert (scattered, redirected, by_layer.tolist(), by_law.tolist()) == (0, 0, [0], [0])
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        bare.phase_layered(laws, cum, None, None, C, SEED, 1)
    assert e.value.code == -3
    bare.close()


def test_device_group_gives_the_unsharded_store(dev, hip):
    n = 3 * 2048 + 77
    laws, weights, edges = CASES["mixture"]
    checked, _, cum, edges_c, center = light._check_layered_phase(laws, weights, edges, CENTER)
    before = upload(dev, n, "f64", state_of(n, "f64"))
    whole = dev.phase_layered(checked, cum, edges_c, center, C, SEED, 4)
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
        got = g.phase_layered(checked, cum, edges_c, center, C, SEED, 4)
        assert got[:2] == whole[:2] and got[2].tolist() == whole[2].tolist() and got[3].tolist() == whole[3].tolist()
        assert 0 < whole[1] < whole[0] == (n + 2) // 3
        for f in range(hip.E):
            assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            g.phase_layered(checked, cum[:, ::-1], edges_c, center, C, SEED, 4)      # rows that decrease
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 4097, 6
STEP = 0.5                             # length of a move: A*n*|dr| = 0.5, about half of the photons scatter per pass
DT = STEP / C
TABLE = hg_table(0.85, 64)


class Probe(phys.DeviceStep):
    """Behind the step: the scatter step's hit count of this pass, and the cosines between the velocities before and after the
    scatter of the photons it hit."""
    _fuse_role = None

    def __init__(self):
        self.hits, self.cosines = [], []

    def _device_run(self, sim):
        self.hits.append(sim.hits)
        v, dv = sim.download("v"), sim.download("dv")
        hit = dv.any(axis=1)
        old = (v - dv)[hit]
        self.cosines.append((v[hit] * old).sum(axis=1) / np.sqrt((v[hit] ** 2).sum(axis=1) * (old ** 2).sum(axis=1)))


def layered_sim(with_step=True, passes=PASSES, devices=None, probe=True, laws=(TABLE,), weights=None, edges=None):
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, devices=devices, exit=lambda s: len(s.ts) >= passes)
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=phys.light.PhotonSource(angular="isotropic")))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
    step = phys.light.LayeredPhaseStep(list(laws), weights, edges) if with_step else None
    look = Probe() if probe else None
    for k, s in enumerate(x for x in (step, look) if x is not None):
        sim.add_step(3 + k, s)
    return sim, step, look


def run(sim):
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    return sim


def test_every_pass_redirects_the_photons_the_scatter_step_hit():
    sim, step, look = layered_sim()
    run(sim)
    assert len(step.data) == PASSES and [int(row[1]) for row in step.data] == look.hits and step._pass == PASSES == sim._launch
    assert all(int(row[2]) == int(row[1]) == int(row[3][0]) == int(row[4][0]) for row in step.data)      # one layer that holds everything
    assert all(N_SIM // 3 < h < 2 * N_SIM // 3 for h in look.hits)     # about half scatter per pass
    mu = np.concatenate(look.cosines)
    _, mean, var = table_moments(TABLE[1], TABLE[2])
    print("mean cosine %.5f, the table's %.5f +- %.5f at 5 sigma" % (mu.mean(), mean, 5 * np.sqrt(var / len(mu))))
    assert abs(mu.mean() - mean) <= 5 * np.sqrt(var / len(mu)), mu.mean()
    assert sim.schedule["fused"] == PASSES and not sim.schedule["fused_multi"]                      # one launch per light step
    assert "one launch per light step" in sim.launch_note and "LayeredPhaseStep" in sim.launch_note
    assert len(sim.objects) == N_SIM
    sim.close(download=False)


def test_the_scatter_step_draws_what_it_draws_without_the_step():
    hits, scattered, r = [], [], []
    for with_step in (True, False):
        sim, step, _ = layered_sim(with_step, passes=1, probe=False)
        run(sim)
        hits.append(sim.hits)
        scattered.append(sim.download("dv").any(axis=1))
        r.append(sim.download("r"))
        if with_step:
            assert step.scattered == step.redirected == sim.hits
            v_with = sim.download("v")
        else:
            assert not np.array_equal(sim.download("v")[scattered[0]], v_with[scattered[0]])       # the step gave them other directions
            assert np.array_equal(sim.download("v")[~scattered[0]], v_with[~scattered[0]])
        sim.close(download=False)
    assert hits[0] == hits[1] > N_SIM // 3 and np.array_equal(scattered[0], scattered[1]) and np.array_equal(r[0], r[1])


def test_two_contexts_on_one_gpu_give_the_unsharded_run():
    out = []
    edges = np.array([0.0, 0.6, 1.2, 2.5]) * STEP                      # the source is a point at the origin: layers of a few moves
    for devices in (None, [0, 0]):
        sim, step, _ = layered_sim(passes=4, devices=devices, probe=False, laws=("rayleigh", ("hg", 0.85)),
                                   weights=[[1, 0], [0.3, 0.7], [0, 1]], edges=edges)
        run(sim)
        order = np.argsort(sim.download("id"))
        out.append((sim.download("r")[order], sim.download("v")[order], [[int(row[1]), int(row[2])] + row[3].tolist() + row[4].tolist() for row in step.data]))
        sim.close(download=False)
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and min(row[1] for row in out[0][2]) > 0 and out[0][2][-1][1] < out[0][2][-1][0]


def test_a_second_phase_step_is_refused_at_the_first_run():
    sim, step, _ = layered_sim(passes=1, probe=False)
    sim.add_step(7, phys.light.PhaseFunctionStep("rayleigh"))
    sim._to_device()
    with pytest.raises(ValueError, match="one phase step"):
        step.run(sim)
    assert step._pass == 0 and step.data == []
    sim.close(download=False)
