"""GPU: ReemissionStep (pcl_step_reemit_parked, light.ReemissionStep).

* ``Device.reemit_parked`` against the numpy restatement (light._reemit_parked) on a state that is uploaded explicitly
  (tests/reemit_reference.py: ``scene``, every special position of it; who is at rest is chosen by ``POPULATIONS``), downloaded
  before and after the call: N at the wave and tile edges, several tiles with a ragged tail, a capacity beyond N, fp64 and fp32
  stores; layers with a law, a yield and a table each, one layer everywhere (r is not read) and one lambertian layer everywhere.
  Counts and by_layer are exact; every row of a particle that is not re-emitted is bit-identical; r, ids and kinds for everybody;
  dr and dv of the re-emitted are exactly 0; their E is the restatement's bit for bit and untouched without a table; their v lies
  within writer_reference.DIR_ULP ulp(c) (DIR_ULP + 0.5 float32 ulp in an fp32 store), the bound derived there for a direction
  built from the project's sincos.
* eta = 0 writes nothing; the same pass gives the same bits, the next pass other directions; scrambled ids and plain Objects; the
  refusals; an empty store; no store; a device group; the step through ``Simulation`` behind a gas.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from reemit_reference import BAD_CALLS, C, CENTER, EDGES, EVERYWHERE, EVERYWHERE_UP, FIELDS, GRID_B, ID_BASE, LAYERED, SEED, abi_args, \
    check_reemit, scene, unit, wide
from writer_reference import same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 2048, 2049, 3 * 2048 + 77]
ROOM = 300                                                             # capacity beyond N
# who is at rest: slot numbers -> a mask
POPULATIONS = {
    "none": lambda i, n: np.zeros(n, dtype=bool),
    "all": lambda i, n: np.ones(n, dtype=bool),
    "every_third": lambda i, n: i % 3 == 0,
    "a_whole_wave": lambda i, n: (i >= 64) & (i < 128) if n > 128 else i < 64,
    "the_ragged_tail": lambda i, n: i >= n // 64 * 64 if n % 64 else i >= n - 1,
}
CONFIGS = {"layered": LAYERED, "everywhere": EVERYWHERE, "everywhere_up": EVERYWHERE_UP}


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


def state_of(n, dtype, population, mixed=False):
    """The scene with everybody moving but the slots of ``population``; ``mixed``: its scrambled ids and plain Objects as well."""
    T = np.float32 if dtype == "f32" else np.float64
    s = scene(n, T)
    i = np.arange(n)
    rest = POPULATIONS[population](i, n)
    v = (C * unit(np.random.RandomState(n).normal(size=(n, 3)))).astype(T).astype(np.float64)
    v[rest] = 0.0
    v[rest & (i % 6 == 0), 1] = -0.0
    v[~rest & (i % 13 == 0)] = [np.nan, 0.0, 0.0]                      # a NaN moves, wherever it stands
    v[~rest & (i % 26 == 1)] = [0.0, -0.0, np.nan]
    up ={f: s[f] for f in FIELDS + ("E",)}
    up.update(v=v, id_base=ID_BASE)
    photon = None
    if mixed:
        up.update(id=s["id"], kind=s["photon"].astype(np.uint8))
        photon = s["photon"]
    return up, photon


def upload(dev, n, dtype, population, mixed=False):
    up, photon = state_of(n, dtype, population, mixed)
    dev.store_alloc(n + ROOM, dtype)
    dev.upload_state(up)
    return dev.download_state(), photon


def call(dev, cfg, n_pass, seed=SEED):
    return dev.reemit_parked(C, cfg["eta"], cfg["angular"], cfg["tables"], cfg["edges"], cfg["center"], seed, n_pass)


def check_call(dev, n, dtype, population, name, n_pass, mixed=False):
    before, photon = upload(dev, n, dtype, population, mixed)
    answer = call(dev, CONFIGS[name], n_pass)
    after = dev.download_state()
    what = "reemit n=%d %s %s %s pass %d%s" % (n, dtype, population, name, n_pass, " mixed" if mixed else "")
    ref = check_reemit(before, after, answer, CONFIGS[name], SEED, n_pass, what, photon)
    assert dev.count == n, what
    return answer, before, after, ref


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_particle_against_the_numpy_restatement(dev, n, dtype):
    for population in POPULATIONS:
        for n_pass, name in enumerate(CONFIGS, 1):
            answer, _, _, ref = check_call(dev, n, dtype, population, name, n_pass)
            assert dev.is_uniform()
            if population == "none":
                assert answer[:2] == (0, 0) and not answer[2].any()
            elif name == "everywhere":
                rest = POPULATIONS[population](np.arange(n), n)
                assert answer[0] == answer[1] == rest.sum() > 0        # eta 1, no layers: whoever is at rest
            elif population == "all" and n >= 2048:
                assert 0 < answer[1] < answer[0]
                assert name != "layered" or (answer[2][[0, 1, 3]] > 0).all() and answer[2][2] == 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_store_that_is_not_uniform(dev, hip, dtype):
    n = 2049
    for name in CONFIGS:
        answer, before, after, ref = check_call(dev, n, dtype, "every_third", name, 6, mixed=True)
        assert not dev.is_uniform() and answer[1] > 0
        kind = dev.download_kind()
        obj = kind == hip.KIND_OBJECT
        assert np.array_equal(obj, np.arange(n) % 17 == 0)             # kinds are never written
        b, a = wide(before), wide(after)
        for f in FIELDS:                                               # Objects at rest are untouched
            assert same_bits(a[f][obj], b[f][obj]), f
        assert not ref["parked"][obj].any() and ((np.arange(n) % 3 == 0) & obj).any()
    # the draws follow the ids: the same state with ids in store order re-emits other photons (layers of eta 0.5 among them)
    plain, _ = upload(dev, n, dtype, "every_third")
    other = call(dev, LAYERED, 6)
    assert other[0] > 0 and not same_bits(wide(dev.download_state())["v"], wide(after)["v"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_eta_zero_writes_nothing(dev, dtype):
    n = 2049
    before, _ = upload(dev, n, dtype, "every_third")
    cfg = dict(LAYERED, eta=np.zeros(4))
    answer = call(dev, cfg, 1)
    after = dev.download_state()
    ref = check_reemit(before, after, answer, cfg, SEED, 1, "eta 0 %s" % dtype)
    assert answer[0] == ref["parked"].sum() > 0 and answer[1] == 0 and not answer[2].any()
    for f in FIELDS:
        for k in range(3):
            assert same_bits(after[f][k], before[f][k]), f
    assert same_bits(after["E"], before["E"])


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_the_same_pass_gives_the_same_bits_and_the_next_other_directions(dev, dtype):
    n = 2049
    out = []
    for n_pass in (3, 3, 4):
        answer, _, after, ref = check_call(dev, n, dtype, "all", "layered", n_pass)
        out.append((answer, after, ref))
    (a0, s0, r0), (a1, s1, r1), (a2, s2, r2) = out
    assert a0[:2] == a1[:2] and a0[2].tolist() == a1[2].tolist()
    for f in FIELDS:
        for k in range(3):
            assert same_bits(s0[f][k], s1[f][k]), f
    assert same_bits(s0["E"], s1["E"])
    sure = r0["reemitted"] & r2["reemitted"]                           # (layer 0 has eta 1: they are many)
    assert sure.sum() > 50 and not (wide(s0)["v"][sure] == wide(s2)["v"][sure]).all(axis=1).any()
    assert not np.array_equal(r0["reemitted"], r2["reemitted"])        # the layers of eta 0.5 draw anew


def test_refused_calls_an_empty_store_and_no_store(dev, hip):
    before, _ = upload(dev, 300, "f64", "every_third")
    for kw in BAD_CALLS:
        keep, args, counts = abi_args(**kw)
        assert dev.lib.pcl_step_reemit_parked(dev.ctx, *args) == -2, kw
        assert counts is None or (counts == -7).all(), kw
    after = dev.download_state()
    for f in FIELDS:
        for k in range(3):
            assert same_bits(after[f][k], before[f][k]), f
    assert same_bits(after["E"], before["E"])
    keep, good, counts = abi_args()                                    # two layers: 2 + 2 counts, no more
    assert dev.lib.pcl_step_reemit_parked(dev.ctx, *good) == 0 and (counts[:4] >= 0).all() and counts[4:].tolist() == [-7, -7]
    assert counts[1] == counts[2] + counts[3] <= counts[0] and counts[2] > 0
    assert np.isin(dev.download(hip.E), GRID_B).sum() == counts[2]     # the first layer has the table
    dev.set_count(0, 0)
    answer = call(dev, LAYERED, 1)
    assert answer[:2] == (0, 0) and answer[2].tolist() == [0, 0, 0, 0]
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        call(bare, EVERYWHERE, 1)
    assert e.value.code == -3
    bare.close()


def test_device_group_gives_the_unsharded_store(dev, hip):
    n = 3 * 2048 + 77
    before, _ = upload(dev, n, "f64", "every_third")
    whole = call(dev, LAYERED, 4)
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
        got = call(g, LAYERED, 4)
        assert got[:2] == whole[:2] and got[2].tolist() == whole[2].tolist() and 0 < whole[1] < whole[0]
        for f in range(hip.E + 1):
            assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            call(g, dict(LAYERED, eta=[0.5, 1.5, 0.0, 0.5]), 4)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 4096, 6
STEP = 0.5                             # length of a move
DT = STEP / C


class AtRest(phys.DeviceStep):
    """Behind the ReemissionStep: the photons at rest, pass by pass."""
    _fuse_role = None

    def __init__(self):
        self.counts = []

    def _device_run(self, sim):
        v = np.stack(sim._dev.download_state()["v"], 1)
        self.counts.append(int((v == 0).all(axis=1).sum()))


def test_a_gas_that_returns_everything_it_absorbs_leaves_nobody_at_rest():
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=lambda s: len(s.ts) >= PASSES)
    src = phys.light.PhotonSource(origin=(2.0, 0.0, 0.0), direction=(1.0, 0.0, 0.0), angular="isotropic")
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
    gas = phys.light.PathAbsorptionStep(0.6)                           # p = 1 - exp(-0.3): about a quarter per pass
    step = phys.light.ReemissionStep(eta=1.0)                          # over all of space, isotropic, at once
    look = AtRest()
    for k, s in enumerate((gas, step, look), 3):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    rows = [[int(row[1]), int(row[2]), row[3].tolist()] for row in step.data]
    absorbed = [int(row[2]) for row in gas.data]
    print("parked, re-emitted, by layer:", rows, "absorbed:", absorbed)
    assert len(rows) == PASSES == step._pass and look.counts == [0] * PASSES
    assert [row[1] for row in rows] == absorbed == [row[0] for row in rows] and min(absorbed) > N_SIM // 8
    assert all(row[2] == [row[1]] for row in rows) and step.reemitted == absorbed[-1] and step.by_layer.tolist() == [absorbed[-1]]
    assert "ReemissionStep" in sim.launch_note or "PathAbsorptionStep" in sim.launch_note
    assert "one launch per light step" in sim.launch_note and len(sim.objects) == N_SIM
    speed = np.sqrt((sim.download("v") ** 2).sum(axis=1))
    assert np.max(np.abs(speed - C)) < 1e-6 * C                        # everybody flies
    sim.close(download=False)
