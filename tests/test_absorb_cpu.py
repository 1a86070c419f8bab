"""CPU: AbsorptionStep -- the constructor's refusals, the numpy restatement of the sweep (light._absorb_scattered) on a seeded
cloud (layers, edges, who is left alone, the binomial of the draw, the tallies against numpy.histogram), the host-resident path,
the plan the step makes, ``_device_run`` on stand-ins, the header and the refusals that need no device.
Everything is exact: the sweep has no sin, cos, exp or division."""
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import _hip, build, light, tally
from absorb_reference import C, CENTER, E_BINS, EDGES, SEED, cloud, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000
OMEGA3 = (1.0, 0.5, 0.0)


@pytest.fixture(scope="module")
def pop():
    return cloud(N)


def absorb(p, omega0, edges=EDGES, E_bins=None, seed=SEED, n_pass=1, dtype=np.float64, center=CENTER):
    return light._absorb_scattered(p["r"], p["v"], p["dv"], p["E"], p["photon"], p["ids"], omega0, edges, center, E_bins, seed, n_pass, dtype)


def interacting(p):
    with np.errstate(invalid="ignore"):
        return (p["dv"] != 0).any(axis=1) & p["photon"]


def layers_of(p):
    """The layer of every row from its distance, independently of the restatement's search: -1 outside or NaN."""
    d = p["r"] - CENTER
    q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    e2 = EDGES * EDGES
    out = np.full(len(q), -1)
    for b in range(len(EDGES) - 1):
        with np.errstate(invalid="ignore"):
            out[(q >= e2[b]) & ((q < e2[b + 1]) | ((b == len(EDGES) - 2) & (q == e2[b + 1])))] = b
    return out


# ------------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("kw, word", [
    (dict(omega0=1.5), "omega0"), (dict(omega0=-0.1), "omega0"), (dict(omega0=np.nan), "omega0"), (dict(omega0="x"), "omega0"),
    (dict(omega0=(0.5, 0.5)), "omega0"),                                                        # a sequence without edges
    (dict(omega0=0.5, edges=(1.0, 2.0)), "omega0"), (dict(omega0=(0.5, 0.5), edges=(1.0, 2.0)), "omega0"),   # length mismatch
    (dict(omega0=(0.5, 1.5), edges=(1.0, 2.0, 3.0)), "omega0"), (dict(omega0=(0.5, np.nan), edges=(1.0, 2.0, 3.0)), "omega0"),
    (dict(omega0=[0.5] * 65, edges=np.arange(66.0)), "edges"),                                  # L > 64
    (dict(omega0=(0.5,), edges=(2.0, 1.0)), "edges"), (dict(omega0=(0.5,), edges=(1.0, 1.0)), "edges"),
    (dict(omega0=(0.5,), edges=(-1.0, 1.0)), "edges"), (dict(omega0=(0.5,), edges=(1.0, np.inf)), "edges"),
    (dict(omega0=(0.5,), edges=(1.0, np.nan)), "edges"), (dict(omega0=(0.5,), edges=(1.0, 1e200)), "edges"),
    (dict(omega0=(0.5,), edges=(0.0, 1e-200)), "edges"), (dict(omega0=(0.5,), edges=(1.0,)), "edges"),
    (dict(center=(0, 0)), "center"), (dict(center=(0, np.nan, 0)), "center"), (dict(center="abc"), "center"),
    (dict(E_bins=(1.0,)), "E_bins"), (dict(E_bins=(2.0, 1.0)), "E_bins"), (dict(E_bins=(1.0, np.nan)), "E_bins"),
    (dict(E_bins=np.arange(1026.0)), "E_bins"),
    (dict(omega0=[0.5] * 64, edges=np.arange(65.0), E_bins=np.arange(200.0)), "E_bins")])       # too many cells
def test_constructor_refusals_name_the_argument(kw, word):
    with pytest.raises(ValueError, match=r"\b%s\b" % word):
        phys.light.AbsorptionStep(**kw)


def test_constructor_keeps_what_it_was_given():
    d = phys.light.AbsorptionStep()
    assert (d.omega0, d.edges, d.E_bins, d.out_fn, d.interacted, d.absorbed, d.data, d._pass) == (1.0, None, None, None, 0, 0, [], 0)
    assert d.center.tolist() == [0, 0, 0] and d.absorbed_by_layer.tolist() == [0] and d.E_hist is None
    assert d._fuse_role is None and d._device_native
    s = phys.light.AbsorptionStep(OMEGA3, edges=EDGES, center=CENTER, E_bins=E_BINS, out_fn="x.csv")
    assert s.omega0.tolist() == list(OMEGA3) and s.edges.tolist() == EDGES.tolist() and s.center.tolist() == CENTER.tolist()
    assert s.E_bins.tolist() == E_BINS.tolist() and s.out_fn == "x.csv"
    assert s.absorbed_by_layer.shape == (3,) and s.E_hist.shape == (3, 8) and s.E_hist.dtype == np.int64
    assert phys.light.AbsorptionStep(0).omega0 == 0.0 and phys.light.AbsorptionStep(0.25).omega0 == 0.25
    assert phys.light.AbsorptionStep([0.5] * 64, edges=np.arange(65.0), E_bins=np.arange(191.0)).E_hist.shape == (64, 190)
    assert phys.light.AbsorptionStep is light.AbsorptionStep
    import phys.light as short
    assert short.AbsorptionStep is light.AbsorptionStep
    assert (_hip.ABSORB_MAX_LAYERS, _hip.ABSORB_MAX_BINS, _hip.ABSORB_MAX_CELLS) == (64, 1024, 12288)


# ------------------------------------------------------------------------------------------------ the restatement
def test_a_conservative_medium_absorbs_nobody_and_draws_nothing(pop, monkeypatch):
    drawn = []
    real = light._philox_block
    monkeypatch.setattr(light, "_philox_block", lambda ids, *a: drawn.append(len(ids)) or real(ids, *a))
    for om, edges in ((1.0, None), ((1.0, 1.0, 1.0), EDGES)):
        o = absorb(pop, om, edges, E_BINS)
        assert not o["absorbed"].any() and not o["absorbed_by_layer"].any() and not o["E_hist"].any()
        assert same_bits(o["v"], pop["v"]) and same_bits(o["dv"], pop["dv"])
        assert np.array_equal(o["interacted"], interacting(pop)) and N // 3 < o["interacted"].sum() < 2 * N // 3
    assert sum(drawn) == 0
    o = absorb(pop, OMEGA3)                                             # only layer 1 draws: layer 0 is conservative, layer 2 is black
    assert drawn[-1] == int((o["layer"] >= 1).sum()) > 0


def test_a_black_medium_absorbs_every_interacting_photon_inside_a_layer(pop):
    o = absorb(pop, (0.0, 0.0, 0.0))
    lay = layers_of(pop)
    go = interacting(pop)
    assert np.array_equal(o["interacted"], go)
    assert np.array_equal(o["layer"], np.where(go, lay, -1))
    assert np.array_equal(o["absorbed"], go & (lay >= 0)) and o["absorbed"].sum() > N // 5
    assert o["absorbed_by_layer"].tolist() == [int((go & (lay == b)).sum()) for b in range(3)] and min(o["absorbed_by_layer"]) > 100
    gone = o["absorbed"]
    assert not o["v"][gone].any() and not o["dv"][gone].any() and not np.signbit(o["v"][gone]).any() and not np.signbit(o["dv"][gone]).any()
    everywhere = absorb(pop, 0.0, None)                                 # no layers: everybody who interacted, NaN positions included
    assert np.array_equal(everywhere["absorbed"], go) and everywhere["absorbed_by_layer"].tolist() == [int(go.sum())]
    assert np.array_equal(everywhere["layer"], np.where(go, 0, -1))


def test_rows_outside_the_layers_nan_rows_and_objects_are_untouched(pop):
    o = absorb(pop, (0.0, 0.0, 0.0), E_bins=E_BINS)
    lay = layers_of(pop)
    k = np.arange(N)
    nan_r, nan_dv, obj = k % 101 == 5, k % 103 == 3, k % 7 == 0
    with np.errstate(invalid="ignore"):
        moved = (pop["dv"] != 0).any(axis=1)
    assert (obj & moved).sum() > 100 and not o["interacted"][obj].any() and not o["absorbed"][obj].any()       # Objects with dv != 0
    assert (nan_r & moved & ~obj).sum() > 20 and o["interacted"][nan_r & moved & ~obj].all() and not o["absorbed"][nan_r].any()
    assert o["interacted"][nan_dv & ~obj].all()                         # NaN != 0: they interacted
    assert o["absorbed"][nan_dv & ~obj & (lay >= 0)].all() and (nan_dv & ~obj & (lay >= 0)).sum() > 20
    outside = interacting(pop) & (lay < 0)
    assert outside.sum() > 1000 and not o["absorbed"][outside].any()
    keep = ~o["absorbed"]
    assert same_bits(o["v"][keep], pop["v"][keep]) and same_bits(o["dv"][keep], pop["dv"][keep])
    assert not o["absorbed"][~interacting(pop)].any()
    # a NaN energy, or one outside the bins, is absorbed and counted by layer but in no bin
    assert o["E_hist"].sum() < o["absorbed_by_layer"].sum() == o["absorbed"].sum()


def test_edges_belong_to_the_upper_layer_and_the_last_edge_to_the_last():
    d = np.array([[1.0, 0, 0],                            # 0: on the first edge: layer 0
                  [0, 2.0, 0],                            # 1: on an inner edge: the upper layer, 1
                  [0, 0, -3.5],                           # 2: on the other inner edge: layer 2
                  [4.0, 0, 0],                            # 3: on the last edge: the last layer
                  [np.nextafter(4.0, 5.0), 0, 0],         # 4: just beyond
                  [np.nextafter(1.0, 0.0), 0, 0],         # 5: just inside the hole
                  [0, np.nextafter(2.0, 0.0), 0],         # 6: just below the inner edge: layer 0
                  [0, 0, -4.0]])                          # 7: on the last edge, the other way
    n = len(d)
    p = {"r": d, "v": np.full((n, 3), C), "dv": np.full((n, 3), 1.0), "E": np.full(n, 2.0), "photon": np.ones(n, dtype=bool),
         "ids": np.arange(n)}
    o = absorb(p, (0.0, 0.0, 0.0), center=np.zeros(3))                  # (about the origin: r - center is d to the last bit)
    assert o["layer"].tolist() == [0, 1, 2, 2, -1, -1, 0, 2]
    assert o["absorbed"].tolist() == [True, True, True, True, False, False, True, True] and o["absorbed_by_layer"].tolist() == [2, 1, 3]
    assert o["interacted"].all()


def test_the_absorbed_fraction_is_binomial():
    n = 200_000
    p = {"r": np.zeros((n, 3)), "v": np.full((n, 3), C), "dv": np.full((n, 3), 1.0), "E": np.full(n, 2.0), "photon": np.ones(n, dtype=bool),
         "ids": np.arange(n) + 7_000_000_001}
    o = absorb(p, 0.7, None)
    assert o["interacted"].sum() == n
    frac = o["absorbed"].mean()
    print("absorbed fraction %.5f (0.3 +- %.5f at 5 sigma)" % (frac, 5 * np.sqrt(0.3 * 0.7 / n)))
    assert abs(frac - 0.3) <= 5 * np.sqrt(0.3 * 0.7 / n)
    # the draw itself: absorbed iff not (u < omega0), u of counter word 12
    u = light._philox_block(p["ids"], SEED, 1, 12)[0]
    assert np.array_equal(o["absorbed"], ~(u < 0.7))
    again, other, same = absorb(p, 0.7, None, n_pass=2), absorb(p, 0.7, None, seed=SEED + 1), absorb(p, 0.7, None)
    assert not np.array_equal(again["absorbed"], o["absorbed"]) and not np.array_equal(other["absorbed"], o["absorbed"])
    assert np.array_equal(same["absorbed"], o["absorbed"])
    for w in (8, 9, 10, 11):                                            # not the ground's or the phase function's numbers
        assert not np.array_equal(light._philox_block(p["ids"][:1000], SEED, 1, w)[0], u[:1000])


def test_tallies_are_numpy_histograms_over_the_masks(pop):
    for om, edges in ((OMEGA3, EDGES), ((0.3, 0.6, 0.9), EDGES), (0.5, None)):
        o = absorb(pop, om, edges, E_BINS)
        rows = 1 if edges is None else 3
        gone = o["absorbed"]
        assert gone.sum() > 500 and o["absorbed_by_layer"].dtype == np.int64 and o["E_hist"].dtype == np.int64
        assert o["absorbed_by_layer"].tolist() == np.histogram(o["layer"][gone], bins=np.arange(rows + 1))[0].tolist()
        assert o["E_hist"].shape == (rows, 8)
        for b in range(rows):
            assert o["E_hist"][b].tolist() == np.histogram(pop["E"][gone & (o["layer"] == b)], bins=E_BINS)[0].tolist(), b
        assert not (gone & ~o["interacted"]).any() and not gone[o["layer"] < 0].any()
    o = absorb(pop, OMEGA3, EDGES, E_BINS)
    assert o["absorbed_by_layer"][0] == 0 and o["absorbed_by_layer"][2] == int((o["layer"] == 2).sum())
    on_edge = dict(pop, E=np.where(np.arange(N) % 2 == 0, E_BINS[-1], E_BINS[3]))               # the last edge is closed, an inner one opens its bin
    h = absorb(on_edge, 0.0, None, E_BINS)["E_hist"][0]
    assert h[-1] > 0 and h[3] > 0 and h.sum() == h[-1] + h[3] == interacting(pop).sum()


def test_fp32_rows_are_zero_either_way_and_layers_and_draws_come_from_the_widened_values():
    p32 = cloud(N, dtype=np.float32)
    assert same_bits(p32["r"], p32["r"].astype(np.float32).astype(np.float64))                  # float32 values, widened
    o64, o32 = absorb(p32, OMEGA3, E_bins=E_BINS), absorb(p32, OMEGA3, E_bins=E_BINS, dtype=np.float32)
    for name in ("v", "dv", "interacted", "absorbed", "layer", "absorbed_by_layer", "E_hist"):
        assert same_bits(o32[name], o64[name]), name
    assert o32["absorbed"].sum() > 500 and not o32["v"][o32["absorbed"]].any()
    # a store's float32 value is what is binned: just below an edge in float64, on it once rounded to float32
    d = np.array([[0.0, np.nextafter(2.0, 0.0), 0.0]])
    one = {"v": np.full((1, 3), C), "dv": np.ones((1, 3)), "E": np.full(1, 2.0), "photon": np.ones(1, dtype=bool), "ids": np.arange(1)}
    assert absorb(dict(one, r=d), OMEGA3, center=np.zeros(3))["layer"].tolist() == [0]
    assert absorb(dict(one, r=d.astype(np.float32).astype(np.float64)), OMEGA3, center=np.zeros(3), dtype=np.float32)["layer"].tolist() == [1]


# ------------------------------------------------------------------------------------------------ the step on the host
def photons(n):
    p = cloud(n, seed=11)
    out = []
    for k in range(n):
        o = phys.light.PhotonObject(E=phys.Measurement(np.double(p["E"][k]), "J**1"), v=phys.light.c * [1, 0, 0]) if p["photon"][k] else phys.Object()
        o.r = phys.Measurement(np.array(p["r"][k]), "m**1")
        o.v, o.dv = np.array(p["v"][k]), np.array(p["dv"][k])
        out.append(o)
    return out, p


class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed = 0.25, SEED

    def __init__(self, objs, py=False):
        self.objects, self.py = objs, py

    def _py_semantics(self):
        return self.py


def test_host_resident_objects_get_the_restatement_s_state(tmp_path):
    n = 700
    objs, p = photons(n)
    sim = HostSim(objs)
    r_code = tally.vec3(objs, "r")                                      # positions in code units, as the step reads them
    E_code = tally.photon_energies(objs, phys.light.PhotonObject)[0]
    step = phys.light.AbsorptionStep(OMEGA3, edges=EDGES, center=CENTER, E_bins=E_BINS, out_fn=str(tmp_path / "absorb.csv"))
    step.run(sim)
    o = light._absorb_scattered(r_code, p["v"], p["dv"], E_code, p["photon"], np.arange(n), OMEGA3, EDGES, CENTER, E_BINS, SEED, 1)
    assert step.absorbed == int(o["absorbed"].sum()) > 30 and step.interacted == int(o["interacted"].sum()) > 200
    assert step.absorbed_by_layer.tolist() == o["absorbed_by_layer"].tolist() and step.E_hist.tolist() == o["E_hist"].tolist()
    row = step.data[0]
    assert len(step.data) == 1 and len(row) == 5 and list(row[:3]) == [0.25, step.interacted, step.absorbed]
    assert row[3].tolist() == o["absorbed_by_layer"].tolist() and row[4].tolist() == o["E_hist"].tolist()
    for k, obj in enumerate(sim.objects):
        assert same_bits(np.asarray(obj.v, dtype=np.float64), o["v"][k]) and same_bits(np.asarray(obj.dv, dtype=np.float64), o["dv"][k]), k
        assert type(obj) is (phys.light.PhotonObject if p["photon"][k] else phys.Object)
    assert same_bits(tally.vec3(objs, "r"), r_code) and sim.launch_note is None
    step.run(sim)                                                       # absorbed photons no longer interact; the others draw again
    again = light._absorb_scattered(r_code, o["v"], o["dv"], E_code, p["photon"], np.arange(n), OMEGA3, EDGES, CENTER, E_BINS, SEED, 2)
    assert step._pass == 2 and step.interacted == int(again["interacted"].sum()) == int(o["interacted"].sum()) - int(o["absorbed"].sum())
    assert step.absorbed == int(again["absorbed"].sum()) and len(step.data) == 2
    step.terminate(sim)
    lines = open(str(tmp_path / "absorb.csv")).read().splitlines()
    assert len(lines) == 2 and lines[0].startswith("0.25, %d, %d, [" % (int(o["interacted"].sum()), int(o["absorbed"].sum())))
    plain = phys.light.AbsorptionStep(0.5)
    plain.run(HostSim(photons(50)[0]))
    assert len(plain.data[0]) == 4 and plain.E_hist is None and plain.absorbed_by_layer.shape == (1,)


def test_python_semantics_are_refused_with_the_reason():
    objs, _ = photons(10)
    step = phys.light.AbsorptionStep(0.5)
    with pytest.raises(ValueError, match="dv = v_old"):
        step.run(HostSim(objs, py=True))
    with pytest.raises(ValueError, match="cl_on"):
        step._device_run(HostSim(objs, py=True))
    assert step._pass == 0 and step.data == []


def test_the_step_is_a_plan_item_of_its_own():
    absorber, redirector = phys.light.AbsorptionStep(0.8), phys.light.PhaseFunctionStep("hg", 0.85)

    class Sim:                                                         # what _build_plan / _multi_eligible ask of a simulation
        fuse, _hip = True, _hip
        steps = {0: phys.UpdateTimeStep(lambda s: np.double(1e-3)), 1: phys.newton.NewtonianKinematicsStep(),
                 2: phys.light.ScatterIsotropicStep(A=1.0, n=1.0), 3: absorber, 4: redirector}

        def _py_semantics(self):
            return False
    sim = Sim()
    plan = phys.Simulation._build_plan(sim)
    assert [kind for kind, _ in plan] == ["single", "fused", "single", "single"] and plan[2][1] is absorber and plan[3][1] is redirector
    sim._plan = plan
    assert not phys.Simulation._multi_eligible(sim)


def fake_sim(dev, scale=2):
    class Sim:
        t, seed, launch_note, _dev = 0.5, 99, None, dev
        _scattered = False
        chunks = []

        def _k_wanted(self):
            return 32

        def _py_semantics(self):
            return False

        def _global(self, values):
            self.chunks.append(len(values))
            return np.asarray(values, dtype=np.int64) * scale           # two ranks with the same tallies
    return Sim()


def test_device_run_notes_the_launch_schedule_and_reduces_the_row():
    class Dev:
        count, calls = 1000, []

        def absorb_scattered(self, *a):
            self.calls.append(a)
            return 70, 7, np.array([1, 2, 4], dtype=np.int64), np.arange(24, dtype=np.int64).reshape(3, 8)
    sim = fake_sim(Dev())
    step = phys.light.AbsorptionStep(OMEGA3, edges=EDGES, center=CENTER, E_bins=E_BINS)
    step._device_run(sim)
    step._device_run(sim)
    assert "AbsorptionStep" in sim.launch_note and "one launch per light step" in sim.launch_note and sim._scattered
    assert (step.interacted, step.absorbed, step.absorbed_by_layer.tolist()) == (140, 14, [2, 4, 8])
    assert step.E_hist.tolist() == (2 * np.arange(24).reshape(3, 8)).tolist() and step.E_hist.dtype == np.int64
    assert len(step.data) == 2 and list(step.data[0][:3]) == [0.5, 140, 14] and step.data[1][3].tolist() == [2, 4, 8]
    assert sim.chunks == [1 + 2 + 3 + 24] * 2                           # one collective per pass
    (a, b) = Dev.calls
    assert a[0].tolist() == list(OMEGA3) and a[1].tolist() == EDGES.tolist() and a[2].tolist() == CENTER.tolist() and a[3].tolist() == E_BINS.tolist()
    assert (a[4], a[5], b[5]) == (99, 1, 2)                             # the step's own pass counter, not sim._next_launch()
    sim2 = fake_sim(Dev())
    sim2.launch_note = "something else"
    step._device_run(sim2)
    assert sim2.launch_note == "something else"


def test_a_row_longer_than_one_collective_is_reduced_in_pieces():
    L, B = 64, 40

    class Dev:
        count = 5

        def absorb_scattered(self, *a):
            return 9, 3, np.arange(L, dtype=np.int64), np.arange(L * B, dtype=np.int64).reshape(L, B)
    sim = fake_sim(Dev(), scale=3)
    step = phys.light.AbsorptionStep([0.5] * L, edges=np.arange(L + 1.0), E_bins=np.arange(B + 1.0))
    step._device_run(sim)
    n = 1 + 2 + L + L * B
    assert n > tally.ALLREDUCE_CHUNK and sim.chunks == [tally.ALLREDUCE_CHUNK, n - tally.ALLREDUCE_CHUNK]
    assert (step.interacted, step.absorbed) == (27, 9) and step.absorbed_by_layer.tolist() == (3 * np.arange(L)).tolist()
    assert step.E_hist.tolist() == (3 * np.arange(L * B).reshape(L, B)).tolist()
    plain = phys.light.AbsorptionStep(0.5)                              # no bins: no histogram in the payload or the row

    class Dev1:
        count = 5

        def absorb_scattered(self, *a):
            return 9, 3, np.array([3], dtype=np.int64), None
    sim1 = fake_sim(Dev1(), scale=1)
    plain._device_run(sim1)
    assert sim1.chunks == [4] and plain.E_hist is None and len(plain.data[0]) == 4 and plain.absorbed_by_layer.tolist() == [3]


def test_multi_device_sums_the_shards_rows():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k, hist=True):
            self.k, self.hist = k, hist

        def absorb_scattered(self, *a, **kw):
            return 10 * self.k, self.k, self.k * np.array([1, 0, 2], dtype=np.int64), self.k * np.ones((3, 4), dtype=np.int64) if self.hist else None
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    inter, gone, by_layer, hist = md.absorb_scattered(OMEGA3, EDGES, CENTER, E_BINS, 1, 1)
    md.shards = [Shard(1, False), Shard(2, False)]
    bare = md.absorb_scattered(OMEGA3, EDGES, CENTER, None, 1, 1)
    md._pool.shutdown()
    assert (inter, gone, by_layer.tolist()) == (1110, 111, [111, 0, 222]) and hist.tolist() == [[111] * 4] * 3
    assert bare[:2] == (30, 3) and bare[2].tolist() == [3, 0, 6] and bare[3] is None


# ------------------------------------------------------------------------------------------------ the library
ENTRIES = ("pcl_step_absorb_scattered", "pcl_group_step_absorb_scattered")


def test_header_declares_both_entry_points_and_the_limits():
    text = open(os.path.join(ROOT, "include", "physicl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and entry in _hip._PROTOTYPES
        assert len(_hip._PROTOTYPES[entry]) == 11
    for name, value in (("PCL_ABSORB_MAX_LAYERS", _hip.ABSORB_MAX_LAYERS), ("PCL_ABSORB_MAX_BINS", _hip.ABSORB_MAX_BINS),
                        ("PCL_ABSORB_MAX_CELLS", _hip.ABSORB_MAX_CELLS)):
        assert re.findall(r"#define\s+%s\s+(\d+)\b" % name, code) == [str(value)], name
    assert "(id_lo, id_hi, pass, 12)" in text                          # the arithmetic is written out, the counter word with it
    # the word is used by nothing else in the library's sources
    used = []
    for f in sorted(os.listdir(build.CSRC)):
        if f.endswith((".hip", ".h")):
            used += [(f, w) for w in re.findall(r"pcl_philox4x32_10\(.*?, (\d+)u, ", open(os.path.join(build.CSRC, f)).read())]
    assert len(used) > 20 and sorted({int(w) for _, w in used}) == [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12]
    used = [(f, w + "u") for f, w in used if w == "12"]
    assert used == [("pcl_surface.hip", "12u")], used


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context, which is refused as well)."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    counts, hist = np.full(2 + 64, -7, dtype=np.int64), np.full(64 * 1024, -7, dtype=np.int64)
    arr = lambda x: np.ascontiguousarray(x, dtype=np.float64)                                                  # noqa: E731
    om3, ed3, eb = arr(OMEGA3), arr(EDGES), arr(E_BINS)
    p = lambda a: None if a is None else a.ctypes.data                                                         # noqa: E731
    good = dict(L=3, om=om3, ed=ed3, ce=arr(CENTER), nE=8, Eb=eb, counts=counts, hist=hist)
    bad = [dict(om=None), dict(counts=None), dict(L=-1), dict(L=65, om=arr([0.5] * 65), ed=arr(np.arange(66.0))),
           dict(om=arr([0.5, 1.5, 0.5])), dict(om=arr([0.5, np.nan, 0.5])), dict(om=arr([-0.1, 0.5, 0.5])),
           dict(L=0, om=arr([1.5]), ed=None), dict(ed=None), dict(ed=arr([1.0, 3.0, 2.0, 4.0])), dict(ed=arr([-1.0, 2.0, 3.0, 4.0])),
           dict(ed=arr([1.0, 2.0, 3.0, np.inf])), dict(ed=arr([1.0, 2.0, 3.0, 1e200])), dict(ce=arr([0, np.nan, 0])),
           dict(nE=-1), dict(nE=1025, Eb=arr(np.arange(1026.0))), dict(Eb=None), dict(hist=None), dict(Eb=arr(E_BINS[::-1])),
           dict(L=64, om=arr([0.5] * 64), ed=arr(np.arange(65.0)), nE=192, Eb=arr(np.arange(193.0)))]          # 2 + 64 * 193 cells
    for kw in bad:
        a = dict(good, **kw)
        args = (a["L"], p(a["om"]), p(a["ed"]), p(a["ce"]), a["nE"], p(a["Eb"]), 1, 1, p(a["counts"]), p(a["hist"]))
        assert lib.pcl_step_absorb_scattered(None, *args) == -2, kw
        assert lib.pcl_group_step_absorb_scattered(None, *args) != 0, kw
    assert (counts == -7).all() and (hist == -7).all()
