"""CPU: LayeredPhaseStep -- the numpy restatement of the sweep (light._layered_phase_redirect) against PhaseFunctionStep's for a
single law, the statistics of a tabulated law and of a mixture by layer, the constructor's and the step's refusals, the
host-resident path, ``_device_run`` on stand-ins, the header and the refusals of the ABI that need no device."""
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import _hip, build, light, tally
from absorb_reference import CENTER, EDGES, same_bits
from layered_phase_reference import BAD_CALLS, C, MIX_LAWS, MIX_WEIGHTS, SEED, SINGLE, abi_args, all_scattered, as_phase, cloud, hg_table, \
    table_moments
from phase_reference import cloud as phase_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000
TABLE_SEED = 20261019                                # chosen here, on the CPU, so that the restatement holds the 5 sigma checks below


def layered(r, v, dv, laws, weights=None, edges=None, center=CENTER, photon=None, ids=None, seed=SEED, n_pass=1, dtype=np.float64):
    n = len(v)
    photon = np.ones(n, dtype=bool) if photon is None else photon
    ids = np.arange(n) + 7_000_000_001 if ids is None else ids
    r = np.zeros((n, 3)) if r is None else r
    return light._layered_phase_redirect(r, v, dv, photon, ids, laws, weights, edges, center, C, seed, n_pass, dtype)


# ------------------------------------------------------------------------------------------------ against the phase function
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("law", SINGLE, ids=str)
def test_a_single_law_without_edges_is_the_phase_function_bit_for_bit(law, dtype):
    v, dv = phase_cloud(N, seed=3, dtype=dtype)
    photon = np.arange(N) % 7 != 0
    ids = np.random.RandomState(2).permutation(N) + 7_000_000_001
    phase, g = as_phase(law)
    for n_pass in (1, 5):
        ref = light._phase_redirect(v, dv, photon, ids, phase, g, C, SEED, n_pass, dtype)
        got = layered(None, v, dv, [law], photon=photon, ids=ids, n_pass=n_pass, dtype=dtype)
        assert same_bits(got["v"], ref["v"]) and same_bits(got["dv"], ref["dv"])
        assert np.array_equal(got["redirected"], ref["redirected"]) and np.array_equal(got["scattered"], ref["redirected"])
        assert np.array_equal(ref["scattered"], ref["redirected"])      # (this cloud's old velocities can all be worked with)
        assert same_bits(got["mu"], ref["mu"]) and same_bits(got["w"], ref["w"])
        assert got["by_layer"].tolist() == got["by_law"].tolist() == [int(ref["redirected"].sum())] and ref["redirected"].sum() > N // 4
    weighted = layered(None, v, dv, [law], weights=[3.0], photon=photon, ids=ids, n_pass=5, dtype=dtype)
    assert same_bits(weighted["v"], got["v"]) and same_bits(weighted["dv"], got["dv"])


def test_old_velocities_that_cannot_be_worked_with_are_not_scattered():
    v, dv = phase_cloud(300, seed=3)
    dv[0] = v[0]                                                        # old velocity zero
    v[3] = np.inf                                                       # old velocity not finite
    dv[6, 1] = np.nan
    got = layered(None, v, dv, ["rayleigh"])
    ref = light._phase_redirect(v, dv, np.ones(300, dtype=bool), np.arange(300) + 7_000_000_001, "rayleigh", 0.0, C, SEED, 1)
    assert ref["scattered"][[0, 3, 6]].all() and not got["scattered"][[0, 3, 6]].any() and not got["redirected"][[0, 3, 6]].any()
    assert np.array_equal(got["scattered"], ref["redirected"]) and same_bits(got["v"], ref["v"]) and same_bits(got["dv"], ref["dv"])


# ------------------------------------------------------------------------------------------------ a tabulated law
def test_a_table_is_sampled_as_the_table_says():
    n, K = 200_000, 512
    law = hg_table(0.85, K)
    F, mean, var = table_moments(law[1], law[2])
    v, dv, ids = all_scattered(n)
    got = layered(None, v, dv, [law], ids=ids, seed=TABLE_SEED)
    assert got["redirected"].all() and got["by_law"].tolist() == [n]
    mu, edges = got["mu"], law[1]
    u_a = light._philox_block(ids, TABLE_SEED, 1, 10)[0]
    k = np.clip(np.searchsorted(F, u_a, side="right") - 1, 0, K - 1)    # the bin the draw falls in
    assert np.all((mu >= edges[k]) & (mu <= edges[k + 1]))              # every mu inside its bin
    count = np.bincount(k, minlength=K)
    prob = np.diff(F)
    sigma = np.sqrt(n * prob * (1.0 - prob))
    worst = np.max(np.abs(count - n * prob) / sigma)
    print("table: worst bin %.2f sigma, mean %.6f (table %.6f +- %.6f at 5 sigma)" % (worst, mu.mean(), mean, 5 * np.sqrt(var / n)))
    assert np.all(np.abs(count - n * prob) <= 5 * sigma)
    assert abs(mu.mean() - mean) <= 5 * np.sqrt(var / n)
    assert abs(mean - 0.85) < 1e-3                                      # (the table is Henyey-Greenstein's, to the bins' width)
    # the cosine between the old and the new direction is the mu that was drawn
    o = v - dv
    cos = (got["v"] * o).sum(axis=1) / (C * np.sqrt((o * o).sum(axis=1)))
    assert np.max(np.abs(cos - mu)) < 1e-12
    # uneven bins: the same rule
    edges2 = np.array([-1.0, -0.5, 0.25, 0.9, 1.0])
    few = layered(None, v[:5000], dv[:5000], [("table", edges2, [1.0, 2.0, 3.0, 40.0])], ids=ids[:5000])
    F2 = table_moments(edges2, [1.0, 2.0, 3.0, 40.0])[0]
    u2 = light._philox_block(ids[:5000], SEED, 1, 10)[0]
    k2 = np.searchsorted(F2, u2, side="right") - 1
    slope = np.diff(edges2) / np.diff(F2)
    assert same_bits(few["mu"], np.fmin(np.fmax(edges2[k2] + (u2 - F2[k2]) * slope[k2], edges2[k2]), edges2[k2 + 1]))
    assert np.bincount(k2, minlength=4).min() > 50


# ------------------------------------------------------------------------------------------------ a mixture by layer
def test_a_mixture_follows_the_layers_weights():
    n = 60000
    r, v, dv = cloud(n, seed=4)
    photon = np.arange(n) % 7 != 0
    got = layered(r, v, dv, MIX_LAWS, MIX_WEIGHTS, EDGES, photon=photon)
    ref = light._phase_redirect(v, dv, photon, np.arange(n) + 7_000_000_001, "rayleigh", 0.0, C, SEED, 1)
    absorb = light._absorb_scattered(r, v, dv, np.ones(n), photon, np.arange(n), (0.0, 0.0, 0.0), EDGES, CENTER, None, SEED, 1)
    assert np.array_equal(got["scattered"], ref["redirected"])          # PhaseFunctionStep's rule
    assert np.array_equal(got["layer"], absorb["layer"])                # AbsorptionStep's layers
    go = got["redirected"]
    assert np.array_equal(go, got["scattered"] & (got["layer"] >= 0))
    outside = got["scattered"] & ~go
    assert outside.sum() > 1000 and (np.isnan(r[:, 2]) & got["scattered"]).sum() > 100 and not go[np.isnan(r[:, 2])].any()
    assert same_bits(got["v"][~go], v[~go]) and same_bits(got["dv"][~go], dv[~go])      # not re-directed: untouched
    assert (got["law"][~go] == -1).all() and np.isnan(got["mu"][~go]).all()
    assert not np.array_equal(got["v"][go], v[go])
    assert got["by_layer"].sum() == got["by_law"].sum() == go.sum() and got["by_layer"].min() > 500
    assert got["by_layer"].tolist() == [int((got["layer"] == b).sum()) for b in range(3)]
    assert got["by_law"].tolist() == [int((got["law"] == j).sum()) for j in range(2)]
    for b, row in enumerate(MIX_WEIGHTS):
        here = got["layer"] == b
        used = np.bincount(got["law"][here], minlength=2)
        for j, w in enumerate(row):
            assert abs(used[j] - w * here.sum()) <= 5 * np.sqrt(here.sum() * w * (1 - w)), (b, j, used)   # one-hot rows: exactly
    # one-hot rows choose without regard to u_s; the mixed row is the first j with u_s < C[b][j]
    u_s = light._philox_block((np.arange(n) + 7_000_000_001)[go], SEED, 1, 13)[0]
    lay, law = got["layer"][go], got["law"][go]
    assert (law[lay == 0] == 0).all() and (law[lay == 2] == 1).all() and u_s[lay == 0].max() > 0.99 and u_s[lay == 2].min() < 0.01
    assert np.array_equal(law[lay == 1], (u_s[lay == 1] >= 0.3).astype(np.int64))
    # what a law makes of a row does not depend on the mixture: the cloud's rows are the single law's rows
    for j, single in enumerate(MIX_LAWS):
        alone = layered(r, v, dv, [single], None, EDGES[[0, -1]], photon=photon)
        mine = got["law"] == j
        assert mine.sum() > 1000 and same_bits(got["v"][mine], alone["v"][mine]) and same_bits(got["dv"][mine], alone["dv"][mine])
    # fp32: layers and draws from the widened values, what is written rounded once
    r32, v32, dv32 = cloud(n, seed=4, dtype=np.float32)
    g64, g32 = (layered(r32, v32, dv32, MIX_LAWS, MIX_WEIGHTS, EDGES, dtype=t) for t in (np.float64, np.float32))
    assert np.array_equal(g64["law"], g32["law"]) and same_bits(g32["v"], g64["v"].astype(np.float32).astype(np.float64))


# ------------------------------------------------------------------------------------------------ refusals
T2 = ("table", [-1.0, 0.0, 1.0], [1.0, 2.0])


@pytest.mark.parametrize("kw, word", [
    (dict(laws=[]), "laws"), (dict(laws=["isotropic"] * 9, weights=[1] * 9), "laws"), (dict(laws="rayleigh"), "laws"),
    (dict(laws=["mie"]), "laws"), (dict(laws=[("hg",)]), "laws"), (dict(laws=[("hg", 0.5, 1)]), "laws"), (dict(laws=[7]), "laws"),
    (dict(laws=[("hg", 1.0)]), "g"), (dict(laws=[("hg", -1.0)]), "g"), (dict(laws=[("hg", np.nan)]), "g"), (dict(laws=[("hg", "x")]), "g"),
    (dict(laws=[("table", [-0.5, 0.0, 1.0], [1.0, 2.0])]), "mu_edges"), (dict(laws=[("table", [-1.0, 0.0, 0.5], [1.0, 2.0])]), "mu_edges"),
    (dict(laws=[("table", [-1.0, 0.0, 0.0, 1.0], [1.0, 2.0, 1.0])]), "mu_edges"), (dict(laws=[("table", [-1.0], [])]), "mu_edges"),
    (dict(laws=[("table", [-1.0, 0.0, 1.0], [1.0, 0.0])]), "p"), (dict(laws=[("table", [-1.0, 0.0, 1.0], [1.0, -2.0])]), "p"),
    (dict(laws=[("table", [-1.0, 0.0, 1.0], [1.0, np.inf])]), "p"), (dict(laws=[("table", [-1.0, 0.0, 1.0], [1.0, np.nan])]), "p"),
    (dict(laws=[("table", [-1.0, 0.0, 1.0], [1.0])]), "p"),
    (dict(laws=[("table", np.linspace(-1, 1, 1026), np.ones(1025))]), "1024"),
    (dict(laws=[("table", np.linspace(-1, 1, 1025), np.ones(1024))] * 2 + [T2], weights=[1, 1, 1]), "2048"),
    (dict(laws=[("table", [-1.0, 0.0, 1.0], [1.0, 1e-300])]), "strictly increasing"),
    (dict(laws=MIX_LAWS), "weights"), (dict(laws=MIX_LAWS, weights=[1, 2, 3]), "weights"), (dict(laws=MIX_LAWS, weights=[[1, 2]] * 2), "weights"),
    (dict(laws=MIX_LAWS, weights=[1, 1], edges=EDGES), "weights"), (dict(laws=MIX_LAWS, weights=[[1, 1]] * 2, edges=EDGES), "weights"),
    (dict(laws=MIX_LAWS, weights=[1, -1]), "weights"), (dict(laws=MIX_LAWS, weights=[0, 0]), "weights"), (dict(laws=MIX_LAWS, weights=[1, np.nan]), "weights"),
    (dict(laws=MIX_LAWS, weights=[[1, 0], [0, 0], [0, 1]], edges=EDGES), "weights"), (dict(laws=MIX_LAWS, weights="ab"), "weights"),
    (dict(laws=["rayleigh"], edges=np.arange(66.0)), "edges"), (dict(laws=["rayleigh"], edges=(2.0, 1.0)), "edges"),
    (dict(laws=["rayleigh"], edges=(-1.0, 1.0)), "edges"), (dict(laws=["rayleigh"], edges=(1.0, 1e200)), "edges"),
    (dict(laws=["rayleigh"], center=(0, 0)), "center"), (dict(laws=["rayleigh"], center=(0, np.nan, 0)), "center")])
def test_constructor_refusals_name_the_argument(kw, word):
    with pytest.raises(ValueError, match=r"\b%s\b" % word) as e:
        phys.light.LayeredPhaseStep(**kw)
    assert re.search(r"\b(laws|weights|edges|center)\b", str(e.value))
    if word in ("1024", "2048"):
        assert "laws" in str(e.value)
    if kw.get("edges") is not None and len(kw["edges"]) == 66:
        assert "64" in str(e.value)
    if len(kw["laws"]) == 9:
        assert "8" in str(e.value)


def test_constructor_keeps_what_it_was_given():
    d = phys.light.LayeredPhaseStep(["rayleigh"])
    assert (d.laws, d.edges, d.out_fn, d.scattered, d.redirected, d.data, d._pass) == (["rayleigh"], None, None, 0, 0, [], 0)
    assert d.weights.tolist() == [[1.0]] and d.cum.tolist() == [[1.0]] and d.center.tolist() == [0, 0, 0]
    assert d.by_layer.tolist() == [0] and d.by_law.tolist() == [0] and d._fuse_role is None and d._device_native
    s = phys.light.LayeredPhaseStep(MIX_LAWS, MIX_WEIGHTS, edges=EDGES, center=CENTER, out_fn="x.csv")
    assert s.laws == ["rayleigh", ("hg", 0.85)] and s.weights.tolist() == MIX_WEIGHTS and s.cum.tolist() == [[1, 1], [0.3, 1], [0, 1]]
    assert s.edges.tolist() == EDGES.tolist() and s.center.tolist() == CENTER.tolist() and s.by_layer.shape == (3,) and s.by_law.shape == (2,)
    t = phys.light.LayeredPhaseStep([T2, ("hg", 0)], [2, 6])            # [M] without edges; F is made exactly
    assert t.weights.tolist() == [[2, 6]] and t.cum.tolist() == [[0.25, 1.0]]
    assert t.laws[0][0] == "table" and t.laws[0][1].tolist() == [-1, 0, 1] and t.laws[0][2].tolist() == [0.0, 1 / 3, 1.0]
    big = phys.light.LayeredPhaseStep([("table", np.linspace(-1, 1, 1025), np.ones(1024))] * 2 + ["isotropic"] * 6, np.ones((64, 8)),
                                      edges=np.arange(65.0))            # the limits themselves
    assert big.cum.shape == (64, 8) and (big.cum[:, -1] == 1.0).all()
    import phys.light as short
    assert short.LayeredPhaseStep is light.LayeredPhaseStep is phys.light.LayeredPhaseStep
    assert (_hip.LPHASE_MAX_LAWS, _hip.LPHASE_MAX_LAYERS, _hip.LPHASE_MAX_NODES, _hip.LPHASE_MAX_TOTAL_NODES, _hip.PHASE_TABLE) == (8, 64, 1024, 2048, 3)


# ------------------------------------------------------------------------------------------------ the step on the host
def objects(n, seed=11):
    r, v, dv = cloud(n, seed=seed)
    out = []
    for k in range(n):
        o = phys.light.PhotonObject(E=phys.Measurement(np.double(1e-19), "J**1"), v=phys.light.c * [1, 0, 0]) if k % 5 else phys.Object()
        o.r = phys.Measurement(np.array(np.nan_to_num(r[k], nan=9.0)), "m**1")
        o.v, o.dv = np.array(v[k]), np.array(dv[k])
        out.append(o)
    return out, v, dv


class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed = 0.25, SEED

    def __init__(self, objs, py=False, steps=None):
        self.objects, self.py, self.steps = objs, py, steps or {}

    def _py_semantics(self):
        return self.py


def test_host_resident_objects_get_the_restatement_s_state(tmp_path):
    n = 900
    objs, v, dv = objects(n)
    photon = np.arange(n) % 5 != 0
    sim = HostSim(objs)
    r_code = tally.vec3(objs, "r")
    step = phys.light.LayeredPhaseStep(MIX_LAWS, MIX_WEIGHTS, edges=EDGES, center=CENTER, out_fn=str(tmp_path / "layered.csv"))
    sim.steps = {0: step}
    step.run(sim)
    c_code = light._c_h_literals()[0]
    ref = light._layered_phase_redirect(r_code, v, dv, photon, np.arange(n), MIX_LAWS, MIX_WEIGHTS, EDGES, CENTER, c_code, SEED, 1)
    assert step.scattered == int(ref["scattered"].sum()) == int(((np.arange(n) % 3 == 0) & photon).sum())
    assert 0 < step.redirected == int(ref["redirected"].sum()) < step.scattered
    assert step.by_layer.tolist() == ref["by_layer"].tolist() and step.by_law.tolist() == ref["by_law"].tolist() and min(step.by_law) > 10
    row = step.data[0]
    assert len(step.data) == 1 and len(row) == 5 and list(row[:3]) == [0.25, step.scattered, step.redirected]
    assert row[3].tolist() == step.by_layer.tolist() and row[4].tolist() == step.by_law.tolist()
    for k, obj in enumerate(sim.objects):
        assert same_bits(np.asarray(obj.v, dtype=np.float64), ref["v"][k]) and same_bits(np.asarray(obj.dv, dtype=np.float64), ref["dv"][k]), k
        assert type(obj) is (phys.light.PhotonObject if photon[k] else phys.Object)
        if not photon[k]:
            assert same_bits(np.asarray(obj.v), v[k]) and same_bits(np.asarray(obj.dv), dv[k])       # plain Objects are untouched
    assert same_bits(tally.vec3(objs, "r"), r_code) and sim.launch_note is None
    step.run(sim)
    assert step._pass == 2 and len(step.data) == 2
    step.terminate(sim)
    lines = open(str(tmp_path / "layered.csv")).read().splitlines()
    assert len(lines) == 2 and lines[0].startswith("0.25, %d, %d, [" % (step.data[0][1], step.data[0][2]))


def test_python_semantics_and_a_second_phase_step_are_refused():
    objs, _, _ = objects(10)
    step = phys.light.LayeredPhaseStep(["rayleigh"])
    with pytest.raises(ValueError, match="dv = v_old"):
        step.run(HostSim(objs, py=True))
    with pytest.raises(ValueError, match="cl_on"):
        step._device_run(HostSim(objs, py=True))
    for other in (phys.light.PhaseFunctionStep("hg", 0.5), phys.light.LayeredPhaseStep(["isotropic"])):
        steps = {0: phys.newton.NewtonianKinematicsStep(), 1: phys.light.ScatterIsotropicStep(A=1.0, n=1.0), 2: step, 3: other}
        with pytest.raises(ValueError, match="one phase step") as e:
            step.run(HostSim(objs, steps=steps))
        assert type(other).__name__ in str(e.value)
        with pytest.raises(ValueError, match="one phase step"):
            step._device_run(HostSim(objs, steps=steps))
    assert step._pass == 0 and step.data == []
    step.run(HostSim(objs, steps={0: phys.light.AbsorptionStep(0.5), 1: step}))      # an absorber is no phase step
    assert step._pass == 1


def test_the_step_is_a_plan_item_of_its_own():
    step = phys.light.LayeredPhaseStep(MIX_LAWS, [1, 1])

    class Sim:                                                         # what _build_plan / _multi_eligible ask of a simulation
        fuse, _hip = True, _hip
        steps = {0: phys.UpdateTimeStep(lambda s: np.double(1e-3)), 1: phys.newton.NewtonianKinematicsStep(),
                 2: phys.light.ScatterIsotropicStep(A=1.0, n=1.0), 3: step, 4: phys.light.AbsorptionStep(0.8)}

        def _py_semantics(self):
            return False
    sim = Sim()
    plan = phys.Simulation._build_plan(sim)
    assert [kind for kind, _ in plan] == ["single", "fused", "single", "single"] and plan[2][1] is step
    sim._plan = plan
    assert not phys.Simulation._multi_eligible(sim)


def test_device_run_notes_the_launch_schedule_and_reduces_the_row():
    class Dev:
        count, calls = 1000, []

        def phase_layered(self, *a):
            self.calls.append(a)
            return 70, 60, np.array([10, 20, 30], dtype=np.int64), np.array([25, 35], dtype=np.int64)

    class Sim:
        t, seed, launch_note, _dev, _scattered, chunks = 0.5, 99, None, Dev(), False, []

        def _k_wanted(self):
            return 32

        def _py_semantics(self):
            return False

        def _global(self, values):
            self.chunks.append(len(values))
            return np.asarray(values, dtype=np.int64) * 2               # two ranks with the same tallies
    sim = Sim()
    step = phys.light.LayeredPhaseStep(MIX_LAWS, MIX_WEIGHTS, edges=EDGES, center=CENTER)
    step._device_run(sim)
    step._device_run(sim)
    assert "LayeredPhaseStep" in sim.launch_note and "one launch per light step" in sim.launch_note and sim._scattered
    assert (step.scattered, step.redirected, step.by_layer.tolist(), step.by_law.tolist()) == (140, 120, [20, 40, 60], [50, 70])
    assert len(step.data) == 2 and list(step.data[1][:3]) == [0.5, 140, 120] and step.data[1][4].tolist() == [50, 70]
    assert sim.chunks == [1 + 2 + 3 + 2] * 2                            # one collective per pass
    a, b = Dev.calls
    assert [law[0] for law in a[0]] == ["rayleigh", "hg"] and a[0][1][1] == 0.85 and a[1].tolist() == [[1, 1], [0.3, 1], [0, 1]]
    assert a[2].tolist() == EDGES.tolist() and a[3].tolist() == CENTER.tolist() and a[4] == light._c_h_literals()[0]
    assert (a[5], a[6], b[6]) == (99, 1, 2)                             # the step's own pass counter


def test_multi_device_sums_the_shards_rows():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def phase_layered(self, *a, **kw):
            return 10 * self.k, self.k, self.k * np.array([1, 0, 2], dtype=np.int64), self.k * np.array([2, 1], dtype=np.int64)
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    scattered, redirected, by_layer, by_law = md.phase_layered(None, None)
    md._pool.shutdown()
    assert (scattered, redirected, by_layer.tolist(), by_law.tolist()) == (1110, 111, [111, 0, 222], [222, 111])


# ------------------------------------------------------------------------------------------------ the library
ENTRIES = ("pcl_step_phase_layered", "pcl_group_step_phase_layered")


def test_header_declares_both_entry_points_and_the_limits():
    text = open(os.path.join(ROOT, "include", "physicl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and len(_hip._PROTOTYPES[entry]) == 15
    for name, value in (("PCL_LPHASE_MAX_LAWS", 8), ("PCL_LPHASE_MAX_LAYERS", 64), ("PCL_LPHASE_MAX_NODES", 1024),
                        ("PCL_LPHASE_MAX_TOTAL_NODES", 2048), ("PCL_PHASE_TABLE", 3)):
        assert re.findall(r"#define\s+%s\s+(\d+)\b" % name, code) == [str(value)], name
    assert "(id_lo, id_hi, pass, 13)" in text and "ONE phase step" in text


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context, which is refused as well)."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in BAD_CALLS:
        keep, args, counts = abi_args(**kw)
        assert lib.pcl_step_phase_layered(None, *args) == -2, kw
        assert lib.pcl_group_step_phase_layered(None, *args) != 0, kw
        assert counts is None or (counts == -7).all()
