"""CPU: PathAbsorptionStep (light.PathAbsorptionStep, light._absorb_path, pcl_step_absorb_path) -- the constructor, the numpy
restatement's rule, draw and statistics, the host-resident path, the header and the bindings and the refusals that need no device."""
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import _hip, build, light, tally
from path_absorb_reference import BAD_CALLS, C, CENTER, E_EDGES, EDGES, ID_BASE, P_CELLS, SEED, abi_args, configs, layout, planted
from writer_reference import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 1.0 / C                                                           # a move of one unit of length


def absorb(state, p=P_CELLS, edges=EDGES, E_edges=E_EDGES, photon=None, ids=None, n_pass=1, dtype=np.float64, seed=SEED):
    n = len(state["E"])
    photon = np.ones(n, dtype=bool) if photon is None else photon
    ids = np.arange(n) + ID_BASE if ids is None else ids
    return light._absorb_path(state["r"], state["v"], state["dv"], state["E"], photon, ids, p, edges, CENTER, E_edges, seed, n_pass, dtype)


# ------------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("kw, word", [
    (dict(k=[1.0, 2.0]), "k"), (dict(k=1.0, edges=EDGES), "k"), (dict(k=[1.0, 2.0, 3.0], edges=EDGES), "k"),
    (dict(k=[1.0, 2.0], E_edges=E_EDGES), "k"), (dict(k=[1.0, 2.0], edges=EDGES, E_edges=E_EDGES), "k"),
    (dict(k=np.ones((3, 2)), edges=EDGES, E_edges=E_EDGES), "k"), (dict(k="thick"), "k"), (dict(k=-1.0), "k"), (dict(k=np.nan), "k"),
    (dict(k=np.inf), "k"), (dict(k=[1.0, -0.5], edges=EDGES), "k"), (dict(k=[1.0, np.nan, 1.0], E_edges=E_EDGES), "k"),
    (dict(k=[1.0], edges=[1.0]), "edges"), (dict(k=[1.0, 1.0], edges=[1.0, 3.0, 2.0]), "edges"), (dict(k=[1.0, 1.0], edges=[-1.0, 2.0, 3.0]), "edges"),
    (dict(k=[1.0, 1.0], edges=[1.0, 2.0, np.inf]), "edges"), (dict(k=[1.0, 1.0], edges=[1.0, 2.0, 1e200]), "edges"),
    (dict(k=np.ones(65), edges=np.arange(66.0)), "edges"), (dict(k=np.ones(3), E_edges=[1.0, 2.0, 1.5, 3.0]), "E_edges"),
    (dict(k=np.ones(3), E_edges=[1.0, np.nan, 2.0, 3.0]), "E_edges"), (dict(k=np.ones(1025), E_edges=np.arange(1026.0)), "E_edges"),
    (dict(k=np.ones((64, 65)), edges=np.arange(65.0), E_edges=np.arange(66.0)), "cells"),
    (dict(k=1.0, center=(0, 0)), "center"), (dict(k=1.0, center=(0, np.nan, 0)), "center"),
])
def test_constructor_refusals_name_the_argument(kw, word):
    with pytest.raises(ValueError, match=r"\b%s\b" % word):
        phys.light.PathAbsorptionStep(**kw)


@pytest.mark.parametrize("dt", [np.nan, np.inf, -1e-9, "soon"])
def test_a_bad_dt_is_refused(dt):
    with pytest.raises(ValueError, match=r"\bdt\b"):
        light._path_probability(1.0, C, dt)
    step = phys.light.PathAbsorptionStep(1.0)
    sim = HostSim([], dt=dt)
    with pytest.raises(ValueError, match=r"\bdt\b"):
        step.run(sim)
    assert step._pass == 0 and step.data == []


def test_constructor_keeps_what_it_was_given_and_the_limits_themselves_pass():
    step = phys.light.PathAbsorptionStep(np.arange(6.0).reshape(2, 3), EDGES, CENTER, E_EDGES)
    assert step.k.shape == (2, 3) and step.k.tolist() == [[0, 1, 2], [3, 4, 5]] and step.edges.tolist() == EDGES.tolist()
    assert step.E_edges.tolist() == E_EDGES.tolist() and step.center.tolist() == CENTER.tolist()
    assert (step.exposed, step.absorbed, step._pass, step.data) == (0, 0, 0, []) and step.absorbed_by_cell.tolist() == [[0] * 3] * 2
    assert phys.light.PathAbsorptionStep(2.5).k.shape == (1, 1)
    assert phys.light.PathAbsorptionStep([1.0, 2.0], edges=EDGES).k.shape == (2, 1)
    assert phys.light.PathAbsorptionStep([1.0, 2.0, 0.0], E_edges=E_EDGES).k.shape == (1, 3)
    big = phys.light.PathAbsorptionStep(np.ones((64, 64)), np.arange(65.0), E_edges=np.arange(65.0))       # 4096 cells
    assert big.absorbed_by_cell.shape == (64, 64) and 64 * 64 == _hip.PATH_ABSORB_MAX_CELLS
    assert phys.light.PathAbsorptionStep(np.ones(1024), E_edges=np.arange(1025.0)).k.shape == (1, _hip.PATH_ABSORB_MAX_BANDS)
    assert phys.light.PathAbsorptionStep(np.ones(64), np.arange(65.0)).k.shape == (_hip.PATH_ABSORB_MAX_LAYERS, 1)
    import phys.light as short
    assert short.PathAbsorptionStep is light.PathAbsorptionStep is phys.light.PathAbsorptionStep


def test_the_probability_is_made_on_the_host_in_float64():
    k = np.array([[0.0, 0.5, 3.0], [1e-12, 40.0, 1e6]])
    p = light._path_probability(k, C, DT)
    assert p.dtype == np.float64 and same_bits(p, -np.expm1(-(k * (C * DT))))
    assert p[0, 0] == 0.0 and p[1, 2] == 1.0 and 0.0 < p[1, 0] < 1e-11 and np.all((p >= 0) & (p <= 1))
    assert same_bits(light._path_probability(k, C, 0.0), np.zeros((2, 3)))                   # no move, no absorption
    quarter = light._path_probability(-np.log(0.75) / (C * DT), C, DT)
    assert abs(float(quarter) - 0.25) <= 1e-15


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_rule_s_edge_cases(dtype):
    n = 6000
    state = layout(n, dtype)
    i = np.arange(n)
    photon = i % 31 != 0
    moving, want_layer, want_band = planted(n)
    for name, (p, edges, E_edges) in configs().items():
        ref = absorb(state, p, edges, E_edges, photon=photon, dtype=dtype)
        go = moving & photon
        layer, band, exposed, gone = ref["layer"], ref["band"], ref["exposed"], ref["absorbed"]
        assert (layer[~go] == -1).all() and (band[~go] == -1).all() and not exposed[~go].any(), name     # at rest, -0.0, an Object
        assert go[39] and go[87] and not go[6] and not go[9] and not go[31], name          # a NaN in v0, v = (0, 0, c); -0.0, at rest, an Object
        assert np.isnan(state["v"][39, 0]) and state["v"][87].tolist() == [0.0, 0.0, dtype(C)] and np.signbit(state["v"][6, 1])
        if edges is None:
            assert (layer[go] == 0).all(), name
        else:
            assert ((layer == want_layer) | (want_layer == -2) | ~go).all() and (layer[go & (want_layer == -2)] >= 0).all(), name
            for mod, b in ((5, 0), (7, 1), (23, 1), (11, -1), (17, -1), (19, -1)):           # on the first, last and inner radius; NaN; outside
                assert (go & (want_layer == b) & (i % mod == 0)).any(), (name, mod)
        has_layer = go & (layer >= 0)
        assert (band[~has_layer] == -1).all(), name                    # a photon in no layer is skipped before E is looked at
        if E_edges is None:
            assert (band[has_layer] == 0).all(), name
        else:
            assert ((band == want_band) | (want_band == -2) | ~has_layer).all() and (band[has_layer & (want_band == -2)] >= 0).all(), name
            for mod, rest, e in ((4, 1, 1), (9, 2, 2), (16, 9, 0), (10, 3, -1), (14, 5, -1), (15, 7, -1)):   # on a band edge, the last, the first; NaN; outside
                assert (has_layer & (want_band == e) & (i % mod == rest)).any(), (name, mod)
        assert np.array_equal(exposed, has_layer & (band >= 0)) and not gone[~exposed].any() and 0 < gone.sum() < exposed.sum(), name
        table = np.asarray(p, dtype=np.float64).reshape(ref["absorbed_by_cell"].shape)
        p_of = table[np.maximum(layer, 0), np.maximum(band, 0)]
        assert not gone[exposed & (p_of == 0.0)].any() and gone[exposed & (p_of == 1.0)].all(), name     # p == 0: nobody; p == 1: everybody
        cells = ref["absorbed_by_cell"]
        assert cells.sum() == gone.sum() and cells.tolist() == [[int((gone & (layer == b) & (band == e)).sum()) for e in range(cells.shape[1])]
                                                                for b in range(cells.shape[0])], name
        for f in ("v", "dv"):                                          # untouched rows keep every bit; absorbed rows are +0.0
            assert same_bits(ref[f][~gone], state[f][~gone]) and same_bits(ref[f][gone], np.zeros((gone.sum(), 3))), (name, f)


def test_a_transparent_gas_draws_nothing_and_a_black_one_takes_everybody(monkeypatch):
    state = layout(3000)
    drawn = []
    real = light._philox_block
    monkeypatch.setattr(light, "_philox_block", lambda ids, seed, w2, w3: drawn.append((len(ids), w3)) or real(ids, seed, w2, w3))
    for seed in (SEED, SEED + 1, 0):
        clear = absorb(state, np.zeros((2, 3)), seed=seed)
        assert not clear["absorbed"].any() and clear["exposed"].sum() > 1000 and same_bits(clear["v"], state["v"]) and same_bits(clear["dv"], state["dv"])
    assert drawn == [(0, 17)] * 3                                      # nobody draws, whatever the seed
    black = absorb(state, np.ones((2, 3)))
    assert np.array_equal(black["absorbed"], black["exposed"]) and black["absorbed_by_cell"].sum() == black["exposed"].sum()
    mixed = absorb(state)                                              # only the cells with p > 0 draw, and only word 17
    p_of = P_CELLS[np.maximum(mixed["layer"], 0), np.maximum(mixed["band"], 0)]
    assert drawn[-1] == (int((mixed["exposed"] & (p_of > 0)).sum()), 17) and {w for _, w in drawn} == {17}


def test_the_draw_is_word_17_by_id_pass_and_seed():
    n = 4000
    state = layout(n)
    ids = np.arange(n) + ID_BASE
    one = absorb(state, 0.5, None, None)
    u = light._philox_block(ids, SEED, 1, 17)[0]
    assert np.array_equal(one["absorbed"], one["exposed"] & (u < 0.5)) and light._PATH_ABSORB_WORD == 17
    for other in (absorb(state, 0.5, None, None, n_pass=2), absorb(state, 0.5, None, None, seed=SEED + 1),
                  absorb(state, 0.5, None, None, ids=ids + 1)):
        assert np.array_equal(other["exposed"], one["exposed"]) and not np.array_equal(other["absorbed"], one["absorbed"])
    perm = np.random.RandomState(3).permutation(n)
    moved = absorb({k: a[perm] for k, a in state.items()}, 0.5, None, None, ids=ids[perm])
    assert np.array_equal(moved["absorbed"], one["absorbed"][perm])    # a photon is its id, wherever it stands
    # independent of the words 12 to 16: an AbsorptionStep or a RecycleStep of the same pass draws what it drew
    for w in range(12, 17):
        a, b = light._philox_block(ids, SEED, 1, w)
        assert not np.array_equal(a, u) and not np.array_equal(b, u) and abs(np.corrcoef(a, u)[0, 1]) < 5.0 / np.sqrt(n), w
    kept = ~one["absorbed"]
    photon = np.ones(n, dtype=bool)
    before = light._absorb_scattered(state["r"], state["v"], state["dv"], state["E"], photon, ids, 0.5, None, CENTER, None, SEED, 1)
    behind = light._absorb_scattered(state["r"], one["v"], one["dv"], state["E"], photon, ids, 0.5, None, CENTER, None, SEED, 1)
    assert np.array_equal(behind["absorbed"][kept], before["absorbed"][kept]) and not behind["interacted"][one["absorbed"]].any()
    assert same_bits(behind["v"][kept], before["v"][kept])


def test_beer_lambert_over_one_pass_and_over_eight():
    """20 000 photons, one layer, p = 0.25: the absorbed count within 5 sigma of n p, the survivors of 8 passes within 5 sigma of
    n 0.75^8 (sigma = sqrt(n q (1 - q)) of the binomial law; the draws are fixed by the seed)."""
    n = 20000
    rng = np.random.RandomState(8)
    v = C * rng.normal(size=(n, 3))
    state = {"r": np.tile(CENTER + [1.5, 0.0, 0.0], (n, 1)), "v": v, "dv": np.zeros((n, 3)), "E": np.ones(n)}
    p = light._path_probability([-np.log(0.75) / (C * DT)], C, DT)
    one = absorb(state, p, [1.0, 2.0], None)
    sigma = np.sqrt(n * 0.25 * 0.75)
    print("absorbed %d of %d at p = 0.25 (5 sigma = %.1f)" % (one["absorbed"].sum(), n, 5 * sigma))
    assert one["exposed"].all() and abs(int(one["absorbed"].sum()) - 5000) <= 5.0 * sigma
    for n_pass in range(1, 9):
        ref = absorb(state, p, [1.0, 2.0], None, n_pass=n_pass)
        state = dict(state, v=ref["v"], dv=ref["dv"])
    left = int((state["v"] != 0).any(axis=1).sum())
    q = 0.75 ** 8
    print("survivors %d of %d after 8 passes, expected %.1f (5 sigma = %.1f)" % (left, n, n * q, 5 * np.sqrt(n * q * (1 - q))))
    assert abs(left - n * q) <= 5.0 * np.sqrt(n * q * (1.0 - q)) and ref["exposed"].sum() > left


# ------------------------------------------------------------------------------------------------ the step on the host
class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed = 0.25, SEED

    def __init__(self, objs, py=False, dt=DT):
        self.objects, self.py, self.dt = objs, py, dt

    def _py_semantics(self):
        return self.py


def objects(n):
    state = layout(n)
    out = []
    for k in range(n):
        E = phys.Measurement(np.double(np.nan_to_num(state["E"][k], nan=9.0)), "J**1")
        o = phys.light.PhotonObject(E=E, v=phys.light.c * [1, 0, 0]) if k % 4 else phys.Object()
        o.r = phys.Measurement(np.array(np.nan_to_num(state["r"][k], nan=9.0)), "m**1")
        o.v, o.dv = np.array(state["v"][k]), np.array(state["dv"][k])
        o.dr = phys.Measurement(np.array(state["dr"][k]), "m**1")
        out.append(o)
    return out


@pytest.mark.parametrize("py", [False, True])
def test_host_resident_objects_get_the_restatement_s_state(tmp_path, py):
    n = 900
    objs = objects(n)
    photon = np.arange(n) % 4 != 0
    sim = HostSim(objs, py=py)                                         # the step reads no dv rule: cl_on=False is not refused
    r0, v0, dr0, dv0 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    E0 = tally.photon_energies(objs, phys.light.PhotonObject)[0]
    k = np.array([[0.0, 0.5, 40.0], [1.0, 2.0, 0.25]])
    step = phys.light.PathAbsorptionStep(k, EDGES, CENTER, E_EDGES, out_fn=str(tmp_path / "gas.csv"))
    step.run(sim)
    p = light._path_probability(k, light._c_h_literals()[0], DT)
    ref = light._absorb_path(r0, v0, dv0, E0, photon, np.arange(n), p, EDGES, CENTER, E_EDGES, SEED, 1)
    gone = ref["absorbed"]
    assert step.exposed == int(ref["exposed"].sum()) > step.absorbed == int(gone.sum()) > 0 and not ref["exposed"][~photon].any()
    assert step.absorbed_by_cell.tolist() == ref["absorbed_by_cell"].tolist() and step.absorbed_by_cell[0, 0] == 0 and sim.launch_note is None
    assert len(step.data) == 1 and list(step.data[0][:3]) == [0.25, step.exposed, step.absorbed]
    assert step.data[0][3].tolist() == ref["absorbed_by_cell"].tolist()
    r1, v1, dr1, dv1 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    assert same_bits(v1, ref["v"]) and same_bits(dv1, ref["dv"]) and same_bits(r1, r0) and same_bits(dr1, dr0)
    assert same_bits(v1[gone], np.zeros((gone.sum(), 3))) and same_bits(v1[~gone], v0[~gone]) and same_bits(dv1[~gone], dv0[~gone])
    assert same_bits(tally.photon_energies(objs, phys.light.PhotonObject)[0], E0)
    for j, obj in enumerate(objs):
        assert type(obj) is (phys.light.PhotonObject if photon[j] else phys.Object)
    step.run(sim)                                                      # a second pass: its own counter word, the absorbed are at rest now
    again = light._absorb_path(r0, ref["v"], ref["dv"], E0, photon, np.arange(n), p, EDGES, CENTER, E_EDGES, SEED, 2)
    assert step._pass == 2 and len(step.data) == 2 and step.exposed == int(again["exposed"].sum()) == int((ref["exposed"] & ~gone).sum())
    assert step.absorbed == int(again["absorbed"].sum())
    step.terminate(sim)
    lines = open(str(tmp_path / "gas.csv")).read().splitlines()
    assert len(lines) == 2 and lines[0].replace(" ", "").startswith("0.25,%d,%d," % (step.data[0][1], step.data[0][2]))


def test_the_step_is_a_plan_item_of_its_own():
    step = phys.light.PathAbsorptionStep(1.0)

    class Sim:                                                         # what _build_plan / _multi_eligible ask of a simulation
        fuse, _hip = True, _hip
        steps = {0: phys.UpdateTimeStep(lambda s: np.double(1e-3)), 1: phys.newton.NewtonianKinematicsStep(),
                 2: phys.light.ScatterIsotropicStep(A=1.0, n=1.0), 3: step, 4: phys.light.SurfaceReflectStep(1.0, albedo=0.0)}

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

        def absorb_path(self, *a):
            self.calls.append(a)
            return 70, 6, np.array([[1, 2, 0], [0, 0, 3]])

    class Sim:
        t, seed, launch_note, _dev, _scattered, chunks = 0.5, 99, None, Dev(), False, []

        def _k_wanted(self):
            return 32

        def _dt_code(self):
            return DT

        def _py_semantics(self):
            return True                                                # not refused: the step needs no dv rule

        def _global(self, values):
            self.chunks.append(len(values))
            return np.asarray(values, dtype=np.int64) * 2               # two ranks with the same tallies
    sim = Sim()
    k = np.array([[0.0, 0.5, 40.0], [1.0, 2.0, 0.25]])
    step = phys.light.PathAbsorptionStep(k, EDGES, CENTER, E_EDGES)
    step._device_run(sim)
    step._device_run(sim)
    assert "PathAbsorptionStep" in sim.launch_note and "one launch per light step" in sim.launch_note and sim._scattered
    assert (step.exposed, step.absorbed) == (140, 12) and step.absorbed_by_cell.tolist() == [[2, 4, 0], [0, 0, 6]]
    assert len(step.data) == 2 and list(step.data[1][:3]) == [0.5, 140, 12] and step.data[1][3].tolist() == [[2, 4, 0], [0, 0, 6]]
    assert sim.chunks == [1 + 2 + 6] * 2                                # one collective per pass
    a, b = Dev.calls
    assert same_bits(a[0], light._path_probability(k, light._c_h_literals()[0], DT)) and a[1].tolist() == EDGES.tolist()
    assert a[2].tolist() == CENTER.tolist() and a[3].tolist() == E_EDGES.tolist() and (a[4], a[5], b[5]) == (99, 1, 2)


def test_multi_device_sums_the_shards_tallies():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def absorb_path(self, *a, **kw):
            return 10 * self.k, self.k, np.array([[self.k, 0, 2 * self.k]])
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    exposed, gone, cells = md.absorb_path(None)
    md._pool.shutdown()
    assert (exposed, gone, cells.tolist()) == (1110, 111, [[111, 0, 222]])


# ------------------------------------------------------------------------------------------------ the library
ENTRIES = ("pcl_step_absorb_path", "pcl_group_step_absorb_path")


def test_header_declares_both_entry_points_and_the_limits():
    text = open(os.path.join(ROOT, "include", "physicl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and len(_hip._PROTOTYPES[entry]) == 11
    for name, value in (("PCL_PATH_ABSORB_MAX_LAYERS", _hip.PATH_ABSORB_MAX_LAYERS), ("PCL_PATH_ABSORB_MAX_BANDS", _hip.PATH_ABSORB_MAX_BANDS),
                        ("PCL_PATH_ABSORB_MAX_CELLS", _hip.PATH_ABSORB_MAX_CELLS)):
        assert re.findall(r"#define\s+%s\s+(\d+)\b" % name, code) == [str(value)], name
    assert (_hip.PATH_ABSORB_MAX_LAYERS, _hip.PATH_ABSORB_MAX_BANDS, _hip.PATH_ABSORB_MAX_CELLS) == (64, 1024, 4096)
    # the largest call's tables and cells fit below 64 KiB of LDS
    assert (4096 + 65 + 1025) * 8 + (2 + 4096) * 4 < 64 * 1024
    assert "(id_lo, id_hi, pass, 17)" in text and "17 is used by nothing else" in " ".join(text.split()).replace("* ", "")
    assert hasattr(_hip.Device, "absorb_path") and hasattr(_hip.DeviceGroup, "absorb_path")


def test_the_counter_word_is_a_named_constant_used_nowhere_else():
    (unit,) = [u for u in build.ADDONS if any(s["entries"] == ENTRIES for s in u["sweeps"])]     # the unit that holds this sweep
    src = open(unit["src"]).read()
    assert re.findall(r"\b(kPathAbsorbWord) = (\d+)", src) == [("kPathAbsorbWord", "17")]
    assert len(re.findall(r"pcl_philox4x32_10\([^;]*?, kPathAbsorbWord, ", src)) == 1
    named = {}
    literal = []
    for f in sorted(os.listdir(build.CSRC)):
        if f.endswith((".hip", ".h")):
            text = open(os.path.join(build.CSRC, f)).read()
            literal += re.findall(r"pcl_philox4x32_10\(.*?, (\d+)u, ", text)
            named.update({name: int(w) for name, w in re.findall(r"\b(k\w+Word) = (\d+)", text)})
    assert sorted({int(w) for w in literal}) == [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12]           # what tests/test_absorb_cpu.py pins
    assert [name for name, w in named.items() if w == 17] == ["kPathAbsorbWord"] and len(set(named.values())) == len(named)
    assert sorted(named.values()) == [13, 14, 15, 16, 17]


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context, which is refused as well); the outputs stay as they
    were."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in [{}] + BAD_CALLS:
        keep, args, (counts, cells) = abi_args(**kw)
        assert lib.pcl_step_absorb_path(None, *args) == -2, kw
        assert lib.pcl_group_step_absorb_path(None, *args) != 0, kw
        assert (counts is None or (counts == -7).all()) and (cells is None or (cells == -7).all()), kw
