"""CPU: RecycleStep (light.RecycleStep, light._recycle_spent, pcl_step_recycle_spent) -- the constructor, the numpy restatement's
rule and distributions, the host-resident path, the header and the bindings and the refusals that need no device."""
import os
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import _hip, build, light, tally
from recycle_reference import BAD_CALLS, C, CDF, CENTER, GRID, ID_BASE, SEED, TOP, abi_args, expected_masks, layout, source
from source_reference import check_cone, check_disc, check_gaussian, check_isotropic, check_lambertian
from writer_reference import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 20000


def recycle(state, src, top=TOP, at_rest=True, spectrum=None, photon=None, ids=None, n_pass=1, dtype=np.float64, seed=SEED):
    n = len(state["E"])
    photon = np.ones(n, dtype=bool) if photon is None else photon
    ids = np.arange(n) + ID_BASE if ids is None else ids
    return light._recycle_spent(state["r"], state["v"], state["E"], photon, ids, src, top, CENTER, at_rest, spectrum, C, seed, n_pass, dtype)


# ------------------------------------------------------------------------------------------------ the constructor
@pytest.mark.parametrize("kw, word", [
    (dict(source=None), "source"), (dict(source="isotropic"), "source"), (dict(top=0.0), "top"), (dict(top=-1.0), "top"),
    (dict(top=np.nan), "top"), (dict(top=np.inf), "top"), (dict(top=1e200), "top"), (dict(top="high"), "top"),
    (dict(center=(0, 0)), "center"), (dict(center=(0, np.nan, 0)), "center"), (dict(at_rest=False), "at_rest"),
    (dict(spectrum=5), "spectrum"), (dict(spectrum=([1.0, 2.0], [0.5, 1.0, 1.0])), "spectrum"), (dict(spectrum=([], [])), "spectrum"),
    (dict(spectrum=(np.ones(1025), np.linspace(0, 1, 1025))), "spectrum"), (dict(spectrum=([1.0, 2.0], [0.5, 0.9])), "cdf"),
    (dict(spectrum=([1.0, 2.0], [0.7, 0.5])), "cdf"), (dict(spectrum=([1.0, 2.0], [np.nan, 1.0])), "cdf"),
    (dict(spectrum=([1.0, np.inf], [0.5, 1.0])), "grid"), (dict(spectrum=(["a", "b"], [0.5, 1.0])), "spectrum"),
    (dict(spectrum=phys.light.generate_photons_bulk(10, min=1.0, max=2.0)), "spectrum"),
])
def test_constructor_refusals_name_the_argument(kw, word):
    args = dict(source=source())
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        phys.light.RecycleStep(**args)


def test_constructor_keeps_what_it_was_given():
    src = source()
    step = phys.light.RecycleStep(src, top=TOP, center=CENTER, spectrum=(GRID, CDF))
    assert step.source is src and step.top == TOP and step.center.tolist() == CENTER.tolist() and step.rest_on is True
    assert step.spectrum[0].tolist() == GRID.tolist() and step.spectrum[1].tolist() == CDF.tolist()
    assert (step.at_rest, step.escaped, step.recycled, step._pass, step.data) == (0, 0, 0, 0, [])
    assert phys.light.RecycleStep(src).top is None and phys.light.RecycleStep(src, top=2.0, at_rest=False).rest_on is False
    batch = phys.light.generate_photons_bulk(10, min=1e-19, max=5e-19, T=5800.0, bins=200)
    cdf, grid = batch.table
    taken = phys.light.RecycleStep(src, spectrum=batch).spectrum      # a batch keeps (cdf, grid): the order is swapped
    assert same_bits(taken[0], np.asarray(grid, dtype=np.float64)) and same_bits(taken[1], np.asarray(cdf, dtype=np.float64))
    big = phys.light.RecycleStep(src, spectrum=(np.ones(1024), np.linspace(0, 1, 1024)))       # the limit itself
    assert len(big.spectrum[1]) == 1024 == _hip.RECYCLE_MAX_BINS
    import phys.light as short
    assert short.RecycleStep is light.RecycleStep is phys.light.RecycleStep
    assert "keeps its colour" in light.RecycleStep.__doc__ and "monochromatic" in light.RecycleStep.__doc__


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_rule_s_edge_cases(dtype):
    n = 3000
    state = layout(n, dtype)
    i = np.arange(n)
    photon = i % 17 != 0
    for at_rest, top in ((True, TOP), (True, None), (False, TOP)):
        ref = recycle(state, source(), top=top, at_rest=at_rest, photon=photon, dtype=dtype)
        rest, gone = expected_masks(n, at_rest, top is not None, photon)
        assert np.array_equal(ref["at_rest"], rest) and np.array_equal(ref["escaped"], gone), (at_rest, top)
        assert np.array_equal(ref["spent"], rest | gone) and rest.sum() + gone.sum() == ref["spent"].sum()
        assert (rest.sum() > 0) == at_rest and (gone.sum() > 0) == (top is not None)
        spent = ref["spent"]
        for f in ("r", "v"):                                           # who is not spent keeps every bit
            assert same_bits(ref[f][~spent], state[f][~spent]), f
        assert same_bits(ref["E"], state["E"])                         # no spectrum: every slot keeps its colour
        assert np.isnan(ref["dr"][~spent]).all() and same_bits(ref["dr"][spent], np.zeros((spent.sum(), 3)))
        assert same_bits(ref["dv"][spent], np.zeros((spent.sum(), 3)))
        assert np.isfinite(ref["r"][spent]).all() and np.isfinite(ref["v"][spent]).all()
    # -0.0 is at rest, a NaN in v is not; on the sphere and a NaN in r are not gone, inf is
    ref = recycle(state, source())
    assert ref["at_rest"][6] and not ref["at_rest"][39] and not ref["escaped"][39]          # 39 = 3 * 13: a NaN in v, inside
    assert ref["escaped"][5] and not ref["escaped"][7] and not ref["escaped"][35] and not ref["escaped"][55]
    far = dict(state, r=state["r"].copy())
    far["r"][1] = [np.inf, 0.0, 0.0]
    far["r"][2] = [1e200, 0.0, 0.0]                                    # q overflows to inf
    got = recycle(far, source())
    assert got["escaped"][1] and got["escaped"][2] and not ref["escaped"][1] and not ref["escaped"][2]
    # behind the step nobody is spent: the source lies inside the top
    again = recycle(dict(state, r=ref["r"], v=ref["v"]), source(), photon=np.ones(n, dtype=bool), n_pass=2)
    left = np.flatnonzero(again["spent"])
    assert not ref["spent"][left].any() and not again["spent"][ref["spent"]].any()


def test_a_beam_and_a_point_are_exact_and_written():
    state = layout(500)
    src = source("beam", "point")
    ref = recycle(state, src)
    spent = ref["spent"]
    assert same_bits(ref["v"][spent], np.tile(C * src.d, (spent.sum(), 1))) and same_bits(ref["r"][spent], np.tile(src.origin, (spent.sum(), 1)))
    low = recycle(layout(500, np.float32), src, dtype=np.float32)
    assert same_bits(low["v"][low["spent"]][0], (C * src.d).astype(np.float32).astype(np.float64))


def test_the_draws_follow_the_id_the_pass_and_the_seed():
    state = layout(600)
    src = source()
    one = recycle(state, src, n_pass=1)
    spent = one["spent"]
    for other in (recycle(state, src, n_pass=2), recycle(state, src, seed=SEED + 1), recycle(state, src, ids=np.arange(600) + ID_BASE + 1)):
        assert np.array_equal(other["spent"], spent)
        assert not (other["v"][spent] == one["v"][spent]).all(axis=1).any()
        assert not (other["r"][spent] == one["r"][spent]).all(axis=1).any()
    perm = np.random.RandomState(3).permutation(600)
    moved = recycle({k: a[perm] for k, a in state.items()}, src, ids=(np.arange(600) + ID_BASE)[perm])
    assert same_bits(moved["v"], one["v"][perm]) and same_bits(moved["r"], one["r"][perm])  # a photon is its id, wherever it stands
    # the blocks are the ones the header names: words 14 and 15 of (id, pass)
    k = int(np.flatnonzero(spent)[0])
    u_a, u_b = light._philox_block([ID_BASE + k], SEED, 1, 14)
    mu = 1.0 - 2.0 * u_a
    s = np.sqrt((1.0 - mu) * (1.0 + mu))
    psi = (u_b * 2.0) * np.pi
    want = C * (((s * np.cos(psi)) * src.e1 + (s * np.sin(psi)) * src.e2) + mu * src.d)
    assert same_bits(one["v"][k], want.reshape(3))
    u_c, u_d = light._philox_block([ID_BASE + k], SEED, 1, 15)
    rho, phi = src.radius * np.sqrt(u_c), (u_d * 2.0) * np.pi
    assert same_bits(one["r"][k], (src.origin + ((rho * np.cos(phi)) * src.e1 + (rho * np.sin(phi)) * src.e2)).reshape(3))


def everybody_at_rest(n):
    return {"r": np.tile(CENTER, (n, 1)), "v": np.zeros((n, 3)), "E": np.ones(n)}


def test_recycled_directions_and_positions_are_the_source_s():
    state = everybody_at_rest(N)
    iso = recycle(state, source("isotropic", "disc"))
    assert iso["spent"].all()
    check_isotropic(iso["v"] / C)
    src = source("isotropic", "disc")
    off = iso["r"] - src.origin
    check_disc(np.sqrt((off * off).sum(axis=1)), src.radius, slack=1e-15)
    assert np.max(np.abs(off @ src.d)) <= 1e-15                        # in the plane through the origin perpendicular to d
    assert np.max(np.abs(np.sqrt(((iso["v"] / C) ** 2).sum(axis=1)) - 1.0)) <= 1e-15
    src = source("cone", "gaussian")
    cone = recycle(state, src)
    check_cone((cone["v"] / C) @ src.d, src.half_angle, slack=1e-15)
    off = cone["r"] - src.origin
    check_gaussian(np.sqrt((off * off).sum(axis=1)), src.radius)
    src = source("lambertian", "point", oblique=False)
    lam = recycle(state, src)
    check_lambertian((lam["v"] / C) @ src.d)
    assert same_bits(lam["r"], np.tile(src.origin, (N, 1)))


def test_table_energies_are_members_of_the_grid_with_the_cdf_s_frequencies():
    ref = recycle(everybody_at_rest(N), source(), spectrum=(GRID, CDF))
    E = ref["E"]
    assert np.isin(E, GRID).all()
    p = np.diff(np.concatenate([[0.0], CDF]))
    got = np.array([(E == g).sum() for g in GRID])
    assert got[1] == 0                                                 # a bin without mass is never drawn
    assert np.all(np.abs(got - N * p) <= 5.0 * np.sqrt(N * p * (1.0 - p))), (got, N * p)
    u = light._philox_block(np.arange(N) + ID_BASE, SEED, 1, 16)[0]
    first = np.array([int(np.flatnonzero(CDF >= x)[0]) for x in u[:500]])                  # the first x with cdf[x] >= u, by hand
    assert same_bits(E[:500], GRID[first])
    low = recycle(everybody_at_rest(100), source(), spectrum=(GRID * 1.1, CDF), dtype=np.float32)
    assert same_bits(low["E"], low["E"].astype(np.float32).astype(np.float64))             # rounded once to the store's dtype
    kept = recycle(layout(700), source(), spectrum=(GRID, CDF))
    assert same_bits(kept["E"][~kept["spent"]], layout(700)["E"][~kept["spent"]])


# ------------------------------------------------------------------------------------------------ the step on the host
class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed = 0.25, SEED

    def __init__(self, objs, py=False):
        self.objects, self.py = objs, py

    def _py_semantics(self):
        return self.py


def objects(n):
    state = layout(n)
    out = []
    for k in range(n):
        o = phys.light.PhotonObject(E=phys.Measurement(np.double(1e-19), "J**1"), v=phys.light.c * [1, 0, 0]) if k % 4 else phys.Object()
        o.r = phys.Measurement(np.array(np.nan_to_num(state["r"][k], nan=1.0)), "m**1")
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
    src = source("cone", "gaussian")
    step = phys.light.RecycleStep(src, top=TOP, center=CENTER, spectrum=(GRID, CDF), out_fn=str(tmp_path / "recycle.csv"))
    step.run(sim)
    c_code = light._c_h_literals()[0]
    ref = light._recycle_spent(r0, v0, E0, photon, np.arange(n), src, TOP, CENTER, True, (GRID, CDF), c_code, SEED, 1)
    spent = ref["spent"]
    assert step.at_rest == int(ref["at_rest"].sum()) > 0 and step.escaped == int(ref["escaped"].sum()) > 0
    assert step.recycled == step.at_rest + step.escaped == int(spent.sum()) and not spent[~photon].any()
    assert len(step.data) == 1 and list(step.data[0]) == [0.25, step.at_rest, step.escaped] and sim.launch_note is None
    r1, v1, dr1, dv1 = (tally.vec3(objs, f) for f in ("r", "v", "dr", "dv"))
    E1 = tally.photon_energies(objs, phys.light.PhotonObject)[0]
    assert same_bits(r1, ref["r"]) and same_bits(v1, ref["v"])
    assert same_bits(dr1[spent], np.zeros((spent.sum(), 3))) and same_bits(dv1[spent], np.zeros((spent.sum(), 3)))
    assert same_bits(dr1[~spent], dr0[~spent]) and same_bits(dv1[~spent], dv0[~spent])
    assert same_bits(E1[photon], ref["E"][photon]) and np.isin(E1[spent], GRID).all() and same_bits(E1[~spent & photon], E0[~spent & photon])
    for k, obj in enumerate(objs):
        assert type(obj) is (phys.light.PhotonObject if photon[k] else phys.Object)
    step.run(sim)
    assert step._pass == 2 and len(step.data) == 2 and step.recycled == 0         # behind the step nobody is spent
    step.terminate(sim)
    lines = open(str(tmp_path / "recycle.csv")).read().splitlines()
    assert len(lines) == 2 and lines[0].replace(" ", "") == "0.25,%d,%d" % (step.data[0][1], step.data[0][2])


def test_the_step_is_a_plan_item_of_its_own():
    step = phys.light.RecycleStep(source(), top=TOP)

    class Sim:                                                         # what _build_plan / _multi_eligible ask of a simulation
        fuse, _hip = True, _hip
        steps = {0: phys.UpdateTimeStep(lambda s: np.double(1e-3)), 1: phys.newton.NewtonianKinematicsStep(),
                 2: phys.light.ScatterIsotropicStep(A=1.0, n=1.0), 3: phys.light.SurfaceReflectStep(1.0, albedo=0.0), 4: step}

        def _py_semantics(self):
            return False
    sim = Sim()
    plan = phys.Simulation._build_plan(sim)
    assert [kind for kind, _ in plan] == ["single", "fused", "single", "single"] and plan[3][1] is step
    sim._plan = plan
    assert not phys.Simulation._multi_eligible(sim)


def test_device_run_notes_the_launch_schedule_and_reduces_the_row():
    class Dev:
        count, calls = 1000, []

        def recycle_spent(self, *a):
            self.calls.append(a)
            return 70, 60

    class Sim:
        t, seed, launch_note, _dev, _scattered, chunks = 0.5, 99, None, Dev(), False, []

        def _k_wanted(self):
            return 32

        def _py_semantics(self):
            return True                                                # not refused: the step needs no dv rule

        def _global(self, values):
            self.chunks.append(len(values))
            return np.asarray(values, dtype=np.int64) * 2               # two ranks with the same tallies
    sim = Sim()
    src = source()
    step = phys.light.RecycleStep(src, top=TOP, center=CENTER, spectrum=(GRID, CDF))
    step._device_run(sim)
    step._device_run(sim)
    assert "RecycleStep" in sim.launch_note and "one launch per light step" in sim.launch_note and sim._scattered
    assert (step.at_rest, step.escaped, step.recycled) == (140, 120, 260)
    assert len(step.data) == 2 and list(step.data[1]) == [0.5, 140, 120]
    assert sim.chunks == [1 + 2] * 2                                    # one collective per pass
    a, b = Dev.calls
    assert a[0] is src and a[1] == light._c_h_literals()[0] and a[2] is True and a[3] == TOP and a[4].tolist() == CENTER.tolist()
    assert a[5][0].tolist() == GRID.tolist() and a[5][1].tolist() == CDF.tolist()
    assert (a[6], a[7], b[7]) == (99, 1, 2)                             # the step's own pass counter


def test_multi_device_sums_the_shards_counts():
    from concurrent.futures import ThreadPoolExecutor
    from physicl_amd.multidev import MultiDevice

    class Shard:
        def __init__(self, k):
            self.k = k

        def recycle_spent(self, *a, **kw):
            return 10 * self.k, self.k
    md = MultiDevice.__new__(MultiDevice)
    md.shards, md._pool = [Shard(1), Shard(10), Shard(100)], ThreadPoolExecutor(max_workers=3)
    assert md.recycle_spent(None, None) == (1110, 111)
    md._pool.shutdown()


# ------------------------------------------------------------------------------------------------ the library
ENTRIES = ("pcl_step_recycle_spent", "pcl_group_step_recycle_spent")


def test_header_declares_both_entry_points_and_the_binding_knows_them():
    text = open(os.path.join(ROOT, "include", "physicl_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for entry in ENTRIES:
        assert re.search(r"\b%s\s*\(" % entry, code) and entry in _hip.EXPORTS and len(_hip._PROTOTYPES[entry]) == 12
    assert re.findall(r"#define\s+PCL_RECYCLE_MAX_BINS\s+(\d+)\b", code) == ["1024"]
    for word in (14, 15, 16):
        assert "(id_lo, id_hi, pass, %d)" % word in text                # the arithmetic is written out, the counter words with it
    assert "words 14, 15 and 16 are used by nothing else" in text
    assert hasattr(_hip.Device, "recycle_spent") and hasattr(_hip.DeviceGroup, "recycle_spent")


def test_the_new_counter_words_are_named_constants():
    (unit,) = [u for u in build.ADDONS if any(s["entries"] == ENTRIES for s in u["sweeps"])]     # the unit that holds this sweep
    src = open(unit["src"]).read()
    names = dict(re.findall(r"\b(kRecycle\w+Word) = (\d+)", src))
    assert names == {"kRecycleDirWord": "14", "kRecyclePosWord": "15", "kRecycleEnergyWord": "16"}
    for name in names:
        assert len(re.findall(r"pcl_philox4x32_10\([^;]*?, %s, " % name, src)) == 1, name
    used = []
    for f in sorted(os.listdir(build.CSRC)):
        if f.endswith((".hip", ".h")):
            used += re.findall(r"pcl_philox4x32_10\(.*?, (\d+)u, ", open(os.path.join(build.CSRC, f)).read())
    assert sorted({int(w) for w in used}) == [0, 1, 2, 3, 4, 5, 8, 9, 10, 11, 12]             # what tests/test_absorb_cpu.py pins
    assert light._RECYCLE_WORDS == (14, 15, 16)


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context, which is refused as well)."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in [{}] + BAD_CALLS:
        keep, args, counts = abi_args(_hip, **kw)
        assert lib.pcl_step_recycle_spent(None, *args) == -2, kw
        assert lib.pcl_group_step_recycle_spent(None, *args) != 0, kw
        assert counts is None or (counts == -7).all()
