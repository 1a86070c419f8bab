"""CPU: GridPhaseStep (physicl_amd/light_grid.py) -- the constructor's refusals, the numpy restatement of pcl_step_phase_grid against an
independent loop over Python scalars on a scene of edge cases, the two equivalences the shared Philox words give (LayeredPhaseStep on
a radius axis, PhaseFunctionStep on one cell), the mean cosine per mixture, and the step on host-resident objects."""
import bisect
import math
import re

import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import _hip, build, light, light_grid, tally
from absorb_reference import CENTER, EDGES, same_bits
from grid_phase_reference import THREE_LAWS, THREE_MIXTURES
from layered_phase_reference import C, MIX_LAWS, MIX_WEIGHTS, SEED, all_scattered, cloud, hg_table, table_moments
from test_layered_phase_cpu import HostSim, objects

GRID = dict(axes=("x", "y", "z"), edges=[[0.0, 1.0, 2.0, 4.0], [-1.0, 0.0, 1.0], [0.0, 0.5, 3.0]])       # 3 x 2 x 2
MAP = np.array([[[0, 1], [2, -1]], [[1, 2], [0, 1]], [[2, 0], [-1, 2]]])
T2 = ("table", [-1.0, 0.0, 1.0], [1.0, 2.0])


def grid_phase(r, v, dv, laws, weights, axes, edges, mixture=None, outside=None, center=(0, 0, 0), photon=None, ids=None, n_pass=1,
               dtype=np.float64):
    n = len(v)
    photon = np.ones(n, dtype=bool) if photon is None else photon
    ids = np.arange(n) + 7_000_000_001 if ids is None else ids
    return light_grid._grid_phase_redirect(r, v, dv, photon, ids, laws, weights, axes, edges, mixture, outside, center, C, SEED, n_pass, dtype)


# ------------------------------------------------------------------------------------------------ refusals
ONE = dict(laws=["rayleigh"], weights=None, axes=("x",), edges=[[0.0, 1.0, 2.0]])
MIX = dict(laws=MIX_LAWS, weights=MIX_WEIGHTS, axes=("x",), edges=[[0.0, 1.0, 2.0]], mixture=[0, 2])


@pytest.mark.parametrize("kw, word", [
    (dict(ONE, laws=[]), "laws"), (dict(ONE, laws=["isotropic"] * 9, weights=[1] * 9), "laws"), (dict(ONE, laws="rayleigh"), "laws"),
    (dict(ONE, laws=["mie"]), "laws"), (dict(ONE, laws=[("hg", 1.0)]), "g"), (dict(ONE, laws=[("hg", np.nan)]), "g"),
    (dict(ONE, laws=[("table", [-0.5, 0.0, 1.0], [1.0, 2.0])]), "mu_edges"), (dict(ONE, laws=[("table", [-1.0, 0.0, 1.0], [1.0, 0.0])]), "p"),
    (dict(ONE, laws=[("table", np.linspace(-1, 1, 1026), np.ones(1025))]), "1024"),
    (dict(ONE, laws=[("table", np.linspace(-1, 1, 1025), np.ones(1024))] * 2 + [T2], weights=[1, 1, 1]), "2048"),
    (dict(MIX, weights=None), "weights"), (dict(MIX, weights=[1, 2, 3]), "weights"), (dict(MIX, weights=[[1, 2, 3]] * 3), "weights"),
    (dict(MIX, weights=[[1, -1]] * 3), "weights"), (dict(MIX, weights=[[1, 0], [0, 0], [0, 1]]), "weights"), (dict(MIX, weights=[[1, np.nan]] * 3), "weights"),
    (dict(MIX, weights="ab"), "weights"), (dict(MIX, weights=[[1, 1]] * 65), "weights"), (dict(MIX, weights=np.ones((2, 2, 2))), "weights"),
    (dict(MIX, axes=("x", "x"), edges=[[0, 1]] * 2), "axes"), (dict(MIX, axes=("w",)), "axes"), (dict(MIX, axes=()), "axes"),
    (dict(MIX, axes=("x", "y")), "edges"), (dict(MIX, edges=[[0.0, 2.0, 1.0]]), "axis 'x'"), (dict(MIX, edges=[np.arange(1026.0)]), "axis 'x'"),
    (dict(MIX, axes=("r",), edges=[[-1.0, 1.0, 2.0]]), "axis 'r'"),
    (dict(MIX, axes=("x", "y", "z"), edges=[np.arange(1025.0), np.arange(1025.0), [0.0, 1.0, 2.0]], mixture=None), "cells"),
    (dict(MIX, center=(0, 0)), "center"), (dict(MIX, center=(0, np.nan, 0)), "center"),
    (dict(MIX, mixture=None), "mixture"), (dict(MIX, mixture=[0.0, 1.0]), "mixture"), (dict(MIX, mixture=[0, 3]), "mixture"),
    (dict(MIX, mixture=[-2, 0]), "mixture"), (dict(MIX, mixture=[0, 1, 2]), "mixture"), (dict(MIX, mixture=[[0, 1]]), "mixture"),
    (dict(MIX, mixture=[True, False]), "mixture"), (dict(MIX, mixture="ab"), "mixture"),
    (dict(MIX, outside=3), "outside"), (dict(MIX, outside=-1), "outside"), (dict(MIX, outside=1.0), "outside"), (dict(MIX, outside=True), "outside"),
    (dict(ONE, outside=1), "outside")])
def test_constructor_refusals_name_the_argument(kw, word):
    with pytest.raises(ValueError, match=r"%s(?!\w)" % re.escape(word)) as e:
        phys.light.GridPhaseStep(**kw)
    assert re.search(r"\b(laws|weights|axes|edges|axis|center|mixture|outside|grid)\b", str(e.value))
    if word in ("1024", "2048"):
        assert "laws" in str(e.value)
    if np.shape(kw.get("weights")) == (65, 2):
        assert "64" in str(e.value)


def test_tables_and_edges_beyond_the_workgroup_s_memory_are_refused_with_both_sizes():
    table = ("table", np.linspace(-1, 1, 1025), np.ones(1024))
    big = dict(laws=[table, table], weights=[1, 1], axes=("x", "y"), edges=[np.arange(1025.0), np.arange(1025.0)])
    with pytest.raises(ValueError, match="laws") as e:
        phys.light.GridPhaseStep(**big)
    need = _hip.phase_grid_lds_bytes(1, 2, 2050, 2050)
    assert need == 8 * (2 + 2050 + 2 + 3 * 2050 + 3) + 4 * 5 > _hip.PHASE_GRID_LDS_BYTES == 65536
    for number in (2050, 24 * 2050, 8 * 2050, need, 65536):              # the tables' nodes and bytes, the edges' (2050 as well), the sum, the bound
        assert re.search(r"\b%d\b" % number, str(e.value)), number
    assert "edges" in str(e.value)
    phys.light.GridPhaseStep(**dict(big, laws=[table, "rayleigh"]))      # either fits with a small other
    phys.light.GridPhaseStep(**dict(big, edges=[np.arange(3.0), np.arange(3.0)]))


def test_constructor_keeps_what_it_was_given():
    d = phys.light.GridPhaseStep(["rayleigh"], None, ("x",), [[0.0, 1.0]])
    assert (d.laws, d.outside, d.out_fn, d.scattered, d.redirected, d.data, d._pass) == (["rayleigh"], None, None, 0, 0, [], 0)
    assert d.weights.tolist() == [[1.0]] and d.cum.tolist() == [[1.0]] and d.center.tolist() == [0, 0, 0] and d.mixture.tolist() == [0]
    assert d.by_mixture.tolist() == [0] and d.by_law.tolist() == [0] and d._fuse_role is None and d._device_native
    s = phys.light.GridPhaseStep(MIX_LAWS, MIX_WEIGHTS, "xyz", GRID["edges"], mixture=MAP, outside=np.int64(1), center=CENTER, out_fn="x.csv")
    assert s.laws == ["rayleigh", ("hg", 0.85)] and s.weights.tolist() == MIX_WEIGHTS and s.cum.tolist() == [[1, 1], [0.3, 1], [0, 1]]
    assert s.axes == ("x", "y", "z") and s.mixture.shape == (3, 2, 2) and s.mixture.dtype == np.int64 and s.outside == 1 and type(s.outside) is int
    assert s.by_mixture.shape == (3,) and s.by_law.shape == (2,) and s.center.tolist() == CENTER.tolist()
    t = phys.light.GridPhaseStep([T2, ("hg", 0)], [2, 6], ("r",), [[0.0, 1.0, 2.0]])           # [M] is one mixture; no map: row 0 everywhere
    assert t.weights.tolist() == [[2, 6]] and t.cum.tolist() == [[0.25, 1.0]] and t.mixture.tolist() == [0, 0]
    big = phys.light.GridPhaseStep(["isotropic"] * 8, np.ones((64, 8)), ("x", "y"), [np.arange(1025.0)] * 2, np.zeros((1024, 1024), dtype=np.uint8))
    assert big.cum.shape == (64, 8) and big.mixture.shape == (1024, 1024)                       # the limits themselves
    import phys.light as short
    assert short.GridPhaseStep is light.GridPhaseStep is light_grid.GridPhaseStep is phys.light.GridPhaseStep
    assert issubclass(light_grid.GridPhaseStep, light.LayeredPhaseStep) and tally.writer_family(d) == "phase"
    assert "GridPhaseStep" in light_grid.GridPhaseStep._NOTE and "_STREAM" not in vars(light_grid.GridPhaseStep)
    assert (_hip.PHASE_GRID_MAX_MIXTURES, _hip.PHASE_GRID_MAX_CELLS, _hip.PHASE_GRID_ALONE, _hip.PHASE_GRID_LDS_BYTES) == (64, 1 << 20, 255, 65536)
    text = open(build.ABI_HEADER).read()
    for name, value in (("MAX_MIXTURES", "64"), ("MAX_CELLS", r"\(1 << 20\)"), ("ALONE", "255"), ("LDS_BYTES", "65536")):
        assert re.search(r"#define PCL_PHASE_GRID_%s %s(?!\w)" % (name, value), text), name


# ------------------------------------------------------------------------------------------------ the restatement, against a loop
def edge_scene():
    """Photons exactly on the first, an inner and the last edge of each axis of the 3 x 2 x 2 grid, just outside either end, inside every
    cell, with a NaN in each coordinate; every row scattered but: plain Objects (index % 11 == 5), rows that did not scatter (% 13 ==
    7) and rows whose old velocity has o.o == 0 (% 17 == 3: v == dv) or inf (% 19 == 4: a component of 1e200)."""
    ex, ey, ez = (np.array(e) for e in GRID["edges"])
    xs = [ex[0], ex[1], ex[-1], np.nextafter(ex[0], -np.inf), np.nextafter(ex[-1], np.inf), 0.5, 1.5, 3.0, np.nan]
    ys = [ey[0], ey[1], ey[-1], np.nextafter(ey[0], -np.inf), np.nextafter(ey[-1], np.inf), -0.5, 0.5, np.nan]
    zs = [ez[0], ez[1], ez[-1], np.nextafter(ez[0], -np.inf), np.nextafter(ez[-1], np.inf), 0.25, 2.0, np.nan]
    r = np.array([[x, y, z] for x in xs for y in ys for z in zs])
    n = len(r)
    v, dv, ids = all_scattered(n, seed=3)
    i = np.arange(n)
    photon = i % 11 != 5
    dv[i % 13 == 7] = 0.0
    dv[i % 17 == 3] = v[i % 17 == 3]
    v[i % 19 == 4, 1] = 1e200
    return r, v, dv, photon, ids


def loop(r, v, dv, photon, ids, laws, weights, axes, edges, mixture, outside, center, n_pass):
    """Per particle, on Python scalars: (re-directed with which mixture or None, which law), and the two scalar counts."""
    col = {"x": 0, "y": 1, "z": 2}
    cum = [np.cumsum(row) / np.sum(row) for row in np.asarray(weights, dtype=np.float64)]
    out, scattered = [], 0
    for k in range(len(r)):
        o = [float(v[k][a]) - float(dv[k][a]) for a in range(3)]
        oo = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
        if not (photon[k] and any(float(x) != 0.0 for x in dv[k]) and 0.0 < oo < math.inf):
            out.append((None, None))
            continue
        scattered += 1
        cell, inside = 0, True
        for a, e in zip(axes, edges):
            e = [float(x) for x in e]
            if a == "r":
                d = [float(r[k][j]) - float(center[j]) for j in range(3)]
                q, e = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], [x * x for x in e]
            else:
                q = float(r[k][col[a]])
            if not (e[0] <= q <= e[-1]):                                # a NaN compares false
                inside = False
                break
            cell = cell * (len(e) - 1) + min(bisect.bisect_right(e, q) - 1, len(e) - 2)
        m = int(np.asarray(mixture).reshape(-1)[cell]) if inside else (-1 if outside is None else outside)
        if m < 0:
            out.append((None, None))
            continue
        u_s = float(light._philox_block(np.array([ids[k]]), SEED, n_pass, 13)[0][0])
        law = next(j for j in range(len(laws)) if u_s < cum[m][j] or j == len(laws) - 1)
        out.append((m, law))
    return out, scattered


@pytest.mark.parametrize("outside", [None, 1])
def test_the_restatement_finds_cell_mixture_and_law_as_a_loop_over_scalars_does(outside):
    r, v, dv, photon, ids = edge_scene()
    got = grid_phase(r, v, dv, THREE_LAWS, THREE_MIXTURES, GRID["axes"], GRID["edges"], MAP, outside, photon=photon, ids=ids, n_pass=5)
    want, scattered = loop(r, v, dv, photon, ids, THREE_LAWS, THREE_MIXTURES, GRID["axes"], GRID["edges"], MAP, outside, (0, 0, 0), 5)
    assert got["mixture"].tolist() == [-1 if m is None else m for m, _ in want]
    assert got["law"].tolist() == [-1 if j is None else j for _, j in want]
    assert got["scattered"].sum() == scattered and got["redirected"].tolist() == [m is not None for m, _ in want]
    assert got["by_mixture"].tolist() == [sum(m == b for m, _ in want) for b in range(3)] and got["by_mixture"].min() > 0
    assert got["by_law"].tolist() == [sum(j == b for _, j in want) for b in range(3)] and got["by_law"].min() > 0
    go = got["redirected"]
    assert 0 < go.sum() < scattered < photon.sum() and same_bits(got["v"][~go], v[~go]) and same_bits(got["dv"][~go], dv[~go])
    i = np.arange(len(r))
    assert not got["scattered"][(i % 11 == 5) | (i % 13 == 7) | (i % 17 == 3) | (i % 19 == 4)].any()
    nan = np.isnan(r).any(axis=1) & got["scattered"]
    assert nan.sum() > 10 and go[nan].all() == (outside is not None) and (got["mixture"][nan] == (-1 if outside is None else outside)).all()
    # on an edge: the first edge is inside, an inner edge belongs to the upper bin, the last edge to the last bin; just outside is outside
    cells = {tuple(p): light._cell_of_positions(np.array([p], dtype=np.float64), GRID["axes"], [np.array(e) for e in GRID["edges"]], np.zeros(3))
             for p in ([0.0, -1.0, 0.0], [1.0, 0.0, 0.5], [4.0, 1.0, 3.0], [np.nextafter(4.0, 5.0), 0.5, 1.0])}
    assert [(bool(ok[0]), int(c[0])) for ok, c in cells.values()][:3] == [(True, 0), (True, 7), (True, 11)] and not list(cells.values())[3][0][0]
    # a one-hot row and a row whose first law has no weight: law 0 alone, and never law 0
    assert (got["law"][got["mixture"] == 0] == 0).all() and (got["law"][got["mixture"] == 2] >= 1).all()
    # the turn is the layered step's: every re-directed row is the single law's row
    for j, single in enumerate(THREE_LAWS):
        alone = grid_phase(r, v, dv, [single], None, ("x",), [[-1.0, 1.0]], None, 0, photon=photon, ids=ids, n_pass=5)
        mine = got["law"] == j
        assert same_bits(got["v"][mine], alone["v"][mine]) and same_bits(got["dv"][mine], alone["dv"][mine])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_radius_axis_with_its_layers_as_mixtures_is_the_layered_step_bit_for_bit(dtype):
    n = 6000
    r, v, dv = cloud(n, seed=4, dtype=dtype)
    photon, ids = np.arange(n) % 7 != 0, np.arange(n) + 7_000_000_001
    ref = light._layered_phase_redirect(r, v, dv, photon, ids, MIX_LAWS, MIX_WEIGHTS, EDGES, CENTER, C, SEED, 2, dtype)
    got = grid_phase(r, v, dv, MIX_LAWS, MIX_WEIGHTS, ("r",), [EDGES], np.arange(3), None, CENTER, photon=photon, ids=ids, n_pass=2, dtype=dtype)
    assert set(got) == (set(ref) - {"layer", "by_layer"}) | {"mixture", "by_mixture"}
    for key in ref:
        assert same_bits(ref[key], got[{"layer": "mixture", "by_layer": "by_mixture"}.get(key, key)]), key
    assert 0 < ref["redirected"].sum() < ref["scattered"].sum() and ref["by_layer"].min() > 50


@pytest.mark.parametrize("law", ["isotropic", ("hg", 0.85), ("hg", -0.3), "rayleigh"])
def test_one_cell_one_law_and_outside_zero_is_the_phase_function_bit_for_bit(law):
    n = 3000
    r, v, dv = cloud(n, seed=5)
    photon, ids = np.arange(n) % 7 != 0, np.arange(n) + 7_000_000_001
    phase, g = (law, 0.0) if isinstance(law, str) else law
    ref = light._phase_redirect(v, dv, photon, ids, phase, g, C, SEED, 3)
    got = grid_phase(r, v, dv, [law], None, ("x", "y", "z"), [[0.0, 1.0]] * 3, None, 0, photon=photon, ids=ids, n_pass=3)
    for key in ("v", "dv", "redirected", "mu", "w"):
        assert same_bits(ref[key], got[key]), key
    assert same_bits(got["scattered"], got["redirected"]) and 0 < (got["mixture"] == 0).sum() == got["by_law"][0] == got["by_mixture"][0]


# ------------------------------------------------------------------------------------------------ the cosines
N_COS = 20000
COS_SEED = 20261021                                # chosen here, on the CPU, so that the restatement holds the 5 sigma checks below
COS_TABLE = hg_table(0.6, 32)
COS_LAWS = ("rayleigh", ("hg", 0.85), COS_TABLE, "isotropic")
COS_MIXTURES = [[1, 0, 0, 0], [0.1, 0.9, 0, 0], [0, 0.3, 0.5, 0.2]]


def law_moments(law):
    """(mean, variance) of the cosine under a law, from the law's own moments: isotropic 0 and 1/3; Rayleigh 0 and 2/5; Henyey-
    Greenstein g and (1 + 2 g^2) / 3 - g^2 (its second Legendre moment is g^2); a table's from its bins."""
    if law == "isotropic":
        return 0.0, 1.0 / 3.0
    if law == "rayleigh":
        return 0.0, 0.4
    if law[0] == "hg":
        return law[1], (1.0 + 2.0 * law[1] ** 2) / 3.0 - law[1] ** 2
    return table_moments(law[1], law[2])[1:]


def test_the_mean_cosine_of_a_mixture_is_the_weighted_mean_of_its_laws():
    n = 3 * N_COS
    v, dv, ids = all_scattered(n, seed=6)
    r = np.zeros((n, 3))
    r[:, 0] = np.arange(n) % 3 + 0.5                                    # mixture m in the cell [m, m + 1) of x
    got = light_grid._grid_phase_redirect(r, v, dv, np.ones(n, dtype=bool), ids, COS_LAWS, COS_MIXTURES, ("x",), [[0.0, 1.0, 2.0, 3.0]],
                                          [0, 1, 2], None, (0, 0, 0), C, COS_SEED, 1)
    assert got["by_mixture"].tolist() == [N_COS] * 3
    moments = [law_moments(law) for law in COS_LAWS]
    for m, row in enumerate(COS_MIXTURES):
        mu = got["mu"][got["mixture"] == m]
        mean = sum(w * mj for w, (mj, _) in zip(row, moments))
        var = sum(w * (vj + mj * mj) for w, (mj, vj) in zip(row, moments)) - mean * mean
        print("mixture %d: mean cosine %.5f, the laws' %.5f +- %.5f at 5 sigma" % (m, mu.mean(), mean, 5 * np.sqrt(var / N_COS)))
        assert len(mu) == N_COS and abs(mu.mean() - mean) <= 5 * np.sqrt(var / N_COS), m
        w = got["w"][got["mixture"] == m]
        o = (v - dv)[got["mixture"] == m]
        cosine = (got["v"][got["mixture"] == m] * o).sum(axis=1) / (C * np.sqrt((o * o).sum(axis=1)))      # of the state itself
        assert np.max(np.abs(cosine - mu)) < 1e-12 and np.max(np.abs((w * w).sum(axis=1) - 1)) < 1e-12


# ------------------------------------------------------------------------------------------------ the step on the host
HOST = dict(laws=THREE_LAWS, weights=THREE_MIXTURES, axes=("x", "y", "z"), edges=[np.linspace(CENTER[k] - 3.0, CENTER[k] + 3.0, 4) for k in range(3)],
            mixture=(np.arange(27).reshape(3, 3, 3) % 4) - 1, outside=1, center=CENTER)


def test_host_resident_objects_get_the_restatement_s_state(tmp_path):
    n = 900
    objs, v, dv = objects(n)
    photon = np.arange(n) % 5 != 0
    sim = HostSim(objs)
    r_code = tally.vec3(objs, "r")
    step = phys.light.GridPhaseStep(out_fn=str(tmp_path / "grid.csv"), **HOST)
    sim.steps = {0: step}
    step.run(sim)
    c_code = light._c_h_literals()[0]
    ref = light_grid._grid_phase_redirect(r_code, v, dv, photon, np.arange(n), HOST["laws"], HOST["weights"], HOST["axes"], HOST["edges"],
                                          HOST["mixture"], HOST["outside"], HOST["center"], c_code, SEED, 1)
    assert step.scattered == int(ref["scattered"].sum()) == int(((np.arange(n) % 3 == 0) & photon).sum())
    assert 0 < step.redirected == int(ref["redirected"].sum()) < step.scattered
    assert step.by_mixture.tolist() == ref["by_mixture"].tolist() and step.by_law.tolist() == ref["by_law"].tolist() and min(step.by_law) > 10
    row = step.data[0]
    assert len(step.data) == 1 and len(row) == 5 and list(row[:3]) == [0.25, step.scattered, step.redirected]
    assert row[3].tolist() == step.by_mixture.tolist() and row[4].tolist() == step.by_law.tolist()
    for k, obj in enumerate(sim.objects):
        assert same_bits(np.asarray(obj.v, dtype=np.float64), ref["v"][k]) and same_bits(np.asarray(obj.dv, dtype=np.float64), ref["dv"][k]), k
        assert type(obj) is (phys.light.PhotonObject if photon[k] else phys.Object)
        if not photon[k]:
            assert same_bits(np.asarray(obj.v), v[k]) and same_bits(np.asarray(obj.dv), dv[k])       # plain Objects are untouched
    assert same_bits(tally.vec3(objs, "r"), r_code) and sim.launch_note is None
    step.run(sim)
    assert step._pass == 2 and step._n_pass == 2 and len(step.data) == 2
    step.terminate(sim)
    lines = open(str(tmp_path / "grid.csv")).read().splitlines()
    assert len(lines) == 2 and lines[0].startswith("0.25, %d, %d, [" % (step.data[0][1], step.data[0][2]))


def test_python_semantics_and_a_second_phase_step_are_refused():
    objs, _, _ = objects(10)
    step = phys.light.GridPhaseStep(**HOST)
    with pytest.raises(ValueError, match="dv = v_old") as e:
        step.run(HostSim(objs, py=True))
    assert "GridPhaseStep" in str(e.value)
    with pytest.raises(ValueError, match="cl_on"):
        step._device_run(HostSim(objs, py=True))
    for other in (phys.light.PhaseFunctionStep("hg", 0.5), phys.light.LayeredPhaseStep(["isotropic"]), phys.light.GridPhaseStep(**HOST)):
        steps = {0: phys.newton.NewtonianKinematicsStep(), 1: phys.light.ScatterIsotropicStep(A=1.0, n=1.0), 2: step, 3: other}
        with pytest.raises(ValueError, match="one phase step") as e:
            step.run(HostSim(objs, steps=steps))
        assert type(other).__name__ in str(e.value) and "this GridPhaseStep" in str(e.value)
        with pytest.raises(ValueError, match="one phase step"):
            step._device_run(HostSim(objs, steps=steps))
        if isinstance(other, phys.light.LayeredPhaseStep):              # the older step's own refusal sees the new one
            with pytest.raises(ValueError, match="one phase step") as e:
                other.run(HostSim(objs, steps=steps))
            assert "GridPhaseStep" in str(e.value)
    assert step._pass == 0 and step.data == []
    step.run(HostSim(objs, steps={0: phys.light.GridScatterStep(1.0, ("x",), [[0.0, 1.0]]), 1: step}))      # a scatterer is no phase step
    assert step._pass == 1


def test_device_run_hands_the_sweep_its_arguments_and_records_the_global_row():
    """With a stand-in device: what ``phase_grid`` is handed, the launch note, the one collective and the row."""
    class Dev:
        count = 7

        def phase_grid(self, *a):
            self.args = a
            return 5, 4, np.array([1, 0, 3]), np.array([2, 1, 1])

    class Sim(HostSim):
        _residency, hits = "device", 0
        _dev = Dev()

        def _k_wanted(self):
            return 8

        def _global(self, flat):
            self.flat = list(flat)
            return [2 * x for x in flat]                                 # two ranks with the same shard
    step = phys.light.GridPhaseStep(**HOST)
    sim = Sim([], steps={0: step})
    step._device_run(sim)
    laws, cum, axes, edges, center, mixture, outside, c, seed, n_pass = sim._dev.args
    assert [law[0] for law in laws] == ["rayleigh", "hg", "isotropic"] and cum.tolist() == step.cum.tolist() and axes == ("x", "y", "z")
    assert mixture is step.mixture and outside == 1 and center.tolist() == CENTER.tolist() and (seed, n_pass) == (SEED, 1)
    assert c == light._c_h_literals()[0] and len(edges) == 3
    assert sim.flat == [7, 5, 4, 1, 0, 3, 2, 1, 1] and "GridPhaseStep" in sim.launch_note and "one launch per light step" in sim.launch_note
    assert (step.scattered, step.redirected, step.by_mixture.tolist(), step.by_law.tolist()) == (10, 8, [2, 0, 6], [4, 2, 2])
    assert step.by_mixture.dtype == np.int64 and list(step.data[0][:3]) == [0.25, 10, 8] and sim._scattered is True
