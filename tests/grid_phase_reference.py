"""Scenes for the tests of GridPhaseStep (tests/test_grid_phase_cpu.py and the test_writers_grid_phase_* GPU files), the comparison
of a sweep on two downloaded states (``check_grid``: layered_phase_reference.check_layered's conditions) and the ABI by hand.  Not
a test file: a helper they import.  The population is layered_phase_reference.cloud's -- positions up to 5.2 from absorb_reference's
CENTER, every third row scattered, a NaN position in some --; the restatement of the kernel is
physicl_amd.light_grid._grid_phase_redirect."""
import numpy as np

import writer_reference as W
from absorb_reference import CENTER, EDGES
from layered_phase_reference import C, MIX_LAWS, MIX_WEIGHTS, SEED, cloud, hg_table
from physicl_amd import light_grid

assert C == W.C and SEED == 0x5EED5A7F
BOX = [np.linspace(CENTER[k] - 3.0, CENTER[k] + 3.0, 5) for k in range(3)]      # 4 x 4 x 4 about the cloud's centre: some stand outside
THREE_LAWS = ("rayleigh", ("hg", 0.85), "isotropic")
THREE_MIXTURES = [[1, 0, 0], [0.3, 0.7, 0], [0, 0.2, 0.8]]                     # a one-hot row, a mixture, a row whose first law has no weight


def _box_map():
    ix, iy, iz = np.indices((4, 4, 4))
    return (ix + 2 * iy + 3 * iz) % 4 - 1                                       # -1 (left alone), 0, 1, 2


def _field_map():
    ix, iy, iz = np.indices((17, 16, 16))
    return (ix + iy) % 2                                                        # a checkerboard of columns, as the grid scatter's field


def scenes():
    """{name: dict(laws, weights, axes, edges, mixture, outside, center)} of the GPU tests."""
    field = [np.linspace(CENTER[0] - 4.25, CENTER[0] + 4.25, 18), np.linspace(CENTER[1] - 4.0, CENTER[1] + 4.0, 17),
             np.linspace(CENTER[2] - 4.0, CENTER[2] + 4.0, 17)]
    table = hg_table(0.85, 64)
    out = {
        "xyz": dict(laws=THREE_LAWS, weights=THREE_MIXTURES, axes=("x", "y", "z"), edges=BOX, mixture=_box_map(), outside=None),
        "xyz, outside a row": dict(laws=THREE_LAWS, weights=THREE_MIXTURES, axes=("x", "y", "z"), edges=BOX, mixture=_box_map(), outside=2),
        "r": dict(laws=MIX_LAWS, weights=MIX_WEIGHTS, axes=("r",), edges=[EDGES], mixture=np.arange(3), outside=None),
        "zr": dict(laws=MIX_LAWS, weights=MIX_WEIGHTS, axes=("z", "r"), edges=[np.linspace(CENTER[2] - 3.0, CENTER[2] + 3.0, 4), EDGES],
                   mixture=np.array([[0, 1, 2], [-1, 2, 0], [1, -1, 1]]), outside=0),
        "field 17x16x16": dict(laws=MIX_LAWS, weights=[[1, 0], [0.1, 0.9]], axes=("x", "y", "z"), edges=field, mixture=_field_map(), outside=0),
        "table": dict(laws=(table, "rayleigh"), weights=[[0.6, 0.4], [0, 1]], axes=("x",),
                      edges=[[CENTER[0] - 2.0, CENTER[0] + 0.5, CENTER[0] + 3.0]], mixture=np.array([0, 1]), outside=None),
    }
    for s in out.values():
        s["center"] = CENTER
    return out


def state_of(n, dtype, seed=1):
    """What a test uploads: the cloud, a dr and energies of no consequence, ids from W.ID_BASE (above 2^32) on."""
    r, v, dv = cloud(n, seed=seed + n, dtype=np.float32 if dtype == "f32" else np.float64)
    rng = np.random.RandomState(n)
    return {"r": r, "v": v, "dr": rng.normal(size=(n, 3)), "dv": dv, "E": 1.0 + rng.uniform(size=n), "id_base": W.ID_BASE}


def args_of(scene):
    """(laws, cum, axes, edges, center, mixture, outside) as ``Device.phase_grid`` takes them, checked."""
    laws, _, cum, axes, edges, mixture, outside, center = light_grid._check_grid_phase(
        scene["laws"], scene["weights"], scene["axes"], scene["edges"], scene["mixture"], scene["outside"], scene["center"])
    return laws, cum, axes, edges, center, mixture, outside


def call(dev, scene, n_pass, seed=SEED):
    return dev.phase_grid(*args_of(scene), C, seed, n_pass)


# ------------------------------------------------------------------------------------------------ a sweep against its restatement
def check_grid(before, after, answer, scene, c, seed, n_pass, what):
    """A state downloaded before the sweep (tests/writer_reference.py: ``snapshot``), the state downloaded after it and the sweep's
    answer ``(scattered, redirected, by_mixture, by_law)`` against light_grid._grid_phase_redirect, under check_layered's conditions:
    every tally exact; E, ids and kinds, r and dr of everybody and every row of a particle that is not re-directed bit-identical;
    re-directed rows within the bounds tests/writer_reference.py derives for the phase function's v and dv.  Returns the
    restatement's dict."""
    bw, aw = W.wide(before), W.wide(after)
    T = np.asarray(before["E"]).dtype.type
    ref = light_grid._grid_phase_redirect(bw["r"], bw["v"], bw["dv"], W.photons(before), before["id"], scene["laws"], scene["weights"],
                                          scene["axes"], scene["edges"], scene["mixture"], scene["outside"], scene["center"], c, seed,
                                          n_pass, T)
    scattered, redirected, by_mixture, by_law = answer
    by_mixture, by_law = np.asarray(by_mixture).tolist(), np.asarray(by_law).tolist()
    print("%s: scattered %d, redirected %d, by mixture %s, by law %s" % (what, scattered, redirected, by_mixture, by_law))
    assert (scattered, redirected) == (int(ref["scattered"].sum()), int(ref["redirected"].sum())), what
    assert by_mixture == ref["by_mixture"].tolist() and by_law == ref["by_law"].tolist(), what
    assert sum(by_mixture) == sum(by_law) == redirected, what
    go = ref["redirected"]
    for f in set(before) - set(W.FIELDS) - {"count"}:                  # E, ids, kinds
        assert W.same_bits(before[f], after[f]), (what, f)
    for f in W.FIELDS:                                                 # not re-directed: bit-identical; r and dr: everybody
        assert W.same_bits(aw[f][~go], bw[f][~go]), (what, f)
    assert W.same_bits(aw["r"], bw["r"]) and W.same_bits(aw["dr"], bw["dr"]), what
    v_unit, v_bound = (W.ulp(c), W.DIR_ULP) if T is np.float64 else (W.ulp(c, np.float32), W.DIR_ULP + 0.5)
    v_err = np.max(np.abs(aw["v"][go] - ref["v"][go])) / v_unit        # (somebody is re-directed: the callers' populations see to it)
    dv_err = np.max(np.abs(aw["dv"][go] - ref["dv"][go])) / v_unit
    print("%s: v %.3g ulp(c) (bound %g), dv %.3g ulp(c) (bound %g)" % (what, v_err, v_bound, dv_err, v_bound + 1))
    assert v_err <= v_bound and dv_err <= v_bound + 1.0, what
    return ref


# ------------------------------------------------------------------------------------------------ the ABI, by hand
def abi_args(**kw):
    """The arguments of a good call -- three laws (a table the third), three mixtures, a 2 x 3 grid over x and the radius -- and what
    ``kw`` changes of them."""
    arr = lambda x, t=np.float64: None if x is None else np.ascontiguousarray(x, dtype=t)                   # noqa: E731
    a = dict(M=3, kinds=[2, 1, 3], g=[0.0, 0.85, 0.0], T=[0, 0, 2], mu=[-1.0, 0.0, 1.0], F=[0.0, 0.25, 1.0], K=3,
             cum=[[1, 1, 1], [0.3, 0.8, 1], [0, 0, 1]], A=2, coords=[0, 3], bins=[2, 3], edges=[CENTER[0] - 3.0, CENTER[0], CENTER[0] + 3.0] + list(EDGES),
             center=CENTER, map=[0, 1, 2, 255, 2, 0], outside=1, c=C, counts=np.full(2 + 64 + 8, -7, dtype=np.int64))
    a.update(kw)
    keep = [arr(a["kinds"], np.int32), arr(a["g"]), arr(a["T"], np.int32), arr(a["mu"]), arr(a["F"]), arr(a["cum"]), arr(a["coords"], np.int32),
            arr(a["bins"], np.int32), arr(a["edges"]), arr(a["center"]), arr(a["map"], np.uint8)]
    p = [None if x is None else x.ctypes.data for x in keep]
    counts = a["counts"]
    return keep, (a["M"], p[0], p[1], p[2], p[3], p[4], a["K"], p[5], a["A"], p[6], p[7], p[8], p[9], p[10], int(a["outside"]), float(a["c"]),
                  1, 1, None if counts is None else counts.ctypes.data), counts


def lds_limit_args(over):
    """(the arguments, the bytes) of a call at the largest LDS size the header's bound accepts (``over=False``) and of one a table
    node beyond it (``over=True``): three laws, two of them tables (one of the 1024 bins a table may have), 64 mixtures, a grid of
    1024 x 1024 bins in x and y -- 2050 edges -- and as many nodes in the second table as fit.
    Bytes: 8 * (K*M + E + M + 3*T + (3*M + 1)//2) + 4 * (2 + K + M), T the nodes of both tables."""
    K, M, E = 64, 3, 2050
    fixed = 8 * (K * M + E + M + (3 * M + 1) // 2) + 4 * (2 + K + M)
    nodes = (65536 - fixed) // 24 + (1 if over else 0)
    bins = nodes - 1025 - 1                                            # of the second table
    assert 1 <= bins <= 1024 and (fixed + 24 * nodes > 65536) == bool(over) and fixed + 24 * (nodes + 1) > 65536
    mu = np.concatenate([np.linspace(-1.0, 1.0, 1025), np.linspace(-1.0, 1.0, bins + 1)])
    F = np.concatenate([np.linspace(0.0, 1.0, 1025), np.linspace(0.0, 1.0, bins + 1)])
    edges = np.concatenate([np.linspace(CENTER[0] - 4.0, CENTER[0] + 4.0, 1025), np.linspace(CENTER[1] - 4.0, CENTER[1] + 4.0, 1025)])
    cells = (np.arange(1024 * 1024) % K).astype(np.uint8)
    return dict(M=M, kinds=[3, 3, 2], g=[0.0, 0.0, 0.0], T=[1024, bins, 0], mu=mu, F=F, K=K, cum=np.tile([0.4, 0.8, 1.0], (K, 1)), A=2,
                coords=[0, 1], bins=[1024, 1024], edges=edges, map=cells, outside=0), fixed + 24 * nodes


BAD_CALLS = [dict(kinds=None), dict(cum=None), dict(coords=None), dict(bins=None), dict(edges=None), dict(map=None), dict(counts=None),
             dict(g=None), dict(T=None), dict(mu=None), dict(F=None),                            # (the laws' own arrays, where a law reads them)
             dict(M=0), dict(M=9), dict(K=0), dict(K=65), dict(A=0), dict(A=4), dict(outside=-2), dict(outside=3), dict(c=np.inf),
             dict(kinds=[2, 1, 4]), dict(g=[0.0, 1.0, 0.0]), dict(T=[0, 0, 0]), dict(T=[0, 0, 1025]),
             dict(mu=[-1.0, 1.0, 1.0]), dict(F=[0.0, 0.0, 1.0]),
             dict(cum=[[1, 1, 1], [0.3, 0.2, 1], [0, 0, 1]]), dict(cum=[[1, 1, 1], [0.3, 0.8, 0.9], [0, 0, 1]]),
             dict(coords=[0, 0]), dict(coords=[0, 4]), dict(bins=[0, 3]), dict(bins=[1025, 3]),
             dict(edges=[1.0, 0.0, 2.0] + list(EDGES)), dict(edges=[0.0, 1.0, 2.0, -1.0, 2.0, 3.0, 4.0]), dict(edges=[0.0, np.nan, 2.0] + list(EDGES)),
             dict(center=[0, np.nan, 0]),
             dict(map=[0, 1, 3, 255, 2, 0]), dict(map=[0, 1, 254, 255, 2, 0]),                  # a byte that is neither a row nor 255
             dict(A=3, coords=[0, 1, 2], bins=[1024, 1024, 2], edges=np.concatenate([np.linspace(0, 1, 1025)] * 2 + [[0.0, 1.0, 2.0]]),
                  map=np.zeros(8, dtype=np.uint8)),                                              # 2^21 cells (refused before the map is read)
             dict(M=3, kinds=[3, 3, 3], T=[1024, 1024, 1], mu=np.concatenate([np.linspace(-1, 1, 1025)] * 2 + [[-1.0, 1.0]]),
                  F=np.concatenate([np.linspace(0, 1, 1025)] * 2 + [[0.0, 1.0]])),              # 2049 bins in all
             lds_limit_args(over=True)[0]]                                                      # one bin beyond the LDS bound
