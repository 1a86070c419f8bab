"""A second restatement, the scene and the comparison for the tests of ReemissionStep (tests/test_reemit_cpu.py and the GPU tests).
Not a test file: a helper they import.

``reemit_parked_loop`` is pcl_step_reemit_parked once more, a plain loop over the photons in Python floats, written from the rule
in include/physicl_hip.h; it shares nothing with the vectorised physicl_amd.light._reemit_parked but the Philox block and the table
search (and numpy's sin / cos, so that the two can be compared bit for bit).

The scene (``scene``), slot i, about CENTER with the layers EDGES = 0, 1, 2, 3, 4:
    at rest                              iff i % 2 == 0   (of these, i % 6 == 0 carries a -0.0)
    a NaN in v0 / v2                     iff i % 13 == 0 / i % 26 == 1   (written last: such a slot moves)
    a plain Object                       iff i % 17 == 0
    exactly at CENTER (q == 0)           iff i % 10 == 0  (layer 0 is lambertian: no vertical)
    on the inner edge 1 (q == 1)         iff i % 14 == 2  (layer 1, not 0)
    on the outermost edge 4 (q == 16)    iff i % 18 == 4  (the last layer is closed)
    just outside it                      iff i % 22 == 6  (in no layer)
    a NaN in r                           iff i % 34 == 8
    everybody else: a random radius up to 4.4 (some outside), in a random direction.
All special positions are exact in float32 as well.  Ids are scrambled.
"""
import bisect
import math

import numpy as np

from physicl_amd import light
from writer_reference import DIR_ULP, same_bits, ulp

C = 299792458.0
SEED = 0x5EED5A7F
ID_BASE = 7_000_000_001
CENTER = np.array([0.5, -0.25, 0.125])               # exact in float32, and so is CENTER + (k, 0, 0) for the edges k
EDGES = np.array([0.0, 1.0, 2.0, 3.0, 4.0])
ETA = np.array([1.0, 0.5, 0.0, 0.5])
ANGULAR = ("lambertian", "isotropic", "isotropic", "lambertian")
GRID_A = np.array([1.25, 1.5, 2.0, 2.75, 3.5, 4.25])  # float32 values
CDF_A = np.array([0.0, 0.1, 0.1, 0.45, 0.45, 1.0])   # cdf[0] == 0 and repeated values: bins without mass
GRID_B = np.array([7.5, 8.25, 9.0])
CDF_B = np.array([0.3, 0.6, 1.0])
TABLES = ((GRID_A, CDF_A), None, (GRID_B, CDF_B), (GRID_B, CDF_B))
FIELDS = ("r", "v", "dr", "dv")
LAYERED = dict(eta=ETA, angular=ANGULAR, tables=TABLES, edges=EDGES, center=CENTER)
# the other paths of the kernel: one layer everywhere (r is not read), and one lambertian layer everywhere (r is read for the vertical)
EVERYWHERE = dict(eta=1.0, angular="isotropic", tables=None, edges=None, center=CENTER)
EVERYWHERE_UP = dict(eta=0.5, angular="lambertian", tables=[(GRID_B, CDF_B)], edges=None, center=CENTER)


def unit(x):
    return x / np.sqrt((x * x).sum(axis=1))[:, None]


def scene(n, dtype=np.float64, seed=1):
    """{"r", "v", "dr", "dv": (n, 3), "E": (n,)} of float64 arrays that hold ``dtype`` values, ``photon`` and ``id``, laid out as the
    module's docstring says."""
    rng = np.random.RandomState(seed + n)
    i = np.arange(n)
    r = CENTER + rng.uniform(0.0, 4.4, size=n)[:, None] * unit(rng.normal(size=(n, 3)))
    v = C * unit(rng.normal(size=(n, 3)))
    v[i % 2 == 0] = 0.0
    v[i % 6 == 0, 1] = -0.0
    for m, k, x in ((10, 0, 0.0), (14, 2, 1.0), (18, 4, 4.0)):
        r[i % m == k] = CENTER + np.array([x, 0.0, 0.0])
    r[i % 22 == 6] = [np.nextafter(dtype(CENTER[0] + 4.0), dtype(np.inf)), CENTER[1], CENTER[2]]
    r[i % 34 == 8, 2] = np.nan
    v[i % 13 == 0, 0] = np.nan
    v[i % 26 == 1, 2] = np.nan
    state = {"r": r, "v": v, "dr": rng.normal(size=(n, 3)), "dv": rng.normal(size=(n, 3)), "E": 1.0 + rng.uniform(size=n)}
    state = {k: a.astype(dtype).astype(np.float64) for k, a in state.items()}
    state["photon"] = i % 17 != 0
    state["id"] = ID_BASE + np.random.RandomState(5).permutation(n).astype(np.int64)
    return state


def reemit_parked_loop(r, v, E, photon, ids, eta, angular, tables, edges, center, c, seed, n_pass, dtype=np.float64):
    """pcl_step_reemit_parked, photon by photon (the module's docstring).  The arguments and the dict of light._reemit_parked."""
    r, v = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v))
    n = len(v)
    E = np.array(E, dtype=np.float64).reshape(-1)
    rows = 1 if edges is None else len(edges) - 1
    eta = [float(x) for x in np.broadcast_to(np.asarray(eta, dtype=np.float64).reshape(-1), (rows,))]
    lam = [a == "lambertian" for a in ((angular,) * rows if isinstance(angular, str) else angular)]
    tables = [None] * rows if tables is None else list(tables)
    e2 = None if edges is None else [float(e) * float(e) for e in edges]
    cx = [float(x) for x in center]
    store = (lambda x: float(np.float32(x))) if dtype is np.float32 else float
    draw, (dir_a, dir_b), energy = (light._philox_block(ids, seed, n_pass, w) for w in (18, 19, 20))
    draw, energy = draw[0], energy[0]
    dr, dv = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    parked, reemitted, layer = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.full(n, -1, dtype=np.int64)
    by_layer = np.zeros(rows, dtype=np.int64)
    for i in range(n):
        v0, v1, v2 = (float(x) for x in v[i])
        if not (v0 == 0.0 and v1 == 0.0 and v2 == 0.0) or not photon[i]:
            continue
        d = [float(r[i, k]) - cx[k] for k in range(3)]
        q = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        b = 0
        if e2 is not None:
            if not (e2[0] <= q <= e2[-1]):                              # (False for a NaN)
                continue
            b = rows - 1
            while q < e2[b]:                                            # [e2_b, e2_(b+1)), the last one closed
                b -= 1
        parked[i], layer[i] = True, b
        if not eta[b] > 0.0 or not float(draw[i]) < eta[b]:
            continue
        u_a, u_b = float(dir_a[i]), float(dir_b[i])
        if lam[b]:
            if not (0.0 < q < math.inf):
                continue
            s = math.sqrt(q)
            w = [d[k] / s for k in range(3)]
            mu = math.sqrt(1.0 - u_a)
        else:
            w, mu = [1.0, 0.0, 0.0], 1.0 - 2.0 * u_a
        sg = math.copysign(1.0, w[2])
        aa = -1.0 / (sg + w[2])
        bb, sw0 = (w[0] * w[1]) * aa, sg * w[0]
        e1 = [1.0 + (sw0 * w[0]) * aa, sg * bb, -sw0]
        f2 = [bb, sg + (w[1] * w[1]) * aa, -w[1]]
        sn = math.sqrt((1.0 - mu) * (1.0 + mu))
        psi = np.float64((u_b * 2.0) * math.pi)
        sc, ss = sn * float(np.cos(psi)), sn * float(np.sin(psi))
        for k in range(3):
            v[i, k] = store(c * ((sc * e1[k] + ss * f2[k]) + mu * w[k]))
        dr[i], dv[i] = 0.0, 0.0
        reemitted[i] = True
        by_layer[b] += 1
        if tables[b] is not None:
            grid, cdf = tables[b]
            E[i] = store(float(grid[bisect.bisect_left([float(x) for x in cdf], float(energy[i]))]))
    return {"r": r, "v": v, "dr": dr, "dv": dv, "E": E, "parked": parked, "reemitted": reemitted, "layer": layer, "by_layer": by_layer}


def same_answer(a, b):
    """Two answers of a restatement, bit for bit (NaN rows of dr and dv included)."""
    return set(a) == set(b) and all(same_bits(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------ a sweep against the restatement
def wide(s):
    return {f: (np.stack(s[f], 1) if isinstance(s[f], (list, tuple)) else np.asarray(s[f])).astype(np.float64) for f in FIELDS}


def check_reemit(before, after, answer, cfg, seed, n_pass, what, photon=None, c=C):
    """A state downloaded before the sweep, the state downloaded after it and the sweep's answer ``(parked, reemitted, by_layer)``
    against light._reemit_parked.  Counts exact; every row of a particle that is not re-emitted bit-identical; r, ids (and E without
    a table) bit-identical for everybody; dr and dv of the re-emitted exactly 0; their E bit-identical to the restatement; their v
    within writer_reference.DIR_ULP ulp(c), DIR_ULP + 0.5 float32 ulp in an fp32 store.  Returns the restatement's dict."""
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    n = len(before["E"])
    photon = np.ones(n, dtype=bool) if photon is None else photon
    E_b, E_a = np.asarray(before["E"]).astype(np.float64), np.asarray(after["E"]).astype(np.float64)
    ref = light._reemit_parked(b["r"], b["v"], E_b, photon, before["id"], cfg["eta"], cfg["angular"], cfg["tables"], cfg["edges"],
                               cfg["center"], c, seed, n_pass, T)
    go = ref["reemitted"]
    parked, reemitted, by_layer = answer
    print("%s: parked %d, re-emitted %d of %d, by layer %s" % (what, ref["parked"].sum(), go.sum(), n, ref["by_layer"].tolist()))
    assert (int(parked), int(reemitted)) == (int(ref["parked"].sum()), int(go.sum())), what
    assert np.asarray(by_layer).tolist() == ref["by_layer"].tolist(), what
    assert np.array_equal(after["id"], before["id"]) and len(after["E"]) == n, what
    assert same_bits(a["r"], b["r"]), what
    for f in FIELDS:
        assert same_bits(a[f][~go], b[f][~go]), (what, f)
    assert same_bits(E_a, ref["E"]), what                              # the re-emitted's: the table's; everybody else's: untouched
    if cfg["tables"] is None:
        assert same_bits(np.asarray(after["E"]), np.asarray(before["E"])), what
    if go.any():
        zero = np.zeros((int(go.sum()), 3))
        assert same_bits(a["dr"][go], zero) and same_bits(a["dv"][go], zero), what           # +0.0, bit for bit
        v_unit, v_bound = (ulp(c), DIR_ULP) if T is np.float64 else (ulp(c, np.float32), DIR_ULP + 0.5)
        v_err = np.max(np.abs(a["v"][go] - ref["v"][go])) / v_unit
        print("%s: direction %.3g ulp(c) (bound %g)" % (what, v_err, v_bound))
        assert v_err <= v_bound, what
    return ref


# ------------------------------------------------------------------------------------------------ the ABI, by hand
def abi_args(**kw):
    """(what must stay alive, the arguments behind the handle, counts) of a good call of pcl_step_reemit_parked -- two layers, the
    first with a table --, and what ``kw`` changes of them (None: NULL)."""
    import ctypes
    a = dict(L=2, edges=np.array([1.0, 2.0, 3.0]), center=CENTER, eta=np.array([0.5, 1.0]), lam=np.array([1, 0], dtype=np.int32),
             off=np.array([0, 3, 3], dtype=np.int32), cdf=CDF_B, grid=GRID_B, c=C, counts=np.full(6, -7, dtype=np.int64))
    a.update(kw)
    arr = lambda x, t: None if x is None else np.ascontiguousarray(x, dtype=t)                              # noqa: E731
    keep = [arr(a["edges"], np.float64), arr(a["center"], np.float64), arr(a["eta"], np.float64), arr(a["lam"], np.int32),
            arr(a["off"], np.int32), arr(a["cdf"], np.float64), arr(a["grid"], np.float64)]
    p = [None if x is None else x.ctypes.data for x in keep]
    counts = a["counts"]
    return keep, (int(a["L"]), p[0], p[1], p[2], p[3], p[4], p[5], p[6], ctypes.c_double(a["c"]), 1, 1,
                  None if counts is None else counts.ctypes.data), counts


BAD_CALLS = [dict(eta=None), dict(lam=None), dict(off=None), dict(counts=None), dict(edges=None), dict(L=-1),
             dict(L=65, edges=np.arange(66.0), eta=np.ones(65), lam=np.zeros(65), off=np.zeros(66)),
             dict(eta=[0.5, 1.5]), dict(eta=[-0.1, 1.0]), dict(eta=[np.nan, 1.0]), dict(lam=[2, 0]), dict(lam=[0, -1]),
             dict(off=[1, 3, 3]), dict(off=[0, 3, 2]), dict(off=[0, -1, 3]), dict(cdf=None), dict(grid=None),
             dict(off=[0, 1025, 1025], cdf=np.linspace(0, 1, 1025), grid=np.ones(1025)),
             dict(off=[0, 1024, 2049], cdf=np.concatenate([np.linspace(0, 1, 1024), np.linspace(0, 1, 1025)]), grid=np.ones(2049)),
             dict(cdf=[0.3, 0.2, 1.0]), dict(cdf=[0.3, 0.6, 0.9]), dict(cdf=[0.3, 0.6, 1.5]), dict(cdf=[0.3, np.nan, 1.0]),
             dict(off=[0, 2, 3]),                                        # the first table then ends in 0.6
             dict(grid=[1.0, np.inf, 2.0]), dict(grid=[1.0, np.nan, 2.0]),
             dict(edges=[1.0, 1.0, 3.0]), dict(edges=[-1.0, 2.0, 3.0]), dict(edges=[1.0, np.nan, 3.0]), dict(edges=[1.0, 2.0, 1e200]),
             dict(center=[0.0, np.nan, 0.0]), dict(center=[np.inf, 0.0, 0.0]), dict(c=np.inf), dict(c=np.nan)]
