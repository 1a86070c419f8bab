"""Scenes, grids, a plain loop and the comparison for the tests of GridScatterStep (tests/test_scatter_grid_cpu.py and the GPU
tests).  Not a test file: a helper they import.

``scatter_grid_loop`` is pcl_step_scatter_grid photon by photon, written from the text of include/physicl_hip.h alone: Python floats
(IEEE doubles, one rounding per operation), tests/scatter_layered_reference.py's Philox4x32-10 block on Python integers and its
linear walk through the edges where the library has a binary search -- and numpy's sin / cos, so that it can be held to
light._scatter_grid bit for bit.  It does not import light.py.

``scene(n, axes, dtype)`` is the edge scene.  Positions are uniform over a box a little larger than the grid, so some stand outside.
Every third slot is planted: its coordinate on one axis (the axes in turn) is, in turn, the axis's first edge, an inner edge, the last
edge, the ``dtype`` value just below the first and the one just above the last (for a radius axis the whole position is the centre
plus that distance along x, which makes q the squared edge exactly).  Beside them: NaN positions, photons at rest (with -0.0), a NaN
in v (moves), energies on the first, an inner and the last band edge, one ``dtype`` value outside either end, NaN energies.  Every
edge is a multiple of 1/8, exact in float32.
"""
import math

import numpy as np

from scatter_layered_reference import C, ID_BASE, SEED, closed_bin, philox, same_answer  # noqa: F401  (the tests import them from here)
from writer_reference import DIR_ULP, photons, same_bits, ulp, wide

CENTER = np.array([0.5, -0.25, 0.125])
E_EDGES = np.array([1.0, 1.5, 2.0, 3.0])
COORD = {"x": 0, "y": 1, "z": 2}
WORDS = (25, 26)


def grid_edges(axes, bins):
    """One edge array per axis: Cartesian axes from -2 to 2, a radius axis from 0.5 to 2.5, in ``bins[a]`` equal bins when that is a
    power of two (multiples of 1/8 or finer powers of two: exact), otherwise with numpy's linspace."""
    return [np.linspace(0.5, 2.5, b + 1) if a == "r" else np.linspace(-2.0, 2.0, b + 1) for a, b in zip(axes, bins)]


def scene(n, axes, edges, dtype=np.float64, seed=3):
    """{"r", "v", "dr", "dv": (n, 3), "E": (n,)} of float64 arrays that hold ``dtype`` values (the module's docstring)."""
    rng = np.random.RandomState(seed + n)
    i = np.arange(n)
    u = rng.normal(size=(n, 3))
    r = rng.uniform(-2.2, 2.2, size=(n, 3)).astype(dtype)
    v = C * u / np.sqrt((u * u).sum(axis=1))[:, None]
    E = rng.uniform(0.8, 3.2, size=n).astype(dtype)
    lo, hi = dtype(-np.inf), dtype(np.inf)
    for k in range(0, n, 3):
        a = (k // 3) % len(axes)
        which = (k // (3 * len(axes))) % 5
        e = edges[a]
        if axes[a] == "r":
            x = dtype(CENTER[0] + [e[0], e[len(e) // 2], e[-1], e[0], e[-1]][which])
            x = np.nextafter(x, lo) if which == 3 else (np.nextafter(x, hi) if which == 4 else x)
            r[k] = [x, CENTER[1], CENTER[2]]
        else:
            x = dtype([e[0], e[len(e) // 2], e[-1], e[0], e[-1]][which])
            r[k, COORD[axes[a]]] = np.nextafter(x, lo) if which == 3 else (np.nextafter(x, hi) if which == 4 else x)
    r[i % 31 == 5, 1] = np.nan
    r[i % 62 == 7, 0] = np.nan
    v[i % 13 == 1] = 0.0
    v[i % 26 == 1, 0] = -0.0
    v[i % 26 == 1, 2] = -0.0
    v[i % 37 == 2, 0] = np.nan
    for mod, rest, value in ((11, 3, 1.5), (11, 4, 3.0), (11, 5, 1.0), (29, 6, np.nan)):
        E[i % mod == rest] = value
    E[i % 29 == 7] = np.nextafter(dtype(3.0), hi)
    E[i % 29 == 8] = np.nextafter(dtype(1.0), lo)
    state = {"r": r, "v": v, "dr": rng.normal(size=(n, 3)), "dv": rng.normal(size=(n, 3)), "E": E}
    return {k: np.asarray(a).astype(dtype).astype(np.float64) for k, a in state.items()}


def probabilities(shape, kind="mixed", seed=9):
    """p of the given shape.  0, 1, or "mixed": zeros, ones and values between them in about equal shares."""
    if not isinstance(kind, str):
        return np.full(shape, float(kind))
    rng = np.random.RandomState(seed + int(np.prod(shape)))
    pick = rng.randint(0, 4, size=shape)
    return np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, rng.choice([0.125, 0.25, 0.5, 0.75], size=shape)))


def scatter_grid_loop(r, v, dv, E, photon, ids, p, axes, edges, center, E_edges, first, c, seed, n_pass, dtype=np.float64):
    """pcl_step_scatter_grid, photon by photon (the module's docstring).  The arguments and the dict of light._scatter_grid."""
    r, v, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v, dv))
    n = len(v)
    cmp_edges = [[float(e) * float(e) for e in ed] if a == "r" else [float(e) for e in ed] for a, ed in zip(axes, edges)]
    Ee = None if E_edges is None else [float(e) for e in E_edges]
    shape = tuple(len(e) - 1 for e in edges) + (() if Ee is None else (len(Ee) - 1,))
    p = [float(x) for x in np.asarray(p, dtype=np.float64).reshape(-1)]
    cx = [float(x) for x in center]
    store = (lambda x: float(np.float32(x))) if dtype is np.float32 else float
    exposed, scattered, written = (np.zeros(n, dtype=bool) for _ in range(3))
    cell = np.full(n, -1, dtype=np.int64)
    cells = [0] * len(p)
    for i in range(n):
        if not photon[i]:
            continue                                                   # never written
        hit = False
        v0, v1, v2 = (float(x) for x in v[i])
        if not (v0 == 0.0 and v1 == 0.0 and v2 == 0.0):                 # moving (a NaN moves, -0.0 == 0)
            x = [float(t) for t in r[i]]
            g = 0
            for a, e in zip(axes, cmp_edges):
                if a == "r":
                    d = [x[k] - cx[k] for k in range(3)]
                    q = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
                else:
                    q = x[COORD[a]]
                b = closed_bin(e, q)
                if b < 0:
                    g = -1
                    break
                g = g * (len(e) - 1) + b
            if g >= 0 and Ee is not None:
                b = closed_bin(Ee, float(E[i]))
                g = g * (len(Ee) - 1) + b if b >= 0 else -1
            if g >= 0:
                cell[i], exposed[i] = g, True
                if p[g] > 0.0:
                    hit = philox(int(ids[i]), int(seed), int(n_pass), WORDS[0])[0] < p[g]
        if hit:
            u_a, u_b = philox(int(ids[i]), int(seed), int(n_pass), WORDS[1])
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
                old = float(v[i, k])
                new = c * ((sc * e1[k] + ss * f2[k]) + mu * w[k])
                v[i, k], dv[i, k] = store(new), store(new - old)
            scattered[i] = written[i] = True
            cells[cell[i]] += 1
        elif first:
            dv[i] = 0.0
            written[i] = True
    return {"v": v, "dv": dv, "exposed": exposed, "scattered": scattered, "written": written, "cell": cell,
            "scattered_by_cell": np.array(cells, dtype=np.int64).reshape(shape)}


def assert_every_outcome(ref, state_v, photon, E_edges, what):
    """Skipped at rest, skipped for want of a cell or a band, exposed and missed, hit: each at least once."""
    photon = np.asarray(photon, dtype=bool)
    v = np.asarray(state_v, dtype=np.float64)
    rest = (v[:, 0] == 0) & (v[:, 1] == 0) & (v[:, 2] == 0) & photon
    counts = {"at rest": int(rest.sum()), "no cell": int((photon & ~rest & ~ref["exposed"]).sum()),
              "exposed miss": int((ref["exposed"] & ~ref["scattered"]).sum()), "hit": int(ref["scattered"].sum())}
    assert not (rest & ref["exposed"]).any() and sum(counts.values()) == int(photon.sum()), (what, counts)
    assert all(n > 0 for n in counts.values()), (what, counts)
    return counts


# ------------------------------------------------------------------------------------------------ a sweep against the restatement
def check_scatter_grid(before, after, answer, p, axes, edges, center, E_edges, first, c, seed, n_pass, what, restate=None):
    """A state downloaded before the sweep, the state downloaded after it and the sweep's answer ``(exposed, scattered,
    scattered_by_cell)`` against the restatement (``restate``: light._scatter_grid by default, which tests/test_scatter_grid_cpu.py
    holds to ``scatter_grid_loop`` bit for bit; the loop itself may be given).  Without tolerance: who is exposed and who is hit (the
    counts and every cell), every row that is not written, the dv = 0 rows, r, dr, E, ids and kinds.  v and dv of the hit rows go
    through the device's own sin / cos: the bounds check_scatter_layered takes from writer_reference (DIR_ULP ulp(c), + 0.5 float32
    ulp in an fp32 store, one more for dv) -- the arithmetic is that sweep's.  Returns the restatement's dict."""
    if restate is None:
        from physicl_amd import light
        restate = light._scatter_grid
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    ref = restate(b["r"], b["v"], b["dv"], np.asarray(before["E"]).astype(np.float64), photons(before), before["id"], p, axes, edges, center,
                  E_edges, first, c, seed, n_pass, T)
    for f in set(before) - {"r", "v", "dr", "dv", "count"}:              # E, ids, kinds
        assert same_bits(before[f], after[f]), (what, f)
    assert before.get("count") == after.get("count") and len(before["E"]) == len(after["E"]), what
    for f in ("r", "dr"):
        assert same_bits(a[f], b[f]), (what, f)
    hit, written = ref["scattered"], ref["written"]
    exposed, scattered, cells = answer
    print("%s: exposed %d, scattered %d of %d" % (what, ref["exposed"].sum(), hit.sum(), len(hit)))
    assert (int(exposed), int(scattered)) == (int(ref["exposed"].sum()), int(hit.sum())), what
    assert np.asarray(cells).shape == ref["scattered_by_cell"].shape and np.array_equal(np.asarray(cells), ref["scattered_by_cell"]), what
    assert int(np.asarray(cells).sum()) == int(scattered) <= int(exposed), what
    for f in ("v", "dv"):
        assert same_bits(a[f][~written], b[f][~written]), (what, f)     # who is not written keeps every bit
    miss = written & ~hit
    assert same_bits(a["v"][miss], b["v"][miss]), what
    assert same_bits(a["dv"][miss], np.zeros((int(miss.sum()), 3))), what                   # +0.0, bit for bit
    assert miss.any() == (bool(first) and bool((photons(before) & ~hit).any())), what
    if hit.any():
        v_unit, v_bound = (ulp(c), DIR_ULP) if T is np.float64 else (ulp(c, np.float32), DIR_ULP + 0.5)
        v_err = np.max(np.abs(a["v"][hit] - ref["v"][hit])) / v_unit
        known = np.isfinite(ref["dv"][hit])                            # (an old velocity with a NaN: dv is NaN on both sides)
        assert np.array_equal(np.isfinite(a["dv"][hit]), known), what
        dv_err = np.max(np.abs(a["dv"][hit][known] - ref["dv"][hit][known])) / v_unit if known.any() else 0.0
        print("%s: v %.3g ulp(c) (bound %g), dv %.3g ulp(c) (bound %g)" % (what, v_err, v_bound, dv_err, v_bound + 1))
        assert v_err <= v_bound, what
        assert dv_err <= v_bound + 1.0, what                           # dv = v - v_old: one more rounding, of a value up to 2c
    return ref


# ------------------------------------------------------------------------------------------------ the ABI, by hand
ABI_AXES, ABI_BINS = ("x", "y", "z"), (2, 2, 2)


def abi_args(**kw):
    """The arguments of a good call (behind the context) -- a 2 x 2 x 2 grid by 3 bands --, and what ``kw`` changes of them: n_axes,
    coords, n_bins, edges, center, B, E_edges, p, first, c, counts, cells."""
    edges = np.concatenate(grid_edges(ABI_AXES, ABI_BINS))
    a = dict(n_axes=3, coords=[0, 1, 2], n_bins=list(ABI_BINS), edges=edges, center=CENTER, B=3, E_edges=E_EDGES,
             p=probabilities((2, 2, 2, 3)), first=1, c=C, counts=np.full(4, -7, dtype=np.int64), cells=np.full(64, -7, dtype=np.int64))
    a.update(kw)
    ints = [None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.int32) for k in ("coords", "n_bins")]
    dbl = [None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.float64) for k in ("edges", "center", "E_edges", "p")]
    ptr = lambda x: None if x is None else x.ctypes.data                                                    # noqa: E731
    return (ints, dbl), (int(a["n_axes"]), ptr(ints[0]), ptr(ints[1]), ptr(dbl[0]), ptr(dbl[1]), int(a["B"]), ptr(dbl[2]), ptr(dbl[3]),
                         int(a["first"]), float(a["c"]), 1, 1, ptr(a["counts"]), ptr(a["cells"])), (a["counts"], a["cells"])


GOOD_P = probabilities((2, 2, 2, 3))
_BIG = dict(n_axes=3, coords=[0, 1, 2], n_bins=[1024, 1024, 2], edges=np.concatenate([np.arange(1025.0), np.arange(1025.0), np.arange(3.0)]),
            B=0, E_edges=None, p=np.zeros(8))                         # 2^21 cells: refused before p is read
BAD_CALLS = [dict(p=None), dict(counts=None), dict(cells=None), dict(coords=None), dict(n_bins=None), dict(edges=None), dict(n_axes=0),
             dict(n_axes=4), dict(coords=[0, 0, 2]), dict(coords=[0, 1, 4]), dict(coords=[-1, 1, 2]), dict(n_bins=[2, 0, 2]),
             dict(n_bins=[2, 1025, 2]), _BIG, dict(B=-1), dict(B=1025), dict(E_edges=None), dict(first=2), dict(first=-1), dict(c=np.nan),
             dict(c=np.inf), dict(p=np.where(GOOD_P == 1.0, 1.5, GOOD_P)), dict(p=np.where(GOOD_P == 1.0, np.nan, GOOD_P)),
             dict(p=np.where(GOOD_P == 0.0, -0.1, GOOD_P)), dict(edges=[-2.0, 0.0, 2.0, -2.0, 2.0, 0.0, -2.0, 0.0, 2.0]),
             dict(edges=[-2.0, 0.0, 2.0, -2.0, 0.0, 0.0, -2.0, 0.0, 2.0]), dict(edges=[-2.0, 0.0, np.inf, -2.0, 0.0, 2.0, -2.0, 0.0, 2.0]),
             dict(coords=[0, 1, 3], edges=[-2.0, 0.0, 2.0, -2.0, 0.0, 2.0, -1.0, 0.0, 2.0]),     # a negative radius
             dict(coords=[0, 1, 3], edges=[-2.0, 0.0, 2.0, -2.0, 0.0, 2.0, 0.0, 1.0, 1e200]),    # its square overflows
             dict(E_edges=[1.0, 2.0, 1.5, 3.0]), dict(E_edges=[1.0, 1.5, np.nan, 3.0]), dict(center=[0, np.nan, 0]),
             dict(center=[np.inf, 0, 0])]
