"""States, tables, a plain loop and the comparison for the tests of LayeredScatterStep (tests/test_scatter_layered_cpu.py and the GPU
tests).  Not a test file: a helper they import.

``scatter_layered_loop`` is pcl_step_scatter_layered photon by photon, written from the text of include/physicl_hip.h alone: Python
floats (IEEE doubles, one rounding per operation), a Philox4x32-10 block of its own on Python integers, a linear walk through the
edges where the library has a binary search -- and numpy's sin / cos, so that it can be held to light._scatter_layered bit for bit.

The states are tests/path_absorb_reference.py's ``layout`` (its docstring lists the planted slots: at rest, -0.0, a NaN in v, r and
E, on the first, an inner and the last layer edge and band edge, outside all layers and bands); ``tables`` makes the edges and the
probabilities for any number of layers and bands so that every planted value stays exactly on an edge: layer edges from 1 to 3 and
band edges from 1 to 3 in equal steps that are powers of two, or [1, 2, 2.5, 3] / [1, 1.5, 2, 3] for three.
"""
import math

import numpy as np

from path_absorb_reference import C, CENTER, ID_BASE, SEED, layout, planted  # noqa: F401  (the tests import them from here)
from physicl_amd import light
from writer_reference import DIR_ULP, photons, same_bits, ulp, wide

M32 = 0xFFFFFFFF
OUTCOMES = ("at rest", "no layer", "no band", "exposed miss", "hit")


def philox(id_, seed, word2, word3):
    """(u53(w0, w1), u53(w2, w3)) of the Philox4x32-10 block with the counter (id_lo, id_hi, word2, word3) and the key (seed_lo,
    seed_hi), on Python integers."""
    c = [id_ & M32, (id_ >> 32) & M32, word2 & M32, word3 & M32]
    k = [seed & M32, (seed >> 32) & M32]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    u53 = lambda a, b: float((a >> 5) * (1 << 26) + (b >> 6)) * (1.0 / 9007199254740992.0)           # noqa: E731
    return u53(c[0], c[1]), u53(c[2], c[3])


def closed_bin(edges, x):
    """[e_b, e_(b+1)), the last one closed; -1 outside the edges and for a NaN."""
    if not (edges[0] <= x <= edges[-1]):
        return -1
    b = len(edges) - 2
    while x < edges[b]:
        b -= 1
    return b


def scatter_layered_loop(r, v, dv, E, photon, ids, p, edges, center, E_edges, first, c, seed, n_pass, dtype=np.float64):
    """pcl_step_scatter_layered, photon by photon (the module's docstring).  The arguments and the dict of light._scatter_layered."""
    r, v, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v, dv))
    n = len(v)
    rows, cols = (1 if e is None else len(e) - 1 for e in (edges, E_edges))
    p = np.asarray(p, dtype=np.float64).reshape(rows, cols)
    e2 = None if edges is None else [float(e) * float(e) for e in edges]
    Ee = None if E_edges is None else [float(e) for e in E_edges]
    cx = [float(x) for x in center]
    store = (lambda x: float(np.float32(x))) if dtype is np.float32 else float
    exposed, scattered, written = (np.zeros(n, dtype=bool) for _ in range(3))
    layer, band = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
    cells = np.zeros((rows, cols), dtype=np.int64)
    for i in range(n):
        if not photon[i]:
            continue                                                   # never written
        hit = False
        v0, v1, v2 = (float(x) for x in v[i])
        if not (v0 == 0.0 and v1 == 0.0 and v2 == 0.0):                 # moving (a NaN moves, -0.0 == 0)
            b = 0
            if e2 is not None:
                d = [float(r[i, k]) - cx[k] for k in range(3)]
                b = closed_bin(e2, (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            layer[i] = b
            if b >= 0:
                e = 0 if Ee is None else closed_bin(Ee, float(E[i]))
                band[i] = e
                if e >= 0:
                    exposed[i] = True
                    pc = float(p[b, e])
                    if pc > 0.0:
                        hit = philox(int(ids[i]), int(seed), int(n_pass), 23)[0] < pc
        if hit:
            u_a, u_b = philox(int(ids[i]), int(seed), int(n_pass), 24)
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
            cells[layer[i], band[i]] += 1
        elif first:
            dv[i] = 0.0
            written[i] = True
    return {"v": v, "dv": dv, "exposed": exposed, "scattered": scattered, "written": written, "layer": layer, "band": band,
            "scattered_by_cell": cells}


def same_answer(a, b):
    """Two answers of a restatement, bit for bit."""
    return set(a) == set(b) and all(same_bits(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------ tables
def edges_of(n, three):
    """n + 1 edges from 1 to 3 on which the layout's planted values (1, 1.5 or 2, 3) lie exactly; None for n == 0."""
    if n == 0:
        return None
    return np.array(three) if n == 3 else np.linspace(1.0, 3.0, n + 1)


def tables(L, B, p="mixed", seed=9):
    """(p [L'][B'], edges, E_edges) for L layers and B bands (0: none).  ``p``: 0, 1, or "mixed": zeros, ones and values between
    them in about equal shares, every one a float64 the device gets as it stands."""
    edges, E_edges = edges_of(L, [1.0, 2.0, 2.5, 3.0]), edges_of(B, [1.0, 1.5, 2.0, 3.0])
    shape = (max(L, 1), max(B, 1))
    if isinstance(p, str):
        rng = np.random.RandomState(seed + 7 * L + B)
        pick = rng.randint(0, 4, size=shape)
        cells = np.where(pick == 0, 0.0, np.where(pick == 1, 1.0, rng.choice([0.125, 0.25, 0.5, 0.75], size=shape)))
        if cells.size == 1:
            cells[...] = 0.5
        elif cells.size <= 4:                                          # few cells: one of each by hand
            cells.flat[:] = ([0.0, 0.5, 1.0, 0.25])[:cells.size]
    else:
        cells = np.full(shape, float(p))
    return cells, edges, E_edges


def assert_every_outcome(ref, state_v, photon, edges, E_edges, what):
    """Skipped at rest, skipped in no layer, skipped in no band, exposed and missed, hit: each at least once (a case without layers or
    bands cannot skip for their lack).  On the numpy side, so that a state cannot hide a branch from the device."""
    photon = np.asarray(photon, dtype=bool)
    rest = light._at_rest(np.asarray(state_v, dtype=np.float64)) & photon
    moving = photon & ~rest
    found = {"at rest": rest & ~ref["exposed"], "no layer": moving & (ref["layer"] < 0),
             "no band": moving & (ref["layer"] >= 0) & (ref["band"] < 0), "exposed miss": ref["exposed"] & ~ref["scattered"],
             "hit": ref["scattered"]}
    counts = {k: int(m.sum()) for k, m in found.items()}
    assert sum(counts.values()) == int(photon.sum()), (what, counts)    # every photon has exactly one outcome
    need = [k for k in OUTCOMES if not (k == "no layer" and edges is None) and not (k == "no band" and E_edges is None)]
    assert all(counts[k] > 0 for k in need), (what, counts)
    return counts


# ------------------------------------------------------------------------------------------------ a sweep against the restatement
def check_scatter_layered(before, after, answer, p, edges, center, E_edges, first, c, seed, n_pass, what):
    """A state downloaded before the sweep, the state downloaded after it and the sweep's answer ``(exposed, scattered,
    scattered_by_cell)`` against light._scatter_layered.  Without tolerance: who is exposed and who is hit (the counts and every cell),
    every row that is not written, the dv = 0 rows, r, dr, E, ids and kinds.  v and dv of the hit rows go through the device's own sin /
    cos: within writer_reference.DIR_ULP ulp(c) and one more for dv (DIR_ULP + 0.5 float32 ulp in an fp32 store), the bound derived there
    for a direction made by the same frame / polar / turned arithmetic and applied to the re-emission's.  Returns the restatement's dict."""
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    ref = light._scatter_layered(b["r"], b["v"], b["dv"], np.asarray(before["E"]).astype(np.float64), photons(before), before["id"], p, edges,
                                 center, E_edges, first, c, seed, n_pass, T)
    for f in set(before) - {"r", "v", "dr", "dv", "count"}:              # E, ids, kinds
        assert same_bits(before[f], after[f]), (what, f)
    assert before.get("count") == after.get("count") and len(before["E"]) == len(after["E"]), what
    for f in ("r", "dr"):
        assert same_bits(a[f], b[f]), (what, f)
    hit, written = ref["scattered"], ref["written"]
    exposed, scattered, cells = answer
    print("%s: exposed %d, scattered %d of %d" % (what, ref["exposed"].sum(), hit.sum(), len(hit)))
    assert (int(exposed), int(scattered)) == (int(ref["exposed"].sum()), int(hit.sum())), what
    assert np.asarray(cells).shape == ref["scattered_by_cell"].shape and np.asarray(cells).tolist() == ref["scattered_by_cell"].tolist(), what
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
def abi_args(**kw):
    """The arguments of a good call (behind the context), and what ``kw`` changes of them: L, B, p, edges, center, E_edges, first, c,
    counts, cells."""
    p, edges, E_edges = tables(3, 3)
    a = dict(L=3, B=3, p=p, edges=edges, center=CENTER, E_edges=E_edges, first=1, c=C, counts=np.full(4, -7, dtype=np.int64),
             cells=np.full(4096 + 2, -7, dtype=np.int64))
    a.update(kw)
    arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)                        # noqa: E731
    keep = [arr(a[k]) for k in ("p", "edges", "center", "E_edges")]
    ptr = lambda x: None if x is None else x.ctypes.data                                                    # noqa: E731
    return keep, (int(a["L"]), int(a["B"]), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), int(a["first"]), float(a["c"]), 1, 1,
                  ptr(a["counts"]), ptr(a["cells"])), (a["counts"], a["cells"])


GOOD_P = tables(3, 3)[0]
BAD_CALLS = [dict(p=None), dict(counts=None), dict(cells=None), dict(L=-1), dict(B=-1), dict(first=2), dict(first=-1), dict(c=np.nan),
             dict(c=np.inf), dict(L=65, p=np.full((65, 3), 0.5), edges=np.arange(66.0)),
             dict(B=1025, p=np.full((3, 1025), 0.5), E_edges=np.arange(1026.0)),
             dict(L=64, B=65, p=np.full((64, 65), 0.5), edges=np.arange(65.0), E_edges=np.arange(66.0)),                 # 4160 cells
             dict(p=np.where(GOOD_P == 1.0, 1.5, GOOD_P)), dict(p=np.where(GOOD_P == 1.0, np.nan, GOOD_P)),
             dict(p=np.where(GOOD_P == 0.0, -0.1, GOOD_P)), dict(L=0, B=0, p=[1.5]), dict(edges=None), dict(E_edges=None),
             dict(edges=[1.0, 3.0, 2.0, 4.0]), dict(edges=[-1.0, 2.0, 2.5, 3.0]), dict(edges=[1.0, 2.0, 2.5, np.inf]),
             dict(edges=[1.0, 2.0, 2.5, 1e200]), dict(edges=[1.0, 1.0, 2.5, 3.0]), dict(E_edges=[1.0, 2.0, 1.5, 3.0]),
             dict(E_edges=[1.0, 1.5, np.nan, 3.0]), dict(E_edges=[1.0, 1.5, 2.0, np.inf]), dict(center=[0, np.nan, 0]),
             dict(center=[np.inf, 0, 0])]
