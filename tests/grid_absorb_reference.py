"""Scenes, tables, a plain loop and the comparison for the tests of GridAbsorptionStep (tests/test_grid_absorb_*.py).  Not a test
file: a helper they import.

``grid_absorb_loop`` is pcl_step_absorb_grid photon by photon, written from the text of include/physicl_hip.h alone: Python floats
(IEEE doubles, one rounding per operation), tests/scatter_layered_reference.py's Philox4x32-10 block on Python integers and its
linear walk through the edges where the library has a binary search.  The rule has no transcendental function, no division and no
square root, so the loop, light_grid._grid_absorb and the device agree bit for bit.  It does not import light.py or light_grid.py.

``scene(n, axes, edges, dtype)`` is tests/scatter_grid_reference.py's edge scene -- positions on the first, an inner and the last edge
and one ``dtype`` value outside either end, NaN positions, photons at rest (with -0.0), a NaN in v (moves), energies on band edges,
outside the bands and NaN -- with the marks this rule reads: every third slot has dv = 0, so there are moving photons that were
scattered and moving photons that were not, photons at rest with dv = 0 and photons at rest with dv != 0 (what the ground parks).
"""
import numpy as np

import scatter_grid_reference as G
from scatter_grid_reference import C, CENTER, COORD, E_EDGES, ID_BASE, SEED, closed_bin, grid_edges, philox, probabilities  # noqa: F401
from writer_reference import photons, same_bits, wide

WORDS = (27, 28)
TABLES = ("k", "omega0", "both")                                       # which tables a call gives
COUNTS = ("exposed", "interacted", "absorbed_path", "absorbed_hit")


def scene(n, axes, edges, dtype=np.float64, seed=3):
    s = G.scene(n, axes, edges, dtype, seed)
    s["dv"][np.arange(n) % 3 == 1] = 0.0
    return s


def tables(shape, which, kind="mixed"):
    """(p, omega0) of the given shape, None for a table ``which`` ("k", "omega0", "both") leaves out.  ``kind``: 0, 1 or "mixed" -- zeros,
    ones and values between them in about equal shares (two different drawings for the two tables)."""
    p = probabilities(shape, kind, seed=9) if which in ("k", "both") else None
    om = probabilities(shape, kind, seed=23) if which in ("omega0", "both") else None
    return p, om


def grid_absorb_loop(r, v, dv, E, photon, ids, p, omega0, axes, edges, center, E_edges, seed, n_pass, dtype=np.float64):
    """pcl_step_absorb_grid, photon by photon (the module's docstring).  The arguments and the dict of light_grid._grid_absorb."""
    r, v, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v, dv))
    n = len(v)
    cmp_edges = [[float(e) * float(e) for e in ed] if a == "r" else [float(e) for e in ed] for a, ed in zip(axes, edges)]
    Ee = None if E_edges is None else [float(e) for e in E_edges]
    shape = tuple(len(e) - 1 for e in edges) + (() if Ee is None else (len(Ee) - 1,))
    p, omega0 = (None if t is None else [float(x) for x in np.asarray(t, dtype=np.float64).reshape(-1)] for t in (p, omega0))
    cx = [float(x) for x in center]
    exposed, interacted, gone_path, gone_hit = (np.zeros(n, dtype=bool) for _ in range(4))
    cell = np.full(n, -1, dtype=np.int64)
    cells = [0] * int(np.prod(shape))
    for i in range(n):
        if not photon[i]:
            continue                                                   # never written
        v0, v1, v2 = (float(x) for x in v[i])
        if v0 == 0.0 and v1 == 0.0 and v2 == 0.0:                       # at rest (-0.0 == 0; a NaN moves)
            continue
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
        if g < 0:
            continue
        cell[i], exposed[i] = g, True
        if omega0 is not None:
            interacted[i] = bool(float(dv[i, 0]) != 0.0 or float(dv[i, 1]) != 0.0 or float(dv[i, 2]) != 0.0)
        if p is not None and p[g] > 0.0:
            gone_path[i] = philox(int(ids[i]), int(seed), int(n_pass), WORDS[0])[0] < p[g]
        if not gone_path[i] and omega0 is not None and interacted[i] and omega0[g] < 1.0:
            gone_hit[i] = not (philox(int(ids[i]), int(seed), int(n_pass), WORDS[1])[0] < omega0[g])
        if gone_path[i] or gone_hit[i]:
            v[i], dv[i] = 0.0, 0.0                                     # parked
            cells[g] += 1
    return {"v": v, "dv": dv, "exposed": exposed, "interacted": interacted, "absorbed_path": gone_path, "absorbed_hit": gone_hit,
            "absorbed": gone_path | gone_hit, "cell": cell, "absorbed_by_cell": np.array(cells, dtype=np.int64).reshape(shape)}


def outcomes(ref, v, dv, photon, which):
    """How often each outcome the rule knows occurs: the population's kinds and what became of them."""
    photon = np.asarray(photon, dtype=bool)
    rest = (v[:, 0] == 0) & (v[:, 1] == 0) & (v[:, 2] == 0) & photon
    marked = (dv != 0).any(axis=1)
    counts = {"plain Object": int((~photon).sum()), "at rest, dv = 0": int((rest & ~marked).sum()), "at rest, dv != 0": int((rest & marked).sum()),
              "moving, no cell": int((photon & ~rest & ~ref["exposed"]).sum()), "moving, scattered": int((ref["exposed"] & marked).sum()),
              "moving, dv = 0": int((ref["exposed"] & ~marked).sum()), "exposed, survives": int((ref["exposed"] & ~ref["absorbed"]).sum())}
    if which in ("k", "both"):
        counts["absorbed along the path"] = int(ref["absorbed_path"].sum())
    if which in ("omega0", "both"):
        counts["absorbed at the interaction"] = int(ref["absorbed_hit"].sum())
        counts["interacted, survives"] = int((ref["interacted"] & ~ref["absorbed"]).sum())
    return counts


def assert_every_outcome(ref, v, dv, photon, which, what, objects=True):
    counts = outcomes(ref, v, dv, photon, which)
    need = [k for k in counts if objects or k != "plain Object"]
    assert all(counts[k] > 0 for k in need), (what, counts)
    assert not (ref["absorbed_path"] & ref["absorbed_hit"]).any() and not (ref["absorbed"] & ~ref["exposed"]).any(), what
    assert not (ref["absorbed_hit"] & ~ref["interacted"]).any() and (which != "k" or not ref["interacted"].any()), what
    return counts


# ------------------------------------------------------------------------------------------------ a sweep against the restatement
def check_grid_absorb(before, after, answer, p, omega0, axes, edges, center, E_edges, seed, n_pass, what, restate=None):
    """A state downloaded before the sweep, the state downloaded after it and the sweep's answer ``(counts[4], absorbed_by_cell)``
    against the restatement (``restate``: light_grid._grid_absorb by default; the loop may be given).  Without tolerance: the four
    counts, every cell, every row of v and dv (the absorbed rows are +0.0, everybody else keeps every bit), r, dr, E, ids and kinds.
    Returns the restatement's dict."""
    if restate is None:
        from physicl_amd import light_grid
        restate = light_grid._grid_absorb
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    ref = restate(b["r"], b["v"], b["dv"], np.asarray(before["E"]).astype(np.float64), photons(before), before["id"], p, omega0, axes, edges,
                  center, E_edges, seed, n_pass, T)
    for f in set(before) - {"r", "v", "dr", "dv", "count"}:              # E, ids, kinds
        assert same_bits(before[f], after[f]), (what, f)
    assert before.get("count") == after.get("count") and len(before["E"]) == len(after["E"]), what
    for f in ("r", "dr"):
        assert same_bits(a[f], b[f]), (what, f)
    counts, cells = answer
    want = [int(ref[k].sum()) for k in COUNTS]
    print("%s: exposed %d, interacted %d, absorbed %d + %d of %d" % ((what,) + tuple(want) + (len(ref["cell"]),)))
    assert [int(x) for x in counts] == want, (what, [int(x) for x in counts], want)
    assert np.asarray(cells).shape == ref["absorbed_by_cell"].shape and np.array_equal(np.asarray(cells), ref["absorbed_by_cell"]), what
    assert int(np.asarray(cells).sum()) == want[2] + want[3] <= want[0], what
    gone = ref["absorbed"]
    for f in ("v", "dv"):
        assert same_bits(a[f], ref[f]), (what, f)                       # every row: the restatement's state, bit for bit
        assert same_bits(a[f][~gone], b[f][~gone]), (what, f)           # who is not absorbed keeps every bit
        assert same_bits(a[f][gone], np.zeros((int(gone.sum()), 3))), (what, f)            # parked: +0.0
    return ref


# ------------------------------------------------------------------------------------------------ the ABI, by hand
ABI_AXES, ABI_BINS = ("x", "y", "z"), (2, 2, 2)
GOOD_P, GOOD_OM = tables((2, 2, 2, 3), "both")


def abi_args(**kw):
    """The arguments of a good call (behind the context) -- a 2 x 2 x 2 grid by 3 bands with both tables --, and what ``kw`` changes
    of them: n_axes, coords, n_bins, edges, center, B, E_edges, p, omega0, counts, cells."""
    edges = np.concatenate(grid_edges(ABI_AXES, ABI_BINS))
    a = dict(n_axes=3, coords=[0, 1, 2], n_bins=list(ABI_BINS), edges=edges, center=CENTER, B=3, E_edges=E_EDGES, p=GOOD_P, omega0=GOOD_OM,
             counts=np.full(6, -7, dtype=np.int64), cells=np.full(64, -7, dtype=np.int64))
    a.update(kw)
    ints = [None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.int32) for k in ("coords", "n_bins")]
    dbl = [None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.float64) for k in ("edges", "center", "E_edges", "p", "omega0")]
    ptr = lambda x: None if x is None else x.ctypes.data                                                    # noqa: E731
    return (ints, dbl), (int(a["n_axes"]), ptr(ints[0]), ptr(ints[1]), ptr(dbl[0]), ptr(dbl[1]), int(a["B"]), ptr(dbl[2]), ptr(dbl[3]),
                         ptr(dbl[4]), 1, 1, ptr(a["counts"]), ptr(a["cells"])), (a["counts"], a["cells"])


_BIG = dict(n_axes=3, coords=[0, 1, 2], n_bins=[1024, 1024, 2], edges=np.concatenate([np.arange(1025.0), np.arange(1025.0), np.arange(3.0)]),
            B=0, E_edges=None, p=np.zeros(8), omega0=None)            # 2^21 cells: refused before a table is read
BAD_CALLS = [dict(p=None, omega0=None), dict(counts=None), dict(cells=None), dict(coords=None), dict(n_bins=None), dict(edges=None),
             dict(n_axes=0), dict(n_axes=4), dict(coords=[0, 0, 2]), dict(coords=[0, 1, 4]), dict(coords=[-1, 1, 2]), dict(n_bins=[2, 0, 2]),
             dict(n_bins=[2, 1025, 2]), _BIG, dict(B=-1), dict(B=1025), dict(E_edges=None),
             dict(p=np.where(GOOD_P == 1.0, 1.5, GOOD_P)), dict(p=np.where(GOOD_P == 1.0, np.nan, GOOD_P)),
             dict(p=np.where(GOOD_P == 0.0, -0.1, GOOD_P)), dict(omega0=np.where(GOOD_OM == 1.0, 1.5, GOOD_OM)),
             dict(omega0=np.where(GOOD_OM == 1.0, np.nan, GOOD_OM)), dict(omega0=np.where(GOOD_OM == 0.0, -0.1, GOOD_OM)),
             dict(p=None, omega0=np.where(GOOD_OM == 0.0, -0.1, GOOD_OM)), dict(p=np.where(GOOD_P == 1.0, np.nan, GOOD_P), omega0=None),
             dict(edges=[-2.0, 0.0, 2.0, -2.0, 2.0, 0.0, -2.0, 0.0, 2.0]), dict(edges=[-2.0, 0.0, np.inf, -2.0, 0.0, 2.0, -2.0, 0.0, 2.0]),
             dict(coords=[0, 1, 3], edges=[-2.0, 0.0, 2.0, -2.0, 0.0, 2.0, -1.0, 0.0, 2.0]),     # a negative radius
             dict(E_edges=[1.0, 2.0, 1.5, 3.0]), dict(E_edges=[1.0, 1.5, np.nan, 3.0]), dict(center=[0, np.nan, 0])]
