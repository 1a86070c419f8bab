"""The walls of a box (pcl_step_box_walls) restated independently, and the scene its tests share.

``box_walls_loop`` is a per-photon loop on Python floats and ints, written from the rule as include/physicl_hip.h states it and not
from light._box_walls: Python's ``+ - * /`` on floats are IEEE-754 double operations rounded once, ``floor`` is taken on the float,
and min / max are C's fmin / fmax written out (of a NaN and a number: the number).  numpy only carries the arrays and rounds what an
fp32 store holds (``numpy.float32``).

``scene(n, lo, hi, dtype)`` is the edge scene, the same for every choice of walls: per axis positions exactly on ``lo`` and on ``hi``,
one ulp (of the store's dtype) on either side of each, 1, 2 and 3 box lengths outside on both sides (about the middle, and exactly on
the images of the walls), NaN and +-inf; photons at rest outside; ``v = (-0.0, 0, 0)`` outside; a NaN velocity outside; plain Objects
among the photons; photons outside on two and on three axes at once (with walls ("periodic", "mirror", "open") that is a photon
outside on an open and a periodic axis, with "open" one outside on two open axes); and a bulk of which 60 % stand inside and 40 % up
to five box lengths outside.  ``BOXES``: the box [-1, 1]^3 and the box R .. R + 40 km of an atmosphere's cloud field.

``check_box_walls(before, after, counts, ...)`` holds two snapshots and a call's answer to a restatement bit for bit, with no
tolerance anywhere; ``assert_every_outcome`` that a case met every outcome the walls in play have.
"""
import math

import numpy as np

import writer_reference as W
from writer_reference import same_bits

C = W.C
R_EARTH = 6371e3
BOXES = {"unit": ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), "high": ((R_EARTH,) * 3, (R_EARTH + 40e3,) * 3)}
WALLS = {"periodic": ("periodic",) * 3, "mirror": ("mirror",) * 3, "open": ("open",) * 3, "mixed": ("periodic", "mirror", "open")}
N_EDGE = 3001                                        # not a multiple of 64, 256 or 2048; the scene straddles slot 2048
MODE_CODES = {None: 0, "periodic": 1, "mirror": 2, "open": 3}
FIELDS = ("r", "v", "dr", "dv")


# ------------------------------------------------------------------------------------------------ the loop
def _fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def _fmin(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def _floor(q):
    return float(math.floor(q)) if math.isfinite(q) else q


def box_walls_loop(r, v, dr, dv, photon, modes, lo, hi, dtype=np.float64):
    """The header's rule, photon by photon.  The keys of light._box_walls' dict that the tests read."""
    stored = (lambda y: float(np.float32(y))) if np.dtype(dtype) == np.float32 else float
    r, v, dr, dv = (np.array(a, dtype=np.float64).reshape(-1, 3).tolist() for a in (r, v, dr, dv))
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]
    cnt = len(r)
    counts = [0] * 8
    moving, parked, folded, multi = ([False] * cnt for _ in range(4))
    for i in range(cnt):
        if not photon[i]:
            continue
        if v[i][0] == 0 and v[i][1] == 0 and v[i][2] == 0:             # -0.0 == 0; a NaN compares unequal: it moves
            continue
        moving[i] = True
        counts[0] += 1
        side = [-1, -1, -1]
        for a in range(3):
            if modes[a] is None:
                continue
            x = r[i][a]
            if not math.isfinite(x):
                continue
            below = x < lo[a]
            above = x >= hi[a] if modes[a] == "periodic" else x > hi[a]
            if below or above:
                side[a] = 0 if below else 1
        open_axes = [a for a in range(3) if modes[a] == "open" and side[a] >= 0]
        if open_axes:
            a = open_axes[0]
            counts[2 + 2 * a + side[a]] += 1
            v[i], dv[i] = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
            parked[i] = True
            continue
        for a in range(3):
            if side[a] < 0:
                continue
            folded[i] = True
            L = hi[a] - lo[a]
            s = r[i][a] - lo[a]
            n = _floor(s / L)
            f = _fmin(_fmax(s - n * L, 0.0), L)
            counts[2 + 2 * a + side[a]] += 1
            if n < -1 or n > 1:
                multi[i] = True
            if modes[a] == "periodic":
                y = lo[a] + f
                if not y < hi[a]:
                    y = lo[a]
                r[i][a] = stored(y)
            else:
                h = n * 0.5
                odd = _floor(h) != h
                y = hi[a] - f if odd else lo[a] + f
                r[i][a] = stored(_fmin(_fmax(y, lo[a]), hi[a]))
                if odd:
                    v[i][a], dv[i][a], dr[i][a] = -v[i][a], -dv[i][a], -dr[i][a]
        if multi[i]:
            counts[1] += 1
    out = {f: np.array(x, dtype=np.float64).reshape(-1, 3) for f, x in (("r", r), ("v", v), ("dr", dr), ("dv", dv))}
    for name, mask in (("moving", moving), ("parked", parked), ("folded", folded), ("multi", multi)):
        out[name] = np.array(mask, dtype=bool)
    out["written"] = out["parked"] | out["folded"]
    out["counts"] = np.array(counts, dtype=np.int64)
    out["crossed"] = out["counts"][2:].reshape(3, 2)
    return out


# ------------------------------------------------------------------------------------------------ the scene
def edge_values(lo, hi, T):
    """The positions every axis holds, as values of the store's dtype ``T``."""
    lo_t, hi_t = T(lo), T(hi)
    L, mid = float(hi) - float(lo), 0.5 * (float(hi) + float(lo))
    vals = [lo_t, hi_t, np.nextafter(lo_t, T(-np.inf)), np.nextafter(lo_t, T(np.inf)), np.nextafter(hi_t, T(-np.inf)),
            np.nextafter(hi_t, T(np.inf))]
    for k in (1, 2, 3):
        vals += [T(mid - k * L), T(mid + k * L), T(lo - k * L), T(hi + k * L), T(mid - (k + 0.3) * L), T(mid + (k - 0.3) * L)]
    vals += [T(np.nan), T(np.inf), T(-np.inf)]
    return np.array(vals, dtype=T)


def scene(n, lo, hi, dtype=np.float64, seed=3):
    """{"r", "v", "dr", "dv": (n, 3) float64 arrays of values the dtype holds; "E"; "photon": bool}"""
    T = np.dtype(dtype).type
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    L = hi - lo
    rng = np.random.RandomState(seed)
    j = np.arange(n)
    u = rng.uniform(size=(n, 3))
    far = rng.uniform(size=(n, 3)) < 0.4 / 1.5                          # per axis: some 40 % of the bulk are outside on some axis
    u = np.where(far, rng.uniform(-5.0, 6.0, size=(n, 3)), u)
    r = (lo + L * u).astype(T)
    d = rng.normal(size=(n, 3))
    v = (C * d / np.sqrt((d * d).sum(axis=1))[:, None]).astype(T)
    dr = (L * 0.01 * rng.normal(size=(n, 3))).astype(T)
    dv = rng.normal(size=(n, 3)).astype(T)
    inside = (lo + L * rng.uniform(0.05, 0.95, size=(n, 3))).astype(T)
    for a in range(3):                                                 # the edge values: every fifth slot, axis by axis, the others inside
        vals = edge_values(lo[a], hi[a], T)
        mine = np.flatnonzero((j % 5 == 0) & ((j // 5) % 3 == a))
        r[mine] = inside[mine]
        r[mine, a] = vals[(mine // 15) % len(vals)]
    out2 = np.flatnonzero(j % 41 == 6)                                  # outside on two axes (which two: in turn), and on all three
    for k, i in enumerate(out2):
        a, b = [(0, 2), (0, 1), (1, 2)][k % 3]
        r[i] = inside[i]
        r[i, a] = T(hi[a] + 0.5 * L[a]) if k % 2 else T(lo[a] - 0.25 * L[a])
        r[i, b] = T(lo[b] - 0.5 * L[b]) if k % 4 < 2 else T(hi[b] + 1.75 * L[b])
    out3 = np.flatnonzero(j % 97 == 8)
    r[out3] = (hi + L * 0.5).astype(T)
    rest = np.flatnonzero(j % 37 == 1)                                  # at rest outside; -0.0 counts as 0
    r[rest] = (lo - L * 1.5).astype(T)
    v[rest] = 0.0
    v[rest[::2], 0] = -0.0
    nan_v = np.flatnonzero(j % 37 == 3)                                 # a NaN velocity moves
    r[nan_v] = (hi + L * 0.25).astype(T)
    v[nan_v] = [np.nan, 0.0, 0.0]
    photon = j % 11 != 4                                                # plain Objects among the photons, inside and outside
    E = np.linspace(1.0, 3.0, n).astype(T)
    return {"r": r.astype(np.float64), "v": v.astype(np.float64), "dr": dr.astype(np.float64), "dv": dv.astype(np.float64),
            "E": E.astype(np.float64), "photon": photon}


def upload_state(state, kind_object=W.KIND_OBJECT, kind_photon=W.KIND_PHOTON):
    """(the dict ``Device.upload_state`` takes, the kinds)"""
    kind = np.where(state["photon"], kind_photon, kind_object).astype(np.uint8)
    return {f: state[f] for f in FIELDS + ("E",)}, kind


# ------------------------------------------------------------------------------------------------ the checks
def check_box_walls(before, after, counts, modes, lo, hi, what, restate=box_walls_loop):
    """Two states (snapshots or probed states) and the call's eight counts against a restatement of ``before``: bit for bit."""
    b, a = W.wide(before), W.wide(after)
    T = np.asarray(before["E"]).dtype.type
    ref = restate(b["r"], b["v"], b["dr"], b["dv"], W.photons(before), modes, lo, hi, dtype=T)
    assert np.asarray(counts).tolist() == np.asarray(ref["counts"]).tolist(), (what, np.asarray(counts).tolist(), ref["counts"].tolist())
    for f in FIELDS:
        if not same_bits(a[f], ref[f]):
            bad = np.flatnonzero((a[f].view(np.uint64) != ref[f].view(np.uint64)).any(axis=1))
            raise AssertionError("%s: %s differs in %d slots, first %d: before %r device %r restatement %r" % (
                what, f, len(bad), bad[0], b[f][bad[0]].tolist(), a[f][bad[0]].tolist(), ref[f][bad[0]].tolist()))
    still = ~ref["written"]                                            # a photon that crosses nothing is not written at all
    for f in FIELDS:
        assert same_bits(a[f][still], b[f][still]), (what, f)
    for f in set(before) - set(FIELDS) - {"count"}:                     # E, ids and kinds are never written
        assert same_bits(np.asarray(before[f]), np.asarray(after[f])), (what, f)
    return ref


def assert_every_outcome(ref, modes, what):
    """The case met every outcome of the walls in play."""
    crossed, photon_moving = np.asarray(ref["crossed"]), int(ref["counts"][0])
    assert 0 < photon_moving < len(ref["moving"]), what
    for a, m in enumerate(modes):
        assert (crossed[a] > 0).all() if m is not None else not crossed[a].any(), (what, a, crossed.tolist())
    if "open" in modes:
        assert ref["parked"].any(), what
    if set(modes) & {"periodic", "mirror"}:
        assert ref["folded"].any() and ref["multi"].any() and (ref["folded"] & ~ref["multi"]).any(), what
    else:
        assert not ref["folded"].any() and not ref["multi"].any(), what
    assert (ref["moving"] & ~ref["written"]).any(), what


# ------------------------------------------------------------------------------------------------ the ABI by hand
def abi_args(modes=(1, 2, 3), lo=(-1.0, -1.0, -1.0), hi=(1.0, 1.0, 1.0), null=None):
    """(what keeps the arrays alive, the arguments behind the handle, the counts' array -- ten cells of -7, or None)"""
    md, lo, hi = np.array(modes, dtype=np.int32), np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
    counts = np.full(10, -7, dtype=np.int64)
    ptr = lambda name, x: None if null == name else x.ctypes.data      # noqa: E731
    return (md, lo, hi, counts), (ptr("modes", md), ptr("lo", lo), ptr("hi", hi), ptr("counts", counts)), (None if null == "counts" else counts)


NAN, INF = float("nan"), float("inf")
BAD_CALLS = [dict(null="modes"), dict(null="lo"), dict(null="hi"), dict(null="counts"), dict(modes=(0, 0, 0)), dict(modes=(4, 1, 1)),
             dict(modes=(1, -1, 1)), dict(modes=(0, 0, 7)), dict(lo=(NAN, -1.0, -1.0)), dict(hi=(1.0, INF, 1.0)), dict(lo=(-1.0, -1.0, -INF)),
             dict(lo=(1.0, -1.0, -1.0)), dict(lo=(2.0, -1.0, -1.0)), dict(lo=(-1e308,) * 3, hi=(1e308,) * 3),
             dict(modes=(0, 1, 0), lo=(0.0, 1.0, 0.0), hi=(1.0, 1.0, 1.0))]
# the bounds of an axis without a wall are not read
GOOD_CALLS = [dict(), dict(modes=(0, 1, 0), lo=(NAN, -1.0, INF), hi=(NAN, 1.0, -INF)), dict(modes=(3, 0, 0), lo=(0.0, 5.0, 5.0), hi=(1.0, 5.0, 4.0))]
