"""A second restatement, the scenes and the comparison for the tests of RefractiveSurfaceStep (tests/test_refract_cpu.py and the GPU
tests).  Not a test file: a helper they import.

``refract_surface_loop`` is pcl_step_refract_surface once more, a plain loop over the photons in float64 scalars, written from the
rule in include/physicl_hip.h; it shares nothing with the vectorised physicl_amd.light._refract_surface but the Philox block.

The scene (``scene``), slot i, a sphere of radius 1 about CENTER, n_inside = 1.5:
    i % 3 == 0   crosses inward:  a hit point on the sphere, a direction into it, the move cut there at a random share
    i % 3 == 1   crosses outward: the same with a direction out of it -- beyond the critical angle for two in five of them
                 (a path so flat that the move's other end lies beyond the sphere's other side crosses nothing, or twice)
    i % 3 == 2   does not cross: somewhere between 0.2 and 2.2 radii, a short move
and, written over these in this order (all exact in float32 as well):
    i % 62 == 16   exactly on the sphere BEFORE the move, inside after it: outside counts, so it crosses inward with t = 0
    i % 66 == 18   inside before, exactly on the sphere AFTER the move: it crosses outward with t = 1
    i % 70 == 20   outside before, exactly on the sphere after: on the sphere is outside, no crossing
    i % 74 == 22   on the sphere, dr = 0 (a == 0): no crossing
    i % 58 == 14   dr infinite: q_prev is infinite, no crossing either way
    i % 34 == 8    a NaN in r;  i % 38 == 10   a NaN in dr: no crossing
    i % 46 == 12   a NaN in v (only with ``nan_v``): it crosses as it would, dv is NaN
    i % 17 == 0    a plain Object: never crosses
Ids are scrambled.
"""
import ctypes

import numpy as np

from physicl_amd import light
from writer_reference import same_bits

C = 299792458.0
SEED = 0x5EED5A7F
ID_BASE = 7_000_000_001
CENTER = np.array([0.5, -0.25, 0.125])               # exact in float32, and so is CENTER + (k/4, 0, 0)
RADIUS, N_IN, N_OUT = 1.0, 1.5, 1.0
FIELDS = ("r", "v", "dr", "dv")
COUNTS = ("in_refracted", "in_reflected", "out_refracted", "out_reflected", "out_total", "overshot")
GLASS = dict(radius=RADIUS, center=CENTER, n_inside=N_IN, n_outside=N_OUT, fresnel=True)
GLASS_PLAIN = dict(GLASS, fresnel=False)
BUBBLE = dict(GLASS, n_inside=1.0, n_outside=1.5)    # total reflection on the way in


def unit(x):
    return x / np.sqrt((x * x).sum(axis=1))[:, None]


def crossing(n, rng, sign):
    """(r - CENTER, dr) of ``n`` moves that meet the unit sphere going inward (sign -1) or outward (+1)."""
    x = unit(rng.normal(size=(n, 3)))
    tang = unit(np.cross(x, rng.normal(size=(n, 3))))
    cosine = rng.uniform(0.02, 1.0, size=n)
    way = sign * cosine[:, None] * x + np.sqrt(1.0 - cosine ** 2)[:, None] * tang
    length, share = rng.uniform(0.02, 0.3, size=n), rng.uniform(0.05, 0.95, size=n)
    return x + ((1.0 - share) * length)[:, None] * way, length[:, None] * way


def scene(n, dtype=np.float64, seed=1, nan_v=True, everybody=False, nobody=False):
    """{"r", "v", "dr", "dv": (n, 3)} of float64 arrays that hold ``dtype`` values, ``photon`` and ``id``, laid out as the module's
    docstring says.  ``everybody``: only inward and outward crossings, no special slots; ``nobody``: only slots that do not cross."""
    rng = np.random.RandomState(seed + n)
    i = np.arange(n)
    d_in, m_in = crossing(n, rng, -1.0)
    d_out, m_out = crossing(n, rng, +1.0)
    m_far = rng.uniform(0.0, 0.05, size=n)[:, None] * unit(rng.normal(size=(n, 3)))
    rad = rng.uniform(0.2, 2.2, size=n)
    rad[np.abs(rad - 1.0) < 0.06] += 0.5
    d_far = rad[:, None] * unit(rng.normal(size=(n, 3)))
    kind = i % 2 if everybody else np.full(n, 2) if nobody else i % 3
    d = np.where((kind == 0)[:, None], d_in, np.where((kind == 1)[:, None], d_out, d_far))
    m = np.where((kind == 0)[:, None], m_in, np.where((kind == 1)[:, None], m_out, m_far))
    v = C * unit(np.where((m * m).sum(axis=1)[:, None] > 0, m, 1.0))
    photon = np.ones(n, dtype=bool)
    if not everybody and not nobody:
        for mod, k, dk, mk in ((62, 16, 0.75, -0.25), (66, 18, 1.0, 0.25), (70, 20, 1.0, -0.25), (74, 22, 1.0, 0.0)):
            d[i % mod == k], m[i % mod == k] = [dk, 0.0, 0.0], [mk, 0.0, 0.0]
        m[i % 58 == 14, 0] = np.inf
        d[i % 34 == 8, 2] = np.nan
        m[i % 38 == 10, 1] = np.nan
        if nan_v:
            v[i % 46 == 12, 1] = np.nan
        photon = i % 17 != 0
    state = {"r": CENTER + d, "v": v, "dr": m, "dv": rng.normal(size=(n, 3))}
    with np.errstate(over="ignore"):
        state = {k: a.astype(dtype).astype(np.float64) for k, a in state.items()}
    state["photon"] = photon
    state["id"] = ID_BASE + np.random.RandomState(5).permutation(n).astype(np.int64)
    return state


def _fmax(a, b):                                      # C's fmax / fmin: a NaN is ignored
    return b if a != a else a if b != b else max(a, b)


def _fmin(a, b):
    return b if a != a else a if b != b else min(a, b)


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def refract_surface_loop(r, dr, v, photon, ids, radius, center, n_inside, n_outside, fresnel, c, seed, n_pass, dtype=np.float64):
    """pcl_step_refract_surface, photon by photon (the module's docstring).  The arguments of light._refract_surface; its dict's ``r,
    v, dr, dv``, the masks and ``counts``."""
    f8 = np.float64
    r, dr, v = (np.array(a, dtype=f8).reshape(-1, 3) for a in (r, dr, v))
    n = len(r)
    dv = np.full((n, 3), np.nan)
    cx = [f8(x) for x in center]
    c, R2 = f8(c), f8(radius) * f8(radius)
    eta_in, eta_out = f8(n_outside) / f8(n_inside), f8(n_inside) / f8(n_outside)
    store = (lambda x: f8(np.float32(x))) if dtype is np.float32 else f8
    draw = light._philox_block(ids, seed, n_pass, 21)[0]
    masks = {k: np.zeros(n, dtype=bool) for k in ("inward", "outward", "crossed", "refracted", "reflected", "total", "overshot")}
    counts = np.zeros(6, dtype=np.int64)
    zero, one, two, half, inf = f8(0.0), f8(1.0), f8(2.0), f8(0.5), f8(np.inf)
    with np.errstate(all="ignore"):
        for i in range(n):
            d = [f8(r[i, k]) - cx[k] for k in range(3)]
            m = [f8(dr[i, k]) for k in range(3)]
            p = [d[k] - m[k] for k in range(3)]
            q_now, q_prev = _dot(d, d), _dot(p, p)
            inward = bool(q_now < R2 and R2 <= q_prev and q_prev < inf)
            outward = bool(q_prev < R2 and R2 <= q_now and q_now < inf)
            if not photon[i] or not (inward or outward):
                continue
            a, b, cq = _dot(m, m), _dot(p, m), q_prev - R2
            sq = np.sqrt(_fmax(b * b - a * cq, zero))
            if inward:
                t = cq / (sq - b)
            else:
                t = (zero - cq) / (sq + b) if b > zero else (sq - b) / a
                t = _fmin(_fmax(t, zero), one)
            x = [p[k] + t * m[k] for k in range(3)]
            xn, sa = np.sqrt(_dot(x, x)), np.sqrt(a)
            nrm = [x[k] / xn for k in range(3)]
            mh = [m[k] / sa for k in range(3)]
            w = (one - t) * sa
            N = nrm if inward else [-nrm[k] for k in range(3)]
            eta = eta_in if inward else eta_out
            ci = _fmax(zero - _dot(mh, N), zero)
            kk = one - (eta * eta) * (one - ci * ci)
            total = bool(kk < zero)
            drawn = False
            if not total:
                ct = ci if eta == one else np.sqrt(kk)
                ec, ect = eta * ci, eta * ct
                rs, rp = (ec - ct) / (ec + ct), (ci - ect) / (ci + ect)
                F = (rs * rs + rp * rp) * half
                if fresnel and F > zero:
                    drawn = bool(f8(draw[i]) < F)
            if total or drawn:
                new = [mh[k] + (two * ci) * N[k] for k in range(3)]
            else:
                new = [eta * mh[k] + (ec - ct) * N[k] for k in range(3)]
            y = [zero] * 3
            for k in range(3):
                vk, drk = c * new[k], w * new[k]
                y[k] = x[k] + drk
                dv[i, k] = store(vk - f8(v[i, k]))
                r[i, k], v[i, k], dr[i, k] = store(cx[k] + y[k]), store(vk), store(drk)
            q_new = _dot(y, y)
            inside = inward != (total or drawn)
            over = bool(q_new >= R2) if inside else bool(q_new < R2)
            masks["inward"][i], masks["outward"][i], masks["crossed"][i] = inward, outward, True
            masks["refracted"][i], masks["reflected"][i], masks["total"][i], masks["overshot"][i] = not (total or drawn), drawn, total, over
            cell = (1 if total or drawn else 0) if inward else (4 if total else 3 if drawn else 2)
            counts[cell] += 1
            counts[5] += over
    out = {"r": r, "v": v, "dr": dr, "dv": dv, "counts": counts}
    out.update(masks)
    return out


def same_answer(ref, loop):
    """The loop's answer and the restatement's, bit for bit (NaN rows of dv included)."""
    return all(same_bits(ref[k], loop[k]) for k in loop)


def refract(fn, state, cfg, n_pass=1, dtype=np.float64, seed=SEED, c=C, **kw):
    a = dict(photon=state["photon"], ids=state["id"])
    a.update(kw)
    return fn(state["r"], state["dr"], state["v"], a["photon"], a["ids"], cfg["radius"], cfg["center"], cfg["n_inside"], cfg["n_outside"],
              cfg["fresnel"], c, seed, n_pass, dtype)


# ------------------------------------------------------------------------------------------------ a sweep against the restatement
def wide(s):
    return {f: (np.stack(s[f], 1) if isinstance(s[f], (list, tuple)) else np.asarray(s[f])).astype(np.float64) for f in FIELDS}


def check_refract(before, after, counts, cfg, seed, n_pass, what, photon=None, c=C):
    """A state downloaded before the sweep, the state downloaded after it and the sweep's six counts against
    light._refract_surface, without a tolerance: r, v, dr and dv of EVERY slot bit for bit (a slot that does not cross keeps what it
    had), E and the ids untouched, the counts equal.  Returns the restatement's dict."""
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    n = len(before["E"])
    photon = np.ones(n, dtype=bool) if photon is None else photon
    ref = light._refract_surface(b["r"], b["dr"], b["v"], photon, before["id"], cfg["radius"], cfg["center"], cfg["n_inside"],
                                 cfg["n_outside"], cfg["fresnel"], c, seed, n_pass, T)
    got = np.asarray(counts, dtype=np.int64)
    print("%s: %s of %d" % (what, dict(zip(COUNTS, ref["counts"].tolist())), n))
    assert got.tolist() == ref["counts"].tolist(), what
    assert np.array_equal(after["id"], before["id"]) and same_bits(np.asarray(after["E"]), np.asarray(before["E"])), what
    hit = ref["crossed"]
    want = dict(ref, dv=np.where(hit[:, None], ref["dv"], b["dv"]))
    for f in FIELDS:
        assert same_bits(a[f], want[f]), (what, f, np.flatnonzero((a[f] != want[f]).any(axis=1))[:5])
    return ref


# ------------------------------------------------------------------------------------------------ the ABI, by hand
def abi_args(**kw):
    """(what must stay alive, the arguments behind the handle, counts) of a good call of pcl_step_refract_surface, and what ``kw``
    changes of them (None: NULL)."""
    a = dict(radius=RADIUS, center=CENTER, n_inside=N_IN, n_outside=N_OUT, fresnel=1, c=C, counts=np.full(8, -7, dtype=np.int64))
    a.update(kw)
    center = None if a["center"] is None else np.ascontiguousarray(a["center"], dtype=np.float64)
    counts = a["counts"]
    return [center], (ctypes.c_double(a["radius"]), None if center is None else center.ctypes.data, ctypes.c_double(a["n_inside"]),
                      ctypes.c_double(a["n_outside"]), int(a["fresnel"]), ctypes.c_double(a["c"]), 1, 1,
                      None if counts is None else counts.ctypes.data), counts


BAD_CALLS = [dict(counts=None), dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(radius=1e200),
             dict(n_inside=0.0), dict(n_inside=-1.5), dict(n_inside=np.nan), dict(n_inside=np.inf),
             dict(n_outside=0.0), dict(n_outside=-1.0), dict(n_outside=np.nan), dict(n_outside=np.inf),
             dict(center=[0.0, np.nan, 0.0]), dict(center=[np.inf, 0.0, 0.0]), dict(c=np.inf), dict(c=np.nan)]
# the same for the constructor: what it is given, and the word its message carries
BAD_STEPS = [(dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=np.nan), "radius"), (dict(radius=np.inf), "radius"),
             (dict(radius=1e200), "radius"), (dict(radius="wide"), "radius"),
             (dict(n_inside=0.0), "n_inside"), (dict(n_inside=-1.5), "n_inside"), (dict(n_inside=np.nan), "n_inside"),
             (dict(n_inside=np.inf), "n_inside"), (dict(n_inside="glass"), "n_inside"),
             (dict(n_outside=0.0), "n_outside"), (dict(n_outside=-1.0), "n_outside"), (dict(n_outside=np.nan), "n_outside"),
             (dict(n_outside=np.inf), "n_outside"), (dict(center=(0, 0)), "center"), (dict(center=(0, np.nan, 0)), "center"),
             (dict(center=(np.inf, 0, 0)), "center")]
