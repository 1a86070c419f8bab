"""A second restatement, the scenes and the comparison for the tests of SpectralSurfaceStep (tests/test_spectral_surface_cpu.py and
the GPU tests).  Not a test file: a helper they import.

``spectral_bounce_loop`` is pcl_step_ground_spectral once more, a plain loop over the photons in float64 scalars, written from the
rule in include/physicl_hip.h; it shares nothing with the vectorised physicl_amd.light._spectral_bounce but the Philox block.

The scene (``scene``): tests/surface_reference.py's cloud about CENTER -- every even slot's move ends inside the sphere of radius 10,
every odd slot's outside -- with an energy per slot, uniform between 1 and 3 (the range of ``fill_photons(.., 1.0, 3.0, ..)``), the
bands' edges inside that range (all exact in float32 as well), so that a tenth of the photons lie in no band on either side.
Written over these, slot i (``special=True``):
    i % 26 == 2    E exactly on the first edge: in band 0
    i % 26 == 4    E exactly on an inner edge (the second): in the band that starts there
    i % 26 == 6    E exactly on the last edge: in the last band, which is closed
    i % 26 == 8    E one step below the first edge;  i % 26 == 10   one step above the last: in no band
    i % 26 == 12   E is NaN: in no band
    i % 34 == 14   a NaN in r;  i % 38 == 16   a NaN in dr;  i % 58 == 18   dr infinite: not hit
    i % 17 == 0    a plain Object (where ``photon`` is used): never hit
Ids are scrambled (``id``) for the callers that use them.
"""
import ctypes
import math

import numpy as np

from physicl_amd import light
from surface_reference import C, CENTER, RADIUS, SEED, cloud
from writer_reference import DIR_ULP, lambertian_position_bound, same_bits, ulp, wide

ID_BASE = 7_000_000_001
FIELDS = ("r", "v", "dr", "dv")
COUNTS = ("reflected", "absorbed", "mirrored", "out_of_band")
W_MAX = 2.8 * RADIUS                                  # the longest move of surface_reference.cloud


def edges_of(B):
    """B + 1 edges from 1.25 to 2.75, exact in float32: the fill's energies reach from 1 to 3, an eighth falls outside on either side."""
    return 1.25 + 1.5 * np.arange(B + 1) / B if B in (1, 3, 1024) else np.linspace(1.25, 2.75, B + 1)


def tables_of(B, seed=3):
    """(albedo [B], specular [B]) with every kind of band: albedo and specular of exactly 0 and 1 among values strictly between."""
    if B == 1:
        return np.array([0.6]), np.array([0.5])
    if B == 3:
        return np.array([0.05, 1.0, 0.5]), np.array([1.0, 0.5, 0.0])
    rng = np.random.RandomState(seed)
    albedo, specular = rng.uniform(0.05, 0.95, size=B), rng.uniform(0.05, 0.95, size=B)
    k = np.arange(B)
    albedo[k % 7 == 1], albedo[k % 7 == 3] = 0.0, 1.0
    specular[k % 5 == 2], specular[k % 5 == 4] = 0.0, 1.0
    return albedo, specular


def config(B, **kw):
    albedo, specular = tables_of(B)
    cfg = dict(radius=RADIUS, center=CENTER, E_edges=edges_of(B), albedo=albedo, specular=specular)
    cfg.update(kw)
    return cfg


def scene(n, dtype=np.float64, seed=1, special=True, B=3):
    """{"r", "v", "dr", "dv": (n, 3), "E": (n,)} of float64 arrays that hold ``dtype`` values, ``photon`` and ``id``, laid out as the
    module's docstring says (``B``: the bands whose edges the special energies sit on)."""
    r, dr, v = cloud(n, seed=seed + n, dtype=dtype)
    rng = np.random.RandomState(seed + 7 * n)
    E = rng.uniform(1.0, 3.0, size=n)
    i = np.arange(n)
    if special:
        e = edges_of(B)
        up, down = dtype(np.inf), dtype(-np.inf)
        E[i % 26 == 2], E[i % 26 == 4], E[i % 26 == 6] = e[0], e[1], e[-1]
        E[i % 26 == 8], E[i % 26 == 10] = np.nextafter(dtype(e[0]), down), np.nextafter(dtype(e[-1]), up)
        E[i % 26 == 12] = np.nan
        r[i % 34 == 14, 2] = np.nan
        dr[i % 38 == 16, 1] = np.nan
        dr[i % 58 == 18, 0] = np.inf
    state = {"r": r, "v": v, "dr": dr, "dv": rng.normal(size=(n, 3)), "E": E}
    with np.errstate(over="ignore"):
        state = {k: a.astype(dtype).astype(np.float64) for k, a in state.items()}
    state["photon"] = i % 17 != 0 if special else np.ones(n, dtype=bool)
    state["id"] = ID_BASE + np.random.RandomState(5).permutation(n).astype(np.int64)
    return state


def _dot(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def spectral_bounce_loop(r, dr, v, E, photon, ids, radius, center, albedo, specular, E_edges, c, seed, n_pass, dtype=np.float64):
    """pcl_step_ground_spectral, photon by photon (the module's docstring).  The arguments of light._spectral_bounce; its dict's ``r, v,
    dr, dv``, the masks, ``band`` and the two rows by band."""
    f8 = np.float64
    r, dr, v = (np.array(a, dtype=f8).reshape(-1, 3) for a in (r, dr, v))
    n = len(r)
    dv = np.zeros((n, 3))
    E = np.asarray(E, dtype=f8).reshape(-1)
    edges = [f8(x) for x in E_edges]
    B = len(edges) - 1
    albedo, specular = [f8(x) for x in albedo], [f8(x) for x in specular]
    cx = [f8(x) for x in center]
    c, R2 = f8(c), f8(radius) * f8(radius)
    store = (lambda x: f8(np.float32(x))) if dtype is np.float32 else f8
    u_refl, u_mirror, (u_a, u_b) = light._philox_block(ids, seed, n_pass, 9)[0], light._philox_block(ids, seed, n_pass, 22)[0], \
        light._philox_block(ids, seed, n_pass, 8)
    masks = {k: np.zeros(n, dtype=bool) for k in ("hit", "reflected", "absorbed", "mirrored", "out_of_band")}
    band = np.full(n, -1, dtype=np.int64)
    by_band = np.zeros((2, B), dtype=np.int64)
    zero, one, two, inf = f8(0.0), f8(1.0), f8(2.0), f8(np.inf)
    with np.errstate(all="ignore"):
        for i in range(n):
            d = [f8(r[i, k]) - cx[k] for k in range(3)]
            m = [f8(dr[i, k]) for k in range(3)]
            p = [d[k] - m[k] for k in range(3)]
            q_now, q_prev = _dot(d, d), _dot(p, p)
            if not photon[i] or not (q_now < R2 and R2 <= q_prev and q_prev < inf):
                continue
            masks["hit"][i] = True
            e, b = f8(E[i]), -1
            if edges[0] <= e <= edges[B]:                              # (False for a NaN)
                b = B - 1
                while e < edges[b]:                                    # [E_b, E_(b+1)), the last one closed
                    b -= 1
            band[i] = b
            refl = mirror = False
            if b < 0:
                masks["out_of_band"][i] = True
            else:
                refl = True if albedo[b] == one else bool(f8(u_refl[i]) < albedo[b])
                if refl:
                    mirror = True if specular[b] == one else False if specular[b] == zero else bool(f8(u_mirror[i]) < specular[b])
                by_band[0 if refl else 1, b] += 1
            masks["reflected"][i], masks["absorbed"][i], masks["mirrored"][i] = refl, not refl, mirror
            a, bq, cq = _dot(m, m), _dot(p, m), q_prev - R2
            disc = bq * bq - a * cq
            disc = zero if disc != disc or disc < zero else disc       # C's fmax: a NaN is ignored
            t = cq / (np.sqrt(disc) - bq)
            x = [p[k] + t * m[k] for k in range(3)]
            vo = [f8(v[i, k]) for k in range(3)]
            if not refl:
                for k in range(3):
                    r[i, k], v[i, k], dr[i, k], dv[i, k] = store(cx[k] + x[k]), zero, store(x[k] - p[k]), store(zero - vo[k])
                continue
            xn, sa = np.sqrt(_dot(x, x)), np.sqrt(a)
            nrm = [x[k] / xn for k in range(3)]
            if mirror:
                mh = [m[k] / sa for k in range(3)]
                dn = _dot(mh, nrm)
                new = [mh[k] - (two * dn) * nrm[k] for k in range(3)]
            else:
                mu = np.sqrt(one - f8(u_a[i]))
                sg = f8(math.copysign(1.0, nrm[2]))
                aa = f8(-1.0) / (sg + nrm[2])
                bb, sn0 = (nrm[0] * nrm[1]) * aa, sg * nrm[0]
                e1 = [one + (sn0 * nrm[0]) * aa, sg * bb, -sn0]
                e2 = [bb, sg + (nrm[1] * nrm[1]) * aa, -nrm[1]]
                s = np.sqrt((one - mu) * (one + mu))
                psi = f8((f8(u_b[i]) * two) * f8(math.pi))
                sc, ss = s * np.cos(psi), s * np.sin(psi)
                new = [(sc * e1[k] + ss * e2[k]) + mu * nrm[k] for k in range(3)]
            w = (one - t) * sa
            for k in range(3):
                vk, drk = c * new[k], w * new[k]
                r[i, k], v[i, k], dr[i, k], dv[i, k] = store(cx[k] + (x[k] + drk)), store(vk), store(drk), store(vk - vo[k])
    out = {"r": r, "v": v, "dr": dr, "dv": dv, "band": band, "reflected_by_band": by_band[0], "absorbed_by_band": by_band[1]}
    out.update(masks)
    return out


def same_answer(ref, loop):
    """The loop's answer and the restatement's, bit for bit."""
    return all(same_bits(ref[k], loop[k]) for k in loop)


def bounce(fn, state, cfg, n_pass=1, dtype=np.float64, seed=SEED, c=C, **kw):
    a = dict(photon=state["photon"], ids=state["id"])
    a.update(kw)
    return fn(state["r"], state["dr"], state["v"], state["E"], a["photon"], a["ids"], cfg["radius"], cfg["center"], cfg["albedo"],
              cfg["specular"], cfg["E_edges"], c, seed, n_pass, dtype)


def outcomes(ref):
    """The shares of the five outcomes among all slots: diffuse, mirrored, absorbed in a band, out of band, not hit."""
    masks = {"diffuse": ref["reflected"] & ~ref["mirrored"], "mirrored": ref["mirrored"], "absorbed_in_band": ref["absorbed"] & ~ref["out_of_band"],
             "out_of_band": ref["out_of_band"], "not_hit": ~ref["hit"]}
    return {k: float(m.mean()) for k, m in masks.items()}


def assert_every_outcome(ref, what):
    """Somebody reflects diffusely, somebody is mirrored, somebody is absorbed in a band, somebody is out of band, somebody is not hit."""
    share = outcomes(ref)
    assert min(share.values()) > 0.0, (what, share)
    return share


# ------------------------------------------------------------------------------------------------ a sweep against the restatement
def check_spectral(before, after, answer, cfg, seed, n_pass, what, photon=None, c=C, w_max=W_MAX):
    """A state downloaded before the sweep, the state downloaded after it and the sweep's answer ``(counts, reflected_by_band,
    absorbed_by_band)`` against light._spectral_bounce.  Without a tolerance: the four counts and both rows by band; E, ids untouched;
    every row of a slot that is not hit; r, v, dr and dv of the parked and of the mirrored.  The lambertian lanes: the bounds of
    writer_reference.check_surface (DIR_ULP, lambertian_position_bound), no looser.  Returns the restatement's dict."""
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    n = len(before["E"])
    photon = np.ones(n, dtype=bool) if photon is None else photon
    center, radius = np.asarray(cfg["center"], dtype=np.float64), cfg["radius"]
    ref = light._spectral_bounce(b["r"], b["dr"], b["v"], np.asarray(before["E"]).astype(np.float64), photon, before["id"], radius, center,
                                 cfg["albedo"], cfg["specular"], cfg["E_edges"], c, seed, n_pass, T)
    counts, by_refl, by_gone = answer
    want = [int(ref[k].sum()) for k in COUNTS]
    print("%s: %s of %d" % (what, dict(zip(COUNTS, want)), n))
    assert [int(x) for x in counts] == want, what
    assert np.asarray(by_refl).tolist() == ref["reflected_by_band"].tolist(), what
    assert np.asarray(by_gone).tolist() == ref["absorbed_by_band"].tolist(), what
    assert np.array_equal(after["id"], before["id"]) and same_bits(np.asarray(after["E"]), np.asarray(before["E"])), what
    hit, diffuse = ref["hit"], ref["reflected"] & ~ref["mirrored"]
    for f in FIELDS:                                                   # untouched: bit-identical, dv included
        assert same_bits(a[f][~hit], b[f][~hit]), (what, f)
    exact = hit & ~diffuse                                             # parked (out of band among them) and mirrored
    for f in FIELDS:
        assert same_bits(a[f][exact], ref[f][exact]), (what, f, np.flatnonzero(exact & (a[f] != ref[f]).any(axis=1))[:5])
    if diffuse.any():
        mag = float(np.max(np.abs(center))) + radius + w_max
        pos = lambertian_position_bound(w_max, mag, c)
        if T is np.float64:
            v_unit, v_bound, r_bound = ulp(c), DIR_ULP, pos
        else:
            v_unit, v_bound, r_bound = ulp(c, np.float32), DIR_ULP + 0.5, pos + ulp(mag, np.float32)
        v_err = np.max(np.abs(a["v"][diffuse] - ref["v"][diffuse])) / v_unit
        r_err = np.max(np.abs((a["r"][diffuse] - center) - (ref["r"][diffuse] - center)))
        dr_err = np.max(np.abs(a["dr"][diffuse] - ref["dr"][diffuse]))
        dv_err = np.max(np.abs(a["dv"][diffuse] - ref["dv"][diffuse])) / v_unit
        print("%s: v %.3g ulp(c) (bound %g), r %.3g (bound %.3g), dr %.3g, dv %.3g ulp(c)" % (what, v_err, v_bound, r_err, r_bound, dr_err, dv_err))
        assert v_err <= v_bound, what
        assert r_err <= r_bound and dr_err <= r_bound, what
        assert dv_err <= v_bound + 1.0, what                           # dv = v - v_old: one more rounding, of a value up to 2c
    return ref


# ------------------------------------------------------------------------------------------------ the ABI, by hand
def abi_args(**kw):
    """(what must stay alive, the arguments behind the handle, counts, bands) of a good call of pcl_step_ground_spectral with three
    bands, and what ``kw`` changes of them (None: NULL)."""
    albedo, specular = tables_of(3)
    a = dict(radius=RADIUS, center=CENTER, n_bands=3, E_edges=edges_of(3), albedo=albedo, specular=specular, c=C,
             counts=np.full(6, -7, dtype=np.int64), bands=np.full(8, -7, dtype=np.int64))
    a.update(kw)
    keep = {k: None if a[k] is None else np.ascontiguousarray(a[k], dtype=np.float64) for k in ("center", "E_edges", "albedo", "specular")}
    ptr = lambda x: None if x is None else x.ctypes.data                                                          # noqa: E731
    return keep, (ctypes.c_double(a["radius"]), ptr(keep["center"]), int(a["n_bands"]), ptr(keep["E_edges"]), ptr(keep["albedo"]),
                  ptr(keep["specular"]), ctypes.c_double(a["c"]), 1, 1, ptr(a["counts"]), ptr(a["bands"])), a["counts"], a["bands"]


BAD_CALLS = [dict(counts=None), dict(bands=None), dict(E_edges=None), dict(albedo=None), dict(specular=None),
             dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(radius=1e200),
             dict(center=[0.0, np.nan, 0.0]), dict(center=[np.inf, 0.0, 0.0]), dict(n_bands=0), dict(n_bands=-1), dict(n_bands=1025),
             dict(E_edges=[1.0, np.nan, 2.0, 3.0]), dict(E_edges=[1.0, np.inf, 2.0, 3.0]), dict(E_edges=[1.0, 2.0, 2.0, 3.0]),
             dict(E_edges=[1.0, 2.0, 1.5, 3.0]), dict(albedo=[0.5, -0.1, 0.5]), dict(albedo=[0.5, 1.5, 0.5]), dict(albedo=[0.5, np.nan, 0.5]),
             dict(specular=[-0.1, 0.5, 0.5]), dict(specular=[0.5, 0.5, 1.5]), dict(specular=[np.nan, 0.5, 0.5]), dict(c=np.inf), dict(c=np.nan)]
# the same for the constructor: what it is given, and the word its message carries
BAD_STEPS = [(dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=np.nan), "radius"), (dict(radius=np.inf), "radius"),
             (dict(radius=1e200), "radius"), (dict(radius="wide"), "radius"), (dict(center=(0, 0)), "center"),
             (dict(center=(0, np.nan, 0)), "center"), (dict(center=(np.inf, 0, 0)), "center"),
             (dict(E_edges=[1.0]), "E_edges"), (dict(E_edges=np.arange(1026.0)), "E_edges"), (dict(E_edges=[1.0, np.nan, 2.0, 3.0]), "E_edges"),
             (dict(E_edges=[1.0, np.inf, 2.0, 3.0]), "E_edges"), (dict(E_edges=[1.0, 2.0, 2.0, 3.0]), "E_edges"),
             (dict(E_edges=[1.0, 2.0, 1.5, 3.0]), "E_edges"), (dict(E_edges="blue"), "E_edges"),
             (dict(albedo=[0.5, -0.1, 0.5]), "albedo"), (dict(albedo=[0.5, 1.5, 0.5]), "albedo"), (dict(albedo=[0.5, np.nan, 0.5]), "albedo"),
             (dict(albedo=[0.5, 0.5]), "albedo"), (dict(albedo=0.5), "albedo"), (dict(albedo="green"), "albedo"),
             (dict(specular=[-0.1, 0.5, 0.5]), "specular"), (dict(specular=[0.5, 0.5, 1.5]), "specular"), (dict(specular=np.nan), "specular"),
             (dict(specular=1.5), "specular"), (dict(specular=[0.5, 0.5]), "specular"), (dict(specular="wet"), "specular")]
