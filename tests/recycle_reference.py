"""States, sources and the comparison for the tests of RecycleStep (tests/test_recycle_cpu.py and the GPU tests).  Not a test file: a
helper they import.  The restatement of the kernel itself is physicl_amd.light._recycle_spent; the bounds of the rows that go
through sin / cos are the ones tests/test_gpu_source.py states for the very same arithmetic (pcl_store_apply_source).

The layout of a state (``layout``), slot i:
    at rest                       iff i % 3 == 0   (of these, i % 6 == 0 carries a -0.0)
    at center + (2*top, 0, 0)     iff i % 5 == 0
    exactly at center + (top,0,0) iff i % 7 == 0   (TOP*TOP is exact)
    a NaN in r                    iff i % 11 == 0
    a NaN in v                    iff i % 13 == 0  (written last: such a slot is not at rest)
    everybody else moves at c, inside.
"""
import numpy as np

from physicl_amd import light
from writer_reference import DIR_ULP, same_bits, ulp

C = 299792458.0
SEED = 0x5EED5A7F
ID_BASE = 7_000_000_001
TOP = 3.0                                            # 9.0 is exact in both precisions
CENTER = np.array([0.5, -0.25, 0.125])               # exact in float32 as well, and so are CENTER + (TOP, 0, 0) and + (2 TOP, 0, 0)
FIELDS = ("r", "v", "dr", "dv")
GRID = np.array([1.25, 1.5, 2.0, 2.75, 3.5])         # float32 values
CDF = np.array([0.1, 0.1, 0.45, 0.8, 1.0])           # a bin without mass among them


def source(angular="isotropic", spatial="disc", oblique=True):
    """A source inside TOP about CENTER: at most |origin - CENTER| + 9 * radius = 0.6 + 0.9 away from it."""
    kw = dict(origin=CENTER + np.array([0.25, 0.5, -0.25]), direction=(1.0, -2.0, 0.5) if oblique else (0.0, 0.0, -1.0), angular=angular,
              spatial=spatial)
    if angular == "cone":
        kw["half_angle"] = 0.4
    if spatial != "point":
        kw["radius"] = 0.1
    return light.PhotonSource(**kw)


def unit(x):
    return x / np.sqrt((x * x).sum(axis=1))[:, None]


def layout(n, dtype=np.float64, seed=1):
    """{"r", "v", "dr", "dv": (n, 3), "E": (n,)} of float64 arrays that hold ``dtype`` values, laid out as the module's docstring
    says."""
    rng = np.random.RandomState(seed + n)
    i = np.arange(n)
    r = CENTER + rng.uniform(0.0, 0.9 * TOP, size=n)[:, None] * unit(rng.normal(size=(n, 3)))
    v = C * unit(rng.normal(size=(n, 3)))
    rest = i % 3 == 0
    v[rest] = 0.0
    v[i % 6 == 0, 1] = -0.0
    r[i % 5 == 0] = CENTER + np.array([2.0 * TOP, 0.0, 0.0])
    r[i % 7 == 0] = CENTER + np.array([TOP, 0.0, 0.0])
    r[i % 11 == 0, 2] = np.nan
    v[i % 13 == 0, 0] = np.nan
    state = {"r": r, "v": v, "dr": rng.normal(size=(n, 3)), "dv": rng.normal(size=(n, 3)), "E": 1.0 + rng.uniform(size=n)}
    return {k: a.astype(dtype).astype(np.float64) for k, a in state.items()}


def expected_masks(n, at_rest=True, top=True, photon=None):
    """(rest, gone) by the layout's own arithmetic on the slot numbers -- what the restatement must find."""
    i = np.arange(n)
    photon = np.ones(n, dtype=bool) if photon is None else photon
    rest = (i % 3 == 0) & (i % 13 != 0) & at_rest
    outside = (i % 5 == 0) & (i % 7 != 0) & (i % 11 != 0)
    gone = outside & ~rest & top
    return rest & photon, gone & photon


def wide(s):
    return {f: (np.stack(s[f], 1) if isinstance(s[f], (list, tuple)) else np.asarray(s[f])).astype(np.float64) for f in FIELDS}


def check_recycle(before, after, counts, src, top, center, at_rest, spectrum, seed, n_pass, what, photon=None):
    """A state downloaded before the sweep, the state downloaded after it and the sweep's answer against the numpy restatement.
    Tallies exact; every field of every particle that is not spent bit-identical, all of E without a spectrum, ids always; dr and dv
    of the spent exactly 0, table energies bit-identical; v and r of the spent within the source's bounds (exact for a beam and a
    point).  Returns the restatement's dict."""
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    n = len(before["E"])
    photon = np.ones(n, dtype=bool) if photon is None else photon
    E_b, E_a = np.asarray(before["E"]).astype(np.float64), np.asarray(after["E"]).astype(np.float64)
    ref = light._recycle_spent(b["r"], b["v"], E_b, photon, before["id"], src, top, center, at_rest, spectrum, C, seed, n_pass, T)
    spent = ref["spent"]
    print("%s: at rest %d, escaped %d of %d" % (what, ref["at_rest"].sum(), ref["escaped"].sum(), n))
    assert tuple(int(x) for x in counts) == (int(ref["at_rest"].sum()), int(ref["escaped"].sum())), what
    assert np.array_equal(after["id"], before["id"]) and len(after["E"]) == n, what
    for f in FIELDS:
        assert same_bits(a[f][~spent], b[f][~spent]), (what, f)
    assert same_bits(E_a[~spent], E_b[~spent]), what
    if spectrum is None:
        assert same_bits(np.asarray(after["E"]), np.asarray(before["E"])), what
    else:
        assert same_bits(E_a[spent], ref["E"][spent]), what
    if not spent.any():
        return ref
    zero = np.zeros((int(spent.sum()), 3))
    assert same_bits(a["dr"][spent], zero) and same_bits(a["dv"][spent], zero), what           # +0.0, bit for bit
    if src.angular == "beam":
        assert same_bits(a["v"][spent], ref["v"][spent]), what
    else:
        v_unit, v_bound = (ulp(C), DIR_ULP) if T is np.float64 else (ulp(C, np.float32), DIR_ULP + 0.5)
        v_err = np.max(np.abs(a["v"][spent] - ref["v"][spent])) / v_unit
        print("%s: direction %.3g ulp(c) (bound %g)" % (what, v_err, v_bound))
        assert v_err <= v_bound, what
    if src.spatial == "point":
        assert same_bits(a["r"][spent], ref["r"][spent]), what
    else:
        # tests/test_gpu_source.py: r - origin per component within 4 ulp(9 * radius) in fp64 (rho*cos, *e1_k, rho*sin, *e2_k, +,
        # origin +, behind a sincos good to 1 ulp and the gaussian's log); an fp32 store holds the fp64 value rounded once: the
        # two roundings differ by at most one float32 ulp at the magnitude of r, |origin| + 9 * radius
        origin = np.asarray(src.origin)
        if T is np.float64:
            pos_unit, pos_bound = float(np.spacing(9.0 * src.radius)), 4.0
            pos_err = np.max(np.abs((a["r"][spent] - origin) - (ref["r"][spent] - origin))) / pos_unit
        else:
            pos_unit, pos_bound = float(np.spacing(np.float32(np.max(np.abs(origin)) + 9.0 * src.radius))), 1.0
            pos_err = np.max(np.abs(a["r"][spent] - ref["r"][spent])) / pos_unit
        print("%s: position %.3g units (bound %g)" % (what, pos_err, pos_bound))
        assert pos_err <= pos_bound, what
    return ref


# ------------------------------------------------------------------------------------------------ the ABI, by hand
def abi_args(hip, **kw):
    """The arguments of a good call (behind the context), and what ``kw`` changes of them.  Source fields: angular, spatial, origin,
    e1, e2, d, cos_half_angle, radius."""
    src = source("cone", "gaussian")
    a = dict(src=True, c=C, at_rest=1, top=TOP, center=CENTER, n_E=len(CDF), cdf=CDF, grid=GRID, counts=np.full(4, -7, dtype=np.int64),
             angular=hip.SRC_ANGULAR[src.angular], spatial=hip.SRC_SPATIAL[src.spatial], origin=src.origin, e1=src.e1, e2=src.e2, d=src.d,
             cos_half_angle=src.cos_half_angle, radius=src.radius)
    a.update(kw)
    vec = lambda x: (hip.c_double * 3)(*[float(t) for t in x])                                               # noqa: E731
    st = hip.SourceStruct(vec(a["origin"]), vec(a["e1"]), vec(a["e2"]), vec(a["d"]), int(a["angular"]), int(a["spatial"]),
                          float(a["cos_half_angle"]), float(a["radius"]))
    arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)                        # noqa: E731
    keep = [st, arr(a["center"]), arr(a["cdf"]), arr(a["grid"])]
    p = [None if x is None else x.ctypes.data for x in keep[1:]]
    counts = a["counts"]
    import ctypes
    return keep, (ctypes.addressof(st) if a["src"] else None, float(a["c"]), int(a["at_rest"]), float(a["top"]), p[0], int(a["n_E"]), p[1],
                  p[2], 1, 1, None if counts is None else counts.ctypes.data), counts


BAD_CALLS = [dict(src=False), dict(counts=None), dict(angular=4), dict(angular=-1), dict(spatial=3), dict(spatial=-1),
             dict(origin=[0, np.nan, 0]), dict(e1=[np.inf, 0, 0]), dict(e2=[0, 0, np.nan]), dict(d=[np.nan, 0, 0]), dict(c=np.inf),
             dict(c=np.nan), dict(center=[0, np.nan, 0]), dict(cos_half_angle=1.5), dict(cos_half_angle=np.nan), dict(radius=-1.0),
             dict(radius=np.inf), dict(top=np.nan), dict(top=np.inf), dict(top=1e200), dict(at_rest=0, top=0.0), dict(at_rest=0, top=-1.0),
             dict(n_E=-1), dict(n_E=1025, cdf=np.linspace(0, 1, 1025), grid=np.ones(1025)), dict(cdf=None), dict(grid=None),
             dict(cdf=[0.1, 0.05, 0.45, 0.8, 1.0]), dict(cdf=[0.1, 0.1, 0.45, 0.8, 0.9]), dict(cdf=[0.1, 0.1, 0.45, 0.8, 1.5]),
             dict(cdf=[0.1, np.nan, 0.45, 0.8, 1.0]), dict(grid=[1.0, 2.0, np.inf, 3.0, 4.0]), dict(grid=[1.0, 2.0, np.nan, 3.0, 4.0])]
