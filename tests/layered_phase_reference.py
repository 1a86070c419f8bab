"""Populations, laws and layers for the tests of LayeredPhaseStep (tests/test_layered_phase_cpu.py and the GPU tests), and the
comparison of a sweep on two downloaded states (``check_layered``: tests/test_gpu_writer_store_states.py and
test_writer_trips_gpu.py).  Not a test file: a helper they import.  The velocities are tests/phase_reference.py's cloud, the layers
tests/absorb_reference.py's; the restatement of the kernel itself is physicl_amd.light._layered_phase_redirect."""
import numpy as np

import writer_reference as W
from absorb_reference import CENTER, EDGES
from phase_reference import C, SEED, cloud as phase_cloud, unit
from physicl_amd import light

assert C == 299792458.0 and SEED == 0x5EED5A7F
SINGLE = ["isotropic", ("hg", 0.85), ("hg", -0.5), "rayleigh", ("hg", 1e-12), ("hg", -1e-300)]      # the laws PhaseFunctionStep has
AS_PHASE = {"isotropic": ("isotropic", 0.0), "rayleigh": ("rayleigh", 0.0)}
MIX_LAWS = ("rayleigh", ("hg", 0.85))
MIX_WEIGHTS = [[1, 0], [0.3, 0.7], [0, 1]]                          # three layers: molecular, a mixture, a cloud


def as_phase(law):
    """(phase, g) of PhaseFunctionStep for a law of SINGLE."""
    return AS_PHASE.get(law, law)


def hg_table(g, bins):
    """("table", mu_edges, p): the Henyey-Greenstein density at the centres of ``bins`` equal bins."""
    edges = np.linspace(-1.0, 1.0, bins + 1)
    mid = 0.5 * (edges[1:] + edges[:-1])
    return ("table", edges, (1.0 - g * g) / (1.0 + g * g - 2.0 * g * mid) ** 1.5)


def table_moments(mu_edges, p):
    """(F, mean, variance) of the piecewise-constant density: F as the step makes it, the moments from the bins' own."""
    mu_edges, p = np.asarray(mu_edges, dtype=np.float64), np.asarray(p, dtype=np.float64)
    m = p * np.diff(mu_edges)
    F = np.concatenate([[0.0], np.cumsum(m) / np.sum(m)])
    F[-1] = 1.0
    lo, hi = mu_edges[:-1], mu_edges[1:]
    mass = np.diff(F)
    mean = float(np.sum(mass * 0.5 * (lo + hi)))
    second = float(np.sum(mass * (lo * lo + lo * hi + hi * hi) / 3.0))
    return F, mean, second - mean * mean


def cases():
    """{name: (laws, weights, edges)} of the GPU tests; the centre is CENTER wherever there are edges."""
    table = hg_table(0.85, 64)
    out = {"single %s" % (law if isinstance(law, str) else "%s %g" % law): ([law], None, None) for law in SINGLE}
    out["mixture"] = (MIX_LAWS, MIX_WEIGHTS, EDGES)
    out["table"] = ([table], None, EDGES[[0, -1]])                  # one layer with a hole inside and an outside
    out["table+rayleigh"] = ([table, "rayleigh"], [[0.6, 0.4], [0, 1]], EDGES[[0, 2, 3]])
    return out


def cloud(n, seed=1, dtype=np.float64):
    """(r, v, dv) as (n, 3) float64 arrays holding ``dtype`` values: ``v, dv`` of phase_reference.cloud (every third row was
    scattered), ``r`` at distances uniform in [0, 5.2) from CENTER -- inside the hole below EDGES[0], in every layer and beyond
    EDGES[-1].  Scattered rows with index % 33 == 6 have a NaN in r: in no layer."""
    v, dv = phase_cloud(n, seed=seed, dtype=dtype)
    rng = np.random.RandomState(seed + 77)
    r = CENTER + rng.uniform(0.0, 5.2, size=n)[:, None] * unit(rng.normal(size=(n, 3)))
    r[np.arange(n) % 33 == 6, 2] = np.nan
    return r.astype(dtype).astype(np.float64), v, dv


def all_scattered(n, seed=1):
    """(v, dv, ids): every row scattered, old directions everywhere on the sphere."""
    rng = np.random.RandomState(seed)
    old, new = C * unit(rng.normal(size=(n, 3))), C * unit(rng.normal(size=(n, 3)))
    return new, new - old, np.arange(n, dtype=np.int64) + 7_000_000_001


# ------------------------------------------------------------------------------------------------ a sweep against its restatement
def check_layered(before, after, answer, laws, weights, edges, center, c, seed, n_pass, what):
    """A state downloaded before the sweep (tests/writer_reference.py: ``snapshot``), the state downloaded after it and the sweep's
    answer ``(scattered, redirected, by_layer, by_law)`` against light._layered_phase_redirect: every tally exact; E, ids and kinds,
    r and dr of everybody and every row of a particle that is not re-directed bit-identical; re-directed rows within the bounds
    tests/writer_reference.py derives for the phase function's v and dv.  Returns the restatement's dict."""
    bw, aw = W.wide(before), W.wide(after)
    T = np.asarray(before["E"]).dtype.type
    ref = light._layered_phase_redirect(bw["r"], bw["v"], bw["dv"], W.photons(before), before["id"], laws, weights, edges, center, c,
                                        seed, n_pass, T)
    scattered, redirected, by_layer, by_law = answer
    by_layer, by_law = np.asarray(by_layer).tolist(), np.asarray(by_law).tolist()
    print("%s: scattered %d, redirected %d, by layer %s, by law %s" % (what, scattered, redirected, by_layer, by_law))
    assert (scattered, redirected) == (int(ref["scattered"].sum()), int(ref["redirected"].sum())), what
    assert by_layer == ref["by_layer"].tolist() and by_law == ref["by_law"].tolist(), what
    assert sum(by_layer) == sum(by_law) == redirected, what
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
    """The arguments of a good call of the three-layer mixture with a table as a third law, and what ``kw`` changes of them."""
    arr = lambda x, t=np.float64: None if x is None else np.ascontiguousarray(x, dtype=t)                   # noqa: E731
    a = dict(M=3, kinds=[2, 1, 3], g=[0.0, 0.85, 0.0], K=[0, 0, 2], mu=[-1.0, 0.0, 1.0], F=[0.0, 0.25, 1.0], L=3,
             cum=[[1, 1, 1], [0.3, 0.8, 1], [0, 0, 1]], edges=EDGES, center=CENTER, c=C, counts=np.full(2 + 64 + 8, -7, dtype=np.int64))
    a.update(kw)
    keep = [arr(a["kinds"], np.int32), arr(a["g"]), arr(a["K"], np.int32), arr(a["mu"]), arr(a["F"]), arr(a["cum"]), arr(a["edges"]), arr(a["center"])]
    p = [None if x is None else x.ctypes.data for x in keep]
    counts = a["counts"]
    return keep, (a["M"], p[0], p[1], p[2], p[3], p[4], a["L"], p[5], p[6], p[7], float(a["c"]), 1, 1, None if counts is None else counts.ctypes.data), counts


BAD_CALLS = [dict(kinds=None), dict(cum=None), dict(counts=None), dict(M=0), dict(M=9), dict(L=-1), dict(L=65), dict(c=np.inf),
             dict(kinds=[2, 1, 4]), dict(kinds=[2, -1, 3]), dict(g=[0.0, 1.0, 0.0]), dict(g=[0.0, np.nan, 0.0]), dict(g=None),
             dict(K=[0, 0, 0]), dict(K=[0, 0, 1025]), dict(K=None), dict(mu=None), dict(F=None),
             dict(mu=[-0.5, 0.0, 1.0]), dict(mu=[-1.0, 0.0, 0.5]), dict(mu=[-1.0, 1.0, 1.0]), dict(mu=[-1.0, np.nan, 1.0]),
             dict(F=[0.1, 0.25, 1.0]), dict(F=[0.0, 0.25, 0.9]), dict(F=[0.0, 0.0, 1.0]), dict(F=[0.0, 1.0, 1.0]), dict(F=[0.0, np.nan, 1.0]),
             dict(cum=[[1, 1, 1], [0.3, 0.2, 1], [0, 0, 1]]), dict(cum=[[1, 1, 1], [0.3, 0.8, 0.9], [0, 0, 1]]),
             dict(cum=[[1, 1, 1], [-0.1, 0.8, 1], [0, 0, 1]]), dict(cum=[[1, 1, 1], [np.nan, 0.8, 1], [0, 0, 1]]), dict(cum=[[1, 1, 1.5]] * 3),
             dict(edges=None), dict(edges=[1.0, 3.0, 2.0, 4.0]), dict(edges=[-1.0, 2.0, 3.0, 4.0]), dict(edges=[1.0, 2.0, 3.0, 1e200]),
             dict(center=[0, np.nan, 0]),
             dict(M=3, kinds=[3, 3, 3], K=[1024, 1024, 1], mu=np.concatenate([np.linspace(-1, 1, 1025)] * 2 + [[-1.0, 1.0]]),
                  F=np.concatenate([np.linspace(0, 1, 1025)] * 2 + [[0.0, 1.0]]))]         # 2049 bins in all
