"""What the tests of the three sweeps that WRITE the store share (pcl_surface.hip: k_surface_reflect, k_phase_redirect,
k_absorb_scattered).  Not a test file: a helper tests/test_gpu_surface.py and test_gpu_scatter_phase.py import their bounds from
(tests/test_gpu_scatter_absorb.py has none: it is exact), and tests/test_gpu_writer_store_states.py and
test_gpu_writer_atmosphere_pass.py everything else.

* the bounds of the rows that go through sin / cos (derived once, below);
* ``check_surface / check_phase / check_absorb``: a state downloaded before a sweep, the state downloaded after it and the
  sweep's answer against the numpy restatement (light._surface_bounce, _phase_redirect, _absorb_scattered) -- counts exact,
  untouched rows bit-identical, absorption exact everywhere;
* the store states the project's hot path leaves behind (``reach``), what follows a sweep (``aftermath``) and the inputs
  (sphere, layers) with which every sweep has work in every state.

Bounds.  Everything up to sin / cos is bit for bit the restatement's; sin / cos are the project's pcl_sincos_2pi on the device and
libm in numpy.  The project's contract for a direction built from its sincos is 4 ulp(c), and behind the sincos
v_k = c * ((s*cos)*e1_k + (s*sin)*e2_k + mu*w_k)  performs DIR_OPS = 8 rounded operations per component (s*cos, *e1_k, s*sin,
*e2_k, +, mu*w_k, +, c*): DIR_ULP = 4 + 8/2 = 8 ulp(c); an fp32 store holds the fp64 value rounded once more: 8.5 ulp of
float32 c.  dv = v - v_old is one more rounding, of a value up to 2c: one ulp(c) more.  The ground's lambertian position
(tests/test_gpu_surface.py): dr_k = w*dir_k carries dir_k's share of that bound -- 7.5 ulp(c)/c relative to 1 (the c* is not
performed), times w -- plus POS_OPS = 3 more rounded operations (w*, x_k +, center_k +), each worth half an ulp of the largest
magnitude in play, |center_k| + R + w <= MAG: (w/c) * 7.5 ulp(c) + 3/2 ulp(MAG); fp32: one float32 ulp(MAG) more.
"""
import numpy as np

from physicl_amd import light

C = 299792458.0
DIR_OPS, POS_OPS = 8, 3
DIR_ULP = 4 + DIR_OPS / 2
FIELDS = ("r", "v", "dr", "dv")
KIND_OBJECT, KIND_PHOTON = 0, 1                      # include/physicl_hip.h (PCL_KIND_OBJECT, PCL_KIND_PHOTON)


def ulp(x, dtype=np.float64):
    return float(np.spacing(dtype(abs(x))))


def lambertian_position_bound(w_max, mag, c=C):
    """The fp64 bound of r - center and dr of a lambertian bounce whose remaining move is at most ``w_max`` long, ``mag`` the
    largest magnitude in play (the module's docstring)."""
    return w_max / c * (DIR_ULP - 0.5) * ulp(c) + POS_OPS / 2 * ulp(mag)


# ------------------------------------------------------------------------------------------------ states and their comparison
def snapshot(dev):
    """All thirteen rows, ids, kinds and the count, downloaded: the store is dense and dr / dv are real afterwards."""
    s = dev.download_state()
    s["kind"] = dev.download_kind()
    s["count"] = dev.count
    return s


def wide(s):
    """{"r", "v", "dr", "dv"}: (n, 3) float64 arrays of a state whose groups are three rows or one (n, 3) array."""
    return {f: (np.stack(s[f], 1) if isinstance(s[f], (list, tuple)) else np.asarray(s[f])).astype(np.float64) for f in FIELDS}


def photons(s):
    kind = s.get("kind")
    return np.ones(len(s["E"]), dtype=bool) if kind is None else np.asarray(kind) != KIND_OBJECT


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_state(a, b, what):
    """Two snapshots (or probed states), bit for bit."""
    assert set(a) == set(b), what
    for f in FIELDS:
        for k in range(3):
            assert same_bits(np.asarray(a[f])[k] if isinstance(a[f], (list, tuple)) else a[f][:, k],
                             np.asarray(b[f])[k] if isinstance(b[f], (list, tuple)) else b[f][:, k]), (what, f, k)
    for f in set(a) - set(FIELDS) - {"count"}:
        assert same_bits(a[f], b[f]), (what, f)
    assert a.get("count") == b.get("count"), what


def _left_alone(before, after, what):
    for f in set(before) - set(FIELDS) - {"count"}:                    # E, ids, kinds
        assert same_bits(before[f], after[f]), (what, f)
    assert before.get("count") == after.get("count") and len(before["E"]) == len(after["E"]), what


# ------------------------------------------------------------------------------------------------ a sweep against its restatement
def check_surface(before, after, counts, radius, center, albedo, mode, c, seed, n_pass, w_max, what):
    """tests/test_gpu_surface.py's check_call on two states that are already there.  Returns the restatement's dict."""
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    center = np.asarray(center, dtype=np.float64)
    ref = light._surface_bounce(b["r"], b["dr"], b["v"], photons(before), before["id"], radius, center, albedo, mode, c, seed, n_pass, T)
    hit, refl, gone = ref["hit"], ref["reflected"], ref["absorbed"]
    assert tuple(int(x) for x in counts) == (int(refl.sum()), int(gone.sum())), what
    _left_alone(before, after, what)
    for f in FIELDS:                                                   # untouched: bit-identical, dv included
        assert np.array_equal(a[f][~hit], b[f][~hit]), (what, f)
    exact = hit if mode == "specular" else gone
    for f in FIELDS:
        assert np.array_equal(a[f][exact], ref[f][exact]), (what, f)
    if mode == "lambertian" and refl.any():
        mag = float(np.max(np.abs(center))) + radius + w_max
        pos = lambertian_position_bound(w_max, mag, c)
        if T is np.float64:
            v_unit, v_bound, r_bound = ulp(c), DIR_ULP, pos
        else:
            v_unit, v_bound, r_bound = ulp(c, np.float32), DIR_ULP + 0.5, pos + ulp(mag, np.float32)
        v_err = np.max(np.abs(a["v"][refl] - ref["v"][refl])) / v_unit
        r_err = np.max(np.abs((a["r"][refl] - center) - (ref["r"][refl] - center)))
        dr_err = np.max(np.abs(a["dr"][refl] - ref["dr"][refl]))
        dv_err = np.max(np.abs(a["dv"][refl] - ref["dv"][refl])) / v_unit
        print("%s: v %.3g ulp(c) (bound %g), r %.3g (bound %.3g), dr %.3g, dv %.3g ulp(c)" % (what, v_err, v_bound, r_err, r_bound, dr_err, dv_err))
        assert v_err <= v_bound, what
        assert r_err <= r_bound and dr_err <= r_bound, what
        assert dv_err <= v_bound + 1.0, what                           # dv = v - v_old: one more rounding, of a value up to 2c
    return ref


def check_phase(before, after, count, phase, g, c, seed, n_pass, what):
    """tests/test_gpu_scatter_phase.py's check_call on two states that are already there.  Returns the restatement's dict."""
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    ref = light._phase_redirect(b["v"], b["dv"], photons(before), before["id"], phase, g, c, seed, n_pass, T)
    go = ref["redirected"]
    assert int(count) == int(go.sum()), what
    _left_alone(before, after, what)
    for f in FIELDS:                                                   # not re-directed: bit-identical; r and dr: everybody
        assert np.array_equal(a[f][~go], b[f][~go]), (what, f)
    assert np.array_equal(a["r"], b["r"]) and np.array_equal(a["dr"], b["dr"]), what
    if go.any():
        v_unit, v_bound = (ulp(c), DIR_ULP) if T is np.float64 else (ulp(c, np.float32), DIR_ULP + 0.5)
        v_err = np.max(np.abs(a["v"][go] - ref["v"][go])) / v_unit
        dv_err = np.max(np.abs(a["dv"][go] - ref["dv"][go])) / v_unit
        print("%s: v %.3g ulp(c) (bound %g), dv %.3g ulp(c) (bound %g)" % (what, v_err, v_bound, dv_err, v_bound + 1))
        assert v_err <= v_bound, what
        assert dv_err <= v_bound + 1.0, what                           # dv = v - v_old: one more rounding, of a value up to 2c
    return ref


def check_absorb(before, after, answer, omega0, edges, center, E_bins, seed, n_pass, what):
    """tests/test_gpu_scatter_absorb.py's check_call on two states that are already there: no tolerance anywhere.  ``answer``:
    (interacted, absorbed, absorbed_by_layer, E_hist | None).  Returns the restatement's dict."""
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    ref = light._absorb_scattered(b["r"], b["v"], b["dv"], np.asarray(before["E"]).astype(np.float64), photons(before), before["id"],
                                  omega0, edges, center, E_bins, seed, n_pass, T)
    _left_alone(before, after, what)
    for f in ("r", "dr"):
        assert same_bits(a[f], b[f]), (what, f)
    for f in ("v", "dv"):
        assert same_bits(a[f], ref[f].astype(T).astype(np.float64)), (what, f)
    interacted, absorbed, by_layer, E_hist = answer
    assert (int(interacted), int(absorbed)) == (int(ref["interacted"].sum()), int(ref["absorbed"].sum())), what
    assert np.asarray(by_layer).tolist() == ref["absorbed_by_layer"].tolist(), what
    assert (E_hist is None) == (E_bins is None), what
    if E_bins is not None:
        assert np.asarray(E_hist).tolist() == ref["E_hist"].tolist(), what
    return ref


# ------------------------------------------------------------------------------------------------ the store states
DT = 0.0005
STEP = C * DT                                        # the length of a move
SEED, FILL_SEED, N_PASS = 5, 11, 7
ID_BASE = 7_000_000_001
N, CAPACITY = 3 * 2048 + 77, 5 * 2048                # several tiles, a ragged last wave, room behind the particles
# S3 alone is larger: the alive path compacts only a store of more than 65536 slots (PCL_ALIVE_MIN_SLOTS' default), and it is the
# dense store behind the sweep that has to be that large -- 0.95**2 of N_S3 are left by then, 68 457 +- 80
N_S3, CAPACITY_S3 = 37 * 2048 + 77, 38 * 2048
SCATTER = dict(A=3e-6, n=1.0, flags=0, c=C, h=0.0)   # A*n*|dr| = 0.45: about half scatter per move
DELETE_A = 1e-6                                      # A*n*|dr| = 0.15 removed per body
DELETE_A_CHAIN = 3.3e-7                              # S3's chain in front of the sweep: 0.05 per body
DELETE_A_S3 = 1.5e-6                                 # S3's bodies behind it: 0.22 per body, fewer than half are left after three
S3_CHAIN = 2
STATES = ("S1", "S2", "S3", "S4", "S5")
MOVES = {"S1": 2, "S2": 3, "S3": S3_CHAIN, "S4": 4, "S5": 2}          # Newton moves a state has behind it
W_MAX = 1.001 * STEP                                 # the longest move: |v| dt with |v| = c to a few ulp, in either precision
LAWS = (("hg", 0.85), ("rayleigh", 0.0))
OMEGA0 = (0.5, 1.0, 0.2)
E_EDGES = np.linspace(1.1, 2.9, 9)                   # the fill's energies reach from 1 to 3: some fall outside


class Source:
    """An isotropic gaussian spot off the centre (what _hip._source reads), tests/test_gpu_shell.py's."""
    origin, e1, e2, d = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "gaussian", 0.0, 0.5 * STEP


def sphere(state):
    """(radius, centre) of the ground for a state: a sphere of one move's radius whose near side the photons that never
    scattered reach with their last move -- its centre 0.4 moves beyond where they stand, along a direction off the axes.
    After the four passes of S4 few have never scattered: its sphere stands two moves out, among the random walkers."""
    d = np.array([2.0, 1.0, -2.0]) / 3.0
    return 1.0 * STEP, np.asarray(Source.origin) + (2.0 if state == "S4" else MOVES[state] + 0.4) * STEP * d


def layer_edges(state):
    """Three layers about the source: the photons that never scattered stand MOVES moves out, in the last layer (black-ish), the
    random walkers further in, in the first (grey) and the second (conservative)."""
    m = MOVES[state]
    return np.array([0.2, 0.55 * m, 0.9 * m, m + 2.5]) * STEP


def s5_kind():
    return np.where(np.arange(N) % 7 == 0, KIND_OBJECT, KIND_PHOTON).astype(np.uint8)


def s5_ids():
    return ID_BASE + np.random.RandomState(5).permutation(N).astype(np.int64)


def scatter_args(hip, step):
    return dict(SCATTER, rng_mode=hip.RNG_PHILOX, seed=SEED, step=step)


def reach(hip, dev, state, dtype):
    """Bring ``dev`` into ``state`` with a fresh store of ``dtype``.  Returns the launch index of the next step."""
    n, cap = (N_S3, CAPACITY_S3) if state == "S3" else (N, CAPACITY)
    dev.store_alloc(cap, dtype)
    dev.fill_photons(n, ID_BASE, C, 1.0, 3.0, FILL_SEED)
    dev.apply_source(Source, C, FILL_SEED)
    if state == "S5":                                # every 7th a plain Object, ids in scrambled order: both are staged
        dev.upload_ids(s5_ids())
        dev.upload_kind(s5_kind())
    step = 1
    if state in ("S1", "S2", "S5"):                  # S1: dr and dv implicit
        for _ in range(2):
            dev.step_fused(DT, scatter=scatter_args(hip, step), planes=None, sync=False, lazy=True)
            step += 1
    if state == "S2":                                # ... behind an alive mask
        out = dev.step_fused_delete(DT, DELETE_A, 1.0, seed=SEED, step=step, planes=None, lazy=True)
        assert 0 < out["N"] < n
        step += 1
    if state == "S3":                                # a delete-only chain from a fresh fill: dv is known to be zero
        for _ in range(S3_CHAIN):
            out = dev.step_fused_delete(DT, DELETE_A_CHAIN, 1.0, seed=SEED, step=step, planes=None, lazy=True)
            step += 1
        assert 65536 < out["N"] < n
    if state == "S4":                                # what a K-pass launch leaves behind
        dev.step_fused_multi(DT, 4, scatter_args(hip, step))
        step += 4
    return step


def aftermath(hip, dev, state, step, lazy, bodies=None):
    """What the loop does next.  S3: delete bodies until a compaction has happened (``bodies`` of them if given); every other
    state: one fused step with a scatter, one delete body.  Returns the number of delete bodies.  (S3's launch indices advance by
    two: a run of consecutive indices is taken for a loop, whose bodies the library works out many at a time, ahead of their calls,
    and a store of this size is compacted only between two such launches.)"""
    if state != "S3":
        dev.step_fused(DT, scatter=scatter_args(hip, step), planes=None, sync=False, lazy=lazy)
        dev.step_fused_delete(DT, DELETE_A, 1.0, seed=SEED, step=step + 1, planes=None, lazy=lazy)
        return 1
    slots0, done = dev.slots, 0
    while (dev.slots >= slots0) if bodies is None else (done < bodies):
        assert done < 16, "no compaction within 16 delete bodies"
        dev.step_fused_delete(DT, DELETE_A_S3, 1.0, seed=SEED, step=step + 1 + 2 * done, planes=None, lazy=lazy)
        done += 1
    return done


def upload_plain(dev, state, capacity, dtype):
    """``state`` (a snapshot) into a fresh store of ``dev``: ids of their own only where they are not id[0] + index, kinds only
    where a plain Object is among them."""
    dev.store_alloc(capacity, dtype)
    ids, kind = np.asarray(state["id"]), np.asarray(state["kind"])
    up = {f: np.stack(state[f], 1) for f in FIELDS}
    up.update(E=state["E"], id_base=int(ids[0]) if len(ids) else 0)
    if len(ids) and not np.array_equal(ids, ids[0] + np.arange(len(ids), dtype=np.int64)):
        up["id"] = ids
    if (kind == KIND_OBJECT).any():
        up["kind"] = kind
    dev.upload_state(up)
