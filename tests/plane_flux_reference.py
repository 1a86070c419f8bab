"""What the plane flux map tests share: a slow, independent per-particle restatement of pcl_step_plane_flux's rule
(``plane_flux_loop``, as detector_reference.detector_image_loop is for the detector), the exact crossing point in rationals, the
hand-made edge cases with their written-out answers, and the scenes of the device tests.  NumPy and the standard library only."""
import math
from fractions import Fraction

import numpy as np

NAN, INF = float("nan"), float("inf")
AXES = {"x": (0, 1, 2), "y": (1, 0, 2), "z": (2, 0, 1)}               # the normal, then (u, v)


# ------------------------------------------------------------------------------------------------ the loop
def plane_flux_loop(r, dr, E, photon, axis, levels, edges, E_edges=None):
    """The rule of include/physicl_hip.h (pcl_step_plane_flux), particle by particle and level by level, in Python floats (IEEE
    doubles, one rounding per operation); the bins by a linear scan of the products, not by a search."""
    a, tu, tv = AXES[axis]
    levels = [float(x) for x in levels]
    ue, ve = ([float(x) for x in e] for e in edges)
    Ee = None if E_edges is None else [float(x) for x in E_edges]
    S, nB = len(levels), 1 if Ee is None else len(Ee) - 1
    counts = np.zeros((2, S), dtype=np.int64)
    maps = np.zeros((2, S, nB, len(ue) - 1, len(ve) - 1), dtype=np.int64)

    def bin_of(e, H, D):                                               # None: outside, or not finite
        if not math.isfinite(H) or not (e[0] * D <= H <= e[-1] * D):
            return None
        return max(k for k in range(len(e) - 1) if e[k] * D <= H)      # the last bin is closed

    for i in range(len(r)):
        now, m = float(r[i][a]), float(dr[i][a])
        prev = now - m
        for s, X in enumerate(levels):
            if prev < X and now >= X:
                d = 0
            elif prev >= X and now < X:
                d = 1
            else:
                continue
            counts[d, s] += 1
            band = 0
            if Ee is not None:
                e = float(E[i])
                if not photon[i] or not (Ee[0] <= e <= Ee[-1]):
                    continue
                band = max(k for k in range(nB) if Ee[k] <= e)
            D, G = abs(m), abs(X - prev)
            if not math.isfinite(D):
                continue
            cell = []
            for t, e in ((tu, ue), (tv, ve)):
                p = float(r[i][t]) - float(dr[i][t])
                cell.append(bin_of(e, p * D + float(dr[i][t]) * G, D))
            if None not in cell:
                maps[d, s, band, cell[0], cell[1]] += 1
    return counts, maps


def exact_points(r, dr, axis, levels):
    """[(particle, direction, level, x_u, x_v)] for every crossing the rule's compares find: the point where the straight move met the
    plane, as Fractions from the float64 inputs -- ``(r_t - dr_t) + dr_t * (X - prev) / m`` with ``prev = r_a - dr_a`` exact."""
    a, tu, tv = AXES[axis]
    out = []
    for i in range(len(r)):
        now, m = float(r[i][a]), float(dr[i][a])
        prev = now - m                                                 # the rule's own compares decide who crossed
        if not math.isfinite(m) or m == 0.0 or not math.isfinite(now):
            continue
        for s, X in enumerate(levels):
            X = float(X)
            d = 0 if prev < X and now >= X else 1 if prev >= X and now < X else None
            if d is None:
                continue
            frac = (Fraction(X) - (Fraction(now) - Fraction(m))) / Fraction(m)
            pt = [Fraction(float(r[i][t])) - Fraction(float(dr[i][t])) + Fraction(float(dr[i][t])) * frac for t in (tu, tv)]
            out.append((i, d, s, pt[0], pt[1]))
    return out


# ------------------------------------------------------------------------------------------------ hand-made edge cases
EDGE_AXIS, EDGE_LEVELS = "z", [0.0, 1.0]
EDGE_EDGES = [[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0]]                      # x, y
EDGE_BANDS = [1.0, 2.0, 3.0]


def edge_cases(dtype=np.float64):
    """(r, dr, E, photon): sixteen particles, each one sentence of the rule; every value is exact in fp32 as well (the particle just
    outside the map sits one ulp of ``dtype`` beyond the last edge)."""
    out1 = float(np.nextafter(dtype(1.0), dtype(2.0)))
    rows = [
        # r                      dr                    E    photon
        ((0.5, 0.5, 0.0),       (0.0, 0.0, -0.5),     1.5, 1),        # 0  ends exactly on level 0 from above: on the plane is above, no crossing
        ((0.5, 0.5, 0.0),       (0.0, 0.0, 0.5),      1.5, 1),        # 1  ends exactly on level 0 from below: up
        ((0.5, 0.5, -0.5),      (0.0, 0.0, -0.5),     2.0, 1),        # 2  starts exactly on level 0, moves down: down (G = 0); E on an inner band edge
        ((0.5, 0.5, 0.5),       (0.0, 0.0, 0.5),      1.5, 1),        # 3  starts exactly on level 0, moves up: was above already
        ((0.5, 0.5, 0.0),       (0.0, 0.0, 0.0),      1.5, 1),        # 4  m = 0
        ((0.5, 0.5, NAN),       (0.0, 0.0, 0.5),      1.5, 1),        # 5  NaN in r_a
        ((0.5, 0.5, 0.25),      (0.0, 0.0, NAN),      1.5, 1),        # 6  NaN in dr_a
        ((NAN, 0.5, 0.25),      (0.0, 0.0, 0.5),      1.5, 1),        # 7  NaN in r_u: up through level 0, in no cell
        ((0.5, 0.5, 0.75),      (0.0, NAN, -0.5),     1.5, 1),        # 8  NaN in dr_v: down through level 1, in no cell
        ((0.75, 0.5, 1.5),      (1.0, 0.0, 2.0),      3.0, 1),        # 9  up through both levels; at level 0 x = 0 exactly, the inner edge: the upper bin; E on the last band edge
        ((1.0, 0.5, 0.5),       (0.0, 0.0, 1.0),      1.5, 1),        # 10 x = 1 exactly, the last edge: closed
        ((out1, 0.5, 0.5),      (0.0, 0.0, 1.0),      1.5, 1),        # 11 x one ulp beyond the last edge: counted, in no cell
        ((0.5, 0.5, 0.5),       (0.0, 0.0, INF),      1.5, 1),        # 12 D infinite: up through level 0 (prev = -inf), in no cell
        ((-0.5, -0.5, 0.25),    (0.0, 0.0, 0.5),      1.5, 0),        # 13 a plain Object: counted; in a cell only without bands
        ((-0.5, 0.5, 0.25),     (0.0, 0.0, 0.5),      5.0, 1),        # 14 an energy in no band: counted; in a cell only without bands
        ((-0.25, -1.0, -0.5),   (-0.5, -1.0, -2.0),   1.0, 1),        # 15 down through both levels with a transverse move; E on the first band edge
    ]
    r = np.array([row[0] for row in rows], dtype=dtype)
    dr = np.array([row[1] for row in rows], dtype=dtype)
    E = np.array([row[2] for row in rows], dtype=dtype)
    return r, dr, E, np.array([row[3] for row in rows], dtype=bool)


def edge_case_answers(bands):
    """(counts, maps) of the edge cases, written out by hand: {(dir, level, band, iu, iv): n}."""
    counts = np.array([[8, 1], [2, 2]], dtype=np.int64)                # up: 1 7 9 10 11 12 13 14 | 9;  down: 2 15 | 8 15
    if bands:
        cells = {(0, 0, 0, 1, 1): 2,                                   # 1, 10
                 (0, 0, 1, 1, 1): 1, (0, 1, 1, 1, 1): 1,               # 9 at level 0 and at level 1
                 (1, 0, 1, 1, 1): 1,                                   # 2
                 (1, 1, 0, 1, 0): 1, (1, 0, 0, 0, 0): 1}               # 15 at level 1: (0.125, -0.25), at level 0: (-0.125, -0.75)
    else:
        cells = {(0, 0, 0, 1, 1): 3,                                   # 1, 9, 10
                 (0, 1, 0, 1, 1): 1,                                   # 9 at level 1
                 (0, 0, 0, 0, 0): 1, (0, 0, 0, 0, 1): 1,               # 13, 14
                 (1, 0, 0, 1, 1): 1,                                   # 2
                 (1, 1, 0, 1, 0): 1, (1, 0, 0, 0, 0): 1}               # 15
    maps = np.zeros((2, 2, 2 if bands else 1, 2, 2), dtype=np.int64)
    for at, n in cells.items():
        maps[at] = n
    return counts, maps


def assert_edge_case_tallies(counts, maps, bands):
    want = edge_case_answers(bands)
    assert np.array_equal(counts, want[0]), (counts.tolist(), want[0].tolist())
    assert np.array_equal(maps, want[1]), (np.argwhere(maps != want[1]).tolist(), bands)


# ------------------------------------------------------------------------------------------------ scenes
LEVELS16 = np.linspace(-1.5, 1.5, 16)
E_BANDS = np.array([1.0, 1.5, 2.0, 3.0])
_SCENES = {}


def scene(N, dtype="f64", objects=False, spread=0.8):
    """(r, dr, E, photon) in the store's precision, made once per key: a cloud about the origin whose moves (``spread``: their size)
    cross the levels of LEVELS16 both ways along every axis, with dr = 0, NaN coordinates, and energies on, beside and outside the
    edges of E_BANDS."""
    key = (N, dtype, objects, spread)
    if key not in _SCENES:
        T = np.float64 if dtype == "f64" else np.float32
        rng = np.random.default_rng(N % 1000 + 11)
        r = (rng.normal(size=(N, 3)) * 1.5).astype(T)
        dr = (rng.normal(size=(N, 3)) * spread).astype(T)
        dr[3::17] = 0
        r[5::41, 1] = NAN
        r[7::43, 2] = NAN
        dr[9::47, 0] = NAN
        E = rng.uniform(0.5, 3.5, N).astype(T)
        E[1::29], E[2::31], E[4::37], E[6::43] = 1.0, 2.0, 3.0, NAN
        photon = rng.random(N) < 0.7 if objects else np.ones(N, dtype=bool)
        _SCENES[key] = (r, dr, E, photon)
    return _SCENES[key]


def crossers(st, axis, levels):
    """Who crosses some level: the lanes that stay in the kernel's body behind the ballots."""
    a = AXES[axis][0]
    now, m = st[0][:, a].astype(np.float64), st[1][:, a].astype(np.float64)
    with np.errstate(invalid="ignore"):
        prev = now - m
        X = np.asarray(levels, dtype=np.float64)[:, None]
        return (((prev < X) & (now >= X)) | ((prev >= X) & (now < X))).any(axis=0)


# the configurations of the device tests: name -> (axis, levels, [u edges, v edges], band edges or None)
def configs():
    lin = lambda n, h=3.0: np.linspace(-h, h, n + 1)                   # noqa: E731
    return {
        "z_1_level_lds": ("z", [0.25], [lin(8), lin(16)], None),                              # 256 cells
        "x_16_levels_lds": ("x", LEVELS16, [lin(8), lin(16)], None),                          # 4096 cells: the last LDS size
        "y_16_levels_bands_global": ("y", LEVELS16, [lin(8), lin(16)], E_BANDS),              # 12288 cells
        "z_just_above_4096": ("z", LEVELS16, [lin(8), lin(17)], None),                        # 4352 cells
        "y_1024_bins_lds": ("y", [-0.5, 0.5], [lin(1024), lin(1)], None),                     # 4096 cells behind the edges of 1024 bins: 24 632 B of LDS
        "x_bands_lds": ("x", [-0.5, 0.0, 0.5], [lin(7), lin(5)], E_BANDS),                    # 630 cells, bands
        "z_wide_bins": ("z", [0.0], [lin(1024), lin(256)], None),                             # 2 x 262144 cells, the longest searches
    }
