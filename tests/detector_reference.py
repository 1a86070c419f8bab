"""For the tests of the detector's image (pcl_step_detector_image, DetectorMeasureStep): a per-particle Python loop written
from the header's text -- the numpy restatement the package answers with on the host path (light._detector_image) is the
yardstick of the GPU tests and is held against this loop --, and the inputs the CPU and GPU tests share: five configurations
and, per aperture, a pencil of photons aimed at the aperture with the edge cases planted into it.

All arithmetic is float64, one rounding per operation, in the order the header writes it; there is no division and no square
root, so every operation here is the device's operation."""
import math

import numpy as np

NAN = float("nan")


def detector_image_loop(r, dr, E, photon, position, frame, radius, x_edges, y_edges, E_edges=None):
    """(counts int64[2] = [through, seen], image int64[max(bands, 1), ny, nx]), one particle at a time in plain Python floats
    (IEEE doubles).  A bin is found by walking the edges: [e_b*wn, e_(b+1)*wn), the last one closed."""
    p = [float(x) for x in position]
    e1, e2, n = ([float(x) for x in row] for row in np.asarray(frame, dtype=np.float64).reshape(3, 3))
    xe, ye = [float(x) for x in x_edges], [float(x) for x in y_edges]
    Ee = None if E_edges is None else [float(x) for x in E_edges]
    nx, ny, nE = len(xe) - 1, len(ye) - 1, 0 if Ee is None else len(Ee) - 1
    R2 = float(radius) * float(radius)
    counts = np.zeros(2, dtype=np.int64)
    image = np.zeros((max(nE, 1), ny, nx), dtype=np.int64)

    def dot(a, u):
        return (a[0] * u[0] + a[1] * u[1]) + a[2] * u[2]

    def walk(edges, nb, v, scale):
        for b in range(nb):
            lo, hi = edges[b] * scale, edges[b + 1] * scale
            if lo <= v and (v < hi or (b == nb - 1 and v <= hi)):
                return b
        return None

    for i in range(len(r)):
        x, m = [float(v) for v in r[i]], [float(v) for v in dr[i]]
        a = [x[0] - p[0], x[1] - p[1], x[2] - p[2]]
        b = [a[0] - m[0], a[1] - m[1], a[2] - m[2]]
        s_now, s_prev = dot(a, n), dot(b, n)
        if not (s_prev > 0.0 and s_now <= 0.0):
            continue
        D = s_prev - s_now
        H = [b[k] * D + m[k] * s_prev for k in range(3)]
        hh, lim = dot(H, H), R2 * (D * D)
        if not (hh <= lim and lim < math.inf):
            continue
        counts[0] += 1
        wn, ax, ay = -dot(m, n), -dot(m, e1), -dot(m, e2)
        if not (wn > 0.0 and wn < math.inf and xe[0] * wn <= ax <= xe[nx] * wn and ye[0] * wn <= ay <= ye[ny] * wn):
            continue
        counts[1] += 1
        col, row, band = walk(xe, nx, ax, wn), walk(ye, ny, ay, wn), 0
        if nE:
            e = float(E[i])
            if not photon[i] or not (Ee[0] <= e <= Ee[nE]):
                continue
            band = walk(Ee, nE, e, 1.0)
        image[band, row, col] += 1
    return counts, image


# ------------------------------------------------------------------------------------------------ configurations
E_BANDS = np.array([1.0, 1.5, 2.0, 2.25, 3.0])
X33 = (np.arange(34) - 16.5) / 16.0              # 33 columns of 1/16 over [-1.03125, 1.03125]: dyadic, a pixel centred on the axis
Y17 = (np.arange(18) - 8.5) / 8.0                # 17 rows of 1/8 over [-1.0625, 1.0625]
ALIGNED = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])          # e1, e2, n: looking up the z axis


def tilted_frame():
    """An orthonormal frame with no axis-aligned vector (made as DetectorMeasureStep makes it, here by hand)."""
    n = np.array([1.0, 2.0, -2.0]) / 3.0
    up = np.array([0.3, 1.0, 0.2])
    e1 = up - np.dot(up, n) * n
    e1 = e1 / np.sqrt(np.dot(e1, e1))
    return np.stack([e1, np.cross(n, e1), n])


def configs():
    """name -> dict(position, frame, radius, x_edges, y_edges, E_edges): with and without bands, a 1 x 1 and a 33 x 17 image, an
    axis-aligned frame (the planted cases are exact in it) and a tilted one."""
    p, q = (0.5, -1.0, 2.0), (-0.75, 0.3, 1.1)
    one = np.array([-0.5, 0.5])
    fx, fy = np.linspace(-np.tan(0.7), np.tan(0.7), 34), np.linspace(-np.tan(0.5), np.tan(0.5), 18)
    return {
        "aligned_33x17_bands": dict(position=p, frame=ALIGNED, radius=0.25, x_edges=X33, y_edges=Y17, E_edges=E_BANDS),
        "aligned_33x17": dict(position=p, frame=ALIGNED, radius=0.25, x_edges=X33, y_edges=Y17, E_edges=None),
        "aligned_1x1": dict(position=p, frame=ALIGNED, radius=0.25, x_edges=one, y_edges=one, E_edges=None),
        "tilted_33x17": dict(position=q, frame=tilted_frame(), radius=0.3, x_edges=fx, y_edges=fy, E_edges=None),
        "tilted_1x1_bands": dict(position=q, frame=tilted_frame(), radius=0.3, x_edges=one, y_edges=one, E_edges=E_BANDS),
    }


# ------------------------------------------------------------------------------------------------ inputs
# The planted cases, in the aperture's own coordinates (along e1, e2, n), for radius 0.25 and the edges X33, Y17, E_BANDS: where the
# move began, the move, E, photon.  Every number is a short dyadic fraction, so the axis-aligned configurations see them exactly, in
# fp32 stores too.  What each must give there is in planted_answers().
PLANTED = [
    ((0.0625, 0.0, 0.0), (0.0, 0.0, -0.5), 2.0, 1),                # 0  s_prev == 0: starts on the plane, has not arrived
    ((0.0625, 0.0, 0.5), (0.0, 0.0, -0.5), 1.0, 1),                # 1  s_now == 0: ends on the plane, has arrived; straight on; E on the first edge
    ((0.25, 0.0, 0.5), (0.0, 0.0, -1.0), 1.5, 1),                  # 2  a hit exactly on the rim: inside; E on an inner band edge
    ((0.25 + 2.0 ** -10, 0.0, 0.5), (0.0, 0.0, -1.0), 2.0, 1),     # 3  just outside the rim: not through
    ((0.109375, 0.0, 0.5), (-0.21875, 0.0, -1.0), 2.0, 1),         # 4  ax = X33[20] * wn: exactly on an inner pixel edge, the column to its right
    ((0.515625, 0.0, 0.5), (-1.03125, 0.0, -1.0), 2.0, 1),         # 5  ax = X33[33] * wn: exactly on the last edge, closed
    ((0.515625 + 2.0 ** -11, 0.0, 0.5), (-1.03125 - 2.0 ** -10, 0.0, -1.0), 2.0, 1),     # 6  just beyond it: through, not seen
    ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 2.0, 1),                    # 7  dr == 0, on the aperture's centre
    ((NAN, 0.0, 0.5), (0.0, 0.0, -1.0), 2.0, 1),                   # 8  NaN in r
    ((0.0, 0.0625, 0.5), (0.0, 0.0, -1.0), 2.0, 0),                # 9  a plain Object: seen, in no cell with bands
    ((0.0, -0.0625, 0.5), (0.0, 0.0, -1.0), 3.5, 1),               # 10 E outside the bands: seen, in no cell with bands
    ((0.0, 0.125, 0.5), (0.0, 0.0, -1.0), 3.0, 1),                 # 11 E on the last band edge: the last band
    ((0.0, 0.0, -0.5), (0.0, 0.0, 1.0), 2.0, 1),                   # 12 back to front: no crossing
    ((0.0, 0.53125, 0.5), (0.0, -1.0625, -1.0), NAN, 1),           # 13 ay on the last y edge; E NaN
]
EVERY = 67                                                        # slot i holds planted case i % EVERY, where there is one


def planted_answers(bands):
    """(through, seen, {(band, row, col): count}) of the PLANTED cases alone in the aligned 33 x 17 configurations, by hand."""
    # through: 1, 2, 4, 5, 6, 9, 10, 11, 13; seen: all of them but 6
    cells = {(0, 8, 16): 1, (1, 8, 16): 1, (2, 8, 20): 1, (2, 8, 32): 1, (3, 8, 16): 1} if bands else \
        {(0, 8, 16): 5, (0, 8, 20): 1, (0, 8, 32): 1, (0, 16, 16): 1}
    return 9, 8, cells


def planted_state(cfg):
    """(r, dr, E, photon) of the PLANTED cases alone, float64."""
    e1, e2, n = np.asarray(cfg["frame"], dtype=np.float64)
    p = np.asarray(cfg["position"], dtype=np.float64)
    to_world = lambda v: v[0] * e1 + v[1] * e2 + v[2] * n                      # noqa: E731
    b = np.array([to_world(row[0]) for row in PLANTED])
    m = np.array([to_world(row[1]) for row in PLANTED])
    return p + (b + m), m, np.array([row[2] for row in PLANTED]), np.array([bool(row[3]) for row in PLANTED])


_SCENES = {}


def geometry(name):
    """The aperture a configuration looks through: "aligned" or "tilted" (position, frame and radius; the images differ)."""
    return name.split("_")[0]


def scene(N, dtype, name):
    """(r, dr, E, photon) in the store's precision for the aperture of configuration ``name``, made once per (N, dtype, aperture):
    a pencil of moves through the aperture's plane from directions spread over and beyond every configuration's field of view, hit
    points over and beyond the disc, moves that fall short of the plane or go the wrong way, plain Objects among the photons -- and
    the PLANTED cases in the slots i with i % EVERY < len(PLANTED)."""
    key = (N, dtype, geometry(name))
    if key not in _SCENES:
        cfg = configs()[name]
        T = np.float64 if dtype == "f64" else np.float32
        e1, e2, n = np.asarray(cfg["frame"], dtype=np.float64)
        p = np.asarray(cfg["position"], dtype=np.float64)
        rng = np.random.default_rng(N % 1000 + 11)
        tx, ty = rng.uniform(-1.25, 1.25, N), rng.uniform(-1.25, 1.25, N)         # (the widest edges are +-1.0625)
        m = -(n[None, :] + tx[:, None] * e1 + ty[:, None] * e2) * rng.uniform(0.5, 1.5, N)[:, None]
        m[rng.random(N) < 0.1] *= -1.0                                          # the wrong way
        rho, phi = 1.3 * cfg["radius"] * np.sqrt(rng.random(N)), rng.uniform(0.0, 2.0 * np.pi, N)
        hit = rho[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
        b = hit - rng.uniform(0.1, 1.3, N)[:, None] * m                         # (a fraction above 1: the move falls short)
        r, E = p + (b + m), rng.uniform(0.5, 3.5, N)
        photon = rng.random(N) >= 0.1
        pr, pm, pE, pph = planted_state(cfg)
        at = np.flatnonzero(np.arange(N) % EVERY < len(PLANTED))
        r[at], m[at], E[at], photon[at] = pr[at % EVERY], pm[at % EVERY], pE[at % EVERY], pph[at % EVERY]
        _SCENES[key] = (r.astype(T), m.astype(T), E.astype(T), photon)
    return _SCENES[key]
