"""The numpy restatement of pcl_step_shell_crossings (include/physicl_hip.h), for the tests of the shell tallies, and the
per-particle Python loop it is checked against.

All arithmetic is float64, one rounding per operation, in the order the header writes it: d = r - c, p = d - dr,
q = (a0*a0 + a1*a1) + a2*a2; outward iff q_prev < R*R <= q_now, inward iff q_now < R*R <= q_prev; E binned as
numpy.histogram bins it; mu binned as W = s*|s| against w_b * D with w_b = e_b*|e_b|, D = q_now * (dr.dr) -- no square
root, no division, so every operation here is the device's operation."""
import math

import numpy as np


def _q(a):
    return (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]


def shell_crossings(r, dr, E, photon, radii, center=(0.0, 0.0, 0.0), E_edges=None, mu_edges=None):
    """(counts int64[2, S], E_hist int64[2, S, B_E] | None, mu_hist int64[2, S, B_mu] | None); [0] outward, [1] inward.
    ``r``, ``dr``: (n, 3), any float dtype (an fp32 store's rows widen exactly); ``photon``: who carries an energy."""
    r, dr = np.asarray(r, dtype=np.float64).reshape(-1, 3), np.asarray(dr, dtype=np.float64).reshape(-1, 3)
    E, photon = np.asarray(E, dtype=np.float64).reshape(-1), np.asarray(photon, dtype=bool).reshape(-1)
    radii = np.asarray(radii, dtype=np.float64).reshape(-1)
    S, n = len(radii), len(r)
    with np.errstate(all="ignore"):
        d = r - np.asarray(center, dtype=np.float64).reshape(3)
        q_now, q_prev = _q(d), _q(d - dr)
        s = (d[:, 0] * dr[:, 0] + d[:, 1] * dr[:, 1]) + d[:, 2] * dr[:, 2]
        W, D = s * np.abs(s), q_now * _q(dr)
    counts = np.zeros((2, S), dtype=np.int64)
    E_hist = None if E_edges is None else np.zeros((2, S, len(E_edges) - 1), dtype=np.int64)
    mu_hist = None if mu_edges is None else np.zeros((2, S, len(mu_edges) - 1), dtype=np.int64)
    R2 = radii * radii
    with np.errstate(invalid="ignore"):
        sides = np.stack([(q_prev < R2[:, None]) & (q_now >= R2[:, None]), (q_prev >= R2[:, None]) & (q_now < R2[:, None])])   # [2, S, n]
    if mu_edges is not None:
        e = np.asarray(mu_edges, dtype=np.float64)
        w, B = e * np.abs(e), len(e) - 1
        hit = np.flatnonzero(sides.any(axis=(0, 1)))             # only a particle that crossed something is binned
        Wh, Dh = W[hit], D[hit]
        bin_h = np.full(len(hit), -1)
        with np.errstate(all="ignore"):
            usable = (Dh > 0) & np.isfinite(Dh) & np.isfinite(Wh)
            for b in range(B):
                lo, hi = w[b] * Dh, w[b + 1] * Dh
                inside = (lo <= Wh) & ((Wh <= hi) if b == B - 1 else (Wh < hi)) & usable
                assert np.all(bin_h[inside] == -1)               # a particle is in one bin at most
                bin_h[inside] = b
        mu_bin = np.full(n, -1)
        mu_bin[hit] = bin_h
    for k in range(S):
        for way in range(2):
            c = sides[way, k]
            counts[way, k] = np.count_nonzero(c)
            if E_hist is not None:
                E_hist[way, k] = np.histogram(E[c & photon & ~np.isnan(E)], bins=np.asarray(E_edges, dtype=np.float64))[0]
            if mu_hist is not None:
                mu_hist[way, k] = np.bincount(mu_bin[c & (mu_bin >= 0)], minlength=B)
    return counts, E_hist, mu_hist


def shell_crossings_loop(r, dr, E, photon, radii, center=(0.0, 0.0, 0.0), E_edges=None, mu_edges=None):
    """The same, one particle at a time in plain Python floats (IEEE doubles), straight from the header's text."""
    S = len(radii)
    counts = np.zeros((2, S), dtype=np.int64)
    E_hist = None if E_edges is None else np.zeros((2, S, len(E_edges) - 1), dtype=np.int64)
    mu_hist = None if mu_edges is None else np.zeros((2, S, len(mu_edges) - 1), dtype=np.int64)
    c = [float(x) for x in center]
    fin = math.isfinite
    for i in range(len(r)):
        x, m = [float(v) for v in r[i]], [float(v) for v in dr[i]]
        d = [x[0] - c[0], x[1] - c[1], x[2] - c[2]]
        p = [d[0] - m[0], d[1] - m[1], d[2] - m[2]]
        q_now = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        q_prev = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
        s = (d[0] * m[0] + d[1] * m[1]) + d[2] * m[2]
        dd = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]
        W, D = s * abs(s), q_now * dd
        for k in range(S):
            R2 = float(radii[k]) * float(radii[k])
            if q_prev < R2 and q_now >= R2:
                way = 0
            elif q_prev >= R2 and q_now < R2:
                way = 1
            else:
                continue
            counts[way, k] += 1
            if E_hist is not None and photon[i]:
                e, B = float(E[i]), len(E_edges) - 1
                for b in range(B):
                    if E_edges[b] <= e and (e < E_edges[b + 1] or (b == B - 1 and e == E_edges[B])):
                        E_hist[way, k, b] += 1
            if mu_hist is not None and fin(D) and fin(W) and D != 0:
                B = len(mu_edges) - 1
                w = [float(e) * abs(float(e)) for e in mu_edges]
                for b in range(B):
                    if w[b] * D <= W and (W < w[b + 1] * D or (b == B - 1 and W <= w[B] * D)):
                        mu_hist[way, k, b] += 1
    return counts, E_hist, mu_hist


E_EDGES = np.array([1.0, 1.5, 2.0, 2.25, 3.0])
MU_EDGES = np.array([-1.0, -0.5, -0.1, 0.0, 0.3, 0.8, 1.0])
EDGE_RADII = [5.0, 0.5, 2.0]


def edge_cases():
    """(r, dr, E, photon) of the hand-made cases, for the radii EDGE_RADII about the origin, E_EDGES and MU_EDGES."""
    nan = float("nan")
    rows = [
        ((3, 4, 0), (1.5, 2, 0), 1.0, 1),            # arrives exactly on the sphere R = 5 (q = 25): outward once ...
        ((6, 8, 0), (3, 4, 0), 1.5, 1),              # ... and moving on from (3, 4, 0) it is not counted again; E on an inner edge
        ((1.5, 2, 0), (-1.5, -2, 0), 3.0, 1),        # starts exactly on the sphere and moves in: inward; E on the last edge
        ((1, 0, 0), (2, 0, 0), 2.0, 1),              # a chord through the shell R = 0.5: no crossing of it
        ((1, 1, 1), (0, 0, 0), 2.0, 1),              # dr = 0
        ((nan, 0, 0), (1, 0, 0), 2.0, 1),            # a NaN coordinate
        ((0, 0, 0), (3, 0, 0), 2.5, 1),              # q_now = 0, inward through 2 and 0.5: D = 0, counted, in no mu bin
        ((0, 0, 3), (0, 0, 2), 3.5, 1),              # outward through 2, E outside the edges
        ((0, 0, -3), (0, 0, -2), nan, 1),            # E NaN
        ((0, 3, 0), (0, 2, 0), 2.0, 0),              # a plain Object: counted, no E
        ((0, 1, 0), (0, -2, 0), 1.0, 1),             # inward through 2, straight down: mu = -1 on the first edge; E on the first edge
        ((0, 2.5, 0), (0, 1, 0), 2.2, 1),            # outward through 2, straight up: mu = +1 on the last edge (closed)
        ((2.5, 0, 0), (1, 1, 0), 2.2, 1),            # outward, oblique
        ((1.9, 0, 0), (0, 2, 0), 2.2, 1),            # inward through 2 at a right angle to the radius: s = 0, mu = 0 on an inner edge
    ]
    r, dr, E, ph = (np.array([row[k] for row in rows], dtype=np.float64) for k in range(4))
    return r, dr, E, ph.astype(bool)


def assert_edge_case_tallies(counts, E_hist, mu_hist):
    """What edge_cases() must give for EDGE_RADII, E_EDGES, MU_EDGES, worked out by hand."""
    assert counts[:, 0].tolist() == [1, 1]                         # R = 5: row 0 out (row 1 does not count again), row 2 in
    assert counts[:, 1].tolist() == [0, 1]                         # R = 0.5: only the particle that ends on the centre; the chord is not seen
    assert counts[:, 2].tolist() == [5, 3]                         # R = 2: rows 7, 8, 9, 11, 12 out; rows 6, 10, 13 in
    assert E_hist[0, 0].tolist() == [1, 0, 0, 0] and E_hist[1, 0].tolist() == [0, 0, 0, 1]        # first edge: first bin; last edge: last bin
    assert E_hist[1, 1].tolist() == [0, 0, 0, 1] and mu_hist[1, 1].sum() == 0                     # D = 0: an energy, no direction
    assert E_hist[0, 2].tolist() == [0, 0, 2, 0]                   # of the 5: one outside the edges, one NaN, one plain Object
    assert mu_hist[1, 0].tolist() == [1, 0, 0, 0, 0, 0]            # row 2, straight down: mu = -1 on the first edge
    assert mu_hist[1, 2].tolist() == [1, 0, 0, 1, 0, 0]            # row 10 straight down, row 13 with mu = 0 in [0, 0.3); row 6 in no bin
    assert mu_hist[0, 2].tolist() == [0, 0, 0, 0, 1, 4]            # four straight up, mu = +1 in the closed last bin; row 12 at 0.707
