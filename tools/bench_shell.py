#!/usr/bin/env python3
"""What one shell-crossing tally (Device.shell_crossings, ShellCrossingMeasureStep) costs on the device.

    python tools/bench_shell.py [--n 100000000] [--runs 5] [--dtype f64] [--no-numpy]

One store of ``--n`` photons, one process: an isotropic gaussian spot, four lazy K-step passes of Newton + scatter, so the
cloud straddles the shells and about half of it scattered in its last move.  Wall time around the synchronising call,
``--runs`` repeats after one warm-up call, the median is quoted with the spread (max - min) / median.  One JSON line each:
  plane_spectra        the yardstick: Device.plane_spectra with three planes, one per axis, 50 bins -- r and dr of three axes,
                       the same 48 B per slot (fp64), same store, same process
  shells_counts        4 shells, counts only, and its ratio to the yardstick (the aim: within 1.25)
  shells_16_counts     16 shells, counts only
  shells_E50_mu20      4 shells x 50 energy bins x 20 direction bins
  shells_limit         4 shells x 512 x 512 bins: the 8192-cell limit (40 KiB of LDS per workgroup, three workgroups per CU)
  download_numpy       the only way to the tally without this call: download of r, dr and E plus numpy (``--no-numpy``
                       skips it), one run, and its ratio to shells_E50_mu20
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicl_amd import _hip as hip  # noqa: E402
from physicl_amd.light import _shell_tallies  # noqa: E402

C_LIT, DT = 299792458.0, 0.0005
STEP = C_LIT * DT
ORIGIN = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP)
CENTER = (ORIGIN[0] + 0.25 * STEP, ORIGIN[1], ORIGIN[2] - 0.125 * STEP)       # off the source


class Source:
    origin, e1, e2, d = ORIGIN, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "gaussian", 0.0, 0.5 * STEP


def timed(fn, runs):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def stats(t):
    med = statistics.median(t)
    return {"s": t, "median_s": med, "spread": (max(t) - min(t)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    esz = 8 if a.dtype == "f64" else 4
    base = {"n": a.n, "dtype": a.dtype}

    def emit(case, **kw):
        print(json.dumps(dict(base, case=case, **kw)), flush=True)

    dev = hip.Device(0)
    try:
        dev.store_alloc(a.n, a.dtype)
        dev.fill_photons(a.n, 0, C_LIT, 1.0, 3.0, 1)
        dev.apply_source(Source, C_LIT, 1)
        sc = dict(A=3e-6, n=1.0, flags=0, c=C_LIT, h=0.0, rng_mode=hip.RNG_PHILOX, seed=1, step=1)
        dev.step_fused_multi(DT, 4, sc, [], raw=True)
        nan = float("nan")
        planes = np.array([[ORIGIN[0], nan, nan], [nan, ORIGIN[1], nan], [nan, nan, ORIGIN[2]]])
        e_edges, mu_edges = np.linspace(1.0, 3.0, 51), np.linspace(-1.0, 1.0, 21)
        radii = [1.0 * STEP, 2.0 * STEP, 3.0 * STEP, 3.5 * STEP]
        dev.plane_spectra(planes, e_edges)               # the first look at the store pays the core's materialise pass
        y = stats(timed(lambda: dev.plane_spectra(planes, e_edges), a.runs))
        emit("plane_spectra", GBps=6 * esz * a.n / y["median_s"] / 1e9, **y)
        cases = [("shells_counts", radii, None, None), ("shells_16_counts", np.linspace(0.25, 4.0, 16) * STEP, None, None),
                 ("shells_E50_mu20", radii, e_edges, mu_edges),
                 ("shells_limit", radii, np.linspace(1.0, 3.0, 513), np.linspace(-1.0, 1.0, 513))]
        binned = None
        for name, ra, ee, me in cases:
            got = dev.shell_crossings(ra, CENTER, ee, me)
            s = stats(timed(lambda: dev.shell_crossings(ra, CENTER, ee, me), a.runs))
            emit(name, out=int(got[0][0].sum()), inward=int(got[0][1].sum()), GBps=6 * esz * a.n / s["median_s"] / 1e9,
                 over_plane_spectra=s["median_s"] / y["median_s"], **s)
            if name == "shells_E50_mu20":
                binned = (got, s)
        y2 = stats(timed(lambda: dev.plane_spectra(planes, e_edges), a.runs))     # the yardstick again, behind the cases
        emit("plane_spectra_again", GBps=6 * esz * a.n / y2["median_s"] / 1e9, **y2)
        if not a.no_numpy:
            def host_way():
                r = np.stack([dev.download(hip.R0 + k) for k in range(3)], 1)
                dr = np.stack([dev.download(hip.DR0 + k) for k in range(3)], 1)
                E = dev.download(hip.E)
                return _shell_tallies(r, dr, E, np.ones(len(E), dtype=bool), radii, np.array(CENTER), e_edges, mu_edges)
            t0 = time.perf_counter()
            h = host_way()
            t = time.perf_counter() - t0
            assert all(np.array_equal(x, w) for x, w in zip(h, binned[0]))
            emit("download_numpy", s=[t], median_s=t, over_shells=t / binned[1]["median_s"])
    finally:
        dev.close()


if __name__ == "__main__":
    main()
