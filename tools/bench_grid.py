#!/usr/bin/env python3
"""What one position grid (Device.position_grid, PositionGridMeasureStep) costs on the device.

    python tools/bench_grid.py [--n 100000000] [--runs 5] [--dtype f64] [--no-numpy]

One store of ``--n`` photons, one process.  Wall time around the synchronising call, ``--runs`` repeats, the median is quoted
with the spread (max - min) / median.  Cases, one JSON line each:
  one_cell_lds / one_cell_global   (c) the untouched fill, every photon in one cell of a 16^3 grid, both accumulation forms
  materialise                      the first grid call after a lazy K-step launch against the second one on the same state:
                                   the difference is the core's materialise pass
  spread_lds                       (a) a spread population (isotropic source, scatter steps), 3 Cartesian axes, 16^3 cells,
                                   workgroup histograms in LDS; 24 B x N over its time as a fraction of 8 TB/s
  spread_lds_as_global             the same grid with PCL_GRID_LDS_CELLS=0: the switch-over's measurement
  spread_global                    (b) the same axes at 2^20 cells (1024 x 32 x 32), 64-bit atomics on the device grid
  radius                           (d) a radius profile of 1000 shells about the source
  plane_spectra                    yardstick 1: Device.plane_spectra with three planes, one per axis (r and dr of three axes:
                                   twice the bytes of (a)), same store, same process
  download_histogramdd             yardstick 2, the only way to the grid without this call: download of the three r rows plus
                                   numpy.histogramdd (``--no-numpy`` skips it), and its ratio to (a)
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

C_LIT, DT = 299792458.0, 0.0005
STEP = C_LIT * DT
ORIGIN = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP)


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


def with_form(cells, fn):
    """fn() with the switch-over forced: ``cells`` = PCL_GRID_LDS_CELLS for the call(s), None = the library's default."""
    old = os.environ.pop("PCL_GRID_LDS_CELLS", None)
    if cells is not None:
        os.environ["PCL_GRID_LDS_CELLS"] = str(cells)
    try:
        return fn()
    finally:
        os.environ.pop("PCL_GRID_LDS_CELLS", None)
        if old is not None:
            os.environ["PCL_GRID_LDS_CELLS"] = old


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

    def lin(k, nb, half=4.0):
        return np.linspace(ORIGIN[k] - half * STEP, ORIGIN[k] + half * STEP, nb + 1)

    dev = hip.Device(0)
    try:
        dev.store_alloc(a.n, a.dtype)
        dev.fill_photons(a.n, 0, C_LIT, 1.0, 3.0, 1)
        # (c) every photon at the origin
        cube = [np.linspace(-1.0, 1.0, 17)] * 3
        for name, cells in (("one_cell_lds", 8192), ("one_cell_global", 0)):
            g = with_form(cells, lambda: dev.position_grid("xyz", cube))
            assert g[8, 8, 8] == a.n == g.sum()
            emit(name, cells=g.size, **stats(with_form(cells, lambda: timed(lambda: dev.position_grid("xyz", cube), a.runs))))
        # spread the cloud: K-step launches (lazy), so the first call below pays the materialise pass
        dev.apply_source(Source, C_LIT, 1)
        sc = dict(A=3e-6, n=1.0, flags=0, c=C_LIT, h=0.0, rng_mode=hip.RNG_PHILOX, seed=1, step=1)
        dev.step_fused_multi(DT, 4, sc, [], raw=True)
        axes, edges = "xyz", [lin(k, 16) for k in range(3)]
        first = timed(lambda: dev.position_grid(axes, edges), 1)[0]
        second = timed(lambda: dev.position_grid(axes, edges), 1)[0]
        emit("materialise", first_s=first, second_s=second, materialise_s=first - second)
        # (a), and the same grid through the global form
        want = dev.position_grid(axes, edges)
        a_stats = stats(timed(lambda: dev.position_grid(axes, edges), a.runs))
        emit("spread_lds", cells=want.size, in_grid=int(want.sum()), cells_hit=int(np.count_nonzero(want)), GBps=3 * esz * a.n / a_stats["median_s"] / 1e9,
             fraction_of_8TBps=3 * esz * a.n / a_stats["median_s"] / 8e12, **a_stats)
        g = with_form(0, lambda: dev.position_grid(axes, edges))
        assert np.array_equal(g, want)
        emit("spread_lds_as_global", cells=g.size, **stats(with_form(0, lambda: timed(lambda: dev.position_grid(axes, edges), a.runs))))
        # (b) 2^20 cells
        big = [lin(0, 1024), lin(1, 32), lin(2, 32)]
        g = dev.position_grid(axes, big)
        assert g.sum() == want.sum() and g.size == 1 << 20
        emit("spread_global", cells=g.size, cells_hit=int(np.count_nonzero(g)), **stats(timed(lambda: dev.position_grid(axes, big), a.runs)))
        # (d) a radius profile
        shells = [np.linspace(0.0, 5.0 * STEP, 1001)]
        g = dev.position_grid("r", shells, ORIGIN)
        emit("radius", cells=g.size, in_grid=int(g.sum()), cells_hit=int(np.count_nonzero(g)), **stats(timed(lambda: dev.position_grid("r", shells, ORIGIN), a.runs)))
        # yardstick 1: three planes, one per axis
        nan = float("nan")
        planes = np.array([[ORIGIN[0], nan, nan], [nan, ORIGIN[1], nan], [nan, nan, ORIGIN[2]]])
        e_edges = np.linspace(1.0, 3.0, 51)
        dev.plane_spectra(planes, e_edges)
        y_stats = stats(timed(lambda: dev.plane_spectra(planes, e_edges), a.runs))
        emit("plane_spectra", GBps=6 * esz * a.n / y_stats["median_s"] / 1e9, grid_over_spectra=a_stats["median_s"] / y_stats["median_s"], **y_stats)
        # yardstick 2: download + numpy
        if not a.no_numpy:
            def host_way():
                r = np.stack([dev.download(hip.R0 + k) for k in range(3)], 1)
                return np.histogramdd(r, bins=edges)[0]
            t0 = time.perf_counter()
            h = host_way()
            t = time.perf_counter() - t0
            assert np.array_equal(h.astype(np.int64), want)
            emit("download_histogramdd", s=[t], median_s=t, over_grid=t / a_stats["median_s"])
    finally:
        dev.close()


if __name__ == "__main__":
    main()
