#!/usr/bin/env python3
"""What one pass of the absorption along the path (Device.absorb_path, PathAbsorptionStep) costs on the device.

    python tools/bench_path_absorb.py [--n 10000000,100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons per size, one process.  A call changes the photons it absorbs, so the state is made anew before every
timed call, on the device (not timed): the photons are put on one point (Device.apply_source, isotropic) and moved one Newton step
of 150 km, so that everybody stands one STEP from the origin of the source and moves; for the case at rest a black gas
(Device.absorb_path with p = 1) parks everybody first.  What is quoted is the wall time around the synchronising call, ``--runs``
repeats after one warm-up call, the median with the spread (max - min) / median.  One JSON line each:
  phase_nobody_scattered   the yardstick: Device.phase_redirect (hg 0.85) with nobody scattered -- the three dv rows, 24 B per slot
                           (fp64), on the same store in the same process; once more behind the cases
  everybody_at_rest        the three v rows and nothing else: 24 B per slot
  nobody_absorbed_layers   p = 0 in four layers, everybody moving: v0 and the three r rows, 32 B per slot; nobody draws
  nobody_absorbed_cells    p = 0 in four layers of 64 bands: v0, r and E, 40 B per slot, and two binary searches in LDS
  half_absorbed            p = 0.5 everywhere, no layers, no bands: v0, one Philox block per slot, six rows written for every other
No ratio is fixed in advance: ``over_yardstick`` is the case's median over the first yardstick's.
bytes_per_slot = 1 word (v0) + share_at_rest * 2 words (v1, v2) + share_moving * (3 words with layers (r) + 1 with bands (E)) +
share_absorbed * 6 words (v and dv written).
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

C_LIT, H_LIT, DT = 299792458.0, 6.62607015e-34, 0.0005
STEP = C_LIT * DT
ORIGIN = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP)


class Isotropic:
    origin, e1, e2, d = ORIGIN, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "point", 0.0, 0.0


LAYERS = np.array([0.0, 0.5, 0.9, 1.1, 2.0]) * STEP            # after the move everybody stands STEP from ORIGIN: in the third layer
BANDS = np.linspace(1.0, 3.0, 65)                               # the fill's energies reach from 1 to 3
# case -> (everybody parked first, p, edges, E_edges)
CASES = [("everybody_at_rest", True, np.full(4, 0.5), LAYERS, None),
         ("nobody_absorbed_layers", False, np.zeros(4), LAYERS, None),
         ("nobody_absorbed_cells", False, np.zeros((4, 64)), LAYERS, BANDS),
         ("half_absorbed", False, 0.5, None, None)]


def stats(t):
    med = statistics.median(t)
    return {"s": t, "median_s": med, "spread": (max(t) - min(t)) / med}


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}

    def emit(case, **kw):
        print(json.dumps(dict(base, case=case, **kw)), flush=True)

    dev = hip.Device(0)
    try:
        dev.store_alloc(n, dtype)
        dev.fill_photons(n, 0, C_LIT, 1.0, 3.0, 1)

        def reset(parked, launch):
            dev.apply_source(Isotropic, C_LIT, 1)
            dev.step_newton(DT)
            # pcoll = A*n*|dr| = 0: nobody interacts, dv = 0 is written for everybody
            dev.step_scatter_isotropic(0.0, 1.0, 0, C_LIT, H_LIT, None, hip.RNG_PHILOX, 1, launch)
            if parked:
                assert dev.absorb_path(1.0, None, None, None, 1, launch)[1] == n
            dev.sync()

        def yardstick(name):
            reset(False, 0)
            dev.phase_redirect("hg", 0.85, C_LIT, 1, 1)         # the first look at the store pays the core's materialise pass
            t, got = [], 0
            for k in range(runs):
                t0 = time.perf_counter()
                got = dev.phase_redirect("hg", 0.85, C_LIT, 1, 2 + k)
                t.append(time.perf_counter() - t0)
            y = stats(t)
            emit(name, out=int(got), bytes_per_slot=3 * esz, GBps=3 * esz * n / y["median_s"] / 1e9, **y)
            return y
        y = yardstick("phase_nobody_scattered")
        for case, parked, p, edges, E_edges in CASES:
            t, got = [], None
            for k in range(runs + 1):
                reset(parked, 1 + k)
                t0 = time.perf_counter()
                got = dev.absorb_path(p, edges, ORIGIN, E_edges, 1, 1 + k)
                if k:                                         # (the first call is the warm-up)
                    t.append(time.perf_counter() - t0)
            s = stats(t)
            moving, gone = 0.0 if parked else 1.0, got[1] / n
            bps = (1 + 2 * (1.0 - moving) + moving * (3 * (edges is not None) + (E_edges is not None)) + 6 * gone) * esz
            emit(case, layers=0 if edges is None else len(edges) - 1, bands=0 if E_edges is None else len(E_edges) - 1,
                 share_exposed=got[0] / n, share_absorbed=gone, bytes_per_slot=bps, GBps=bps * n / s["median_s"] / 1e9,
                 over_yardstick=s["median_s"] / y["median_s"], **s)
        yardstick("phase_nobody_scattered_again")
    finally:
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="10000000,100000000", help="store sizes, comma separated")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtype", default="f64")
    a = ap.parse_args()
    for n in (int(float(x)) for x in a.n.split(",")):
        bench(n, a.runs, a.dtype)


if __name__ == "__main__":
    main()
