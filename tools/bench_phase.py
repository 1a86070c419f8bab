#!/usr/bin/env python3
"""What one pass of the phase function (Device.phase_redirect, PhaseFunctionStep) costs on the device.

    python tools/bench_phase.py [--n 100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons, one process.  A call changes the photons it re-directs, so the state is made anew before every
timed call, on the device (not timed): the photons are put on one point (Device.apply_source, isotropic), moved one Newton step
of 150 km and handed to the scatter step (Device.step_scatter_isotropic, constant n) with the collision probability of the case
-- it leaves dv = v' - v_old on the photons it hits and dv = 0 on the others, which is what the sweep reads.  What is quoted is
the wall time around the synchronising call, ``--runs`` repeats after one warm-up call, the median with the spread
(max - min) / median.  One JSON line each:
  surface_nobody_hit   the yardstick: Device.surface_reflect about a sphere the cloud is wholly outside of -- r and dr of three
                       axes, 48 B per slot (fp64), same store, same process; once more behind the cases
  nobody_scattered     collision probability 0: the three dv rows are read and nothing else, 24 B per slot; its ratio to the
                       yardstick (the condition: its median is not above the yardstick's median plus the yardstick's own spread)
  tenth_scattered      collision probability 0.1, spread evenly over the store (every wave diverges)
  all_scattered        collision probability above 1: every photon; Henyey-Greenstein (g = 0.85) and Rayleigh
Scattered lanes also load v (3 words) and write v and dv (6 words): bytes_per_slot = 3 words + share * 9 words.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicl_amd import _hip as hip  # noqa: E402

C_LIT, H_LIT, DT = 299792458.0, 6.62607015e-34, 0.0005
STEP = C_LIT * DT
ORIGIN = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP)


class Isotropic:
    origin, e1, e2, d = ORIGIN, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "point", 0.0, 0.0


FAR = tuple(o + 100.0 * STEP * a for o, a in zip(ORIGIN, Isotropic.d))     # a sphere of radius STEP there: nobody is hit
# case -> (collision probability of the scatter step that prepares the state, the laws timed)
CASES = [("nobody_scattered", 0.0, [("hg", 0.85)]),
         ("tenth_scattered", 0.1, [("hg", 0.85)]),
         ("all_scattered", 2.0, [("hg", 0.85), ("rayleigh", 0.0)])]


def stats(t):
    med = statistics.median(t)
    return {"s": t, "median_s": med, "spread": (max(t) - min(t)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtype", default="f64")
    a = ap.parse_args()
    esz = 8 if a.dtype == "f64" else 4
    base = {"n": a.n, "dtype": a.dtype}

    def emit(case, **kw):
        print(json.dumps(dict(base, case=case, **kw)), flush=True)

    dev = hip.Device(0)
    try:
        dev.store_alloc(a.n, a.dtype)
        dev.fill_photons(a.n, 0, C_LIT, 1.0, 3.0, 1)

        def reset(p, launch):
            dev.apply_source(Isotropic, C_LIT, 1)
            dev.step_newton(DT)
            hits = dev.step_scatter_isotropic(p / STEP, 1.0, 0, C_LIT, H_LIT, None, hip.RNG_PHILOX, 1, launch)   # pcoll = A*n*|dr| = p
            dev.sync()
            return hits

        def yardstick(name):
            reset(0.0, 0)
            dev.surface_reflect(STEP, FAR, 1.0, "lambertian", C_LIT, 1, 1)   # the first look at the store pays the core's materialise pass
            t, got = [], (0, 0)
            for k in range(a.runs):
                t0 = time.perf_counter()
                got = dev.surface_reflect(STEP, FAR, 1.0, "lambertian", C_LIT, 1, 2 + k)
                t.append(time.perf_counter() - t0)
            y = stats(t)
            emit(name, out=int(sum(got)), GBps=6 * esz * a.n / y["median_s"] / 1e9, **y)
            return y
        y = yardstick("surface_nobody_hit")
        for case, p, laws in CASES:
            for phase, g in laws:
                t, got, hits = [], 0, 0
                for k in range(a.runs + 1):
                    hits = reset(p, 1 + k)
                    t0 = time.perf_counter()
                    got = dev.phase_redirect(phase, g, C_LIT, 1, 1 + k)
                    if k:                                     # (the first call is the warm-up)
                        t.append(time.perf_counter() - t0)
                s = stats(t)
                share = got / a.n
                bps = (3 + 9 * share) * esz
                emit(case, phase=phase, g=g, share_scattered=share, scatter_hits=hits, bytes_per_slot=bps,
                     GBps=bps * a.n / s["median_s"] / 1e9, over_yardstick=s["median_s"] / y["median_s"],
                     within=bool(s["median_s"] <= y["median_s"] * (1.0 + y["spread"])), **s)
        yardstick("surface_nobody_hit_again")
    finally:
        dev.close()


if __name__ == "__main__":
    main()
