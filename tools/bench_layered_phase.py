#!/usr/bin/env python3
"""What one pass of the layered phase function (Device.phase_layered, LayeredPhaseStep) costs on the device.

    python tools/bench_layered_phase.py [--n 100000000] [--runs 5] [--dtype f64]

tools/bench_phase.py's method: one store of ``--n`` photons, one process; the state is made anew before every timed call, on
the device (not timed): the photons are put on one point (isotropic), moved one Newton step of 150 km and handed to the scatter
step with the collision probability of the case.  What is quoted is the wall time around the synchronising call, ``--runs``
repeats after one warm-up call, the median with the spread (max - min) / median.  One JSON line each.  The yardstick is
Device.phase_redirect on the same store in the same process, at the same share scattered, before and after the cases:
  phase_nobody_scattered, phase_tenth_scattered, phase_all_scattered (hg, g = 0.85), and ..._again behind the cases
  nobody_scattered     collision probability 0, single hg law: the three dv rows are read and nothing else, 24 B per slot (fp64);
                       the condition: its median is not above the yardstick's nobody-scattered median plus the yardstick's own spread
  tenth_scattered      collision probability 0.1, single hg law
  all_scattered_hg     every photon, single ("hg", 0.85), no layers: the yardstick's 96 B per slot; its ratio to
                       phase_all_scattered is quoted (the project's aim for a sweep of equal bytes: 1.25)
  all_scattered_layers every photon, three layers that all hold photons (Rayleigh | 0.3 Rayleigh + 0.7 hg | hg): r is loaded as well
  all_scattered_table  every photon, one 1024-bin table (Henyey-Greenstein's density at the bins' centres), no layers
Scattered lanes also load v (3 words) and write v and dv (6 words), with layers r (3 words) too.
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
from physicl_amd import light  # noqa: E402

C_LIT, H_LIT, DT = 299792458.0, 6.62607015e-34, 0.0005
STEP = C_LIT * DT
ORIGIN = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP)
G = 0.85


class Isotropic:
    origin, e1, e2, d = ORIGIN, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "point", 0.0, 0.0


def hg_table(bins):
    edges = np.linspace(-1.0, 1.0, bins + 1)
    mid = 0.5 * (edges[1:] + edges[:-1])
    return ("table", edges, (1.0 - G * G) / (1.0 + G * G - 2.0 * G * mid) ** 1.5)


# the photons stand one move from the source, on a sphere: layers about a centre 0.8 moves off it cut that sphere into three
CENTER = (ORIGIN[0] + 0.8 * STEP, ORIGIN[1], ORIGIN[2])
SINGLE = dict(laws=[("hg", G)], weights=None, edges=None)
LAYERS = dict(laws=["rayleigh", ("hg", G)], weights=[[1, 0], [0.3, 0.7], [0, 1]], edges=np.array([0.0, 0.7, 1.3, 3.0]) * STEP)
TABLE = dict(laws=[hg_table(1024)], weights=None, edges=None)
# case -> (collision probability of the scatter step that prepares the state, the step's arguments, the yardstick's case)
CASES = [("nobody_scattered", 0.0, SINGLE, "phase_nobody_scattered"),
         ("tenth_scattered", 0.1, SINGLE, "phase_tenth_scattered"),
         ("all_scattered_hg", 2.0, SINGLE, "phase_all_scattered"),
         ("all_scattered_layers", 2.0, LAYERS, "phase_all_scattered"),
         ("all_scattered_table", 2.0, TABLE, "phase_all_scattered")]
YARDSTICKS = [("phase_nobody_scattered", 0.0), ("phase_tenth_scattered", 0.1), ("phase_all_scattered", 2.0)]


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

        def timed(p, call):
            t, got = [], None
            for k in range(a.runs + 1):
                reset(p, 1 + k)
                t0 = time.perf_counter()
                got = call(1 + k)
                if k:                                         # (the first call is the warm-up)
                    t.append(time.perf_counter() - t0)
            return stats(t), got

        def yardsticks(suffix):
            out = {}
            for name, p in YARDSTICKS:
                y, got = timed(p, lambda n_pass: dev.phase_redirect("hg", G, C_LIT, 1, n_pass))
                share = got / a.n
                emit(name + suffix, share_scattered=share, GBps=(3 + 9 * share) * esz * a.n / y["median_s"] / 1e9, **y)
                out[name] = y
            return out
        yard = yardsticks("")
        for case, p, spec, against in CASES:
            laws, _, cum, edges, center = light._check_layered_phase(spec["laws"], spec["weights"], spec["edges"], CENTER)
            s, got = timed(p, lambda n_pass: dev.phase_layered(laws, cum, edges, center, C_LIT, 1, n_pass))
            scattered, redirected, by_layer, by_law = got
            share = scattered / a.n
            bps = (3 + (9 + (3 if edges is not None else 0)) * share) * esz
            y = yard[against]
            emit(case, share_scattered=share, redirected=redirected, by_layer=by_layer.tolist(), by_law=by_law.tolist(), bytes_per_slot=bps,
                 GBps=bps * a.n / s["median_s"] / 1e9, over_yardstick=s["median_s"] / y["median_s"],
                 within=bool(s["median_s"] <= y["median_s"] * (1.0 + y["spread"])), **s)
        yardsticks("_again")
    finally:
        dev.close()


if __name__ == "__main__":
    main()
