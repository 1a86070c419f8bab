#!/usr/bin/env python3
"""What one pass of the reflecting sphere (Device.surface_reflect, SurfaceReflectStep) costs on the device.

    python tools/bench_surface.py [--n 100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons, one process.  A call changes the photons it hits, so the state is made anew before every timed
call, on the device (not timed): the photons are put on one point (Device.apply_source) and moved one Newton step, so the last
move of every photon is one step of 150 km away from that point.  What is quoted is the wall time around the synchronising
call, ``--runs`` repeats after one warm-up call, the median with the spread (max - min) / median.  One JSON line each:
  shells_1_counts      the yardstick: Device.shell_crossings with one shell, counts only -- r and dr of three axes, 48 B per
                       slot (fp64), same store, same process; once more behind the cases
  nobody_hit           isotropic source, a sphere the cloud is wholly outside of; both modes; its ratio to the yardstick (the aim:
                       within 1.25)
  tenth_hit            isotropic source, a sphere two steps off that the cap u_x > 0.8 of the moves enters: one photon in ten,
                       spread evenly over the store (every wave diverges)
  all_hit              a beam, a sphere just ahead of it that every move enters
Hit lanes also load v (3 words) and write r, v, dr, dv (12 words): bytes_per_slot = 6 words + share_hit * 15 words.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicl_amd import _hip as hip  # noqa: E402

C_LIT, DT = 299792458.0, 0.0005
STEP = C_LIT * DT
ORIGIN = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP)
X = (1.0, 0.0, 0.0)


class Isotropic:
    origin, e1, e2, d = ORIGIN, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), X
    angular, spatial, cos_half_angle, radius = "isotropic", "point", 0.0, 0.0


class Beam(Isotropic):
    d, e1, e2 = (0.6, 0.8, 0.0), (-0.8, 0.6, 0.0), (0.0, 0.0, 1.0)
    angular = "beam"


def off(k, axis=X):
    return tuple(o + k * STEP * a for o, a in zip(ORIGIN, axis))


# case -> (source, centre of the sphere, its radius): the position before the move (ORIGIN) is outside every one of them
CASES = [("nobody_hit", Isotropic, off(100.0), STEP),
         ("tenth_hit", Isotropic, off(2.0), 1.8 ** 0.5 * STEP),          # |u - 2x|^2 = 5 - 4 u_x < 1.8  iff  u_x > 0.8
         ("all_hit", Beam, off(1.2, Beam.d), 0.5 * STEP)]


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

        def reset(source):
            dev.apply_source(source, C_LIT, 1)
            dev.step_newton(DT)
            dev.sync()

        def yardstick(name):
            reset(Isotropic)
            dev.shell_crossings([0.5 * STEP], ORIGIN)         # the first look at the store pays the core's materialise pass
            t = []
            for _ in range(a.runs):
                t0 = time.perf_counter()
                got = dev.shell_crossings([0.5 * STEP], ORIGIN)
                t.append(time.perf_counter() - t0)
            y = stats(t)
            emit(name, out=int(got[0][0].sum()), GBps=6 * esz * a.n / y["median_s"] / 1e9, **y)
            return y
        y = yardstick("shells_1_counts")
        for case, source, center, radius in CASES:
            for mode in ("lambertian", "specular"):
                t, got = [], (0, 0)
                for k in range(a.runs + 1):
                    reset(source)
                    t0 = time.perf_counter()
                    got = dev.surface_reflect(radius, center, 1.0, mode, C_LIT, 1, 1 + k)
                    if k:                                     # (the first call is the warm-up)
                        t.append(time.perf_counter() - t0)
                s = stats(t)
                share = sum(got) / a.n
                bps = (6 + 15 * share) * esz
                emit(case, mode=mode, share_hit=share, bytes_per_slot=bps, GBps=bps * a.n / s["median_s"] / 1e9,
                     over_shells=s["median_s"] / y["median_s"], **s)
        yardstick("shells_1_counts_again")
    finally:
        dev.close()


if __name__ == "__main__":
    main()
