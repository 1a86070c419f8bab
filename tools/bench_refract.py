#!/usr/bin/env python3
"""What one pass of the refracting sphere (Device.refract_surface, RefractiveSurfaceStep) costs on the device, beside the ground's
sweep (Device.surface_reflect) on the same store in the same process.

    python tools/bench_refract.py [--n 100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons, one process.  A call changes the photons that cross, so the state is made anew before every timed
call, on the device (not timed), as tools/bench_surface.py makes it: the photons are put on one point (Device.apply_source) and
moved one Newton step of 150 km.  What is quoted is the wall time around the synchronising call, ``--runs`` repeats after one
warm-up call, the median with the spread (max - min) / median.  One JSON line each:
  nobody_crossing      isotropic source, a sphere the cloud is wholly outside of: the ground (specular), then the refracting sphere
                       with and without Fresnel's draw; 48 B per slot (fp64) are read and nothing is written
  everybody_crossing   a beam, a sphere just ahead of it that every move enters: the ground (specular: no draw; lambertian: one
                       block), then the refracting sphere (n = 1.5) with Fresnel's draw (one block per photon) and without
No ratio is fixed in advance: ``over_ground`` is the case's median over the ground's specular median of the same case.
Crossing lanes also load v (3 words) and write r, v, dr, dv (12 words): bytes_per_slot = 6 words + share_crossing * 15 words.
"""
from bench_surface import Beam, off
from sweep_bench import C_LIT, DT, STEP, Isotropic, emit, main, photons, timed

N_INSIDE = 1.5
# case -> (source, centre of the sphere, its radius): the position before the move is outside every one of them
CASES = [("nobody_crossing", Isotropic, off(100.0), STEP),
         ("everybody_crossing", Beam, off(1.2, Beam.d), 0.5 * STEP)]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def reset(source):
            dev.apply_source(source, C_LIT, 1)
            dev.step_newton(DT)
            dev.sync()

        for case, source, center, radius in CASES:
            sweeps = [("ground_specular", lambda k: sum(dev.surface_reflect(radius, center, 1.0, "specular", C_LIT, 1, 1 + k))),
                      ("ground_lambertian", lambda k: sum(dev.surface_reflect(radius, center, 1.0, "lambertian", C_LIT, 1, 1 + k))),
                      ("refract_fresnel", lambda k: int(dev.refract_surface(radius, N_INSIDE, 1.0, center, True, C_LIT, 1, 1 + k)[:5].sum())),
                      ("refract_plain", lambda k: int(dev.refract_surface(radius, N_INSIDE, 1.0, center, False, C_LIT, 1, 1 + k)[:5].sum()))]
            ground = None
            for name, call in sweeps:
                s, got, _ = timed(runs, lambda k: reset(source), call)
                ground = ground or s["median_s"]
                share = got / n
                bps = (6 + 15 * share) * esz
                emit(base, case, sweep=name, share_crossing=share, bytes_per_slot=bps, GBps=bps * n / s["median_s"] / 1e9,
                     over_ground=s["median_s"] / ground, **s)


if __name__ == "__main__":
    main(bench, "100000000")
