#!/usr/bin/env python3
"""What one pass of the walls of a box (Device.box_walls, BoxBoundaryStep) costs on the device, beside the refracting sphere's sweep
(Device.refract_surface) on the same store in the same process -- the sibling that reads the most similar rows.

    python tools/bench_box_walls.py [--n 100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons, one process.  A call changes the photons that cross, so the state is made anew before every timed
call, on the device (not timed), as tools/bench_refract.py makes it: the photons are put on one point (Device.apply_source,
isotropic) and moved one Newton step of 150 km, so that they stand on a sphere of one STEP about that point.  What is quoted is the
wall time around the synchronising call, ``--runs`` repeats after one warm-up call, the median with the spread (max - min) / median.
One JSON line each:
  refract_nobody_crossing     the yardstick: Device.refract_surface without Fresnel's draw and a sphere the cloud is wholly outside
                              of; r and dr, 48 B per slot (fp64), nothing is written
  periodic_nobody_outside     three periodic walls two STEP from the point: v and r, 48 B per slot, nothing is written
  periodic_everybody_outside  a box that begins two STEP beyond the point on every axis: every photon is outside on all three axes;
                              one division and one floor per axis, r is written (72 B per slot)
  mirror_everybody_outside    the same box with three mirrors: dr and dv are read and, after an odd number of bounces, v, dr and dv of
                              the axis written back beside r (up to 192 B per slot)
  open_everybody_outside      the same box with three open walls: everybody is parked, v and dv are written (96 B per slot)
No ratio is fixed in advance: ``over_refract`` is the case's median over the yardstick's.
"""
from bench_surface import off
from sweep_bench import C_LIT, DT, ORIGIN, STEP, Isotropic, emit, main, photons, timed

NEAR = ([o - 2.0 * STEP for o in ORIGIN], [o + 2.0 * STEP for o in ORIGIN])
AWAY = ([o + 2.0 * STEP for o in ORIGIN], [o + 4.5 * STEP for o in ORIGIN])
# case -> (walls, box, words read and written per slot)
CASES = [("periodic_nobody_outside", "periodic", NEAR, 6), ("periodic_everybody_outside", "periodic", AWAY, 9),
         ("mirror_everybody_outside", "mirror", AWAY, 24), ("open_everybody_outside", "open", AWAY, 12)]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def reset(k):
            dev.apply_source(Isotropic, C_LIT, 1)
            dev.step_newton(DT)
            dev.sync()

        y, got, _ = timed(runs, reset, lambda k: int(dev.refract_surface(STEP, 1.5, 1.0, off(100.0), False, C_LIT, 1, 1 + k)[:5].sum()))
        emit(base, "refract_nobody_crossing", crossing=got, bytes_per_slot=6 * esz, GBps=6 * esz * n / y["median_s"] / 1e9, **y)
        for case, walls, (lo, hi), words in CASES:
            s, got, _ = timed(runs, reset, lambda k: dev.box_walls((walls,) * 3, lo, hi))
            emit(base, case, moving=int(got[0]), multi=int(got[1]), crossed=got[2:].reshape(3, 2).tolist(), bytes_per_slot=words * esz,
                 GBps=words * esz * n / s["median_s"] / 1e9, over_refract=s["median_s"] / y["median_s"], **s)


if __name__ == "__main__":
    main(bench, "100000000")
