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
from sweep_bench import C_LIT, DT, ORIGIN, STEP, Isotropic, emit, main, photons, timed, yardstick

X = Isotropic.d


class Beam(Isotropic):
    d, e1, e2 = (0.6, 0.8, 0.0), (-0.8, 0.6, 0.0), (0.0, 0.0, 1.0)
    angular = "beam"


def off(k, axis=X):
    return tuple(o + k * STEP * a for o, a in zip(ORIGIN, axis))


# case -> (source, centre of the sphere, its radius): the position before the move (ORIGIN) is outside every one of them
CASES = [("nobody_hit", Isotropic, off(100.0), STEP),
         ("tenth_hit", Isotropic, off(2.0), 1.8 ** 0.5 * STEP),          # |u - 2x|^2 = 5 - 4 u_x < 1.8  iff  u_x > 0.8
         ("all_hit", Beam, off(1.2, Beam.d), 0.5 * STEP)]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def reset(source):
            dev.apply_source(source, C_LIT, 1)
            dev.step_newton(DT)
            dev.sync()

        def shells(name):
            y, got = yardstick(runs, lambda: reset(Isotropic), lambda k: dev.shell_crossings([0.5 * STEP], ORIGIN))
            emit(base, name, out=int(got[0][0].sum()), GBps=6 * esz * n / y["median_s"] / 1e9, **y)
            return y
        y = shells("shells_1_counts")
        for case, source, center, radius in CASES:
            for mode in ("lambertian", "specular"):
                s, got, _ = timed(runs, lambda k: reset(source), lambda k: dev.surface_reflect(radius, center, 1.0, mode, C_LIT, 1, 1 + k))
                share = sum(got) / n
                bps = (6 + 15 * share) * esz
                emit(base, case, mode=mode, share_hit=share, bytes_per_slot=bps, GBps=bps * n / s["median_s"] / 1e9,
                     over_shells=s["median_s"] / y["median_s"], **s)
        shells("shells_1_counts_again")


if __name__ == "__main__":
    main(bench, "100000000")
