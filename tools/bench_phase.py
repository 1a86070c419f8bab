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
from sweep_bench import C_LIT, DT, H_LIT, ORIGIN, STEP, Isotropic, emit, hip, main, photons, timed, yardstick

FAR = tuple(o + 100.0 * STEP * a for o, a in zip(ORIGIN, Isotropic.d))     # a sphere of radius STEP there: nobody is hit
# case -> (collision probability of the scatter step that prepares the state, the laws timed)
CASES = [("nobody_scattered", 0.0, [("hg", 0.85)]),
         ("tenth_scattered", 0.1, [("hg", 0.85)]),
         ("all_scattered", 2.0, [("hg", 0.85), ("rayleigh", 0.0)])]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def reset(p, launch):
            dev.apply_source(Isotropic, C_LIT, 1)
            dev.step_newton(DT)
            hits = dev.step_scatter_isotropic(p / STEP, 1.0, 0, C_LIT, H_LIT, None, hip.RNG_PHILOX, 1, launch)   # pcoll = A*n*|dr| = p
            dev.sync()
            return hits

        def ground(name):
            y, got = yardstick(runs, lambda: reset(0.0, 0), lambda k: dev.surface_reflect(STEP, FAR, 1.0, "lambertian", C_LIT, 1, 1 + k))
            emit(base, name, out=int(sum(got)), GBps=6 * esz * n / y["median_s"] / 1e9, **y)
            return y
        y = ground("surface_nobody_hit")
        for case, p, laws in CASES:
            for phase, g in laws:
                s, got, hits = timed(runs, lambda k: reset(p, 1 + k), lambda k: dev.phase_redirect(phase, g, C_LIT, 1, 1 + k))
                share = got / n
                bps = (3 + 9 * share) * esz
                emit(base, case, phase=phase, g=g, share_scattered=share, scatter_hits=hits, bytes_per_slot=bps,
                     GBps=bps * n / s["median_s"] / 1e9, over_yardstick=s["median_s"] / y["median_s"],
                     within=bool(s["median_s"] <= y["median_s"] * (1.0 + y["spread"])), **s)
        ground("surface_nobody_hit_again")


if __name__ == "__main__":
    main(bench, "100000000")
