#!/usr/bin/env python3
"""What one pass of the absorbing medium (Device.absorb_scattered, AbsorptionStep) costs on the device.

    python tools/bench_absorb.py [--n 10000000,100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons per size, one process.  A call changes the photons it absorbs, so the state is made anew before
every timed call, on the device (not timed), as tools/bench_phase.py makes it: the photons are put on one point
(Device.apply_source, isotropic), moved one Newton step of 150 km and handed to the scatter step (Device.step_scatter_isotropic,
constant n) with the collision probability of the case -- it leaves dv = v' - v_old on the photons it hits and dv = 0 on the
others, which is what the sweep reads.  What is quoted is the wall time around the synchronising call, ``--runs`` repeats after
one warm-up call, the median with the spread (max - min) / median.  One JSON line each:
  phase_nobody_scattered   the yardstick: Device.phase_redirect with nobody scattered -- the three dv rows, 24 B per slot (fp64),
                           the same bytes, on the same store in the same process; once more behind the cases
  nobody_interacting       collision probability 0: the three dv rows are read and nothing else
  half_conservative        collision probability 0.5, omega0 = 1: interacting lanes are counted; no r, no draw, no write
  half_grey_one_layer      collision probability 0.5, omega0 = 0.5 in one layer that holds everybody: interacting lanes load r
                           (3 words) and draw, absorbed lanes write v and dv (6 words)
  half_grey_50x50          the same in 50 layers with 50 energy bins: absorbed lanes also load E and add to a histogram cell
No ratio is fixed in advance: ``over_yardstick`` is the case's median over the first yardstick's.
bytes_per_slot = 3 words + share_interacting * 3 words + share_absorbed * (6 words, + 1 with energy bins).
"""
import numpy as np

from sweep_bench import C_LIT, DT, H_LIT, ORIGIN, STEP, Isotropic, emit, hip, main, photons, timed, yardstick

# after the move every photon stands STEP from ORIGIN: about a centre 0.6 STEP off it the distances reach from 0.4 to 1.6 STEP
CENTER = (ORIGIN[0] + 0.6 * STEP, ORIGIN[1], ORIGIN[2])
ONE_LAYER = np.array([0.0, 2.0]) * STEP
LAYERS_50 = np.linspace(0.3, 1.7, 51) * STEP
E_BINS_50 = np.linspace(1.0, 3.0, 51)
# case -> (collision probability of the scatter step that prepares the state, omega0, layer edges, energy edges)
CASES = [("nobody_interacting", 0.0, 0.5, None, None),
         ("half_conservative", 0.5, 1.0, None, None),
         ("half_grey_one_layer", 0.5, [0.5], ONE_LAYER, None),
         ("half_grey_50x50", 0.5, [0.5] * 50, LAYERS_50, E_BINS_50)]


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

        def phase(name):
            y, got = yardstick(runs, lambda: reset(0.0, 0), lambda k: dev.phase_redirect("hg", 0.85, C_LIT, 1, 1 + k))
            emit(base, name, out=int(got), bytes_per_slot=3 * esz, GBps=3 * esz * n / y["median_s"] / 1e9, **y)
            return y
        y = phase("phase_nobody_scattered")
        for case, p, omega0, edges, E_edges in CASES:
            s, got, hits = timed(runs, lambda k: reset(p, 1 + k), lambda k: dev.absorb_scattered(omega0, edges, CENTER, E_edges, 1, 1 + k))
            interacted, absorbed = got[0] / n, got[1] / n
            bps = (3 + 3 * interacted * (edges is not None) + (6 + (E_edges is not None)) * absorbed) * esz
            emit(base, case, layers=0 if edges is None else len(edges) - 1, E_bins=0 if E_edges is None else len(E_edges) - 1,
                 share_interacting=interacted, share_absorbed=absorbed, scatter_hits=hits, bytes_per_slot=bps,
                 GBps=bps * n / s["median_s"] / 1e9, over_yardstick=s["median_s"] / y["median_s"], **s)
        phase("phase_nobody_scattered_again")


if __name__ == "__main__":
    main(bench, "10000000,100000000")
