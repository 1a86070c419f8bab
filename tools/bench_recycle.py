#!/usr/bin/env python3
"""What one pass of the continuous source (Device.recycle_spent, RecycleStep) costs on the device.

    python tools/bench_recycle.py [--n 10000000,100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons per size, one process.  A call changes the photons it re-emits, so the state is made anew before
every timed call, on the device (not timed): the photons are put on one point (Device.apply_source, isotropic) and moved one
Newton step of 150 km, so that everybody stands one STEP from the origin of the source; for the half-spent cases an absorber
(Device.step_scatter_isotropic with collision probability 1, then Device.absorb_scattered with omega0 = 0.5) leaves half of them
at rest.  What is quoted is the wall time around the synchronising call, ``--runs`` repeats after one warm-up call, the median
with the spread (max - min) / median.  One JSON line each:
  phase_nobody_scattered   the yardstick: Device.phase_redirect with nobody scattered -- the three dv rows, 24 B per slot (fp64),
                           on the same store in the same process; once more behind the cases
  nobody_spent_at_rest     at_rest only, nobody at rest: the v rows are read and nothing else -- the yardstick's rows; a lane
                           whose v0 is not zero is decided and does not load v1 and v2, so 8 B per slot, not 24
  nobody_spent_rest_top    at_rest and a top beyond everybody: v0 and the three r rows, 32 B per slot (48 B of rows)
  half_spent               half of the photons at rest, a top beyond everybody: spent lanes draw twice and write r, v, dr, dv
  half_spent_table         the same with a spectrum of 1000 bins: spent lanes draw a third time, search the table and write E
No ratio is fixed in advance: ``over_yardstick`` is the case's median over the first yardstick's.
bytes_per_slot = 1 word (v0) + share_at_rest * 2 words (v1, v2) + share_not_at_rest * 3 words (r, with a top) + share_spent *
(12 words, + 1 with a spectrum).
"""
import numpy as np

from sweep_bench import C_LIT, DT, H_LIT, ORIGIN, STEP, Isotropic, emit, hip, main, photons, timed, yardstick

class Lamp:                                                     # what the spent photons are re-emitted by: two draws each
    origin, e1, e2, d = ORIGIN, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "disc", 0.0, 0.1 * STEP


TOP = 2.0 * STEP                                                # after the move everybody stands STEP from ORIGIN: nobody is beyond
GRID = np.linspace(1.0, 3.0, 1000)
CDF = np.linspace(0.0, 1.0, 1001)[1:]
# case -> (share of the photons left at rest by the absorber that prepares the state, at_rest, top, spectrum)
CASES = [("nobody_spent_at_rest", 0.0, True, None, None),
         ("nobody_spent_rest_top", 0.0, True, TOP, None),
         ("half_spent", 0.5, True, TOP, None),
         ("half_spent_table", 0.5, True, TOP, (GRID, CDF))]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def reset(share, launch):
            dev.apply_source(Isotropic, C_LIT, 1)
            dev.step_newton(DT)
            # pcoll = A*n*|dr|: 1 makes everybody interact, 0 nobody (dv = 0 either way or v' - v_old)
            dev.step_scatter_isotropic((1.0 if share else 0.0) / STEP, 1.0, 0, C_LIT, H_LIT, None, hip.RNG_PHILOX, 1, launch)
            if share:
                dev.absorb_scattered(1.0 - share, None, None, None, 1, launch)
            dev.sync()

        def phase(name):
            y, got = yardstick(runs, lambda: reset(0.0, 0), lambda k: dev.phase_redirect("hg", 0.85, C_LIT, 1, 1 + k))
            emit(base, name, out=int(got), bytes_per_slot=3 * esz, GBps=3 * esz * n / y["median_s"] / 1e9, **y)
            return y
        y = phase("phase_nobody_scattered")
        for case, share, at_rest, top, spectrum in CASES:
            s, got, _ = timed(runs, lambda k: reset(share, 1 + k),
                              lambda k: dev.recycle_spent(Lamp, C_LIT, at_rest, top, ORIGIN, spectrum, 1, 1 + k))
            rest, gone = got[0] / n, got[1] / n
            bps = (1 + 2 * rest + 3 * (1.0 - rest) * (top is not None) + (12 + (spectrum is not None)) * (rest + gone)) * esz
            emit(base, case, top=top is not None, table_bins=0 if spectrum is None else len(spectrum[1]), share_at_rest=rest, share_escaped=gone,
                 bytes_per_slot=bps, GBps=bps * n / s["median_s"] / 1e9, over_yardstick=s["median_s"] / y["median_s"], **s)
        phase("phase_nobody_scattered_again")


if __name__ == "__main__":
    main(bench, "10000000,100000000")
