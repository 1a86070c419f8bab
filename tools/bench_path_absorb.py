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
import numpy as np

from sweep_bench import C_LIT, DT, H_LIT, ORIGIN, STEP, Isotropic, emit, hip, main, photons, timed, yardstick

LAYERS = np.array([0.0, 0.5, 0.9, 1.1, 2.0]) * STEP            # after the move everybody stands STEP from ORIGIN: in the third layer
BANDS = np.linspace(1.0, 3.0, 65)                               # the fill's energies reach from 1 to 3
# case -> (everybody parked first, p, edges, E_edges)
CASES = [("everybody_at_rest", True, np.full(4, 0.5), LAYERS, None),
         ("nobody_absorbed_layers", False, np.zeros(4), LAYERS, None),
         ("nobody_absorbed_cells", False, np.zeros((4, 64)), LAYERS, BANDS),
         ("half_absorbed", False, 0.5, None, None)]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def reset(parked, launch):
            dev.apply_source(Isotropic, C_LIT, 1)
            dev.step_newton(DT)
            # pcoll = A*n*|dr| = 0: nobody interacts, dv = 0 is written for everybody
            dev.step_scatter_isotropic(0.0, 1.0, 0, C_LIT, H_LIT, None, hip.RNG_PHILOX, 1, launch)
            if parked:
                assert dev.absorb_path(1.0, None, None, None, 1, launch)[1] == n
            dev.sync()

        def phase(name):
            y, got = yardstick(runs, lambda: reset(False, 0), lambda k: dev.phase_redirect("hg", 0.85, C_LIT, 1, 1 + k))
            emit(base, name, out=int(got), bytes_per_slot=3 * esz, GBps=3 * esz * n / y["median_s"] / 1e9, **y)
            return y
        y = phase("phase_nobody_scattered")
        for case, parked, p, edges, E_edges in CASES:
            s, got, _ = timed(runs, lambda k: reset(parked, 1 + k), lambda k: dev.absorb_path(p, edges, ORIGIN, E_edges, 1, 1 + k))
            moving, gone = 0.0 if parked else 1.0, got[1] / n
            bps = (1 + 2 * (1.0 - moving) + moving * (3 * (edges is not None) + (E_edges is not None)) + 6 * gone) * esz
            emit(base, case, layers=0 if edges is None else len(edges) - 1, bands=0 if E_edges is None else len(E_edges) - 1,
                 share_exposed=got[0] / n, share_absorbed=gone, bytes_per_slot=bps, GBps=bps * n / s["median_s"] / 1e9,
                 over_yardstick=s["median_s"] / y["median_s"], **s)
        phase("phase_nobody_scattered_again")


if __name__ == "__main__":
    main(bench, "10000000,100000000")
