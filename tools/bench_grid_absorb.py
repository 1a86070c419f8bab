#!/usr/bin/env python3
"""What one pass of the absorption on a grid of cells (Device.absorb_grid, GridAbsorptionStep) costs on the device, beside one pass
of the scattering on a grid at p = 0 and one pass of the path absorption by layer on the same store, in the same run.

    python tools/bench_grid_absorb.py [--n 100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons per size, one process, made as tools/bench_grid_scatter.py makes its ``spread`` state: the photons are
put on one point (Device.apply_source, isotropic), moved one Newton step and handed dv = 0 by a scatter step that hits nobody.  The
tables are transparent (p = 0) and conservative (omega0 = 1): nothing is drawn or written, so the store stays as it is and a call
costs what it reads -- v0 and the three r rows, as the grid scatter at p = 0, plus the three dv rows of every moving photon when an
omega0 is given.  What is quoted is the wall time around the synchronising call, ``--runs`` repeats after one warm-up call, the
median with the spread (max - min) / median.  One JSON line each:
  scatter_grid_p0          the yardstick: Device.scatter_grid with p = 0, first = 0 on the LDS form's grid
  absorb_path_p0           Device.absorb_path with p = 0 and one layer: reads v0 only (no layer, no r)
  k / omega0 / both        Device.absorb_grid with that table or both, in the LDS form (16 x 16 x 16 cells with one table, 8 x 16 x 16
                           with both) and in the global form (17 x 16 x 16 cells)
  both_black               p = 1 and omega0 = 0 in the LDS form: every photon is absorbed along the path and parked -- one Philox block,
                           v and dv written, the tally; the state is made anew before every timed call
No ratio is fixed in advance: ``over_yardstick`` is the case's median over scatter_grid_p0's.  The argument arrays are made once,
outside the timed calls.
"""
import numpy as np

from sweep_bench import C_LIT, DT, H_LIT, ORIGIN, STEP, Isotropic, emit, hip, main, photons, timed, yardstick

AXES = ("x", "y", "z")
FORMS = [("lds", {"k": (16, 16, 16), "omega0": (16, 16, 16), "both": (8, 16, 16)}), ("global", dict.fromkeys(("k", "omega0", "both"), (17, 16, 16)))]


def edges_of(bins):
    return [ORIGIN[k] + np.linspace(-1.25, 1.25, b + 1) * STEP for k, b in enumerate(bins)]


def bench(n, runs, dtype):
    with photons(n, dtype) as dev:
        def reset(launch):
            dev.apply_source(Isotropic, C_LIT, 1)
            dev.step_newton(DT)
            # pcoll = A*n*|dr| = 0: nobody interacts, dv = 0 is written for everybody
            dev.step_scatter_isotropic(0.0, 1.0, 0, C_LIT, H_LIT, None, hip.RNG_PHILOX, 1, launch)
            dev.sync()

        base = {"n": n, "dtype": dtype}
        bins = (16, 16, 16)
        clear = np.zeros(bins)
        y, got = yardstick(runs, lambda: reset(0), lambda k: dev.scatter_grid(clear, AXES, edges_of(bins), None, None, False, C_LIT, 1, 1 + k)[0])
        emit(base, "scatter_grid_p0", grid="16x16x16", exposed=int(got), **y)
        s, got = yardstick(runs, lambda: None, lambda k: dev.absorb_path(0.0, None, ORIGIN, None, 1, 1 + k)[0])
        emit(base, "absorb_path_p0", exposed=int(got), over_yardstick=s["median_s"] / y["median_s"], **s)
        for form, grids in FORMS:
            for which in ("k", "omega0", "both"):
                bins = grids[which]
                p, om = (np.zeros(bins) if which != "omega0" else None), (np.ones(bins) if which != "k" else None)
                edges = edges_of(bins)
                assert hip.absorb_grid_lds_form(2 if which == "both" else 1, sum(b + 1 for b in bins), int(np.prod(bins))) == (form == "lds")
                s, got = yardstick(runs, lambda: None, lambda k: dev.absorb_grid(p, om, AXES, edges, None, None, 1, 1 + k)[0])
                emit(base, which, form=form, grid="x".join(map(str, bins)), share_exposed=int(got[0]) / n, absorbed=int(got[2] + got[3]),
                     over_yardstick=s["median_s"] / y["median_s"], **s)
        bins = (8, 16, 16)
        p, om, edges = np.ones(bins), np.zeros(bins), edges_of(bins)
        s, got, _ = timed(runs, lambda k: reset(1 + k), lambda k: dev.absorb_grid(p, om, AXES, edges, None, None, 1, 1 + k))
        emit(base, "both_black", form="lds", grid="8x16x16", share_absorbed=int(got[0][2]) / n, cells_hit=int((got[1] > 0).sum()),
             over_yardstick=s["median_s"] / y["median_s"], **s)


if __name__ == "__main__":
    main(bench, "100000000")
