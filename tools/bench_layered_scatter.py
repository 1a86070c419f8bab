#!/usr/bin/env python3
"""What one pass of the scattering by layer and band (Device.scatter_layered, LayeredScatterStep) costs on the device, beside one
pass of the absorption along the path on the same store.

    python tools/bench_layered_scatter.py [--n 100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons per size, one process.  A call changes the photons it scatters, so the state is made anew before every
timed call, on the device (not timed), as tools/bench_path_absorb.py makes it: the photons are put on one point (Device.apply_source,
isotropic) and moved one Newton step, so that everybody stands one STEP from the origin of the source and moves.  What is quoted is
the wall time around the synchronising call, ``--runs`` repeats after one warm-up call, the median with the spread (max - min) /
median.  One JSON line each, for 1 cell (no layers, no bands) and for 64 layers x 64 bands:
  absorb_path_p0           the yardstick: Device.absorb_path with p = 0 on the same tables -- what the p = 0, first = 0 row below reads;
                           once more behind the cases
  p0_behind                p = 0, first = 0: v0, with layers the three r rows, with bands E; nothing is drawn or written
  p0_first                 p = 0, first = 1: the same reads, and the three dv rows written for everybody (24 B per slot in fp64)
  p1_behind / p1_first     p = 1: one Philox block for the draw, one for the direction, the sin / cos, v read and v and dv written
No ratio is fixed in advance: ``over_yardstick`` is the case's median over the first yardstick's of its tables.
bytes_per_slot = 1 word (v0) + 3 words with layers (r) + 1 with bands (E) + share_scattered * (2 words read (v1, v2) + 6 written
(v, dv)) + with first: (1 - share_scattered) * 3 words written (dv).
"""
import numpy as np

from sweep_bench import C_LIT, DT, H_LIT, ORIGIN, STEP, Isotropic, emit, hip, main, photons, timed, yardstick

LAYERS = np.linspace(0.0, 2.0, 65) * STEP                       # after the move everybody stands STEP from ORIGIN: in the 33rd layer
BANDS = np.linspace(1.0, 3.0, 65)                               # the fill's energies reach from 1 to 3
TABLES = [("1_cell", (1, 1), None, None), ("64x64_cells", (64, 64), LAYERS, BANDS)]
CASES = [("p0_behind", 0.0, False), ("p0_first", 0.0, True), ("p1_behind", 1.0, False), ("p1_first", 1.0, True)]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    with photons(n, dtype) as dev:
        def reset(launch):
            dev.apply_source(Isotropic, C_LIT, 1)
            dev.step_newton(DT)
            # pcoll = A*n*|dr| = 0: nobody interacts, dv = 0 is written for everybody
            dev.step_scatter_isotropic(0.0, 1.0, 0, C_LIT, H_LIT, None, hip.RNG_PHILOX, 1, launch)
            dev.sync()

        for name, shape, edges, E_edges in TABLES:
            base = {"n": n, "dtype": dtype, "tables": name}
            reads = 1 + 3 * (edges is not None) + (E_edges is not None)

            def gas(case):
                y, got = yardstick(runs, lambda: reset(0), lambda k: dev.absorb_path(np.zeros(shape), edges, ORIGIN, E_edges, 1, 1 + k)[1])
                emit(base, case, out=int(got), bytes_per_slot=reads * esz, GBps=reads * esz * n / y["median_s"] / 1e9, **y)
                return y
            y = gas("absorb_path_p0")
            for case, p, first in CASES:
                s, got, _ = timed(runs, lambda k: reset(1 + k),
                                  lambda k: dev.scatter_layered(np.full(shape, p), edges, ORIGIN, E_edges, first, C_LIT, 1, 1 + k))
                hit = got[1] / n
                bps = (reads + 8 * hit + 3 * first * (1.0 - hit)) * esz
                emit(base, case, first=int(first), share_exposed=got[0] / n, share_scattered=hit, bytes_per_slot=bps,
                     GBps=bps * n / s["median_s"] / 1e9, over_yardstick=s["median_s"] / y["median_s"], **s)
            gas("absorb_path_p0_again")


if __name__ == "__main__":
    main(bench, "100000000")
