#!/usr/bin/env python3
"""What one pass of the phase function by grid cell (Device.phase_grid, GridPhaseStep) costs on the device.

    python tools/bench_grid_phase.py [--n 100000000] [--runs 5] [--dtype f64]

tools/bench_layered_phase.py's method: one store of ``--n`` photons, one process; the state is made anew before every timed call, on
the device (not timed): the photons are put on one point (isotropic), moved one Newton step of 150 km and handed to the scatter step
with a collision probability of a third.  What is quoted is the wall time around the synchronising call, ``--runs`` repeats after one
warm-up call, the median with the spread (max - min) / median.  One JSON line each.  The yardstick is Device.phase_layered on the same
store in the same process, with the same two laws in three layers that all hold photons, before and after the cases:
  layered, and layered_again behind the cases
  grid_64      4 x 4 x 4 cells of 0.6 moves about the source, cloudy cells on a checkerboard (0.1 Rayleigh + 0.9 hg), Rayleigh in the
               clear cells and outside: a map of 64 bytes
  grid_4352    17 x 16 x 16 cells over the same box: a map of 4352 bytes; the difference to grid_64 is the longer searches (4 and 5 probes
               an axis against 2) and the map's spread over cache lines
  grid_r64     one radius axis of 64 bins about ``layered``'s centre: ``layered``'s own distance and one search, so what it costs over
               ``layered`` is the map's read
Scattered lanes load dv (3 words, everybody), v (3) and r (3), read one byte of the map and write v and dv (6 words).
"""
import numpy as np

from sweep_bench import C_LIT, DT, H_LIT, ORIGIN, STEP, Isotropic, emit, hip, main, photons, timed
from physicl_amd import light, light_grid  # noqa: E402

G = 0.85
P_SCATTER = 1.0 / 3.0
LAWS = ["rayleigh", ("hg", G)]
CENTER = (ORIGIN[0] + 0.8 * STEP, ORIGIN[1], ORIGIN[2])                 # tools/bench_layered_phase.py's: the layers cut the photons' sphere in three
LAYERS = dict(weights=[[1, 0], [0.3, 0.7], [0, 1]], edges=np.array([0.0, 0.7, 1.3, 3.0]) * STEP)
MIXTURES = [[1, 0], [0.1, 0.9]]                                         # clear, cloudy


def box(shape):
    """``shape`` cells over the box of 1.2 moves about the source (the photons stand one move out: some are outside), a checkerboard."""
    edges = [ORIGIN[k] + np.linspace(-1.2, 1.2, nb + 1) * STEP for k, nb in enumerate(shape)]
    return dict(axes=("x", "y", "z"), edges=edges, mixture=np.indices(shape).sum(axis=0) % 2, center=(0, 0, 0))


CASES = [("grid_64", box((4, 4, 4))), ("grid_4352", box((17, 16, 16))),
         ("grid_r64", dict(axes=("r",), edges=[np.linspace(0.0, 3.0, 65) * STEP], mixture=np.arange(64) % 2, center=CENTER))]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def reset(launch):
            dev.apply_source(Isotropic, C_LIT, 1)
            dev.step_newton(DT)
            hits = dev.step_scatter_isotropic(P_SCATTER / STEP, 1.0, 0, C_LIT, H_LIT, None, hip.RNG_PHILOX, 1, launch)   # pcoll = A*n*|dr|
            dev.sync()
            return hits

        def yardstick(name):
            laws, _, cum, edges, center = light._check_layered_phase(LAWS, LAYERS["weights"], LAYERS["edges"], CENTER)
            y, got, _ = timed(runs, lambda k: reset(1 + k), lambda k: dev.phase_layered(laws, cum, edges, center, C_LIT, 1, 1 + k))
            share = got[0] / n
            emit(base, name, share_scattered=share, redirected=got[1], by_layer=got[2].tolist(), by_law=got[3].tolist(),
                 GBps=(3 + 12 * share) * esz * n / y["median_s"] / 1e9, **y)
            return y
        y = yardstick("layered")
        for case, spec in CASES:
            laws, _, cum, axes, edges, mixture, outside, center = light_grid._check_grid_phase(
                LAWS, MIXTURES, spec["axes"], spec["edges"], spec["mixture"], 0, spec["center"])
            s, got, _ = timed(runs, lambda k: reset(1 + k),
                              lambda k: dev.phase_grid(laws, cum, axes, edges, center, mixture, outside, C_LIT, 1, 1 + k))
            scattered, redirected, by_mixture, by_law = got
            share = scattered / n
            emit(base, case, cells=int(mixture.size), share_scattered=share, redirected=redirected, by_mixture=by_mixture.tolist(),
                 by_law=by_law.tolist(), GBps=(3 + 12 * share) * esz * n / s["median_s"] / 1e9, over_layered=s["median_s"] / y["median_s"], **s)
        yardstick("layered_again")


if __name__ == "__main__":
    main(bench, "100000000")
