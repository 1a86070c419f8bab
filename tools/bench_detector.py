#!/usr/bin/env python3
"""What one detector image (Device.detector_image, DetectorMeasureStep) costs on the device.

    python tools/bench_detector.py [--n 100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons, one process: a beam from the point ORIGIN along +x, one Newton step, so every photon has made the same
move of one STEP.  Wall time around the synchronising call, ``--runs`` repeats after one warm-up call, the median is quoted with the
spread (max - min) / median.  Both calls read r and dr of three axes, 48 B per slot in fp64.  One JSON line each:
  shell_one            the yardstick: Device.shell_crossings with one shell that everybody crosses, counts only
  nobody_through       a 64 x 64 camera whose plane the beam never reaches: the two ballots per trip find nothing, no atomics at all
  everybody_seen       the same camera half a STEP down the beam, facing it, its disc wider than the beam: every photon goes through and is
                       seen, in the one pixel the beam's direction lies in -- 64-bit atomics of every lane on one device cell, the worst
                       an image can meet (a real aperture is small: hits are rare)
  everybody_seen_bands the same with 8 bands: E and a second binary search per photon; the cells are eight
  shell_one_again      the yardstick again, behind the cases
``over_shell`` is a case's median over the first yardstick's.
"""
import numpy as np

from sweep_bench import C_LIT, DT, ORIGIN, STEP, emit, main, photons, yardstick


class Beam:                                                     # every photon on ORIGIN, flying along +x
    origin, e1, e2, d = ORIGIN, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "beam", "point", 1.0, 0.0


FRAME = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])          # e1, e2, n: looking back down the beam
EDGES = np.linspace(-1.0, 1.0, 65)
BANDS = np.linspace(1.0, 3.0, 9)
AHEAD = (ORIGIN[0] + 0.5 * STEP, ORIGIN[1], ORIGIN[2])          # the move ends half a STEP behind this plane
FAR = (ORIGIN[0] + 5.0 * STEP, ORIGIN[1], ORIGIN[2])            # never reached
CASES = [("nobody_through", FAR, None), ("everybody_seen", AHEAD, None), ("everybody_seen_bands", AHEAD, BANDS)]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def prepare():
            dev.apply_source(Beam, C_LIT, 1)
            dev.step_newton(DT)
        shell = lambda k: dev.shell_crossings([0.5 * STEP], ORIGIN)              # noqa: E731
        y, got = yardstick(runs, prepare, shell)
        assert int(got[0][0][0]) == n
        emit(base, "shell_one", out=int(got[0][0][0]), GBps=6 * esz * n / y["median_s"] / 1e9, **y)
        for name, position, bands in CASES:
            s, (counts, image) = yardstick(runs, lambda: None, lambda k: dev.detector_image(position, FRAME, 0.25 * STEP, EDGES, EDGES, bands))
            assert counts.tolist() == ([0, 0] if position is FAR else [n, n]) and image.sum() == counts[1]
            emit(base, name, through=int(counts[0]), seen=int(counts[1]), cells_lit=int(np.count_nonzero(image)),
                 GBps=6 * esz * n / s["median_s"] / 1e9, over_shell=s["median_s"] / y["median_s"], **s)
        y2, _ = yardstick(runs, lambda: None, shell)
        emit(base, "shell_one_again", GBps=6 * esz * n / y2["median_s"] / 1e9, over_shell=y2["median_s"] / y["median_s"], **y2)


if __name__ == "__main__":
    main(bench, "100000000")
