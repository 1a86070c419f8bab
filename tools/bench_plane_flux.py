#!/usr/bin/env python3
"""What one flux map of planes (Device.plane_flux, PlaneFluxMapStep) costs on the device.

    python tools/bench_plane_flux.py [--n 100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons, one process: an isotropic point source on ORIGIN, one Newton step, so every photon has made a move of one
STEP in a direction of its own.  Wall time around the synchronising call, ``--runs`` repeats after one warm-up call, the median is quoted
with the spread (max - min) / median.  The yardsticks read r and dr of three axes, 48 B per slot in fp64; the flux map reads r and dr
of the normal axis (16 B per slot) and, for the lanes that crossed, of the two transverse axes -- whole cache lines, so what deferring
those loads saves depends on the crossing fraction.  One JSON line each:
  shell_one            the yardstick: Device.shell_crossings with one shell that everybody crosses, counts only
  detector_nobody      Device.detector_image with a 64 x 64 camera whose plane nobody reaches
  half_lds, half_global        one level a thousandth of a STEP above ORIGIN: half of the photons cross (all upward); 8 x 8 columns (128 cells, the LDS form)
                               and 64 x 64 columns (8192 cells, 64-bit atomics on the device block)
  twentieth_lds, twentieth_global   one level 0.9 STEP up: a twentieth crosses, in the same two forms
  half_lds_bands       the first case with 8 bands: E and a third binary search per crossing photon
  shell_one_again      the yardstick again, behind the cases
``over_shell`` is a case's median over the first yardstick's; ``GBps_all`` counts 48 B a slot as if every lane loaded everything.
"""
import numpy as np

from sweep_bench import C_LIT, DT, ORIGIN, STEP, emit, main, photons, yardstick      # (puts the repository root on sys.path)

from physicl_amd import _hip  # noqa: E402


class Point:                                                    # every photon on ORIGIN, flying its own way
    origin, e1, e2, d = ORIGIN, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "point", 0.0, 0.0


FRAME = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])          # e1, e2, n: looking back along x
FAR = (ORIGIN[0] + 5.0 * STEP, ORIGIN[1], ORIGIN[2])            # never reached
BANDS = np.linspace(1.0, 3.0, 9)


def columns(n):
    return [ORIGIN[k] + np.linspace(-1.5, 1.5, n + 1) * STEP for k in (1, 2)]


CASES = [("half_lds", 0.001, 8, None), ("half_global", 0.001, 64, None), ("twentieth_lds", 0.9, 8, None), ("twentieth_global", 0.9, 64, None),
         ("half_lds_bands", 0.001, 8, BANDS)]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def prepare():
            dev.apply_source(Point, C_LIT, 1)
            dev.step_newton(DT)
        shell = lambda k: dev.shell_crossings([0.5 * STEP], ORIGIN)              # noqa: E731
        y, got = yardstick(runs, prepare, shell)
        assert int(got[0][0][0]) == n
        emit(base, "shell_one", out=int(got[0][0][0]), GBps=6 * esz * n / y["median_s"] / 1e9, **y)
        s, (counts, image) = yardstick(runs, lambda: None, lambda k: dev.detector_image(FAR, FRAME, 0.25 * STEP, np.linspace(-1, 1, 65), np.linspace(-1, 1, 65)))
        assert counts.tolist() == [0, 0]
        emit(base, "detector_nobody", GBps=6 * esz * n / s["median_s"] / 1e9, over_shell=s["median_s"] / y["median_s"], **s)
        for name, up, n_col, bands in CASES:
            level, edges = [ORIGIN[0] + up * STEP], columns(n_col)
            form = _hip.plane_flux_lds_form(1, n_col, n_col, 0 if bands is None else len(bands) - 1)
            assert form == name.split("_")[1].startswith("lds")
            s, (counts, maps) = yardstick(runs, lambda: None, lambda k: dev.plane_flux("x", level, edges, bands))
            assert counts[1][0] == 0 and 0 < counts[0][0] < n and maps.sum() == counts[0][0]       # every crossing lands: the map spans the sphere
            emit(base, name, lds_form=bool(form), crossed=int(counts[0][0]), fraction=float(counts[0][0]) / n, cells_lit=int(np.count_nonzero(maps)),
                 GBps_all=6 * esz * n / s["median_s"] / 1e9, over_shell=s["median_s"] / y["median_s"], **s)
        y2, _ = yardstick(runs, lambda: None, shell)
        emit(base, "shell_one_again", GBps=6 * esz * n / y2["median_s"] / 1e9, over_shell=y2["median_s"] / y["median_s"], **y2)


if __name__ == "__main__":
    main(bench, "100000000")
