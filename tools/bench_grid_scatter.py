#!/usr/bin/env python3
"""What one pass of the scattering on a grid of cells (Device.scatter_grid, GridScatterStep) costs on the device, beside one pass of
the scattering by layer and band on the same store.

    python tools/bench_grid_scatter.py [--n 100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons per size, one process.  A call changes the photons it scatters, so the state is made anew before every
timed call, on the device (not timed), as tools/bench_layered_scatter.py makes it: the photons are put on one point
(Device.apply_source, isotropic) -- ``one_cell``: they stay there, every photon of the store in ONE cell of the grid, what every bulk
run starts from -- and ``spread``: moved one Newton step, so that they stand on a sphere of one STEP about that point, which crosses
thousands of cells of the large grid.  What is quoted is the wall time around the synchronising call, ``--runs`` repeats after one
warm-up call, the median with the spread (max - min) / median.  One JSON line each, for the LDS form (16 x 16 x 16 cells: the table
and a workgroup's tallies in LDS) and the global form (128 x 128 x 64 = 2^20 cells: p read from device memory, hits added there):
  scatter_layered_p0       the yardstick: Device.scatter_layered with p = 0, first = 0 and one cell on the same store
  table_copies             what the call moves over the host link and nothing else, in the same context, through the ABI's own
                           copies (pcl_dev_alloc, pcl_h2d, pcl_d2h, pcl_dev_free): one block for the table, the table up, as many
                           bytes of tallies back -- 8 MB each way in the global form.  ``copy_share`` in the rows below is this
                           case's median over the row's; what is left of the difference to the LDS form's row -- which reads the
                           same rows of the store -- is the host's check and copy of the table and the reads of p
  p0_behind                p = 0, first = 0: v0 and the three r rows; nothing is drawn or written
  p1_behind / p1_first     p = 1: one Philox block for the draw, one for the direction, the sin / cos, v read and v and dv written, and
                           the tally: with ``one_cell`` every hit of the store lands in one cell
No ratio is fixed in advance: ``over_yardstick`` is the case's median over the yardstick's.  The argument arrays are made once,
outside the timed calls.
"""
import numpy as np

from sweep_bench import C_LIT, DT, H_LIT, ORIGIN, STEP, Isotropic, emit, hip, main, photons, timed, yardstick

AXES = ("x", "y", "z")
GRIDS = [("lds_16x16x16", (16, 16, 16)), ("global_128x128x64", (128, 128, 64))]
CASES = [("p0_behind", 0.0, False), ("p1_behind", 1.0, False), ("p1_first", 1.0, True)]


def edges_of(bins):
    return [ORIGIN[k] + np.linspace(-1.25, 1.25, b + 1) * STEP for k, b in enumerate(bins)]


def bench(n, runs, dtype):
    with photons(n, dtype) as dev:
        def reset(launch, move):
            dev.apply_source(Isotropic, C_LIT, 1)
            if move:
                dev.step_newton(DT)
            # pcoll = A*n*|dr| = 0: nobody interacts, dv = 0 is written for everybody
            dev.step_scatter_isotropic(0.0, 1.0, 0, C_LIT, H_LIT, None, hip.RNG_PHILOX, 1, launch)
            dev.sync()

        def copies(table):
            block = hip.DeviceArray.from_host(dev, table)               # one allocation, the table up
            block.get()                                                 # as many bytes back as the tallies have
            block.free()

        copy = {}
        for name, bins in GRIDS:
            table = np.zeros(bins)
            s, _, _ = timed(runs, lambda k: dev.sync(), lambda k: copies(table))
            copy[name] = s["median_s"]
            emit({"n": n, "dtype": dtype, "grid": name}, "table_copies", table_MB=table.nbytes / 1e6, **s)
        for where, move in (("spread", True), ("one_cell", False)):
            y, got = yardstick(runs, lambda: reset(0, move), lambda k: dev.scatter_layered(0.0, None, ORIGIN, None, False, C_LIT, 1, 1 + k)[1])
            emit({"n": n, "dtype": dtype, "photons": where}, "scatter_layered_p0", out=int(got), **y)
            for name, bins in GRIDS:
                edges = edges_of(bins)
                base = {"n": n, "dtype": dtype, "photons": where, "grid": name}
                for case, p, first in CASES:
                    table = np.full(bins, p)                        # (made once: not part of the timed call)
                    s, got, _ = timed(runs, lambda k: reset(1 + k, move),
                                      lambda k: dev.scatter_grid(table, AXES, edges, None, None, first, C_LIT, 1, 1 + k))
                    emit(base, case, first=int(first), share_exposed=got[0] / n, share_scattered=got[1] / n,
                         cells_hit=int((got[2] > 0).sum()), over_yardstick=s["median_s"] / y["median_s"],
                         copy_share=copy[name] / s["median_s"], **s)


if __name__ == "__main__":
    main(bench, "100000000")
