#!/usr/bin/env python3
"""What one pass of the re-emission in place (Device.reemit_parked, ReemissionStep) costs on the device.

    python tools/bench_reemit.py [--n 10000000,100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons per size, one process.  A call changes the photons it re-emits, so the state is made anew before every
timed call, on the device (not timed): the photons are put on one point (Device.apply_source, isotropic) and moved one Newton step
of 150 km, so that everybody stands one STEP from the origin of the source and moves; then a grey gas (Device.absorb_path with p =
the share wanted) parks that share.  What is quoted is the wall time around the synchronising call, ``--runs`` repeats after one
warm-up call, the median with the spread (max - min) / median.  One JSON line each:
  phase_nobody_scattered   the yardstick: Device.phase_redirect (hg 0.85) with nobody scattered -- the three dv rows, 24 B per slot
                           (fp64), on the same store in the same process (tools/bench_phase.py's figure); once more behind the cases
  nobody_parked            four layers, two of them with a table: everybody moves and is decided by v0 alone: 8 B per slot
  one_percent_parked       the same with 1 % parked, all of them re-emitted
  everybody_parked         the same with everybody parked and re-emitted
  everybody_parked_plain   no layers, no table: r and E are never touched
No ratio is fixed in advance: ``over_yardstick`` is the case's median over the first yardstick's.
bytes_per_slot = 1 word (v0) + share_parked * (2 words (v1, v2) + 3 with layers (r)) + share_reemitted * (9 words written (v, dr, dv)
+ 1 with a table (E)).
"""
import numpy as np

from sweep_bench import C_LIT, DT, H_LIT, ORIGIN, STEP, Isotropic, emit, hip, main, photons, timed, yardstick

LAYERS = np.array([0.0, 0.5, 0.9, 1.1, 2.0]) * STEP            # after the move everybody stands STEP from ORIGIN: in the third layer
TABLE = (np.linspace(1.0, 3.0, 256), np.linspace(0.0, 1.0, 256))
LAYERED = dict(eta=1.0, angular=("isotropic", "isotropic", "lambertian", "isotropic"), tables=[None, TABLE, TABLE, None], edges=LAYERS)
PLAIN = dict(eta=1.0, angular="isotropic", tables=None, edges=None)
# case -> (the share the gas parks first, the sweep)
CASES = [("nobody_parked", 0.0, LAYERED), ("one_percent_parked", 0.01, LAYERED), ("everybody_parked", 1.0, LAYERED),
         ("everybody_parked_plain", 1.0, PLAIN)]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def reset(share, launch):
            dev.apply_source(Isotropic, C_LIT, 1)
            dev.step_newton(DT)
            # pcoll = A*n*|dr| = 0: nobody interacts, dv = 0 is written for everybody
            dev.step_scatter_isotropic(0.0, 1.0, 0, C_LIT, H_LIT, None, hip.RNG_PHILOX, 1, launch)
            if share:
                dev.absorb_path(share, None, None, None, 1, launch)
            dev.sync()

        def phase(name):
            y, got = yardstick(runs, lambda: reset(0.0, 0), lambda k: dev.phase_redirect("hg", 0.85, C_LIT, 1, 1 + k))
            emit(base, name, out=int(got), bytes_per_slot=3 * esz, GBps=3 * esz * n / y["median_s"] / 1e9, **y)
            return y
        y = phase("phase_nobody_scattered")
        for case, share, cfg in CASES:
            s, got, _ = timed(runs, lambda k: reset(share, 1 + k),
                              lambda k: dev.reemit_parked(C_LIT, cfg["eta"], cfg["angular"], cfg["tables"], cfg["edges"], ORIGIN, 1, 1 + k))
            parked, gone = got[0] / n, got[1] / n
            layers, table = cfg["edges"] is not None, cfg["tables"] is not None
            bps = (1 + parked * (2 + 3 * layers) + gone * (9 + table)) * esz
            emit(base, case, layers=len(cfg["edges"]) - 1 if layers else 0, share_parked=parked, share_reemitted=gone, by_layer=got[2].tolist(),
                 bytes_per_slot=bps, GBps=bps * n / s["median_s"] / 1e9, over_yardstick=s["median_s"] / y["median_s"], **s)
        phase("phase_nobody_scattered_again")


if __name__ == "__main__":
    main(bench, "10000000,100000000")
