#!/usr/bin/env python3
"""What one pass of the layered phase function (Device.phase_layered, LayeredPhaseStep) costs on the device.

    python tools/bench_layered_phase.py [--n 100000000] [--runs 5] [--dtype f64]

tools/bench_phase.py's method: one store of ``--n`` photons, one process; the state is made anew before every timed call, on
the device (not timed): the photons are put on one point (isotropic), moved one Newton step of 150 km and handed to the scatter
step with the collision probability of the case.  What is quoted is the wall time around the synchronising call, ``--runs``
repeats after one warm-up call, the median with the spread (max - min) / median.  One JSON line each.  The yardstick is
Device.phase_redirect on the same store in the same process, at the same share scattered, before and after the cases:
  phase_nobody_scattered, phase_tenth_scattered, phase_all_scattered (hg, g = 0.85), and ..._again behind the cases
  nobody_scattered     collision probability 0, single hg law: the three dv rows are read and nothing else, 24 B per slot (fp64);
                       the condition: its median is not above the yardstick's nobody-scattered median plus the yardstick's own spread
  tenth_scattered      collision probability 0.1, single hg law
  all_scattered_hg     every photon, single ("hg", 0.85), no layers: the yardstick's 96 B per slot; its ratio to
                       phase_all_scattered is quoted (the project's aim for a sweep of equal bytes: 1.25)
  all_scattered_layers every photon, three layers that all hold photons (Rayleigh | 0.3 Rayleigh + 0.7 hg | hg): r is loaded as well
  all_scattered_table  every photon, one 1024-bin table (Henyey-Greenstein's density at the bins' centres), no layers
Scattered lanes also load v (3 words) and write v and dv (6 words), with layers r (3 words) too.
"""
import numpy as np

from sweep_bench import C_LIT, DT, H_LIT, ORIGIN, STEP, Isotropic, emit, hip, main, photons, timed
from physicl_amd import light  # noqa: E402

G = 0.85


def hg_table(bins):
    edges = np.linspace(-1.0, 1.0, bins + 1)
    mid = 0.5 * (edges[1:] + edges[:-1])
    return ("table", edges, (1.0 - G * G) / (1.0 + G * G - 2.0 * G * mid) ** 1.5)


# the photons stand one move from the source, on a sphere: layers about a centre 0.8 moves off it cut that sphere into three
CENTER = (ORIGIN[0] + 0.8 * STEP, ORIGIN[1], ORIGIN[2])
SINGLE = dict(laws=[("hg", G)], weights=None, edges=None)
LAYERS = dict(laws=["rayleigh", ("hg", G)], weights=[[1, 0], [0.3, 0.7], [0, 1]], edges=np.array([0.0, 0.7, 1.3, 3.0]) * STEP)
TABLE = dict(laws=[hg_table(1024)], weights=None, edges=None)
# case -> (collision probability of the scatter step that prepares the state, the step's arguments, the yardstick's case)
CASES = [("nobody_scattered", 0.0, SINGLE, "phase_nobody_scattered"),
         ("tenth_scattered", 0.1, SINGLE, "phase_tenth_scattered"),
         ("all_scattered_hg", 2.0, SINGLE, "phase_all_scattered"),
         ("all_scattered_layers", 2.0, LAYERS, "phase_all_scattered"),
         ("all_scattered_table", 2.0, TABLE, "phase_all_scattered")]
YARDSTICKS = [("phase_nobody_scattered", 0.0), ("phase_tenth_scattered", 0.1), ("phase_all_scattered", 2.0)]


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

        def yardsticks(suffix):                                # the phase function behind the same preparation, state anew every call
            out = {}
            for name, p in YARDSTICKS:
                y, got, _ = timed(runs, lambda k: reset(p, 1 + k), lambda k: dev.phase_redirect("hg", G, C_LIT, 1, 1 + k))
                share = got / n
                emit(base, name + suffix, share_scattered=share, GBps=(3 + 9 * share) * esz * n / y["median_s"] / 1e9, **y)
                out[name] = y
            return out
        yard = yardsticks("")
        for case, p, spec, against in CASES:
            laws, _, cum, edges, center = light._check_layered_phase(spec["laws"], spec["weights"], spec["edges"], CENTER)
            s, got, _ = timed(runs, lambda k: reset(p, 1 + k), lambda k: dev.phase_layered(laws, cum, edges, center, C_LIT, 1, 1 + k))
            scattered, redirected, by_layer, by_law = got
            share = scattered / n
            bps = (3 + (9 + (3 if edges is not None else 0)) * share) * esz
            y = yard[against]
            emit(base, case, share_scattered=share, redirected=redirected, by_layer=by_layer.tolist(), by_law=by_law.tolist(), bytes_per_slot=bps,
                 GBps=bps * n / s["median_s"] / 1e9, over_yardstick=s["median_s"] / y["median_s"],
                 within=bool(s["median_s"] <= y["median_s"] * (1.0 + y["spread"])), **s)
        yardsticks("_again")


if __name__ == "__main__":
    main(bench, "100000000")
