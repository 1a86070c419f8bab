#!/usr/bin/env python3
"""What one ScatterMeasureStep(measure_E=True) row costs on the device: the list form against the binned form.

    python tools/bench_spectrum.py [--n 10000000] [--runs 3] [--dtype f64] [--fractions all,half,1pct]

A bulk population (pcl_store_fill_photons) is moved once, scattered with hit probability p and moved again; the four
planes stand just short of where an unscattered photon ends, so about 1 - p of the store crosses them (all / half / 1 %).
Timed (wall time around the synchronising calls, ``--runs`` runs, the median is quoted):
  list      4 x Device.plane_energies with the copy and .tolist() -- what a row of the list form costs
  binned    one Device.plane_spectra call, 4 planes x 50 bins
  counters  Device.step_counters with the same planes: k_counters, the yardstick for an HBM-bound sweep of such rows
Bytes per slot: binned reads r0 and dr0 (the planes share the axis) and E of the crossing lanes' cache lines (counted in
full: 24 B fp64); counters reads v0..v2, r0 and dr0 (40 B fp64).  One JSON line per case.

    python tools/bench_spectrum.py --loop [--n 1000000] [--passes 220] [--runs 3]

The loop of examples/planck_measure.py on a PhotonBatch (UpdateTime, Newton, wavelength-dependent ScatterSpherical, a
ScatterMeasureStep with the notebook's four planes in every pass), end to end (``sim.run_time``): measure_E=True as lists
against measure_E=True with 50 E_bins, ``--runs`` runs each.

    python tools/bench_spectrum.py --cache [--n 100000000] [--runs 5]

What the wavelength-term cache costs after a binned measure: pcl_step_plane_spectra reads E through pcl_store_field_ptr, which
marks the cache invalid, so the next wavelength-dependent fused step rebuilds it (k_lam4).  Timed: that fused step (synchronous)
behind a plane_spectra call against the same step behind a step_counters call, which leaves the cache alone.
(The list form does not exist beyond its own code path: running this file on an older commit times ``list`` and
``counters`` there and says that ``binned`` is missing.)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicl_amd import _hip as hip  # noqa: E402

C_LIT, DT = 299792458.0, 0.0005
STEP = C_LIT * DT
P_HIT = {"all": 0.0, "half": 0.5, "1pct": 0.995}


def timed(fn, runs):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def planck_loop(n, passes, E_bins):
    import physicl_amd as phys
    from physicl_amd import light, newton
    lo, hi = light.E_from_wavelength(500000e-9), light.E_from_wavelength(100e-9)
    sim = phys.Simulation(cl_on=True, rng="philox", seed=3, exit=lambda s: s.t >= DT * (passes - 0.5))
    sim.add_objs(light.generate_photons_bulk(n, min=lo, max=hi, seed=3, T=2000, bins=5000))
    sim.add_step(0, phys.UpdateTimeStep(lambda x: DT))
    sim.add_step(1, newton.NewtonianKinematicsStep())
    sim.add_step(2, light.ScatterSphericalStep(0.00000000000001, 0.000000000000005, wavelength_dep_scattering=True))
    m = light.ScatterMeasureStep(None, measure_n=True, measure_locs=[[x * C_LIT * DT * 50, 0, 0] for x in range(1, 5)],
                                 measure_E=True, **({} if E_bins is None else {"E_bins": E_bins}))
    sim.add_step(4, m)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    crossed = int(sum(r[2] + r[4] + r[6] + r[8] for r in m.data))
    sim.close(download=False)
    return sim.run_time, len(m.data), crossed


def loop_mode(a):
    from physicl_amd import light
    lo, hi = float(np.asarray(light.E_from_wavelength(500000e-9))), float(np.asarray(light.E_from_wavelength(100e-9)))
    edges = np.linspace(lo, hi * 0.25, 51)
    planck_loop(min(a.n, 10000), 5, edges)                      # library, device and hipRTC warm for both forms
    rec = {"mode": "loop", "n": a.n, "passes": a.passes}
    for name, bins in (("list", None), ("binned", edges), ("list_again", None), ("binned_again", edges)):
        runs = [planck_loop(a.n, a.passes, bins) for _ in range(a.runs)]
        rec[name + "_s"] = [r[0] for r in runs]
        rec[name + "_median_s"] = statistics.median(r[0] for r in runs)
        rec[name + "_rows_crossed"] = [runs[0][1], runs[0][2]]
    print(json.dumps(rec), flush=True)


def cache_mode(a):
    edges = np.linspace(2e-19, 8e-19, 51)
    planes = np.array([[STEP * (1.5 + k), np.nan, np.nan] for k in range(4)])
    dev = hip.Device(0)
    try:
        dev.store_alloc(a.n, a.dtype)
        dev.fill_photons(a.n, 0, C_LIT, 2e-19, 8e-19, 1)
        sc = dict(A=5e-32, n=1.0, flags=hip.SCATTER_WAVELENGTH, c=C_LIT, h=6.62607015e-34, rng_mode=hip.RNG_PHILOX, seed=1)
        rec = {"mode": "cache", "n": a.n, "dtype": a.dtype}
        step = 0
        for name, measure in (("after_counters", lambda: dev.step_counters(planes)), ("after_spectra", lambda: dev.plane_spectra(planes, edges)),
                              ("after_counters_again", lambda: dev.step_counters(planes))):
            t = []
            for _ in range(a.runs + 1):
                measure()
                step += 1
                t0 = time.perf_counter()
                dev.step_fused(DT, scatter=dict(sc, step=step), planes=[], sync=True, lazy=True)
                t.append(time.perf_counter() - t0)
            rec[name + "_fused_s"] = t[1:]
            rec[name + "_fused_median_s"] = statistics.median(t[1:])
        print(json.dumps(rec), flush=True)
    finally:
        dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--cache", action="store_true")
    ap.add_argument("--passes", type=int, default=220)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--fractions", default="all,half,1pct")
    ap.add_argument("--skip-list", action="store_true", help="do not time the list form (1e8 photons: a 1e8-element Python list per plane)")
    a = ap.parse_args()
    if a.n is None:
        a.n = 1_000_000 if a.loop else 100_000_000 if a.cache else 10_000_000
    if a.loop:
        return loop_mode(a)
    if a.cache:
        return cache_mode(a)
    esz = 8 if a.dtype == "f64" else 4
    edges = np.linspace(1.0, 3.0, 51)
    planes = np.array([[STEP * (1.99 + 0.001 * k), np.nan, np.nan] for k in range(4)])
    for frac in a.fractions.split(","):
        dev = hip.Device(0)
        try:
            dev.store_alloc(a.n, a.dtype)
            dev.fill_photons(a.n, 0, C_LIT, 1.0, 3.0, 1)
            dev.step_newton(DT)
            if P_HIT[frac] > 0:
                dev.step_scatter_isotropic(P_HIT[frac] / STEP, 1.0, 0, C_LIT, 0.0, None, hip.RNG_PHILOX, 1, 1)
            dev.step_newton(DT)
            cnt = dev.step_counters(planes)                     # warm-up of the yardstick, and the crossing counts
            rec = {"n": a.n, "dtype": a.dtype, "case": frac, "crossing": [int(x) for x in cnt[4:]]}
            t = timed(lambda: dev.step_counters(planes), a.runs)
            rec["counters_s"] = t
            rec["counters_GBps"] = 5 * esz * a.n / statistics.median(t) / 1e9
            if not a.skip_list:
                def lists():
                    return [dev.plane_energies(pl, n_hint=int(cnt[4 + p])).tolist() for p, pl in enumerate(planes)]
                lists()
                t = timed(lists, a.runs)
                rec["list_s"], rec["list_median_s"] = t, statistics.median(t)
            if hasattr(dev, "plane_spectra"):
                counts, hist = dev.plane_spectra(planes, edges)
                assert np.array_equal(counts, cnt[4:])
                t = timed(lambda: dev.plane_spectra(planes, edges), a.runs)
                rec["binned_s"], rec["binned_median_s"] = t, statistics.median(t)
                rec["binned_GBps"] = 3 * esz * a.n / statistics.median(t) / 1e9
                rec["in_bins"] = [int(x) for x in hist.sum(axis=1)]
            else:
                rec["binned_s"] = None
            print(json.dumps(rec), flush=True)
        finally:
            dev.close()


if __name__ == "__main__":
    main()
