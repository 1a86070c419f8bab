#!/usr/bin/env python3
"""The flow of the reference's examples/planck_distribution.ipynb with its own spellings (``import phys``, dict
constructor, ScatterSphericalStep, TracePathMeasureStep(id_info_fn, trace_dv), ScatterMeasureStep(measure_E=True)):
photons drawn from a 2000 K Planck distribution, wavelength-dependent scattering, and at four distances the energy
spectrum of the photons passing by -- blue is scattered out of the beam first.

    python examples/planck_measure.py [n_photons] [steps]
    python examples/planck_measure.py [n_photons] [steps] --binned     the four planes as 50-bin histograms (E_bins=), on a
                                                                       PhotonBatch created in device memory: any size
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import phys                      # noqa: E402   (the reference's older package name)
import phys.light                # noqa: E402
import phys.newton               # noqa: E402

binned = "--binned" in sys.argv
argv = [x for x in sys.argv[1:] if x != "--binned"]
n = int(argv[0]) if len(argv) > 0 else 2000
steps = int(argv[1]) if len(argv) > 1 else 220
T = 2000


def run_binned():
    """The same flow with the spectra binned on the device: photons from the binned Planck sampler as a PhotonBatch, the
    device RNG, and per plane a histogram over 50 energy bins instead of the list of energies."""
    lo, hi = phys.light.E_from_wavelength(500000e-9), phys.light.E_from_wavelength(100e-9)
    edges = np.linspace(float(np.asarray(lo)), float(np.asarray(hi)) * 0.25, 51)
    sim = phys.Simulation({"cl_on": True, "rng": "philox", "seed": 3, "exit": lambda cond: cond.t >= 0.0005 * (steps - 0.5)})
    sim.add_objs(phys.light.generate_photons_bulk(n, min=lo, max=hi, seed=3, T=T, bins=5000))
    sim.add_step(0, phys.UpdateTimeStep(lambda x: 0.0005))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    sim.add_step(2, phys.light.ScatterSphericalStep(0.00000000000001, 0.000000000000005, wavelength_dep_scattering=True))
    sim.add_step(4, phys.light.ScatterMeasureStep(None, measure_n=True,
                                                  measure_locs=[[x * (phys.light.c) * 0.0005 * 50, 0, 0] for x in range(1, 5)],
                                                  measure_E=True, E_bins=edges))
    sim.start()
    sim.join()
    assert sim.error is None
    planes = sim.steps[4].data
    print("%d photons, %d steps, run time %.2f s (binned spectra)" % (n, len(planes), sim.run_time))
    mid = 0.5 * (edges[:-1] + edges[1:])
    for y in range(4 if len(planes) else 0):
        k = max(range(len(planes)), key=lambda i: planes[i][2 + 2 * y])     # the step in which the unscattered photons pass
        cnt, hist = planes[k][2 + 2 * y], planes[k][3 + 2 * y]
        peak = 1e9 * float(phys.light.wavelength_from_E(mid[int(np.argmax(hist))])) if hist.sum() else float("nan")
        print("plane %d (step %d): %4d photons pass, %d in the bins, fullest bin around %.0f nm" % (y + 1, k + 1, cnt, hist.sum(), peak))


if binned:
    run_binned()
    sys.exit(0)
np.random.seed(3)
E = [phys.light.planck_phot_distribution(phys.light.E_from_wavelength(500000e-9), phys.light.E_from_wavelength(100e-9), T,
                                         bins=5000) for x in range(n)]
phot = phys.light.generate_photons_from_E(E)

sim = phys.Simulation({"cl_on": True, "exit": lambda cond: cond.t >= 0.0005 * (steps - 0.5)})
sim.add_objs(phot)
sim.add_step(0, phys.UpdateTimeStep(lambda x: 0.0005))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterSphericalStep(0.00000000000001, 0.000000000000005, wavelength_dep_scattering=True))
sim.add_step(3, phys.light.TracePathMeasureStep(None, id_info_fn=lambda x: str(x.E), trace_dv=True))
sim.add_step(4, phys.light.ScatterMeasureStep(None, measure_n=True,
                                              measure_locs=[[x * (phys.light.c) * 0.0005 * 50, 0, 0] for x in range(1, 5)],
                                              measure_E=True))
sim.start()
sim.join()
assert sim.error is None

trace, planes = sim.steps[3].data, sim.steps[4].data
scatterings = sum(z[1] for z in trace[1:])
print("%d photons, %d steps, %d scatterings in total, run time %.2f s" % (n, len(planes), scatterings, sim.run_time))
for y in range(4):
    k = 50 * (y + 1) - 1                                      # the step in which unscattered photons reach plane y
    if k < len(planes):
        Es = np.array(planes[k][3 + 2 * y], dtype=float)
        print("plane %d (step %d): %4d photons pass, median wavelength %.0f nm"
              % (y + 1, k + 1, len(Es), 1e9 * float(phys.light.wavelength_from_E(np.median(Es))) if len(Es) else float("nan")))
