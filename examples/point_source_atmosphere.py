#!/usr/bin/env python3
"""A photon source on the Earth's surface under an exponential atmosphere -- the radial variable-n expression of the reference's
examples (n(r) = 2.5e25 m^-3 * exp(-(|r| - 6371 km) / 8.6 km)) with photons that do NOT start at the origin along +x:

    python examples/point_source_atmosphere.py [n_photons] [passes] [--cone | --beam-down | --default]

default: a point source at (6371 km, 0, 0) emitting isotropically; ``--cone``: a 0.3 rad cone pointing up (+x) from a 1 km disc;
``--beam-down``: a 10 km gaussian beam entering from 100 km above the surface along -x; ``--default``: the same step list from
the batch's default source (origin, +x) for comparison.  The photons never exist as Python objects: they are created and given
their positions and directions on the device, and stepped 32 passes per launch like every other bulk run.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import physicl as phys          # noqa: E402
import physicl.light as light   # noqa: E402
import physicl.newton as newton  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(float(args[0])) if len(args) > 0 else 100_000_000
passes = int(args[1]) if len(args) > 1 else 200
R = 6371000.0
if "--cone" in sys.argv:
    source = light.PhotonSource(origin=(R, 0, 0), direction=(1, 0, 0), angular="cone", half_angle=0.3, spatial="disc", radius=1000.0)
elif "--beam-down" in sys.argv:
    source = light.PhotonSource(origin=(R + 100e3, 0, 0), direction=(-1, 0, 0), spatial="gaussian", radius=10e3)
elif "--default" in sys.argv:
    source = None
else:
    source = light.PhotonSource(origin=(R, 0, 0), angular="isotropic")
cl_n = "2.5E+25 * exp(-1 * (sqrt(pow(r0[gid], 2) + pow(r1[gid], 2) + pow(r2[gid], 2)) - 6371000.0)/(8600.0))"
dt = 1e-5                                                      # 3 km per pass

sim = phys.Simulation(cl_on=True, seed=1234, exit=lambda cond: cond.t >= dt * (passes - 0.5))
sim.add_step(0, phys.UpdateTimeStep(lambda c: dt))
sim.add_step(1, newton.NewtonianKinematicsStep())
# (the reference hands the kernel A := n, n := A: with variable_n the user's n scales the expression -- a cross-section of 4e-30 m^2)
sim.add_step(2, light.ScatterIsotropicStep(n=4e-30, A=1.0, variable_n=True, variable_n_fn=cl_n))
signs = light.ScatterSignMeasureStep(None, True)
sim.add_step(3, signs)
shells = light.ScatterMeasureStep(None, True, [[R + 20e3, np.nan, np.nan], [np.nan, 0.0, np.nan]])   # 20 km up; the plane y = 0
sim.add_step(4, shells)
sim.add_objs(light.generate_photons_bulk(n, min=light.E_from_wavelength(700e-9), max=light.E_from_wavelength(200e-9), seed=1234, source=source))

sim.prepare()                                                  # the photons are created now: run_time below is stepping only
sim.start()
sim.join()
if sim.error is not None:
    raise sim.error
steps = len(sim.ts)
print("source:", source)
print("%d photons x %d steps in %.2f s  ->  %.3g particle-steps/s" % (n, steps, sim.run_time, n * steps / sim.run_time))
print("launches by formulation (sim.schedule):", dict(sim.schedule), sim.launch_note or "")
for row in signs.data[-3:]:
    print("[t, N, #vx>0, #vy>0, #vz>0]:", [float(x) for x in row])
for row in shells.data[-3:]:
    print("[t, N, crossed x = R + 20 km, crossed y = 0]:", [float(x) for x in row])
print("scattered in the last step:", sim.hits)
