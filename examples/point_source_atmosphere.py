#!/usr/bin/env python3
"""A photon source on the Earth's surface under an exponential atmosphere -- the radial variable-n expression of the reference's
examples (n(r) = 2.5e25 m^-3 * exp(-(|r| - 6371 km) / 8.6 km)) with photons that do NOT start at the origin along +x:

    python examples/point_source_atmosphere.py [n_photons] [passes] [--cone | --beam-down | --default] [--profile] [--shells]
                                               [--ground [ALBEDO]] [--phase rayleigh | hg:G | isotropic]

default: a point source at (6371 km, 0, 0) emitting isotropically; ``--cone``: a 0.3 rad cone pointing up (+x) from a 1 km disc;
``--beam-down``: a 10 km gaussian beam entering from 100 km above the surface along -x; ``--default``: the same step list from
the batch's default source (origin, +x) for comparison.  The photons never exist as Python objects: they are created and given
their positions and directions on the device, and stepped 32 passes per launch like every other bulk run.  ``--profile``
records where they are every 32 passes -- altitude shells of 5 km up to 200 km (a radius axis about the Earth's centre) and a
y-z image -- as integer grids made on the device (PositionGridMeasureStep), and prints the last profile.  ``--shells``
tallies what passes through the ground and through the spheres 10, 50 and 100 km above it on every pass -- outward and inward
counts per shell and a histogram of the direction cosine against the local vertical (ShellCrossingMeasureStep), the top one
printed.  A flux needs every pass, so with ``--shells`` the run drops to one launch per light step (sim.launch_note says so).
``--ground [ALBEDO]`` gives the problem its ground: the Earth's surface reflects (SurfaceReflectStep, lambertian; ALBEDO defaults
to 0.3, the rest is absorbed and stays on the ground at rest) instead of letting the photons through the planet; the reflected
and absorbed totals are printed, and with ``--shells`` the run is made a second time without the ground and the outward counts
through the top shell (100 km) of the two runs are printed side by side.
``--phase rayleigh``, ``--phase hg:0.85`` or ``--phase isotropic`` puts a PhaseFunctionStep directly behind the scatter step: the
photons it hits leave with an angle drawn from that phase function about the direction they came from (without it they leave
with the reference's own angles, which do not depend on it).  One launch per light step, as with ``--shells``; the number of
photons re-directed is printed.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import physicl as phys          # noqa: E402
import physicl.light as light   # noqa: E402
import physicl.newton as newton  # noqa: E402

argv = sys.argv[1:]
albedo = None
if "--ground" in argv:
    at = argv.index("--ground")
    albedo = 0.3
    if at + 1 < len(argv) and not argv[at + 1].startswith("--"):
        albedo = float(argv.pop(at + 1))
phase = None
if "--phase" in argv:
    at = argv.index("--phase")
    name, _, g_text = (argv.pop(at + 1) if at + 1 < len(argv) else "").partition(":")
    phase = (name, float(g_text) if g_text else 0.0)
args = [a for a in argv if not a.startswith("--")]
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



def run(ground):
    """One run of the step list, with the reflecting ground (``ground``: its albedo) or without (None)."""
    sim = phys.Simulation(cl_on=True, seed=1234, exit=lambda cond: cond.t >= dt * (passes - 0.5))
    sim.add_step(0, phys.UpdateTimeStep(lambda c: dt))
    sim.add_step(1, newton.NewtonianKinematicsStep())
    # (the reference hands the kernel A := n, n := A: with variable_n the user's n scales the expression -- a cross-section of 4e-30 m^2)
    sim.add_step(2, light.ScatterIsotropicStep(n=4e-30, A=1.0, variable_n=True, variable_n_fn=cl_n))
    angles = light.PhaseFunctionStep(*phase) if phase is not None else None
    if angles is not None:                                     # directly behind the scatter step (steps run in the order they were added)
        sim.add_step("phase", angles)
    signs = light.ScatterSignMeasureStep(None, True)
    sim.add_step(3, signs)
    shells = light.ScatterMeasureStep(None, True, [[R + 20e3, np.nan, np.nan], [np.nan, 0.0, np.nan]])   # 20 km up; the plane y = 0
    sim.add_step(4, shells)
    profile = image = tally = floor = None
    if "--profile" in sys.argv:                                # behind the last light step: the 32-pass launches are kept
        profile = light.PositionGridMeasureStep(None, ("r",), [R + np.linspace(0.0, 200e3, 41)], every=32)
        image = light.PositionGridMeasureStep(None, ("y", "z"), [np.linspace(-300e3, 300e3, 129)] * 2, every=32, measure_n=False)
        sim.add_step(5, profile)
        sim.add_step(6, image)
    if "--shells" in sys.argv:                                 # the ground and three altitudes, about the Earth's centre
        tally = light.ShellCrossingMeasureStep(None, R + np.array([0.0, 10e3, 50e3, 100e3]), mu_bins=np.linspace(-1.0, 1.0, 11))
        sim.add_step(7, tally)
    if ground is not None:                                     # last in the pass: the tally before it sees the incoming move
        floor = light.SurfaceReflectStep(R, albedo=ground)
        sim.add_step(8, floor)
    sim.add_objs(light.generate_photons_bulk(n, min=light.E_from_wavelength(700e-9), max=light.E_from_wavelength(200e-9), seed=1234, source=source))
    sim.prepare()                                              # the photons are created now: run_time below is stepping only
    sim.start()
    sim.join()
    if sim.error is not None:
        raise sim.error
    return sim, signs, shells, profile, image, tally, floor, angles


bare_top = None
if albedo is not None and "--shells" in sys.argv:              # the same run without the ground, for the top-of-atmosphere count
    bare = run(None)
    bare_top = int(sum(row[2][3] for row in bare[5].data))
    print("without the ground: %d photons x %d steps in %.2f s" % (n, len(bare[0].ts), bare[0].run_time))
    bare[0].close(download=False)
    del bare
sim, signs, shells, profile, image, tally, floor, angles = run(albedo)
steps = len(sim.ts)
print("source:", source)
print("%d photons x %d steps in %.2f s  ->  %.3g particle-steps/s" % (n, steps, sim.run_time, n * steps / sim.run_time))
print("launches by formulation (sim.schedule):", dict(sim.schedule), sim.launch_note or "")
for row in signs.data[-3:]:
    print("[t, N, #vx>0, #vy>0, #vz>0]:", [float(x) for x in row])
for row in shells.data[-3:]:
    print("[t, N, crossed x = R + 20 km, crossed y = 0]:", [float(x) for x in row])
print("scattered in the last step:", sim.hits)
if angles is not None:
    print("phase function %s (g = %g): %d photons re-directed over %d passes" % (angles.phase, angles.g, sum(int(row[1]) for row in angles.data), len(angles.data)))
if profile is not None and profile.data:
    t, N, shells_now = profile.data[-1]
    print("altitude profile at t = %g s (%d records, one every 32 passes): %d of %d photons between 0 and 200 km" % (float(t), len(profile.data), shells_now.sum(), N))
    for k in range(0, 40, 4):
        print("  %3d - %3d km: %d" % (5 * k, 5 * k + 20, shells_now[k:k + 4].sum()))
    img = image.data[-1][1]
    print("y-z image, 128 x 128 cells of 4.7 km: %d photons inside, %d cells hit, brightest cell %d" % (img.sum(), np.count_nonzero(img), img.max()))
if tally is not None:
    out, inn = (np.array([row[k] for row in tally.data]) for k in (2, 3))
    print("crossings of the ground, 10, 50 and 100 km, summed over %d passes: outward %s, inward %s" % (len(tally.data), out.sum(axis=0).tolist(), inn.sum(axis=0).tolist()))
    for row in tally.data[-3:]:
        print("[t, N, out, in]:", float(row[0]), row[1], row[2].tolist(), row[3].tolist())
    print("escapes through 100 km by direction cosine against the vertical, 10 bins over [-1, 1]:", np.sum([row[4][3] for row in tally.data], axis=0).tolist())
if floor is not None:
    print("the ground (albedo %g, lambertian): %d reflected, %d absorbed over %d passes" % (albedo, sum(int(row[1]) for row in floor.data), sum(int(row[2]) for row in floor.data), len(floor.data)))
    if tally is not None:
        print("outward through the top of the atmosphere (100 km): %d with the ground, %d without" % (int(sum(row[2][3] for row in tally.data)), bare_top))
