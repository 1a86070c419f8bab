#!/usr/bin/env python3
"""A photon source on the Earth's surface under an exponential atmosphere -- the radial variable-n expression of the reference's
examples (n(r) = 2.5e25 m^-3 * exp(-(|r| - 6371 km) / 8.6 km)) with photons that do NOT start at the origin along +x:

    python examples/point_source_atmosphere.py [n_photons] [passes] [--cone | --beam-down | --default] [--profile] [--shells]
                                               [--ground [ALBEDO]] [--phase rayleigh | hg:G | isotropic] [--omega0 W | W1,W2,...]
                                               [--cloud LO,HI[,G]] [--cloud-tau TAU] [--cloud-field NX,NY,NZ:EXTENT:TAU] [--cloud-phase G] [--cloud-absorb OMEGA0[,K]] [--box periodic | mirror | open] [--recycle [TOP]] [--gas LO,HI,K[,EMIN,EMAX]] [--blue-sky]
                                               [--reemit [TG[,TA]]] [--ocean N] [--ground-bands E1,E2,...:a1,a2,...[:s1,...]]
                                               [--camera X,Y,Z:NX,NY,NZ:RADIUS:FOV_DEG:PIXELS] [--flux-map LEVEL[,LEVEL...]:HALF:N]

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
``--omega0 W`` makes the medium absorb: an AbsorptionStep behind the scatter step (and before the phase function) absorbs each
interacting photon with probability 1 - W and leaves it at rest where it was absorbed.  ``--omega0 W1,W2,...`` gives one
single-scattering albedo per altitude shell: the three shells between the ``--shells`` radii (ground, 10, 50, 100 km) with
three values, the forty 5 km shells of ``--profile`` with forty.  One launch per light step; the photons absorbed per layer are
printed beside the top-of-atmosphere and ground counts.
``--cloud LO,HI[,G]`` (altitudes in metres) gives the atmosphere a cloud layer: a LayeredPhaseStep in the place of the phase
function scatters by Rayleigh's law everywhere and, between the altitudes LO and HI, by a mixture of one part Rayleigh and nine
parts Henyey-Greenstein with the mean cosine G (default 0.85).  One launch per light step; the photons re-directed per layer and
per law are printed beside the shell counts.  Not together with ``--phase``: a pass holds one phase step.
``--cloud-tau TAU`` (with ``--cloud``) gives that cloud its own optical thickness: a LayeredScatterStep with the scattering coefficient
``TAU / (HI - LO)`` per metre between LO and HI, behind the clear air's scatter step and in front of the LayeredPhaseStep, which then
turns the cloud's hits about the direction they came from.  ``exposed``, ``scattered`` and ``scattered_by_cell`` summed over the passes
are printed beside the shell counts.  Without it the cloud changes the phase function only and the output is as it was.
``--cloud-field NX,NY,NZ:EXTENT:TAU`` puts a broken cloud field above the source: a GridScatterStep on a box of NX x NY x NZ cells,
EXTENT metres wide in y and z about the source's vertical and reaching from EXTENT / 4 to 3 EXTENT / 4 above the ground (x is the
vertical), whose scattering coefficient is a checkerboard of clear and cloudy columns: ``2 TAU / EXTENT`` per metre where NY- and
NZ-index add up to an even number -- a vertical path through a cloudy column has the optical thickness TAU -- and 0 beside it.  It
stands behind the clear air's scatter step (``first`` resolves to False) and in front of the phase step.  ``exposed``, ``scattered`` and
the column sums of ``scattered_by_cell`` over the passes are printed; with ``--camera`` looking down from above the box, e.g.
``--cloud-field 8,8,8:40000:4 --camera 6421000,0,0:-1,0,0:20000:60:32``, the image shows the gaps.  One launch per light step.
``--cloud-phase G`` (with ``--cloud-field``) gives the field's droplets their phase function: a GridPhaseStep on the field's cells in
the place of the phase function turns a photon scattered in a cloudy cell by a mixture of one part Rayleigh and nine parts
Henyey-Greenstein with the mean cosine G, and one scattered in a clear cell or anywhere outside the box (``outside``) by Rayleigh's law.
``by_mixture`` [clear, cloudy] and ``by_law`` [rayleigh, hg] summed over the passes are printed.  Not together with ``--phase`` or
``--cloud``: a pass holds one phase step.
``--cloud-absorb OMEGA0[,K]`` (with ``--cloud-field``) lets the field absorb: a GridAbsorptionStep on the field's cells behind the phase
step gives the cloudy cells the single-scattering albedo OMEGA0 (the clear ones 1) and, with K, the column of cells at y index 0 and z
index 1 -- a clear one -- the absorption coefficient K per metre: a column of water vapour.  ``exposed``, ``interacted``,
``absorbed_path`` and ``absorbed_hit`` summed over the passes and the column sums of ``absorbed_by_cell`` are printed.
``--box periodic | mirror | open`` (with ``--cloud-field``) gives the scene sides: a BoxBoundaryStep around the cloud field's box on its
two horizontal axes y and z (x, the vertical, has no wall), last in the pass, behind the ground and in front of a re-emission or the
recycling lamp.  ``periodic`` hands a photon that leaves the field sideways back in on the other side -- the boundary condition
domain-averaged fluxes of a cloud field need --, ``mirror`` folds it back at the wall, ``open`` parks it at rest (``--recycle`` then gives
its slot back to the source).  ``moving`` and ``crossed`` of the first and the last pass and their sums are printed, and the number of
photons inside the box's horizontal extent pass by pass: constant with ``periodic`` and ``mirror``.  One launch per light step.
``--recycle [TOP]`` (an altitude in metres, default 100 km) makes the source a continuous one: a RecycleStep at the end of every pass
gives the slots of the photons at rest (absorbed by the ground or the medium) and of those above TOP back to the source.  The
population stays constant; the emission rate (photons recycled per pass) and the counts at rest and through the top are printed as
they settle to the steady state.  One launch per light step.  Not with ``--default``: the step re-emits from a PhotonSource.
``--gas LO,HI,K[,EMIN,EMAX]`` puts an absorbing shell between the altitudes LO and HI (metres): a PathAbsorptionStep behind the scatter,
absorption and phase steps absorbs every photon that moves there with the probability 1 - exp(-K c dt) per pass -- K the absorption
coefficient per metre --, whether it scattered or not, and leaves it at rest.  With EMIN,EMAX (joules) only photons whose energy lies
in that band are absorbed: the escaping spectrum gets a band.  One launch per light step; ``absorbed_by_cell`` summed over the
passes is printed beside the shell counts.  ``--blue-sky`` makes the scatter step wavelength dependent (lambda**-4, scaled so that
550 nm scatters as the grey atmosphere does); with a band the gas then asks for E in every pass, which drops that step's term cache.
``--reemit [TG[,TA]]`` (kelvin, default 288,220) lets what was absorbed radiate again from where it was absorbed: a ReemissionStep behind
the ground and before the lamp of ``--recycle``.  The ground parks the photons it absorbs on its sphere up to rounding, so it gets a
thin shell of its own, R (1 - 1e-6) .. R (1 + 1e-6) -- wide enough for an fp32 store --, which emits cosine-weighted about the local
vertical (lambertian) from a Planck table of the temperature TG between 3 and 100 micrometres; the gas between it and 100 km (what
``--gas`` or ``--omega0`` absorbed there) re-emits isotropically from a table of TA.  ``parked``, ``reemitted`` and ``by_layer`` summed
over the passes are printed beside the shell counts, and a ShellCrossingMeasureStep with one energy bin over the two tables counts the
infrared photons through the ground's sphere: outward the ground's own glow (of the photons it parked a rounding below the sphere),
inward what the gas sends back down -- the greenhouse return flux, which no run without the option has: no photon of the source is
that red.  Try ``--ground 0.3 --gas 0,50000,2e-5 --reemit``.  One launch per light step.
``--ocean N`` puts an ocean of refractive index N under the atmosphere: a RefractiveSurfaceStep at the ground's radius -- photons
that reach the water are refracted into it by Snell's law or reflected off it with Fresnel's probability, and those that come back up
from below are refracted out or, beyond the critical angle, reflected back down -- with the ground 6 km below it (two moves: a photon
must not pass the sea floor within the move that took it into the water), black unless ``--ground`` gives it an albedo.  The step
changes directions, not speeds.  The six counts summed over the passes are printed: ``in_refracted``, ``in_reflected``,
``out_refracted``, ``out_reflected``, ``out_total``, and ``overshot`` (photons whose remaining move took them through the sphere once
more: none, for a sphere this large).  Try ``--ocean 1.33 --shells``.  One launch per light step.  Not with ``--reemit``: its ground
glows at the surface.
``--ground-bands E1,E2,...:a1,a2,...[:s1,...]`` makes the ground spectral: a SpectralSurfaceStep in the place of ``--ground``'s step, with
the band edges E1 < E2 < ... (joules, one more than bands), an albedo per band and -- optionally -- per band (or once for all) the share
of the reflected photons that is mirrored; the others leave cosine-weighted about the local vertical.  A photon that comes down with an
energy in no band is absorbed (``out_of_band``): the ground stays opaque.  ``reflected``, ``absorbed``, ``mirrored`` and ``out_of_band``
summed over the passes and the rows ``reflected_by_band`` / ``absorbed_by_band`` are printed beside the shell counts.  With ``--reemit``
the ground glows between 2e-21 and 6.6e-20 J and the source shines between 2.8e-19 and 9.9e-19 J: try
``--ground-bands 1e-21,1e-19,1e-18:0.02,0.3 --gas 0,50000,2e-5 --reemit --shells`` -- a ground that takes nearly all of the infrared that
the gas sends back down and reflects a third of the sunlight.  One launch per light step.
``--camera X,Y,Z:NX,NY,NZ:RADIUS:FOV_DEG:PIXELS`` puts an instrument into the scene: a DetectorMeasureStep, a disc of RADIUS metres about
(X, Y, Z) (metres from the Earth's centre) whose normal (NX, NY, NZ) points from the detector into the scene, with a square field of
view of FOV_DEG degrees to either side and PIXELS x PIXELS pixels, e.g. ``--camera 6471000,0,0:-1,0,0:20000:60:32`` looks straight down
from 100 km above the source.  Every pass tallies the photons that went through the disc from the front, by the direction they came
from; ``through`` and ``seen`` summed over the passes and a coarse text rendering of the exposure ``step.image`` are printed.  One launch
per light step, as with ``--shells``.
``--flux-map LEVEL[,LEVEL...]:HALF:N`` records the irradiance field: a PlaneFluxMapStep with the horizontal planes LEVEL metres above the
ground (x is the vertical; increasing) and N x N columns over HALF metres to either side of the source's vertical in y and z, in front of
the ground and the walls.  The up and down counts per level summed over the passes are printed, and beside ``--cloud-field`` the downward
map at the lowest level, so the shadow of the cloudy columns is visible: try ``--cloud-field 8,8,8:40000:4 --box periodic --beam-down
--flux-map 5000,35000:20000:8``.  One launch per light step.
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
bands = None
if "--ground-bands" in argv:
    at = argv.index("--ground-bands")
    try:
        parts = [[float(x) for x in part.split(",")] for part in (argv.pop(at + 1) if at + 1 < len(argv) else "").split(":")]
        bands = dict(E_edges=parts[0], albedo=parts[1], specular=0.0 if len(parts) < 3 else parts[2][0] if len(parts[2]) == 1 else parts[2])
        if len(parts) > 3:
            raise ValueError
    except (ValueError, IndexError):
        sys.exit("--ground-bands E1,E2,...:a1,a2,...[:s1,...]: the band edges in joules, an albedo per band and the mirrored share (one, or per band)")
phase = None
if "--phase" in argv:
    at = argv.index("--phase")
    name, _, g_text = (argv.pop(at + 1) if at + 1 < len(argv) else "").partition(":")
    phase = (name, float(g_text) if g_text else 0.0)
omega0 = None
if "--omega0" in argv:
    at = argv.index("--omega0")
    omega0 = [float(x) for x in (argv.pop(at + 1) if at + 1 < len(argv) else "").split(",")]
cloud = None
if "--cloud" in argv:
    at = argv.index("--cloud")
    cloud = [float(x) for x in (argv.pop(at + 1) if at + 1 < len(argv) else "").split(",")]
    if len(cloud) not in (2, 3) or not 0.0 < cloud[0] < cloud[1] < 1000e3:
        sys.exit("--cloud LO,HI[,G]: two altitudes in metres, 0 < LO < HI < 1000 km, and optionally the cloud's mean cosine")
    if phase is not None:
        sys.exit("--cloud and --phase: a pass holds one phase step")
    cloud = (cloud[0], cloud[1], cloud[2] if len(cloud) == 3 else 0.85)
cloud_tau = None
if "--cloud-tau" in argv:
    at = argv.index("--cloud-tau")
    try:
        cloud_tau = float(argv.pop(at + 1))
    except (IndexError, ValueError):
        cloud_tau = -1.0
    if cloud is None or not 0.0 <= cloud_tau < float("inf"):
        sys.exit("--cloud-tau TAU: the cloud's optical thickness, not negative, together with --cloud LO,HI[,G]")
cloud_field = None
if "--cloud-field" in argv:
    at = argv.index("--cloud-field")
    try:
        cells, extent, tau = (argv.pop(at + 1) if at + 1 < len(argv) else "").split(":")
        cloud_field = (tuple(int(x) for x in cells.split(",")), float(extent), float(tau))
        if len(cloud_field[0]) != 3 or min(cloud_field[0]) < 1 or not cloud_field[1] > 0.0 or not 0.0 <= cloud_field[2] < float("inf"):
            raise ValueError
    except ValueError:
        sys.exit("--cloud-field NX,NY,NZ:EXTENT:TAU: the cells of the box, its width in metres and the optical thickness of a cloudy column")
cloud_phase = None
if "--cloud-phase" in argv:
    at = argv.index("--cloud-phase")
    try:
        cloud_phase = float(argv.pop(at + 1))
    except (IndexError, ValueError):
        cloud_phase = 2.0
    if cloud_field is None or cloud is not None or phase is not None or not abs(cloud_phase) < 1.0:
        sys.exit("--cloud-phase G: the droplets' mean cosine, |G| < 1, together with --cloud-field NX,NY,NZ:EXTENT:TAU and without --phase or --cloud")
cloud_absorb = None
if "--cloud-absorb" in argv:
    at = argv.index("--cloud-absorb")
    try:
        cloud_absorb = [float(x) for x in argv.pop(at + 1).split(",")]
    except (IndexError, ValueError):
        cloud_absorb = []
    if cloud_field is None or len(cloud_absorb) not in (1, 2) or not 0.0 <= cloud_absorb[0] <= 1.0 or not 0.0 <= cloud_absorb[-1] < float("inf"):
        sys.exit("--cloud-absorb OMEGA0[,K]: the droplets' single-scattering albedo in [0, 1] and optionally the absorption coefficient per "
                 "metre of one column of cells, together with --cloud-field NX,NY,NZ:EXTENT:TAU")
box = None
if "--box" in argv:
    at = argv.index("--box")
    box = argv.pop(at + 1) if at + 1 < len(argv) else ""
    if box not in ("periodic", "mirror", "open") or cloud_field is None:
        sys.exit("--box periodic | mirror | open: the walls around the box of --cloud-field NX,NY,NZ:EXTENT:TAU")
recycle_top = None
if "--recycle" in argv:
    at = argv.index("--recycle")
    recycle_top = 100e3
    if at + 1 < len(argv) and not argv[at + 1].startswith("--"):
        recycle_top = float(argv.pop(at + 1))
    if not recycle_top > 0.0:
        sys.exit("--recycle TOP: an altitude in metres above the ground")
    if "--default" in argv:
        sys.exit("--recycle needs a source: not with --default")
gas = None
if "--gas" in argv:
    at = argv.index("--gas")
    gas = [float(x) for x in (argv.pop(at + 1) if at + 1 < len(argv) else "").split(",")]
    if len(gas) not in (3, 5) or not 0.0 <= gas[0] < gas[1] or not gas[2] >= 0.0 or (len(gas) == 5 and not gas[3] < gas[4]):
        sys.exit("--gas LO,HI,K[,EMIN,EMAX]: two altitudes in metres, 0 <= LO < HI, a coefficient per metre and optionally an energy band in joules")
reemit = None
if "--reemit" in argv:
    at = argv.index("--reemit")
    reemit = [288.0, 220.0]
    if at + 1 < len(argv) and not argv[at + 1].startswith("--"):
        given = [float(x) for x in argv.pop(at + 1).split(",")]
        reemit[:len(given)] = given
    if len(reemit) != 2 or not min(reemit) > 0.0:
        sys.exit("--reemit [TG[,TA]]: the temperatures of the ground and of the gas in kelvin")
ocean = None
if "--ocean" in argv:
    at = argv.index("--ocean")
    try:
        ocean = float(argv.pop(at + 1))
    except (IndexError, ValueError):
        ocean = None
    if ocean is None or not ocean > 0.0:
        sys.exit("--ocean N: the refractive index of the water, e.g. 1.33")
    if reemit is not None:
        sys.exit("--ocean and --reemit: the re-emitting ground stands at the surface")
    if albedo is None and bands is None:
        albedo = 0.0                                           # a black sea floor
ground = albedo if bands is None else bands                    # None: no ground; a number: a grey one; --ground-bands' tables: a spectral one
OCEAN_DEPTH = 6000.0                                           # two moves: the floor is not passed within the move into the water
camera = None
if "--camera" in argv:
    at = argv.index("--camera")
    try:
        where, look, rest = (argv.pop(at + 1) if at + 1 < len(argv) else "").split(":", 2)
        camera = dict(position=[float(x) for x in where.split(",")], normal=[float(x) for x in look.split(",")])
        camera["radius"], fov_deg, pixels = (float(x) for x in rest.split(":"))
        camera.update(fov=np.radians(fov_deg), pixels=(int(pixels), int(pixels)))
    except ValueError:
        sys.exit("--camera X,Y,Z:NX,NY,NZ:RADIUS:FOV_DEG:PIXELS: a position and a normal (metres, any length), a radius in metres, the half "
                 "angle of the field of view in degrees and the pixels per side")
flux_map = None
if "--flux-map" in argv:
    at = argv.index("--flux-map")
    try:
        lv, half_width, n_col = (argv.pop(at + 1) if at + 1 < len(argv) else "").split(":")
        flux_map = ([float(x) for x in lv.split(",")], float(half_width), int(n_col))
        if not flux_map[1] > 0.0 or flux_map[2] < 1:
            raise ValueError
    except ValueError:
        sys.exit("--flux-map LEVEL[,LEVEL...]:HALF:N: altitudes in metres above the ground (increasing), the map's half width in metres and the columns per side")
CLOUD_WEIGHTS = [[1, 0], [0.1, 0.9], [1, 0]]                  # below the cloud, in it, above it: (Rayleigh, Henyey-Greenstein)
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
SHELL_RADII = R + np.array([0.0, 10e3, 50e3, 100e3])
PROFILE_RADII = R + np.linspace(0.0, 200e3, 41)
layer_edges = None
if omega0 is not None and len(omega0) > 1:                     # one value per altitude shell of --shells / --profile
    fits = [e for flag, e in (("--shells", SHELL_RADII), ("--profile", PROFILE_RADII)) if flag in sys.argv and len(e) - 1 == len(omega0)]
    if not fits:
        sys.exit("--omega0 with %d values needs --shells (3 values: ground, 10, 50, 100 km) or --profile (40 values: 5 km shells)" % len(omega0))
    layer_edges = fits[0]


def run(ground):
    """One run of the step list, with the reflecting ground (``ground``: its albedo, or the tables of a spectral one) or without (None)."""
    sim = phys.Simulation(cl_on=True, seed=1234, exit=lambda cond: cond.t >= dt * (passes - 0.5))
    sim.add_step(0, phys.UpdateTimeStep(lambda c: dt))
    sim.add_step(1, newton.NewtonianKinematicsStep())
    # (the reference hands the kernel A := n, n := A: with variable_n the user's n scales the expression -- a cross-section of 4e-30 m^2)
    blue = "--blue-sky" in sys.argv                           # lambda**-4, equal to the grey cross-section at 550 nm
    sim.add_step(2, light.ScatterIsotropicStep(n=4e-30 * (550e-9 ** 4 if blue else 1.0), A=1.0, variable_n=True, variable_n_fn=cl_n,
                                               wavelength_dep_scattering=blue))
    medium = None
    if omega0 is not None:                                     # behind the scatter step, before the phase function
        medium = light.AbsorptionStep(omega0[0] if layer_edges is None else omega0, edges=layer_edges)
        sim.add_step("absorb", medium)
    angles = light.PhaseFunctionStep(*phase) if phase is not None else None
    droplets = None
    if cloud_tau is not None:                                  # behind the clear air's scatter step, in front of the phase step: first=False
        droplets = light.LayeredScatterStep([cloud_tau / (cloud[1] - cloud[0])], edges=[R + cloud[0], R + cloud[1]])
        sim.add_step("cloud", droplets)
    broken = None
    if cloud_field is not None:                                # a box of cells above the source, cloudy and clear columns in a checkerboard
        (nx, ny, nz), extent, tau = cloud_field
        _, iy, iz = np.indices((nx, ny, nz))
        broken = light.GridScatterStep(np.where((iy + iz) % 2 == 0, 2.0 * tau / extent, 0.0), ("x", "y", "z"),
                                       [R + np.linspace(0.25, 0.75, nx + 1) * extent, np.linspace(-0.5, 0.5, ny + 1) * extent,
                                        np.linspace(-0.5, 0.5, nz + 1) * extent])
        sim.add_step("cloud_field", broken)
        if cloud_phase is not None:                            # the field's cells again: the droplets' forward peak where it is cloudy
            angles = light.GridPhaseStep(["rayleigh", ("hg", cloud_phase)], [[1.0, 0.0], CLOUD_WEIGHTS[1]], broken.axes, broken.edges,
                                         mixture=(broken.k > 0).astype(np.int64), outside=0)
    if cloud is not None:                                      # from the Earth's centre to 1000 km up: Rayleigh, but for the cloud
        angles = light.LayeredPhaseStep(["rayleigh", ("hg", cloud[2])], CLOUD_WEIGHTS, edges=[0.0, R + cloud[0], R + cloud[1], R + 1000e3])
    if angles is not None:                                     # directly behind the scatter step (steps run in the order they were added)
        sim.add_step("phase", angles)
    heat = None
    if cloud_absorb is not None:                               # the field's cells once more: droplets that absorb, and a column of vapour
        column = np.zeros(broken.k.shape)
        column[:, 0, 1 % column.shape[2]] = cloud_absorb[1] if len(cloud_absorb) == 2 else 0.0       # (a clear column, where there is one)
        heat = light.GridAbsorptionStep(broken.axes, broken.edges, k=column if len(cloud_absorb) == 2 else None,
                                        omega0=np.where(broken.k > 0, cloud_absorb[0], 1.0))
        sim.add_step("cloud_absorb", heat)
    vapour = None
    if gas is not None:                                        # behind the scatter, absorption and phase steps, before the ground
        vapour = light.PathAbsorptionStep([gas[2]] if len(gas) == 3 else [[gas[2]]], edges=[R + gas[0], R + gas[1]],
                                          E_edges=None if len(gas) == 3 else gas[3:5])
        sim.add_step("gas", vapour)
    signs = light.ScatterSignMeasureStep(None, True)
    sim.add_step(3, signs)
    shells = light.ScatterMeasureStep(None, True, [[R + 20e3, np.nan, np.nan], [np.nan, 0.0, np.nan]])   # 20 km up; the plane y = 0
    sim.add_step(4, shells)
    profile = image = tally = floor = lamp = eye = None
    if "--profile" in sys.argv:                                # behind the last light step: the 32-pass launches are kept
        profile = light.PositionGridMeasureStep(None, ("r",), [PROFILE_RADII], every=32)
        image = light.PositionGridMeasureStep(None, ("y", "z"), [np.linspace(-300e3, 300e3, 129)] * 2, every=32, measure_n=False)
        sim.add_step(5, profile)
        sim.add_step(6, image)
    if "--shells" in sys.argv:                                 # the ground and three altitudes, about the Earth's centre
        tally = light.ShellCrossingMeasureStep(None, SHELL_RADII, mu_bins=np.linspace(-1.0, 1.0, 11))
        sim.add_step(7, tally)
    if camera is not None:                                     # before the ground, as the shells: it sees the incoming move
        eye = light.DetectorMeasureStep(None, **camera)        # (a malformed camera is a ValueError here, before anything runs)
        sim.add_step("camera", eye)
    irradiance = None
    if flux_map is not None:                                   # before the ground and the walls, as the shells: it sees the incoming move
        sides = np.linspace(-flux_map[1], flux_map[1], flux_map[2] + 1)
        irradiance = light.PlaneFluxMapStep(None, "x", R + np.array(flux_map[0]), [sides, sides])
        sim.add_step("flux_map", irradiance)
    glow = red = None
    if reemit is not None:                                     # Planck tables between 3 and 100 micrometres: the ground's, the gas's
        infrared = [light.generate_photons_bulk(1, min=light.E_from_wavelength(100e-6), max=light.E_from_wavelength(3e-6), T=T, bins=256)
                    for T in reemit]
        grid = np.concatenate([np.asarray(batch.table[1], dtype=np.float64) for batch in infrared])
        # who crosses the ground's sphere with a re-emitted energy (no photon of the source is that red); before the ground, as the shells
        red = light.ShellCrossingMeasureStep(None, [R], E_bins=[0.999 * grid.min(), 1.001 * grid.max()], measure_n=False)
        sim.add_step("infrared", red)
    if ground is not None:                                     # last in the pass: the tally before it sees the incoming move
        depth = OCEAN_DEPTH if ocean is not None else 0.0
        floor = light.SpectralSurfaceStep(R - depth, **ground) if isinstance(ground, dict) else light.SurfaceReflectStep(R - depth, albedo=ground)
        sim.add_step(8, floor)
    sea = None
    if ocean is not None:                                      # behind the sea floor, before the lamp: where a ground would stand
        sea = light.RefractiveSurfaceStep(R, ocean)
        sim.add_step("ocean", sea)
    walls = inside = None
    if box is not None:                                        # last in the pass: behind the ground and the interface, before re-emission and the lamp
        half = 0.5 * cloud_field[1]
        walls = light.BoxBoundaryStep((0.0, -half, -half), (0.0, half, half), walls=(None, box, box))
        sim.add_step("box", walls)
        inside = light.PositionGridMeasureStep(None, ("y", "z"), [[-half, half], [-half, half]])       # behind it: who stands between the walls
        sim.add_step("inside", inside)
    if reemit is not None:                                     # behind everything that parks photons, before the lamp
        # the ground parks photons on the sphere up to rounding: a thin shell of its own, wide enough for an fp32 store
        glow = light.ReemissionStep(infrared, edges=[R * (1.0 - 1e-6), R * (1.0 + 1e-6), R + 100e3], angular=["lambertian", "isotropic"])
        glow.tally = red
        sim.add_step("reemit", glow)
    if recycle_top is not None:                                # the very last: behind the ground
        lamp = light.RecycleStep(source, top=R + recycle_top)
        sim.add_step(9, lamp)
    sim.add_objs(light.generate_photons_bulk(n, min=light.E_from_wavelength(700e-9), max=light.E_from_wavelength(200e-9), seed=1234, source=source))
    sim.prepare()                                              # the photons are created now: run_time below is stepping only
    sim.start()
    sim.join()
    if sim.error is not None:
        raise sim.error
    return sim, signs, shells, profile, image, tally, floor, angles, medium, lamp, vapour, eye, glow, sea, droplets, broken, walls, inside, heat, irradiance


bare_top = None
if ground is not None and "--shells" in sys.argv:              # the same run without the ground, for the top-of-atmosphere count
    bare = run(None)
    bare_top = int(sum(row[2][3] for row in bare[5].data))
    print("without the ground: %d photons x %d steps in %.2f s" % (n, len(bare[0].ts), bare[0].run_time))
    bare[0].close(download=False)
    del bare
sim, signs, shells, profile, image, tally, floor, angles, medium, lamp, vapour, eye, glow, sea, droplets, broken, walls, inside, heat, irradiance = run(ground)
steps = len(sim.ts)
print("source:", source)
print("%d photons x %d steps in %.2f s  ->  %.3g particle-steps/s" % (n, steps, sim.run_time, n * steps / sim.run_time))
print("launches by formulation (sim.schedule):", dict(sim.schedule), sim.launch_note or "")
for row in signs.data[-3:]:
    print("[t, N, #vx>0, #vy>0, #vz>0]:", [float(x) for x in row])
for row in shells.data[-3:]:
    print("[t, N, crossed x = R + 20 km, crossed y = 0]:", [float(x) for x in row])
print("scattered in the last step:", sim.hits)
if cloud is not None:
    by_layer, by_law = (np.sum([row[k] for row in angles.data], axis=0) for k in (3, 4))
    print("cloud between %g and %g km (0.1 rayleigh + 0.9 hg, g = %g) in a rayleigh atmosphere: %d photons scattered, %d re-directed over %d passes" % (
        cloud[0] / 1e3, cloud[1] / 1e3, cloud[2], sum(int(row[1]) for row in angles.data), sum(int(row[2]) for row in angles.data), len(angles.data)))
    print("  by_layer [below, cloud, above]: %s   by_law [rayleigh, hg]: %s" % (by_layer.tolist(), by_law.tolist()))
    if droplets is not None:
        print("  the cloud's own optical thickness %g (k = %g per m, first=%s): %d photons exposed, %d scattered over %d passes; scattered_by_cell %s" % (
            cloud_tau, droplets.k[0, 0], droplets.first, sum(int(row[1]) for row in droplets.data), sum(int(row[2]) for row in droplets.data),
            len(droplets.data), np.sum([row[3] for row in droplets.data], axis=0).tolist()))
elif cloud_phase is not None:
    by_mixture, by_law = (np.sum([row[k] for row in angles.data], axis=0) for k in (3, 4))
    print("cloud field's phase functions (cloudy cells: 0.1 rayleigh + 0.9 hg, g = %g; clear cells and outside: rayleigh): %d photons scattered, "
          "%d re-directed over %d passes" % (cloud_phase, sum(int(row[1]) for row in angles.data), sum(int(row[2]) for row in angles.data), len(angles.data)))
    print("  by_mixture [clear, cloudy]: %s   by_law [rayleigh, hg]: %s" % (by_mixture.tolist(), by_law.tolist()))
elif angles is not None:
    print("phase function %s (g = %g): %d photons re-directed over %d passes" % (angles.phase, angles.g, sum(int(row[1]) for row in angles.data), len(angles.data)))
if broken is not None:
    by_cell = np.sum([row[3] for row in broken.data], axis=0)
    print("cloud field of %d x %d x %d cells, %g km wide, tau = %g in the cloudy columns (k = %g per m, first=%s): %d photons exposed, %d scattered over %d passes" % (
        *by_cell.shape, cloud_field[1] / 1e3, cloud_field[2], broken.k.max(), broken.first, sum(int(row[1]) for row in broken.data),
        sum(int(row[2]) for row in broken.data), len(broken.data)))
    print("  scattered by column (summed over x, rows: y, columns: z):")
    for line in by_cell.sum(axis=0):
        print("   " + " ".join("%8d" % x for x in line))
if heat is not None:
    heating = np.sum([row[5] for row in heat.data], axis=0)
    print("absorption on the field's cells (omega0 = %g in the cloudy cells%s): %d photons exposed, %d interacted, %d absorbed along the path, "
          "%d at the interaction over %d passes" % (cloud_absorb[0], "" if len(cloud_absorb) == 1 else ", k = %g per m in the column y 0, z 1" % cloud_absorb[1],
                                                   *(sum(int(row[k]) for row in heat.data) for k in (1, 2, 3, 4)), len(heat.data)))
    print("  absorbed by column, the heating field (summed over x, rows: y, columns: z):")
    for line in heating.sum(axis=0):
        print("   " + " ".join("%8d" % x for x in line))
if irradiance is not None:
    up, down = (np.sum([row[k] for row in irradiance.data], axis=0) for k in (2, 3))
    print("flux through the planes %s m above the ground over %d passes: up %s, down %s; %d of the crossings inside the map of %d x %d columns, %g km wide" % (
        flux_map[0], len(irradiance.data), up.tolist(), down.tolist(), int(irradiance.up_map.sum() + irradiance.down_map.sum()), flux_map[2], flux_map[2],
        2e-3 * flux_map[1]))
    if broken is not None:
        print("  downward through the lowest level by column (rows: y, columns: z): the cloudy columns' shadow")
        for line in irradiance.down_map[0, 0]:
            print("   " + " ".join("%8d" % x for x in line))
if walls is not None:
    crossed = np.sum([row[3] for row in walls.data], axis=0)
    print("box walls (%s in y and z, %g km apart): moving %d in the first pass and %d in the last; crossed [[x], [y below, above], [z below, above]] %s "
          "in the last pass, %s over %d passes; multi %d" % (box, cloud_field[1] / 1e3, int(walls.data[0][1]), int(walls.data[-1][1]),
                                                           np.asarray(walls.data[-1][3]).tolist(), crossed.tolist(), len(walls.data),
                                                           sum(int(row[2]) for row in walls.data)))
    count = [int(np.asarray(row[2]).sum()) for row in inside.data]
    print("  photons between the walls behind the step: %d in the first pass, %d at the least, %d in the last (of %d)" % (
        count[0], min(count), count[-1], int(inside.data[-1][1])))
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
if floor is not None and bands is not None:
    sums = [sum(int(row[k]) for row in floor.data) for k in range(1, 5)]
    print("the spectral ground (%d bands): %d reflected, %d absorbed, %d mirrored, %d out of band over %d passes" % (len(floor.albedo), *sums, len(floor.data)))
    for b, (lo, hi) in enumerate(zip(floor.E_edges[:-1], floor.E_edges[1:])):
        print("  %.3g - %.3g J (albedo %g, specular %g): %d reflected, %d absorbed" % (
            lo, hi, floor.albedo[b], floor.specular[b], sum(int(row[5][b]) for row in floor.data), sum(int(row[6][b]) for row in floor.data)))
elif floor is not None:
    print("the ground (albedo %g, lambertian): %d reflected, %d absorbed over %d passes" % (albedo, sum(int(row[1]) for row in floor.data), sum(int(row[2]) for row in floor.data), len(floor.data)))
if floor is not None and tally is not None:
    print("outward through the top of the atmosphere (100 km): %d with the ground, %d without" % (int(sum(row[2][3] for row in tally.data)), bare_top))
if sea is not None:
    names = ("in_refracted", "in_reflected", "out_refracted", "out_reflected", "out_total", "overshot")
    sums = np.sum([[int(x) for x in list(row)[1:]] for row in sea.data], axis=0).tolist()
    print("an ocean of n = %g, its floor %g km down, over %d passes: %s" % (ocean, OCEAN_DEPTH / 1e3, len(sea.data),
                                                                            ", ".join("%s %d" % kv for kv in zip(names, sums))))
if medium is not None:
    by_layer = np.sum([row[3] for row in medium.data], axis=0)
    print("the medium (omega0 %s): %d interactions, %d absorbed over %d passes" % (
        ",".join("%g" % w for w in omega0), sum(int(row[1]) for row in medium.data), sum(int(row[2]) for row in medium.data), len(medium.data)))
    if layer_edges is None:
        print("  absorbed anywhere: %d" % by_layer[0])
    else:
        for b in range(len(by_layer)):
            print("  %5.1f - %5.1f km: %d absorbed" % ((layer_edges[b] - R) / 1e3, (layer_edges[b + 1] - R) / 1e3, by_layer[b]))
    if tally is not None:
        print("  beside it: %d left through the top of the atmosphere (100 km)%s" % (
            int(sum(row[2][3] for row in tally.data)), "" if floor is None else ", %d absorbed by the ground" % sum(int(row[2]) for row in floor.data)))
if vapour is not None:
    cells = np.sum([row[3] for row in vapour.data], axis=0)
    print("a gas between %g and %g km (k = %g per m%s): %d photons exposed, %d absorbed over %d passes; absorbed_by_cell %s" % (
        gas[0] / 1e3, gas[1] / 1e3, gas[2], "" if len(gas) == 3 else ", E in [%g, %g] J" % (gas[3], gas[4]), sum(int(row[1]) for row in vapour.data),
        sum(int(row[2]) for row in vapour.data), len(vapour.data), cells.tolist()))
    if tally is not None:
        print("  beside it: %d left through the top of the atmosphere (100 km)%s" % (
            int(sum(row[2][3] for row in tally.data)), "" if floor is None else ", %d absorbed by the ground" % sum(int(row[2]) for row in floor.data)))
if glow is not None:
    by_layer = np.sum([row[3] for row in glow.data], axis=0)
    print("re-emission in place (the ground at %g K, lambertian; the gas up to 100 km at %g K, isotropic): %d parked, %d re-emitted over %d passes; "
          "by_layer [ground, gas] %s" % (reemit[0], reemit[1], sum(int(row[1]) for row in glow.data), sum(int(row[2]) for row in glow.data),
                                         len(glow.data), by_layer.tolist()))
    print("  infrared photons through the ground's sphere: %d outward (the ground's glow, where it parked a rounding below the sphere), %d inward (the return "
          "flux of the gas)" % (
        sum(int(row[3][0][0]) for row in glow.tally.data), sum(int(row[4][0][0]) for row in glow.tally.data)))
if lamp is not None:
    rate = [int(row[1]) + int(row[2]) for row in lamp.data]
    print("a continuous source (photons at rest or above %g km go back to it): %d re-emitted over %d passes, the population stays at %d" % (
        recycle_top / 1e3, sum(rate), len(rate), int(signs.data[-1][1])))
    every = max(len(rate) // 8, 1)
    for k in range(every - 1, len(rate), every):                # the emission rate settling, pass by pass
        row = lamp.data[k]
        print("  pass %4d: emission rate %d per pass (%d at rest: the ground and the medium, %d through the top)" % (k + 1, rate[k], int(row[1]), int(row[2])))
if eye is not None:
    through, seen = (sum(int(row[k]) for row in eye.data) for k in (2, 3))
    print("the camera at %s looking along %s (disc of %g m, +-%g degrees, %d x %d pixels): %d through, %d seen over %d passes" % (
        eye.position.tolist(), eye.frame[2].round(3).tolist(), eye.radius, np.degrees(camera["fov"]), *camera["pixels"], through, seen, len(eye.data)))
    img = eye.image[0]
    rows, cols = min(img.shape[0], 16), min(img.shape[1], 32)   # a coarse rendering: at most 16 lines of 32 characters, each the sum of its pixels
    coarse = np.array([[blk.sum() for blk in np.array_split(line, cols, axis=1)] for line in np.array_split(img, rows, axis=0)])
    shades = " .:-=+*#%@"
    for line in coarse[::-1]:                                   # e2 upwards
        print("  |" + "".join(shades[0 if v == 0 else 1 + min(int(8 * v / max(coarse.max(), 1)), 8)] for v in line) + "|")
    print("  %d photons in the image, %d pixels lit, brightest pixel %d" % (img.sum(), np.count_nonzero(img), img.max()))
