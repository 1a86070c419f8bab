"""physicl.light equivalent: photons, scatter / delete steps and the counting measure steps, all on
the device store.  Public names follow the reference module (physicl/light.py); the OpenCL kernels
it builds at run time are replaced by the hand-written HIP kernels of libphysicl_hip.so."""
import collections.abc
import copy

import numpy as np
import numpy.linalg as np_lin

from . import tally
from .core import DeviceStep, MeasureStep, Object, PhotonBatch, Step
from .units import Measurement

# SI-defined constants (physicl/light.py:14-16); Measurements, so they follow the code scale in force at import
c = Measurement(np.double(299792458), "m**1 s**-1")
h = Measurement(np.double(6.62607015e-34), "J**1 s**1")
kB = Measurement(np.double(1.380649e-23), "J**1 K**-1")


class PhotonObject(Object):
    """Photon: needs an energy ``E`` and ``|v| == |c|`` (physicl/light.py:18-35)."""

    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        if np_lin.norm(self.v) != np_lin.norm(c):
            raise Exception("Not a valid speed.")
        if "E" not in kwargs:
            raise Exception("Needs a valid energy.")


def E_from_wavelength(wavelength):
    return (h * c) / wavelength


def wavelength_from_E(E):
    return (h * c) / E


# ---------------------------------------------------------------------------------------------- Planck sampling
def planck_distribution(E, T):
    """Normalised Planck photon-energy density, J**-1 (physicl/light.py:53-60).  Set-up time only."""
    E_ = E.__unscaled__() if isinstance(E, Measurement) else E
    T_ = T.__unscaled__() if isinstance(T, Measurement) else T
    k_ = kB.__unscaled__()
    # operation order of the reference (bit-exact): 15/(pi^4 kB T) * (E/(kB T))^3 * 1/e^(E/(kB T))
    norm = 15 / (np.pi ** 4 * k_ * T_)
    x = E_ / (k_ * T_)
    return Measurement(norm * (x ** 3) * (1 / (np.e ** (E_ / (k_ * T_)))), "J**-1")


def planck_probability(E_min, E_max, T, integrator=None):
    import scipy.integrate
    integrator = integrator or (lambda fn, a, b: scipy.integrate.quad(fn, a, b))
    return integrator(lambda x: planck_distribution(x, T), E_min, E_max)


_planck_cache = {"key": None, "cdf": None}


def planck_phot_distribution(E_min, E_max, T, bins=1000):
    """One photon energy drawn from the binned Planck CDF (physicl/light.py:73-104)."""
    key = [float(np.asarray(x.__unscaled__() if isinstance(x, Measurement) else x)) for x in (E_min, E_max, T, bins)]
    lo, hi, T_, nb = key
    grid = np.linspace(lo, hi, int(nb))
    if _planck_cache["key"] != key:
        area = [planck_probability(grid[k], grid[k + 1], T_)[0] for k in range(len(grid) - 1)]
        # left-to-right total and running sum, as the reference adds them (light.py:88-94; np.sum would pair the terms up):
        # the table is the reference's bit for bit (tests/golden g7_setup), so a draw picks the same bin
        _planck_cache["key"], _planck_cache["cdf"] = key, np.cumsum(np.array(area) / sum(area))
    cdf = _planck_cache["cdf"]
    u = np.random.rand()
    for k in range(1, len(cdf)):
        if cdf[k] >= u >= cdf[k - 1]:
            return Measurement(grid[k], "J**1")


def generate_photons_from_E(E):
    return [PhotonObject(E=x, v=c * [1, 0, 0]) for x in E]


def generate_photons(n, fn=lambda: np.random.power(3), min=0, max=0, bins=-1, dist=None):
    """``n`` PhotonObjects moving along +x with ``E = min + (max - min) * fn()`` (physicl/light.py:112-128).
    ``bins``/``dist`` are accepted and ignored like in the older scripts (examples/runtime1.py:67).
    For large n use ``generate_photons_bulk``."""
    return [PhotonObject(E=min + (max - min) * fn(), v=Measurement([c, 0, 0], "m**1 s**-1")) for _ in range(int(n))]


class PhotonSource:
    """Where the photons of ``generate_photons_bulk(..., source=)`` start and where they go -- the initial condition of a bulk
    run (the default is what a PhotonBatch has always been: every photon at the origin, moving along +x).

    ``origin``: the source's centre (numbers in code units, or a Measurement).  ``direction``: its axis, any non-zero vector.
    ``angular``: "beam" (every photon along the axis), "isotropic" (uniform on the sphere: cos(polar angle) uniform in [-1, 1]
    -- NOT the reference scatter kernel's angles, which are uniform in the polar angle and so crowd the poles), "cone"
    (uniform in solid angle within ``half_angle`` radians of the axis, 0 < half_angle <= pi) or "lambertian" (cosine-weighted
    hemisphere about the axis: emission from a surface).  ``spatial``: "point", "disc" (uniform over a disc of ``radius``) or
    "gaussian" (a normal spot, sigma = ``radius``), in the plane through ``origin`` perpendicular to the axis.

    The photons are drawn on the device, keyed by the batch's seed and the photon's number (include/physicl_hip.h:
    pcl_store_apply_source), so a sharded run starts from the very same photons.  The frame the draws are laid out in is made
    here in float64: d = direction/|direction|; a = the coordinate axis with the smallest |d_k| (the lowest index on a tie);
    e1 = (a x d)/|a x d|; e2 = d x e1.  For an axis-aligned direction these are exact unit vectors: ``direction=(0, 0, -1)``
    gives v = (0, 0, -c) bit for bit."""

    def __init__(self, origin=(0, 0, 0), direction=(1, 0, 0), angular="beam", half_angle=None, spatial="point", radius=None):
        def vec3(x, what):
            try:
                a = np.array(x, dtype=np.float64).reshape(-1)
            except (TypeError, ValueError):
                raise ValueError("PhotonSource: %s must be three numbers" % what)
            if a.shape != (3,) or not np.all(np.isfinite(a)):
                raise ValueError("PhotonSource: %s must be three finite numbers" % what)
            return a
        self.origin = vec3(origin, "origin") + 0.0
        direction = vec3(direction, "direction")
        norm = float(np.sqrt(np.sum(direction * direction)))
        if not (norm > 0 and np.isfinite(norm)):
            raise ValueError("PhotonSource: direction must be a non-zero vector")
        if angular not in ("beam", "isotropic", "cone", "lambertian"):
            raise ValueError("PhotonSource: angular must be 'beam', 'isotropic', 'cone' or 'lambertian'")
        if spatial not in ("point", "disc", "gaussian"):
            raise ValueError("PhotonSource: spatial must be 'point', 'disc' or 'gaussian'")
        if (angular == "cone") != (half_angle is not None):
            raise ValueError("PhotonSource: half_angle is required for, and only allowed with, angular='cone'")
        if (spatial != "point") != (radius is not None):
            raise ValueError("PhotonSource: radius is required for, and only allowed with, spatial='disc' / 'gaussian'")
        self.angular, self.spatial = angular, spatial
        self.half_angle = self.cos_half_angle = None
        if half_angle is not None:
            half_angle = float(np.asarray(half_angle))
            if not 0.0 < half_angle <= np.pi:
                raise ValueError("PhotonSource: half_angle must lie in (0, pi] radians")
            self.half_angle, self.cos_half_angle = half_angle, float(np.cos(half_angle))
        self.radius = None
        if radius is not None:
            radius = float(np.asarray(radius))
            if not (radius > 0 and np.isfinite(radius)):
                raise ValueError("PhotonSource: radius must be positive and finite")
            self.radius = radius
        d = direction / norm + 0.0                       # (+ 0.0: no negative zeros in the frame)
        a = np.zeros(3)
        a[int(np.argmin(np.abs(d)))] = 1.0               # argmin: the lowest index on a tie
        e1 = np.cross(a, d)
        e1 = e1 / np.sqrt(np.sum(e1 * e1)) + 0.0
        self.d, self.e1, self.e2 = d, e1, np.cross(d, e1) + 0.0
        if self.cos_half_angle is None:
            self.cos_half_angle = 1.0                    # (unused over the ABI without a cone; radius likewise)
        if self.radius is None:
            self.radius = 0.0

    def __repr__(self):
        return "PhotonSource(origin=%s, direction=%s, angular=%r, half_angle=%r, spatial=%r, radius=%r)" % (
            self.origin.tolist(), self.d.tolist(), self.angular, self.half_angle, self.spatial, self.radius if self.spatial != "point" else None)


def generate_photons_bulk(n, min=0, max=0, seed=0, T=None, bins=1000, fn_vec=None, source=None):
    """``n`` photons created directly in device memory when the simulation first needs them (returns a
    PhotonBatch for ``sim.add_objs``).  Default: the distribution of ``generate_photons`` with its default
    sampler.  With a temperature ``T``: energies from the binned Planck distribution between ``min`` and
    ``max`` -- ``generate_photons_from_E([planck_phot_distribution(min, max, T, bins) ...])``
    (physicl/light.py:73-110) for all photons at once; the bin masses use the closed-form integral of the
    Planck density instead of ``bins`` calls to scipy.quad.
    ``fn_vec``: any other sampler, vectorised -- ``fn_vec(size) -> size numbers`` -- the bulk form of ``generate_photons``'s
    ``fn`` (physicl/light.py:112-128: ``E = min + (max - min) * fn()`` per photon): evaluated on the host in chunks of 4M
    photons, in photon order, and uploaded; ``fn_vec=lambda size: np.random.power(3, size)`` after ``np.random.seed(s)``
    gives photon i the energy ``generate_photons`` gives it after the same seed (numpy fills an array from the stream
    its scalar calls walk).  No Python object per photon either way.
    ``source``: a ``PhotonSource`` -- where the photons start and where they go (default: at the origin, along +x); it
    combines with every form of the energies above."""
    if source is not None and not isinstance(source, PhotonSource):
        raise ValueError("generate_photons_bulk: source must be a PhotonSource")
    if fn_vec is not None:
        if T is not None:
            raise ValueError("generate_photons_bulk: give a temperature T or a sampler fn_vec, not both")
        return PhotonBatch(n, min, max, seed, fn_vec=fn_vec, source=source)
    if T is None:
        return PhotonBatch(n, min, max, seed, source=source)
    lo, hi, T_ = (float(np.asarray(v.__unscaled__() if isinstance(v, Measurement) else v)) for v in (min, max, T))
    grid = np.linspace(lo, hi, int(bins))
    xk = grid / (float(np.asarray(kB.__unscaled__())) * T_)
    mass = np.diff(-np.exp(-xk) * (xk ** 3 + 3 * xk ** 2 + 6 * xk + 6))
    cdf = np.cumsum(mass / mass.sum())
    cdf[-1] = 1.0
    scale = float(np.asarray(Measurement(1, "J**1").scale))          # table energies in code units
    return PhotonBatch(n, lo * scale, hi * scale, seed, table=(cdf, grid[:-1] * scale), source=source)


# ---------------------------------------------------------------------------------------------- helpers
def _kernel_const(x):
    """The reference pastes ``str(value)`` into the kernel call and parses it with ``np.double``
    (physicl/light.py:236, 287; physicl/__init__.py:648): the code-unit number."""
    return float(np.double(str(x)))


def _c_h_literals():
    """Values of the literals str(c), str(h).upper() inside the kernel text (physicl/light.py:301, 309)."""
    return float(str(c)), float(str(h).upper())


# ---------------------------------------------------------------------------------------------- delete
class ScatterDeleteStep(DeviceStep):
    """Removes each photon with probability ``A*n*|dr|`` per step (physicl/light.py:225-260): flag kernel
    + stable compaction of the whole state, fused in pcl_step_scatter_delete.  The reference hands its
    kernel ``A := n`` and ``n := A`` (light.py:236); the product is the same."""

    _fuse_role = "scatter_delete"

    def __init__(self, n, A):
        self.n, self.A = n, A
        self.built = False
        self.removed = 0

    def _kernel_consts(self):
        return _kernel_const(self.n), _kernel_const(self.A)      # kernel A := user n, n := user A (light.py:236)

    def _device_run(self, sim):
        hip, dev = sim._hip, sim._dev
        mode = sim._rng_mode()
        if mode == hip.RNG_INPUT:
            sim._host_randoms("delete")
        A_k, n_k = self._kernel_consts()
        alive, removed = dev.step_scatter_delete(A_k, n_k, mode, sim.seed, sim._next_launch())
        g = sim._global([alive, removed])
        sim._alive, self.removed = int(g[0]), int(g[1])


class ScatterDeleteStepReference(ScatterDeleteStep):
    """Second statement of the same step in the reference (physicl/light.py:131-223): same kernel maths with
    the argument order (dx, dy, dz, rand, n, A, result).  Unlike ScatterDeleteStep it has a CPU path
    (``__run_py``, light.py:216-223), selected by ``Simulation(cl_on=False)``: that path removes photons from the list
    it is iterating over, so the object after every removed photon is skipped -- neither tested nor drawing a random
    number (456 instead of the expected 586 removals of 2000 photons per step at pcoll 0.3).  Reproduced as it is."""

    def _device_run(self, sim):
        if not sim._py_semantics():
            return ScatterDeleteStep._device_run(self, sim)
        from . import pyorder
        dev = sim._dev
        A_k, n_k = self._kernel_consts()
        pcoll = dev.scatter_pcoll(A_k, n_k, 0, 0.0, 0.0)                     # n * A * |dr|   light.py:220
        photon = None if sim._all_photons else dev.download_kind() != 0
        alive, removed = dev.step_delete_flags(pyorder.flags_delete_reference_py(pcoll, photon))
        sim._alive, self.removed = alive, removed


# ---------------------------------------------------------------------------------------------- isotropic scatter
class ScatterIsotropicStep(DeviceStep):
    """Isotropic re-direction with probability ``A * n * |dr|`` (physicl/light.py:262-359).

    Options as in the reference: ``wavelength_dep_scattering`` multiplies by ``pow((h*c)/E, -4)``;
    ``variable_n`` replaces ``n`` by the OpenCL-C expression ``variable_n_fn`` over ``r0[gid]``,
    ``r1[gid]``, ``r2[gid]`` (compiled into the kernel with hipRTC).

    Reference quirk kept: the kernel receives ``A := n`` and ``n := A`` (light.py:287), so with
    ``variable_n=True`` the user's ``A`` is unused and ``n`` (default 1) scales the probability.
    """
    _fuse_role = "scatter_iso"

    def __init__(self, **kwargs):
        self.n = kwargs.get("n", 1)
        self.A = kwargs.get("A", 1)
        self.wavelength_dep_scattering = kwargs.get("wavelength_dep_scattering", False)
        self.variable_n = kwargs.get("variable_n", False)
        self.variable_n_fn = kwargs.get("variable_n_fn", None)
        self.prog = None
        self.built = False

    def _kernel_params(self, sim):
        hip = sim._hip
        flags = (hip.SCATTER_WAVELENGTH if self.wavelength_dep_scattering else 0) | \
                (hip.SCATTER_VARIABLE_N if self.variable_n else 0)
        c_lit, h_lit = _c_h_literals()
        expr = str(self.variable_n_fn) if self.variable_n else None
        return dict(A=_kernel_const(self.n), n=_kernel_const(self.A), flags=flags, c=c_lit, h=h_lit, n_expr=expr)

    def _run_py_semantics(self, sim):
        """``Simulation(cl_on=False)``: ScatterIsotropicStep.__run_py (physicl/light.py:335-350) -- per photon one
        draw for the decision and, only on a hit, phi then theta; a hit leaves ``dv = v_old``; ``variable_n`` is
        ignored ("this does not support variable n scattering", light.py:334).  The host walks the np.random stream
        against the device's collision probabilities (physicl_amd/pyorder.py); kernel and write-back run on the device."""
        from . import pyorder
        hip, dev = sim._hip, sim._dev
        flags = hip.SCATTER_WAVELENGTH if self.wavelength_dep_scattering else 0
        A_k, n_k = _kernel_const(self.n), _kernel_const(self.A)
        c_val, h_val = float(np.asarray(c)), float(np.asarray(h))            # the path multiplies the Measurements themselves
        pcoll = dev.scatter_pcoll(A_k, n_k, flags, c_val, h_val)             # n * A * |dr| [* ((h*c)/E)**-4]   light.py:339-341
        photon = None if sim._all_photons else dev.download_kind() != 0
        rtheta, rphi, rand, hits = pyorder.draw_isotropic_py(pcoll, photon)
        for w, arr in enumerate((rtheta, rphi, rand)):
            dev.upload_rand(w, arr)
        got = dev.step_scatter_isotropic(A_k, n_k, flags | hip.SCATTER_PY_DV, c_val, h_val, None, hip.RNG_INPUT, 0, 0)
        if got != hits:
            raise RuntimeError("cl_on=False scatter: the host walked %d hits, the device applied %d" % (hits, got))
        sim._scattered = True
        sim.hits = hits

    def _device_run(self, sim):
        if sim._py_semantics():
            return self._run_py_semantics(sim)
        hip, dev = sim._hip, sim._dev
        p = self._kernel_params(sim)
        mode = sim._rng_mode()
        if mode == hip.RNG_INPUT:
            sim._host_randoms("iso")
        hits = dev.step_scatter_isotropic(p["A"], p["n"], p["flags"], p["c"], p["h"], p["n_expr"], mode, sim.seed,
                                          sim._next_launch())
        sim._scattered = True
        sim.hits = int(sim._global([hits])[0])


class ScatterSphericalStep(ScatterIsotropicStep):
    """Spelling used by the shipped examples: ``ScatterSphericalStep(n, A, wavelength_dep_scattering=...)``
    (examples/runtime1.py:77, examples/variable_n_scattering.ipynb:56)."""

    def __init__(self, n=1, A=1, **kwargs):
        super().__init__(n=n, A=A, **kwargs)


# ---------------------------------------------------------------------------------------------- measure steps
class _CountingMeasure(DeviceStep, MeasureStep):
    """Measure steps whose rows are counters: one fused reduction on the device."""
    _fuse_role = "measure"

    def _n_planes(self):
        return 0

    def _plane_rows(self):
        return []

    def _device_run(self, sim):
        cnt = sim._dev.step_counters(self._plane_rows())
        g = sim._global(cnt)
        self._record(sim, int(g[0]), g[1:4], g[4:])

    def _record_rows(self, sim, ts, n, sign, planes):
        """The rows of several passes at once (a K-pass launch): what ``_record`` appends pass by pass.  With a plain-number
        clock the rows are cut from ONE float array (``np.array([t, N, ...])`` of a float and integers is a float64 array:
        same values, same dtype); a clock with units takes the row-by-row way."""
        if not all(type(t) in (float, np.float64) for t in ts):
            t_keep = sim.t
            for i, t in enumerate(ts):
                sim.t = t
                self._record(sim, int(n[i]), sign[i], planes[i])
            sim.t = t_keep
            return
        cols = self._row_columns(n, sign, planes)
        block = np.empty((len(ts), 1 + len(cols)), dtype=np.float64)
        block[:, 0] = ts
        for c, col in enumerate(cols):
            block[:, 1 + c] = col
        self.data.extend(list(block))

    def _row_columns(self, n, sign, planes):
        raise NotImplementedError


_MAX_E_BINS = 1024            # PCL_SPECTRUM_MAX_BINS: bins of a binned spectrum


def _plane_spectra(r, dr, E, photon, planes, edges):
    """What Device.plane_spectra answers, from (n, 3) float64 positions and last moves: per plane the particles with
    ``r - dr <= loc <= r`` or the other way round, both ends included (physicl/light.py:378-402), and numpy.histogram of the
    crossing photons' energies: (counts, histograms)."""
    counts, hists = [], []
    for loc in planes:
        ax = 0 if not np.isnan(loc[0]) else (1 if not np.isnan(loc[1]) else 2)
        L, x = loc[ax], r[:, ax]
        with np.errstate(invalid="ignore"):
            prev = x - dr[:, ax]
            cross = ((prev <= L) & (L <= x)) | ((prev >= L) & (L >= x))
        counts.append(int(np.count_nonzero(cross)))
        hists.append(np.histogram(E[cross & photon], bins=edges)[0].astype(np.int64))
    return counts, hists


class ScatterMeasureStep(tally.TallyStep, _CountingMeasure):
    """Row per step: ``[t, N, crossings of plane 0, ...]`` (physicl/light.py:361-404).  A plane is a
    3-vector with NaN in the coordinates that do not define it.  With ``measure_E`` each plane's count is followed
    by the list of the crossing photons' energies (object order), gathered on the device.

    ``E_bins`` (not in the reference; needs ``measure_E``): bin edges, in the unit E is stored in.  Each plane's count is
    then followed by the histogram of the crossing photons' energies over those bins -- an int64 array of
    ``len(E_bins) - 1``, what ``numpy.histogram(list, bins=E_bins)[0]`` makes of the list form -- computed on the device
    for all planes in one sweep.  Histograms add, so sharded runs all-reduce them with the counts (also on the library's own
    communicator, which cannot carry the lists).

    The plain and the list form are the reference's and a _CountingMeasure's; only the ``E_bins`` form is a TallyStep."""

    def __init__(self, out_fn, measure_n=True, measure_locs=[], measure_E=False, E_bins=None):
        MeasureStep.__init__(self, out_fn)
        self.measure_locs, self.measure_n, self.measure_E = measure_locs, measure_n, measure_E
        if E_bins is not None and not measure_E:
            raise ValueError("E_bins bins the energies measure_E=True records: pass measure_E=True with it")
        self.E_bins = None if E_bins is None else tally.check_edges("E_bins", E_bins, _MAX_E_BINS)
        if measure_E:
            # rows carry variable-length energy lists: a separate gather per plane after the counters, outside the
            # fused kernels (this instance takes no part in step fusion / steps_per_launch)
            self._fuse_role = None

    def _device_run(self, sim):
        if not self.measure_E:
            return _CountingMeasure._device_run(self, sim)
        if self.E_bins is not None:
            return tally.TallyStep._device_run(self, sim)
        dev = sim._dev
        cnt = dev.step_counters(self._plane_rows())
        glob = sim._global(cnt)                                              # counts over all shards
        hip = sim._hip
        row = [sim.t]
        if self.measure_n:
            row.append(int(glob[hip.CNT_N]))
        for p, loc in enumerate(self._plane_rows()):                        # physicl/light.py:378-402
            row.append(int(glob[hip.CNT_PLANE0 + p]))
            Es = dev.plane_energies(loc, n_hint=int(cnt[hip.CNT_PLANE0 + p]))
            if sim.comm is not None:
                Es = sim.comm.allgather_concat(Es)                           # rank order == particle order
            row.append(Es.tolist())                                          # crossing photons' E, object order
        self.data.append(tally.object_row(row))                              # ragged row, as the reference's np.array(out)

    # -- E_bins: the spectra as histograms, [N, counts, histograms] in one collective ----------------------------------
    def _sweep(self, dev):
        planes, n_bins = self._plane_rows(), len(self.E_bins) - 1
        if planes:
            return dev.plane_spectra(planes, self.E_bins)
        return np.zeros(0, dtype=np.int64), np.zeros((0, n_bins), dtype=np.int64)

    def _host_parts(self, objs):
        """The list the reference builds per plane (physicl/light.py:378-402), binned with numpy.histogram."""
        return _plane_spectra(tally.vec3(objs, "r"), tally.vec3(objs, "dr"), *tally.photon_energies(objs, PhotonObject),
                                    self._plane_rows(), self.E_bins)

    def _cells(self, parts):                           # the measure_E row, each energy list replaced by its histogram
        return [x for nl, hist in zip(*parts) for x in (int(nl), np.array(hist, dtype=np.int64))]

    def _clock(self, sim):
        return sim.t                                   # as every ScatterMeasureStep row carries it (no copy: the reference's row)

    def run(self, sim):
        return (DeviceStep if self.E_bins is None else tally.TallyStep).run(self, sim)

    def terminate(self, sim):
        return (MeasureStep if self.E_bins is None else tally.TallyStep).terminate(self, sim)

    def _n_planes(self):
        return len(self.measure_locs)

    def _plane_rows(self):
        return [np.asarray(loc, dtype=np.float64).reshape(3) for loc in self.measure_locs]

    def _record(self, sim, n, sign, planes):
        row = [sim.t]
        if self.measure_n:
            row.append(n)
        row.extend(int(x) for x in planes)
        self.data.append(np.array(row))

    def _row_columns(self, n, sign, planes):
        return ([n] if self.measure_n else []) + [planes[:, p] for p in range(planes.shape[1])]


class ScatterSignMeasureStep(_CountingMeasure):
    """Row per step: ``[t, N, #v_x>0, #v_y>0, #v_z>0]`` (physicl/light.py:406-431)."""

    def __init__(self, out_fn, measure_n=True):
        MeasureStep.__init__(self, out_fn)
        self.measure_n = measure_n

    def _record(self, sim, n, sign, planes):
        row = [sim.t]
        if self.measure_n:
            row.append(n)
        row.extend(int(x) for x in sign)
        self.data.append(np.array(row))

    def _row_columns(self, n, sign, planes):
        return ([n] if self.measure_n else []) + [sign[:, k] for k in range(3)]


# ---------------------------------------------------------------------------------------------- position grids
def _check_grid(axes, edges, center):
    """(axes as a tuple of names, one float64 edge array per axis, the centre as 3 float64) of a PositionGridMeasureStep,
    or ValueError for everything pcl_step_position_grid would refuse."""
    from ._hip import GRID_COORDS, GRID_MAX_AXES, GRID_MAX_BINS, GRID_MAX_CELLS      # (the header's names and limits: one place)
    try:
        axes = tuple(axes)                              # ("yz" reads as ("y", "z"))
    except TypeError:
        raise ValueError("axes must be a sequence of names out of 'x', 'y', 'z', 'r'") from None
    if not 1 <= len(axes) <= GRID_MAX_AXES:
        raise ValueError("a position grid has one to three axes, got %d" % len(axes))
    if any(not isinstance(a, str) or a not in GRID_COORDS for a in axes) or len(set(axes)) != len(axes):
        raise ValueError("axes must be distinct names out of 'x', 'y', 'z', 'r', got %r" % (axes,))
    try:
        edges = list(edges)
    except TypeError:
        raise ValueError("edges must be one 1-D sequence of numbers (bin edges) per axis") from None
    if len(edges) != len(axes):
        raise ValueError("edges must hold one sequence of bin edges per axis: %d axes, %d sequences" % (len(axes), len(edges)))
    # (a radius axis: the device compares the squared distance with the squared edges)
    edges = [tally.check_edges("axis %r" % a, e, GRID_MAX_BINS, "square" if a == "r" else None) for a, e in zip(axes, edges)]
    cells = int(np.prod([len(e) - 1 for e in edges]))
    if cells > GRID_MAX_CELLS:
        raise ValueError("the grid has %d cells, at most %d are supported" % (cells, GRID_MAX_CELLS))
    return axes, edges, tally.check_center(center)


def _cell_of_positions(r, axes, edges, center):
    """(who has a cell, the cell -- row-major in the order of ``axes``; arbitrary where there is none) of an (n, 3) float64 array of
    positions, as pcl_step_position_grid and pcl_step_scatter_grid find it, with numpy: per axis the bin with e_b <= v < e_(b+1), the
    last bin closed (numpy.histogramdd); a radius axis bins the squared distance ((x-cx)**2 + (y-cy)**2) + (z-cz)**2 against the
    squared edges; a NaN and a position outside any axis's range are in no cell."""
    from ._hip import GRID_COORDS
    ok, cell = np.ones(len(r), dtype=bool), np.zeros(len(r), dtype=np.int64)
    for a, e in zip(axes, edges):
        if a == "r":
            d = r - center
            v, e = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], e * e
        else:
            v = r[:, GRID_COORDS[a]]
        nb = len(e) - 1
        with np.errstate(invalid="ignore"):
            ok &= (v >= e[0]) & (v <= e[-1])
        cell = cell * nb + np.clip(np.searchsorted(e, v, side="right") - 1, 0, nb - 1)
    return ok, cell


def _grid_of_positions(r, axes, edges, center):
    """The grid of pcl_step_position_grid from an (n, 3) float64 array of positions, with numpy (``_cell_of_positions``)."""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    ok, cell = _cell_of_positions(r, axes, edges, center)
    shape = [len(e) - 1 for e in edges]
    return np.bincount(cell[ok], minlength=int(np.prod(shape))).astype(np.int64).reshape(shape)


class PositionGridMeasureStep(tally.TallyStep):
    """Where the particles are (not in the reference): every ``every``-th run of the step records the row ``[t, N, grid]``
    (``[t, grid]`` with ``measure_n=False``), ``grid`` an int64 array with one dimension per axis -- the histogram of the
    positions of EVERY particle over the ``axes``: names out of ``"x"``, ``"y"``, ``"z"`` and ``"r"``, the distance from
    ``center``; ``edges`` holds one sequence of bin edges per axis, in code units (at most 1024 bins per axis, 2**20 cells).
    An altitude profile is ``axes=("r",)`` about the planet's centre, an image two Cartesian axes, a volume density three.
    Counted as ``numpy.histogramdd`` counts: bins ``[e_b, e_b+1)``, the last one closed, a particle outside any axis's
    range in no cell; a radius axis compares the squared distance with the squared edges (no square root is taken).

    The grid is made on the device in one sweep of the resident store (pcl_step_position_grid); grids add, so sharded runs
    all-reduce ``[N, cells]`` in one collective per recorded pass.  The step counts its own runs from 1 and records on run m
    when ``m % every == 0``.  As the last step(s) of a pass it keeps the K-passes-per-launch schedule
    (``Simulation.steps_per_launch``): a launch ends on the pass that is to be recorded."""
    _fuse_role = "snapshot"

    def __init__(self, out_fn, axes, edges, center=(0, 0, 0), every=1, measure_n=True):
        MeasureStep.__init__(self, out_fn)
        self.axes, self.edges, self.center = _check_grid(axes, edges, center)
        if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
            raise ValueError("every must be a whole number of at least 1, got %r" % (every,))
        self.every, self.measure_n = int(every), measure_n
        self._runs = 0

    # a snapshot step rides at the end of a fused group like a counting measure, with no planes and no counter row
    def _n_planes(self):
        return 0

    def _plane_rows(self):
        return []

    def _passes_to_record(self):
        """How many more runs until the one that records (1: the next one)."""
        return self.every - self._runs % self.every

    def _advance(self, runs=1):
        """``runs`` more runs have happened; True if the last of them is one that records."""
        self._runs += runs
        return runs > 0 and self._runs % self.every == 0

    def _due(self):
        return self._advance()

    def _sweep(self, dev):
        return [dev.position_grid(self.axes, self.edges, self.center)]

    def _host_parts(self, objs):
        return [_grid_of_positions(tally.vec3(objs, "r"), self.axes, self.edges, self.center)]

    def _cells(self, parts):
        return [np.array(parts[0], dtype=np.int64)]


# ---------------------------------------------------------------------------------------------- shell crossings
def _check_shells(radii, center, E_bins, mu_bins):
    """(radii, centre, energy edges or None, direction edges or None) of a ShellCrossingMeasureStep as float64 arrays, or
    ValueError for everything pcl_step_shell_crossings would refuse."""
    from ._hip import SHELL_MAX_BINS, SHELL_MAX_CELLS, SHELL_MAX_SHELLS       # (the header's limits: one place)
    try:
        radii = np.array(radii, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("radii must be a 1-D sequence of numbers (shell radii)") from None
    if radii.ndim != 1 or not 1 <= len(radii) <= SHELL_MAX_SHELLS:
        raise ValueError("radii must be a 1-D sequence of 1 to %d shell radii, got shape %r" % (SHELL_MAX_SHELLS, radii.shape))
    with np.errstate(over="ignore"):
        if not np.all(np.isfinite(radii)) or not np.all(radii > 0) or not np.all(np.isfinite(radii * radii)):
            raise ValueError("radii must be finite and positive (their squares finite, too)")
    center = tally.check_center(center)
    E_bins = None if E_bins is None else tally.check_edges("E_bins", E_bins, SHELL_MAX_BINS)
    # (the device compares s*|s| with e*|e| times q*dr.dr)
    mu_bins = None if mu_bins is None else tally.check_edges("mu_bins", mu_bins, SHELL_MAX_BINS, "signed_square")
    cells = 2 * len(radii) * (sum(len(e) - 1 for e in (E_bins, mu_bins) if e is not None))
    if cells > SHELL_MAX_CELLS:
        raise ValueError("2 x %d shells x (E_bins + mu_bins) bins are %d histogram cells, at most %d are supported"
                         % (len(radii), cells, SHELL_MAX_CELLS))
    return np.ascontiguousarray(radii), center, E_bins, mu_bins


def _shell_tallies(r, dr, E, photon, radii, center, E_edges=None, mu_edges=None):
    """What pcl_step_shell_crossings answers, from (n, 3) float64 positions and last moves, the energies and who is a photon,
    with numpy -- every operation the device's operation, one rounding each (include/physicl_hip.h):
    (counts int64[2, S], E_hist int64[2, S, B_E] or None, mu_hist int64[2, S, B_mu] or None), [0] outward, [1] inward."""
    r, dr = np.asarray(r, dtype=np.float64).reshape(-1, 3), np.asarray(dr, dtype=np.float64).reshape(-1, 3)
    R2 = np.asarray(radii, dtype=np.float64) * np.asarray(radii, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = r - np.asarray(center, dtype=np.float64)
        p = d - dr
        q_now = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        q_prev = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
        cross = np.stack([(q_prev < R2[:, None]) & (q_now >= R2[:, None]),          # outward: on the sphere is outside
                          (q_prev >= R2[:, None]) & (q_now < R2[:, None])])         # inward; NaN: neither
    counts = cross.sum(axis=2).astype(np.int64)
    hit = np.flatnonzero(cross.any(axis=(0, 1)))                                    # the histograms look at these only
    cross = cross[:, :, hit]

    def hist(bins, ok, n_bins):
        return np.stack([[np.bincount(bins[c & ok], minlength=n_bins)[:n_bins] for c in side] for side in cross]).astype(np.int64)

    E_hist = mu_hist = None
    if E_edges is not None:                                   # numpy.histogram's bins: [e_b, e_b+1), the last one closed
        e, v = np.asarray(E_edges, dtype=np.float64), np.asarray(E, dtype=np.float64).reshape(-1)[hit]
        with np.errstate(invalid="ignore"):
            ok = (v >= e[0]) & (v <= e[-1]) & np.asarray(photon, dtype=bool).reshape(-1)[hit]
        E_hist = hist(np.clip(np.searchsorted(e, v, side="right") - 1, 0, len(e) - 2), ok, len(e) - 1)
    if mu_edges is not None:                                  # w_b*D <= W < w_(b+1)*D, the last bin closed
        e = np.asarray(mu_edges, dtype=np.float64)
        w, d, m = e * np.abs(e), d[hit], dr[hit]
        with np.errstate(invalid="ignore", over="ignore"):
            s = (d[:, 0] * m[:, 0] + d[:, 1] * m[:, 1]) + d[:, 2] * m[:, 2]
            dd = (m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2]
            W, D = s * np.abs(s), q_now[hit] * dd
            prod = w[None, :] * D[:, None]
            ok = (D > 0) & np.isfinite(D) & np.isfinite(W) & (W >= prod[:, 0]) & (W <= prod[:, -1])
            bins = np.clip((prod[:, :-1] <= W[:, None]).sum(axis=1) - 1, 0, len(e) - 2)   # (the rounded products are monotone in b)
        mu_hist = hist(bins, ok, len(e) - 1)
    return counts, E_hist, mu_hist


class ShellCrossingMeasureStep(tally.TallyStep):
    """What passed through a sphere (not in the reference; ScatterMeasureStep knows axis-aligned planes only): every run
    records the row ``[t, N, out, in]`` (no ``N`` with ``measure_n=False``) -- ``out[s]`` / ``in[s]`` the particles whose
    last move took them out of / into the sphere of radius ``radii[s]`` about ``center`` (code units, at most 16 shells),
    int64 arrays of ``len(radii)``.  With ``E_bins`` (bin edges, in the unit E is stored in) the row goes on with
    ``E_out, E_in``, int64 ``[S, B_E]``: the crossing photons' energies binned as ``numpy.histogram`` bins them; with
    ``mu_bins`` (edges over ``[-1, 1]``) with ``mu_out, mu_in``, int64 ``[S, B_mu]``: the cosine between the move and the
    outward normal where the particle now is.  At most 1024 bins each, ``2 * S * (B_E + B_mu) <= 8192``.

    A crossing is a change of side between the end points of the move, a particle exactly on the sphere being outside:
    outward iff ``q_prev < R*R <= q_now``, inward iff ``q_now < R*R <= q_prev``, ``q`` the squared distance from the centre
    in float64.  Every change of side is counted exactly once, so ``cumsum(out - in)`` is the change of the number of
    particles outside; a chord through the sphere within one move is not seen.  No square root and no division is taken
    anywhere (``mu`` is compared as ``s*|s|`` against ``e*|e| * q * dr.dr``), so numpy restates every cell exactly.

    The tallies are made on the device in one sweep of the resident store (pcl_step_shell_crossings) and add, so sharded
    runs all-reduce ``[N, counts, histograms]`` in one collective per pass.  A flux needs every pass, which the
    K-passes-per-launch kernels cannot carry: a loop with this step runs one launch per light step, as with
    ``ScatterMeasureStep(measure_E=True)``, and ``sim.launch_note`` says so."""
    _fuse_role = None
    _NOTE = "one launch per light step: a ShellCrossingMeasureStep tallies the last move of every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, out_fn, radii, center=(0, 0, 0), E_bins=None, mu_bins=None, measure_n=True):
        MeasureStep.__init__(self, out_fn)
        self.radii, self.center, self.E_bins, self.mu_bins = _check_shells(radii, center, E_bins, mu_bins)
        self.measure_n = measure_n

    def _device_run(self, sim):
        if getattr(sim, "launch_note", self._NOTE) is None and sim._k_wanted() > 1:      # (a device run only: the host path says nothing)
            sim.launch_note = self._NOTE
        tally.TallyStep._device_run(self, sim)

    def _sweep(self, dev):
        return dev.shell_crossings(self.radii, self.center, self.E_bins, self.mu_bins)

    def _host_parts(self, objs):
        return _shell_tallies(tally.vec3(objs, "r"), tally.vec3(objs, "dr"), *tally.photon_energies(objs, PhotonObject),
                                    self.radii, self.center, self.E_bins, self.mu_bins)

    def _cells(self, parts):                           # counts, E_hist, mu_hist: each outward, then inward
        return [np.array(side, dtype=np.int64) for x in parts if x is not None for side in (x[0], x[1])]


# ---------------------------------------------------------------------------------------------- a detector
def _check_detector(position, frame, radius, x_edges, y_edges, E_edges=None):
    """(position, frame (3, 3): e1, e2, n, radius, x edges, y edges, band edges or None) of a detector as float64, or
    ValueError for everything pcl_step_detector_image would refuse."""
    from ._hip import DETECTOR_MAX_BANDS, DETECTOR_MAX_CELLS, DETECTOR_MAX_PIXELS     # (the header's limits: one place)
    try:
        position, frame = np.array(position, dtype=np.float64), np.array(frame, dtype=np.float64)
        radius = float(radius)
    except (TypeError, ValueError):
        raise ValueError("position must be three numbers, frame nine (e1, e2, n) and radius one") from None
    if position.shape != (3,) or not np.all(np.isfinite(position)):
        raise ValueError("position must be three finite numbers, got %r" % (position,))
    if frame.size != 9 or not np.all(np.isfinite(frame)):
        raise ValueError("frame must be nine finite numbers (e1, e2, n), got %r" % (frame,))
    frame = np.ascontiguousarray(frame.reshape(3, 3))
    if not frame[2].any():
        raise ValueError("frame: the normal n must not be zero")
    with np.errstate(over="ignore"):
        if not np.isfinite(radius) or not radius > 0 or not np.isfinite(radius * radius):
            raise ValueError("radius must be finite and positive (its square finite, too), got %r" % radius)
    x_edges = tally.check_edges("x_edges", x_edges, DETECTOR_MAX_PIXELS)
    y_edges = tally.check_edges("y_edges", y_edges, DETECTOR_MAX_PIXELS)
    E_edges = None if E_edges is None else tally.check_edges("E_bins", E_edges, DETECTOR_MAX_BANDS)
    cells = (1 if E_edges is None else len(E_edges) - 1) * (len(y_edges) - 1) * (len(x_edges) - 1)
    if cells > DETECTOR_MAX_CELLS:
        raise ValueError("%d bands x %d x %d pixels are %d image cells, at most %d are supported"
                         % (1 if E_edges is None else len(E_edges) - 1, len(y_edges) - 1, len(x_edges) - 1, cells, DETECTOR_MAX_CELLS))
    return np.ascontiguousarray(position), frame, radius, x_edges, y_edges, E_edges


def _along(a, u):
    """(a0*u0 + a1*u1) + a2*u2 per row of ``a`` (n, 3) with the vector ``u``: the device's order, one rounding each."""
    return (a[:, 0] * u[0] + a[:, 1] * u[1]) + a[:, 2] * u[2]


def _detector_seen(r, dr, position, frame, radius, x_edges, y_edges):
    """Who pcl_step_detector_image counts, particle by particle: (through, seen) as masks, and (wn, ax, ay), the direction each
    came from in the camera's frame -- ax / wn and ay / wn are what the image bins.  _detector_image's first half."""
    r, m = np.asarray(r, dtype=np.float64).reshape(-1, 3), np.asarray(dr, dtype=np.float64).reshape(-1, 3)
    e1, e2, n = np.asarray(frame, dtype=np.float64).reshape(3, 3)
    xe, ye = np.asarray(x_edges, dtype=np.float64), np.asarray(y_edges, dtype=np.float64)
    R2 = np.float64(radius) * np.float64(radius)
    with np.errstate(invalid="ignore", over="ignore"):
        a = r - np.asarray(position, dtype=np.float64)
        b = a - m                                                 # where the move began
        s_now, s_prev = _along(a, n), _along(b, n)
        crossed = (s_prev > 0) & (s_now <= 0)                     # front to back; on the plane at the end: arrived.  NaN: neither
        D = s_prev - s_now
        H = b * D[:, None] + m * s_prev[:, None]                  # the hit point times D
        hh = (H[:, 0] * H[:, 0] + H[:, 1] * H[:, 1]) + H[:, 2] * H[:, 2]
        lim = R2 * (D * D)
        through = crossed & (hh <= lim) & (lim < np.inf)          # the rim is inside
        wn, ax, ay = -_along(m, n), -_along(m, e1), -_along(m, e2)   # the direction it came from: ax / wn, ay / wn
        seen = through & (wn > 0) & (wn < np.inf) & (xe[0] * wn <= ax) & (ax <= xe[-1] * wn) & (ye[0] * wn <= ay) & (ay <= ye[-1] * wn)
    return through, seen, wn, ax, ay


def _detector_image(r, dr, E, photon, position, frame, radius, x_edges, y_edges, E_edges=None):
    """What pcl_step_detector_image answers, from (n, 3) float64 positions and last moves, the energies and who is a photon,
    with numpy -- every operation the device's operation, one rounding each (include/physicl_hip.h):
    (counts int64[2] = [through, seen], image int64[max(bands, 1), ny, nx])."""
    xe, ye = np.asarray(x_edges, dtype=np.float64), np.asarray(y_edges, dtype=np.float64)
    through, seen, wn, ax, ay = _detector_seen(r, dr, position, frame, radius, xe, ye)
    counts = np.array([np.count_nonzero(through), np.count_nonzero(seen)], dtype=np.int64)
    hit = np.flatnonzero(seen)                                    # the image looks at these only: an aperture is small
    nx, ny, nE = len(xe) - 1, len(ye) - 1, 0 if E_edges is None else len(E_edges) - 1
    with np.errstate(over="ignore"):                              # e_b*wn <= ax < e_(b+1)*wn, the last bin closed; the rounded products are monotone in b
        col = np.clip((xe[None, :-1] * wn[hit, None] <= ax[hit, None]).sum(axis=1) - 1, 0, nx - 1)
        row = np.clip((ye[None, :-1] * wn[hit, None] <= ay[hit, None]).sum(axis=1) - 1, 0, ny - 1)
    band = np.zeros(len(hit), dtype=np.int64)
    if nE:                                                        # numpy.histogram's bins; what is no photon or outside the bands: in no cell
        e, v = np.asarray(E_edges, dtype=np.float64), np.asarray(E, dtype=np.float64).reshape(-1)[hit]
        with np.errstate(invalid="ignore"):
            ok = (v >= e[0]) & (v <= e[-1]) & np.asarray(photon, dtype=bool).reshape(-1)[hit]
        band = np.clip(np.searchsorted(e, v, side="right") - 1, 0, nE - 1)
        col, row, band = col[ok], row[ok], band[ok]
    cells = max(nE, 1) * ny * nx
    image = np.bincount((band * ny + row) * nx + col, minlength=cells)[:cells].astype(np.int64).reshape(max(nE, 1), ny, nx)
    return counts, image


def _detector_frame(normal, up=None):
    """The camera's orthonormal frame (3, 3): e1, e2, n -- ``n = normal / |normal|`` (from the detector into the scene), e1 the
    part of ``up`` at a right angle to n, normalised (default: the coordinate axis least aligned with n), ``e2 = n x e1``."""
    try:
        n = np.array(normal, dtype=np.float64)
        u = None if up is None else np.array(up, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("normal (and up) must be three numbers") from None
    if n.shape != (3,) or not np.all(np.isfinite(n)) or not n.any() or not np.isfinite(np_lin.norm(n)) or np_lin.norm(n) == 0:
        raise ValueError("normal must be three finite numbers, not all zero, got %r" % (n,))
    n = n / np_lin.norm(n)
    if u is None:
        u = np.zeros(3)
        u[int(np.argmin(np.abs(n)))] = 1.0
    if u.shape != (3,) or not np.all(np.isfinite(u)):
        raise ValueError("up must be three finite numbers, got %r" % (u,))
    e1 = u - np.dot(u, n) * n
    length = np_lin.norm(e1)
    if not np.isfinite(length) or not length > 1e-8 * max(np_lin.norm(u), np.finfo(np.float64).tiny):
        raise ValueError("up must not be parallel to normal (or zero), got up %r for normal %r" % (u, n))
    e1 = e1 / length
    return np.ascontiguousarray(np.stack([e1, np.cross(n, e1), n]))


class DetectorMeasureStep(tally.TallyStep):
    """What a radiometer at ``position`` looking along ``normal`` sees (not in the reference): a pinhole camera.  The
    instrument is a disc of ``radius`` (code units) about ``position`` whose ``normal`` points from the detector into the scene.
    Every run records the row ``[t, N, through, seen]`` (no ``N`` with ``measure_n=False``) -- ``through``: the particles whose
    last move took them through the disc from the front, ``seen``: those of them that came from a direction inside the field of
    view -- and, with ``frames=True``, the pass's own image behind it.  ``step.image``, int64 ``[max(bands, 1), ny, nx]``, is the
    sum over all passes so far (an exposure); ``step.through`` and ``step.seen`` are the last pass's counts.

    A pixel is a direction: a photon that moved by ``m`` came from ``-m``, in gnomonic (tangent-plane) coordinates ``(-m.e1) /
    (-m.n)``, ``(-m.e2) / (-m.n)`` -- ``e1`` the part of ``up`` at a right angle to the normal (default: the coordinate axis least
    aligned with it), ``e2 = n x e1``; ``step.frame`` holds ``e1, e2, n``.  ``pixels=(nx, ny)`` with ``fov=(half_x, half_y)`` --
    half angles in radians inside (0, pi/2), one number for both, pi/4 without -- makes ``linspace(-tan h, tan h, n + 1)`` edges; ``x_edges`` /
    ``y_edges`` given explicitly win.  With ``E_bins`` (band edges, in the unit E is stored in) only photons whose energy lies
    inside the bands reach the image, one plane per band as ``numpy.histogram`` bins them; a plain ``Object`` or another energy
    is ``seen`` and lands in no cell.  At most 1024 pixels per axis, 1024 bands and 2**20 cells.

    A crossing is a change of side between the end points of the move (``s_prev > 0 >= s_now``, the signed distances from the
    aperture's plane in float64), the hit point is where the straight move met the plane, and the rim belongs to the disc.  No
    division and no square root is taken anywhere, so numpy restates every cell exactly (``light._detector_image``).

    The tally is made on the device in one read-only sweep of the resident store (pcl_step_detector_image) and adds, so sharded
    runs all-reduce ``[N, through, seen, image]`` in one collective per pass.  A flux needs every pass, which the
    K-passes-per-launch kernels cannot carry: a loop with this step runs one launch per light step, as with
    ``ShellCrossingMeasureStep``, and ``sim.launch_note`` says so.  E is asked for only with bands."""
    _fuse_role = None
    _NOTE = "one launch per light step: a DetectorMeasureStep tallies the last move of every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, out_fn, position, normal, radius, pixels=(64, 64), fov=None, x_edges=None, y_edges=None, up=None, E_bins=None,
                 frames=False, measure_n=True):
        MeasureStep.__init__(self, out_fn)
        frame = _detector_frame(normal, up)
        if x_edges is None or y_edges is None:
            try:
                nx, ny = (int(k) for k in pixels)
                half = np.broadcast_to(np.array(np.pi / 4 if fov is None else fov, dtype=np.float64), (2,))
            except (TypeError, ValueError):
                raise ValueError("pixels must be two integers (nx, ny) and fov one or two half angles in radians") from None
            if nx < 1 or ny < 1 or not np.all((half > 0) & (half < np.pi / 2)):       # (False for NaN as well)
                raise ValueError("pixels must be positive and fov half angles inside (0, pi/2), got %r and %r" % (pixels, fov))
            x_edges = np.linspace(-np.tan(half[0]), np.tan(half[0]), nx + 1) if x_edges is None else x_edges
            y_edges = np.linspace(-np.tan(half[1]), np.tan(half[1]), ny + 1) if y_edges is None else y_edges
        self.position, self.frame, self.radius, self.x_edges, self.y_edges, self.E_bins = _check_detector(
            position, frame, radius, x_edges, y_edges, E_bins)
        self.frames, self.measure_n = bool(frames), measure_n
        self.image = np.zeros((1 if self.E_bins is None else len(self.E_bins) - 1, len(self.y_edges) - 1, len(self.x_edges) - 1), dtype=np.int64)
        self.through = self.seen = 0

    def _device_run(self, sim):
        if getattr(sim, "launch_note", self._NOTE) is None and sim._k_wanted() > 1:      # (a device run only: the host path says nothing)
            sim.launch_note = self._NOTE
        tally.TallyStep._device_run(self, sim)

    def _sweep(self, dev):
        return list(dev.detector_image(self.position, self.frame, self.radius, self.x_edges, self.y_edges, self.E_bins))

    def _host_parts(self, objs):
        return list(_detector_image(tally.vec3(objs, "r"), tally.vec3(objs, "dr"), *tally.photon_energies(objs, PhotonObject),
                                    self.position, self.frame, self.radius, self.x_edges, self.y_edges, self.E_bins))

    def _cells(self, parts):                           # (counts, image), global: the exposure goes on
        counts, image = parts
        self.through, self.seen = int(counts[0]), int(counts[1])
        self.image = self.image + np.asarray(image, dtype=np.int64).reshape(self.image.shape)
        return [self.through, self.seen] + ([np.array(image, dtype=np.int64).reshape(self.image.shape)] if self.frames else [])


# ---------------------------------------------------------------------------------------------- surface reflection
_U32 = np.uint64(0xFFFFFFFF)


def _photons(objs):
    """Who is a photon -- exactly ``PhotonObject``, as the light steps decide it."""
    return np.array([type(o) is PhotonObject for o in objs], dtype=bool)


def _philox_block(ids, seed, word2, word3):
    """(u53(w0, w1), u53(w2, w3)) of the Philox4x32-10 block with counter (id_lo, id_hi, word2, word3) and key (seed_lo,
    seed_hi) per id, with numpy -- the block and the 53-bit uniform of include/physicl_hip.h (pcl_store_apply_source)."""
    ids = np.asarray(ids).astype(np.uint64)
    cnt = [ids & _U32, ids >> np.uint64(32), np.full(ids.shape, int(word2) & 0xFFFFFFFF, dtype=np.uint64),
           np.full(ids.shape, int(word3) & 0xFFFFFFFF, dtype=np.uint64)]
    key = [int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF]
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * cnt[0], np.uint64(0xCD9E8D57) * cnt[2]          # 32 x 32 -> 64 bits: no overflow
        cnt = [(p1 >> np.uint64(32)) ^ cnt[1] ^ np.uint64(key[0]), p1 & _U32, (p0 >> np.uint64(32)) ^ cnt[3] ^ np.uint64(key[1]), p0 & _U32]
        key = [(key[0] + 0x9E3779B9) & 0xFFFFFFFF, (key[1] + 0xBB67AE85) & 0xFFFFFFFF]
    u53 = lambda a, b: ((a >> np.uint64(5)) * np.uint64(1 << 26) + (b >> np.uint64(6))).astype(np.float64) * (1.0 / 9007199254740992.0)   # noqa: E731
    return u53(cnt[0], cnt[1]), u53(cnt[2], cnt[3])


def _dot3(x, y):
    return (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]


# The rules the writer sweeps share, each stated once: the restatements below are built from them, and pcl_rules.h holds the
# device's helper wherever a kernel stays the same machine code with it.  Every line is the device's operation, one rounding each.
def _scalar(x, message):
    """``x`` as one float, or ValueError(message)."""
    try:
        return float(np.asarray(x, dtype=np.float64).reshape(()))
    except (TypeError, ValueError):
        raise ValueError(message) from None


def _radius(x, name, message):
    """A radius the device can square: one finite, positive number whose square is finite, too."""
    x = _scalar(x, message)
    if not (np.isfinite(x) and x > 0 and np.isfinite(x * x)):
        raise ValueError("%s must be finite and positive (its square finite, too), got %r" % (name, x))
    return x


def _mean_cosine(g, where=""):
    """The ``g`` of a Henyey-Greenstein law: one finite number with |g| < 1."""
    g = _scalar(g, where + "g must be a number")
    if not (np.isfinite(g) and abs(g) < 1.0):
        raise ValueError("%sg must be finite with |g| < 1, got %r" % (where, g))
    return g


def _dv_rule_refusal(sim, name, what):
    """The steps that read "scattered in this pass" off dv cannot run under the reference's Python semantics."""
    if getattr(sim, "_py_semantics", None) is not None and sim._py_semantics():
        raise ValueError("%s needs cl_on=True: under the reference's Python semantics a scattered photon is left "
                         "with dv = v_old, not v' - v_old, so %s cannot be read off the store" % (name, what))


def _stored(x, dtype):
    """What the store holds of float64 values: rounded once to ``dtype``."""
    return x.astype(dtype).astype(np.float64)


def _scattered(dv, photon):
    """Scattered / interacted in this pass: a photon with dv != 0 (the scatter step leaves 0 on a miss; NaN != 0 is true)."""
    return ((dv[:, 0] != 0) | (dv[:, 1] != 0) | (dv[:, 2] != 0)) & np.asarray(photon, dtype=bool).reshape(-1)


def _workable(oo):
    """An old velocity o with o.o = oo whose direction can be worked with (NaN: False)."""
    return (oo > 0) & (oo < np.inf)


def _at_rest(v):
    """v == (0, 0, 0): -0.0 == 0, a NaN moves."""
    return (v[:, 0] == 0) & (v[:, 1] == 0) & (v[:, 2] == 0)


def _bin_of(values, edges):
    """numpy.histogram's bin of each value: [e_b, e_(b+1)), the last one closed; -1 outside the edges and for a NaN."""
    nb = len(edges) - 1
    out = np.full(len(values), -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        ok = (values >= edges[0]) & (values <= edges[-1])
    out[ok] = np.clip(np.searchsorted(edges, values[ok], side="right") - 1, 0, nb - 1)
    return out


def _layer_of(r_rows, edges, center):
    """The radial layer of each position: the bin of q = d.d, d = r - center, in e*e -- no square root; no edges: layer 0."""
    if edges is None:
        return np.zeros(len(r_rows), dtype=np.int64)
    e = np.asarray(edges, dtype=np.float64)
    d = r_rows - np.asarray(center, dtype=np.float64)
    return _bin_of(_dot3(d, d), e * e)


def _law_mu(kind, g, nodes, F, u_a, ids, seed, n_pass):
    """The cosine of the scattering angle by one law from u_a (Rayleigh's 3/2 mu^2 part draws block 11 as well)."""
    if kind == "hg" and g != 0.0:
        g = np.float64(g)
        gg = g * g
        if abs(g) < 0.5:                                   # the inverse as a polynomial in g: no difference of ones
            s = 1.0 - 2.0 * u_a
            gs, s2 = g * s, s * s
            d = 1.0 - gs
            mu = (g * ((0.5 * (s2 + 3.0) - gs) + gg * (0.5 * (s2 - 1.0))) - s) / (d * d)
        else:                                              # the closed inverse
            g2 = 2.0 * g
            q = (1.0 - gg) / ((1.0 - g) + g2 * u_a)
            mu = ((1.0 + gg) - q * q) / g2
        return np.fmin(np.fmax(mu, -1.0), 1.0)
    if kind == "rayleigh":
        s4 = u_a * 4.0
        j = np.floor(s4)
        mu = 2.0 * (s4 - j) - 1.0
        part = j == 3.0                                    # one in four: the 3/2 mu^2 part of 3/8 (1 + mu^2)
        u_c, u_d = _philox_block(ids[part], seed, n_pass, 11)
        mu[part] = np.copysign(np.fmax(np.fmax(np.abs(mu[part]), u_c), u_d), mu[part])
        return mu
    if kind == "table":                                    # the inverse of the piecewise linear F
        slope = (nodes[1:] - nodes[:-1]) / (F[1:] - F[:-1])
        k = np.clip(np.searchsorted(F, u_a, side="right") - 1, 0, len(nodes) - 2)
        return np.fmin(np.fmax(nodes[k] + (u_a - F[k]) * slope[k], nodes[k]), nodes[k + 1])
    return 1.0 - 2.0 * u_a                                 # uniform on the sphere


def _azimuth(rho, u):
    """(rho cos psi, rho sin psi) of psi = (u*2)*pi, the scatter step's angle (libm's sin / cos here)."""
    psi = (u * 2.0) * np.pi
    return rho * np.cos(psi), rho * np.sin(psi)


def _polar(mu, u_b):
    """(sc, ss): the sine to the cosine mu about the azimuth of u_b."""
    return _azimuth(np.sqrt((1.0 - mu) * (1.0 + mu)), u_b)


def _frame(w):
    """(e1, e2): an orthonormal frame about the unit vectors w (Duff et al. 2017, branch-free)."""
    w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2]
    sg = np.copysign(1.0, w2)
    aa = -1.0 / (sg + w2)
    bb, sw0 = (w0 * w1) * aa, sg * w0
    return np.stack([1.0 + (sw0 * w0) * aa, sg * bb, -sw0], axis=1), np.stack([bb, sg + (w1 * w1) * aa, -w1], axis=1)


def _direction(e1, e2, axis, sc, ss, mu):
    """(sc*e1 + ss*e2) + mu*axis, per row; the frame and the axis one per row, or one for all rows."""
    return (sc[:, None] * e1 + ss[:, None] * e2) + mu[:, None] * axis


def _turn_about(w, mu, u_b):
    """The direction at the cosine mu and the azimuth of u_b about the unit vectors w."""
    return _direction(*_frame(w), w, *_polar(mu, u_b), mu)


def _check_surface(radius, center, albedo, mode):
    """(radius, centre as 3 float64, albedo, mode) of a SurfaceReflectStep, or ValueError for everything
    pcl_step_surface_reflect would refuse."""
    from ._hip import SURFACE_MODES
    radius = _radius(radius, "radius", "radius must be a number")
    center = tally.check_center(center)
    albedo = _scalar(albedo, "albedo must be a number")
    if not 0.0 <= albedo <= 1.0:                          # (False for NaN as well)
        raise ValueError("albedo must lie in [0, 1], got %r" % (albedo,))
    if not isinstance(mode, str) or mode not in SURFACE_MODES:
        raise ValueError("mode must be 'lambertian' or 'specular', got %r" % (mode,))
    return radius, center, albedo, mode


def _surface_bounce(r, dr, v, photon, ids, radius, center, albedo, mode, c, seed, n_pass, dtype=np.float64):
    """What pcl_step_surface_reflect makes of (n, 3) float64 positions, last moves and velocities, who is a photon and the
    particles' ids, with numpy -- every operation the device's operation in the device's order, one rounding each
    (include/physicl_hip.h), and what is written rounded once to ``dtype``.  Everything but sin / cos of the lambertian angle
    (libm here, the library's own on the device) is the device's bit for bit.  A dict: ``r, v, dr, dv`` the new state (float64
    arrays; rows of particles that are not hit are the arguments', zeros in ``dv``), ``hit, reflected, absorbed`` boolean masks, and of the hit
    particles (NaN elsewhere) ``t``, ``x`` (the hit point about the centre), ``nrm`` and -- lambertian -- ``mu``."""
    r, dr, v = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, dr, v))
    center, c, R2 = np.asarray(center, dtype=np.float64), np.float64(c), np.float64(radius) * np.float64(radius)
    hit, p, q_prev = _ground_hits(r, dr, photon, R2, center)
    ids = np.asarray(ids).reshape(-1)[hit]
    refl = np.ones(len(ids), dtype=bool)
    if albedo < 1.0:
        refl = _philox_block(ids, seed, n_pass, 9)[0] < albedo
    return _ground_bounce(r, dr, v, hit, p, q_prev, ids, refl, np.full(len(ids), mode == "specular"), R2, center, c, seed, n_pass, dtype)


def _ground_hits(r, dr, photon, R2, center):
    """The ground's hit test, once: (hit, p, q_prev) -- a photon with q_now < R2 <= q_prev < inf, d = r - center, p = d - dr."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = r - center
        p = d - dr
        q_now, q_prev = _dot3(d, d), _dot3(p, p)
        hit = (q_now < R2) & (q_prev >= R2) & (q_prev < np.inf) & np.asarray(photon, dtype=bool).reshape(-1)
    return hit, p, q_prev


def _ground_bounce(r, dr, v, hit, p, q_prev, ids, refl, mirror, R2, center, c, seed, n_pass, dtype):
    """The ground's hit point, parking and flight, once, for ``_surface_bounce`` and ``_spectral_bounce``: of the ``hit`` particles
    (``ids``, ``refl``, ``mirror``: one value each) those with ``refl`` are reflected -- mirrored where ``mirror``, otherwise
    cosine-weighted about the normal with the block of counter word 8 (drawn for every hit lane that is not ``mirror``: ``mu``) --
    and the others parked on the sphere.  ``_surface_bounce``'s dict; ``r``, ``dr`` and ``v`` are written in place."""
    n = len(r)
    at = np.flatnonzero(hit)
    out = {"hit": hit, "reflected": np.zeros(n, dtype=bool), "absorbed": np.zeros(n, dtype=bool),
           "t": np.full(n, np.nan), "x": np.full((n, 3), np.nan), "nrm": np.full((n, 3), np.nan), "mu": np.full(n, np.nan)}
    out["reflected"][at[refl]], out["absorbed"][at[~refl]] = True, True
    m, p, vo = dr[at], p[at], v[at]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a, b, cq = _dot3(m, m), _dot3(p, m), q_prev[at] - R2
        disc = np.fmax(b * b - a * cq, 0.0)
        t = cq / (np.sqrt(disc) - b)
        x = p + t[:, None] * m
        nrm = x / np.sqrt(_dot3(x, x))[:, None]
        sa = np.sqrt(a)
        mh = m / sa[:, None]
        direction = mh - (2.0 * _dot3(mh, nrm))[:, None] * nrm  # mirrored
        lam = np.flatnonzero(~mirror)
        u_a, u_b = _philox_block(ids[lam], seed, n_pass, 8)
        mu = np.sqrt(1.0 - u_a)                                # cosine-weighted hemisphere
        direction[lam] = _turn_about(nrm[lam], mu, u_b)
        out["mu"][at[lam]] = mu
        w = (1.0 - t) * sa
        v_new = c * direction
        dr_new = w[:, None] * direction
        r_new = center + (x + dr_new)
        dv_new = v_new - vo
        gone = ~refl                                       # absorbed: parked on the sphere, at rest
        r_new[gone], v_new[gone], dr_new[gone], dv_new[gone] = (center + x)[gone], 0.0, (x - p)[gone], (0.0 - vo)[gone]
        for name, new in (("r", r_new), ("v", v_new), ("dr", dr_new), ("dv", dv_new)):
            full = {"r": r, "v": v, "dr": dr}.get(name)
            full = np.zeros((n, 3)) if full is None else full
            full[at] = _stored(new, dtype)
            out[name] = full
    out["t"][at], out["x"][at], out["nrm"][at] = t, x, nrm
    return out


class SurfaceReflectStep(tally.WriterStep):
    """A reflecting sphere: the ground of a radial problem (not in the reference).  Every photon whose last move took it into
    the sphere of ``radius`` about ``center`` (code units) is put back: reflected at the point where the move met the sphere
    -- ``mode="lambertian"``: cosine-weighted about the outward normal, ``"specular"``: mirrored -- with the rest of the move
    flown along the new direction, or, with probability ``1 - albedo``, absorbed: left in the store AT REST on the sphere
    (``v = 0``, ``dr`` the move up to the hit point, ``dv = -v_old``).  Nothing is removed, ``len(sim.objects)`` does not change.
    After each run ``self.reflected`` and ``self.absorbed`` hold the pass's counts (global over shards and ranks) and
    ``self.data`` gains the row ``[t, reflected, absorbed]``; ``out_fn`` takes the rows at the end of the run.

    Put the step LAST in a pass: behind the Newton step, the scatter step and any measures.  Tally the ground with a
    ``ShellCrossingMeasureStep`` of the same radius and centre placed BEFORE it: that tally sees the incoming move, and its
    ``in`` count is this step's ``reflected + absorbed`` (a photon is hit iff ``q_now < R*R <= q_prev``, the shell's own rule in
    float64; a move from infinitely far is counted there and left alone here).  A shell of the same radius BEHIND the step sees
    the outgoing segment, which starts on the sphere: its side there is decided by rounding.  Plain ``Object``s and particles with
    a NaN in ``r`` or ``dr`` are never hit.  The arithmetic is written out in include/physicl_hip.h
    (pcl_step_surface_reflect); ``_surface_bounce`` restates it with numpy.

    Absorbed photons no longer move (Newton: ``dr = v*dt = 0``) and cross nothing, so a ``PositionGridMeasureStep`` shows where
    the light landed.  They are still looked at by the scatter steps: the kernels' hit test is ``pcoll >= rand`` with
    ``pcoll = A*n*|dr| = 0`` for a photon at rest, true only for a draw of exactly 0 -- once in 2**53 draws (and never
    otherwise, unless ``n`` is infinite there: 0*inf is NaN, which compares false).  A ScatterIsotropicStep that does hit
    re-directs the photon with speed c, a ScatterDeleteStep removes it: absorbed photons are recognised by ``v == 0`` only until
    then.  The scatter kernels are left as they are.

    The draws are Philox blocks keyed by ``sim.seed``, the photon's id and the step's pass counter ``_n_pass``, in counter words no
    other kernel uses -- so the scatter steps of a simulation draw what they draw without this step, and a photon draws the same
    numbers however the run is sharded.  They are made on the device with EVERY ``rng=`` setting: the step is not in the
    reference, so there is no host stream to reproduce.

    One launch per light step: the K-passes-per-launch kernels cannot bounce a photon between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list -- what an upload would give them."""
    _STREAM = "ground"                                   # (words 8 and 9, as the spectral ground's)
    _NOTE = "one launch per light step: a SurfaceReflectStep bounces photons off its sphere behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, radius, center=(0, 0, 0), albedo=1.0, mode="lambertian", out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.radius, self.center, self.albedo, self.mode = _check_surface(radius, center, albedo, mode)
        self.reflected = self.absorbed = 0
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_pass(self, sim, reflected, absorbed):
        self.reflected, self.absorbed = int(reflected), int(absorbed)
        self.data.append(tally.object_row([tally._snap(sim.t), self.reflected, self.absorbed]))

    _writes = ("r", "dr", "v", "dv")

    def _sweep(self, sim, prep):
        return [np.array(sim._dev.surface_reflect(self.radius, self.center, self.albedo, self.mode, _c_h_literals()[0], sim.seed, self._n_pass),
                         dtype=np.int64)]

    def _reduce(self, sim, parts):
        return [sim._global(parts[0].tolist())]          # the two counts alone, as ever

    def _host_sweep(self, objs, ids, seed, prep):
        new = _surface_bounce(tally.vec3(objs, "r"), tally.vec3(objs, "dr"), tally.vec3(objs, "v"), _photons(objs), ids,
                              self.radius, self.center, self.albedo, self.mode, _c_h_literals()[0], seed, self._n_pass)
        return new, new["hit"], (new["reflected"].sum(), new["absorbed"].sum())


# ---------------------------------------------------------------------------------------------- a spectral ground
_SPECTRAL_MIRROR_WORD = 22                                     # mirror or Lambert: the counter word (the header lists the words taken)
_SPECTRAL_COUNTS = ("reflected", "absorbed", "mirrored", "out_of_band")


def _check_spectral_surface(radius, albedo, E_edges, center, specular):
    """(radius, albedo [B], energy edges [B + 1], centre, specular [B]) of a SpectralSurfaceStep as float64, or ValueError for
    everything pcl_step_ground_spectral would refuse."""
    from ._hip import SPECTRAL_MAX_BANDS                       # (the header's limit: one place)
    radius = _radius(radius, "radius", "radius must be a number")
    E_edges = tally.check_edges("E_edges", E_edges, SPECTRAL_MAX_BANDS)        # PathAbsorptionStep(E_edges=)'s rule
    B = len(E_edges) - 1
    tables = []
    for name, x, one in (("albedo", albedo, False), ("specular", specular, True)):
        try:
            x = np.array(x, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("%s must be numbers, one per band of E_edges" % name) from None
        if one and x.shape == ():
            x = np.repeat(x, B)
        if x.shape != (B,):
            raise ValueError("%s must hold one value per band of E_edges (%d)%s, got the shape %r" % (name, B, " or be one number" if one else "", x.shape))
        if not np.all((x >= 0.0) & (x <= 1.0)):                # (False for NaN as well)
            raise ValueError("%s must lie in [0, 1], got %r" % (name, x.tolist()))
        tables.append(np.ascontiguousarray(x))
    return radius, tables[0], E_edges, tally.check_center(center), tables[1]


def _spectral_bounce(r, dr, v, E, photon, ids, radius, center, albedo, specular, E_edges, c, seed, n_pass, dtype=np.float64):
    """What pcl_step_ground_spectral makes of (n, 3) float64 positions, last moves and velocities, the energies, who is a photon and
    the particles' ids, with numpy -- ``_surface_bounce``'s arithmetic (``_ground_hits``, ``_ground_bounce``) behind the band lookup
    of ``_absorb_path`` (``_bin_of``) and the draws of include/physicl_hip.h: word 9 iff ``albedo_b < 1``, word 22 by a reflected lane
    iff ``0 < specular_b < 1``, word 8 for Lambert.  ``albedo``, ``specular``: B values each, ``E_edges``: B + 1.  ``_surface_bounce``'s
    dict -- ``absorbed`` includes ``out_of_band`` -- plus ``band`` (int64: of every hit photon, -1 for none and elsewhere), the masks
    ``mirrored`` and ``out_of_band``, and the tallies ``reflected_by_band``, ``absorbed_by_band`` (int64 [B])."""
    r, dr, v = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, dr, v))
    n = len(r)
    center, c, R2 = np.asarray(center, dtype=np.float64), np.float64(c), np.float64(radius) * np.float64(radius)
    albedo, specular, E_edges = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (albedo, specular, E_edges))
    B = len(E_edges) - 1
    hit, p, q_prev = _ground_hits(r, dr, photon, R2, center)
    ids = np.asarray(ids).reshape(-1)[hit]
    b = _bin_of(np.asarray(E, dtype=np.float64).reshape(-1)[hit], E_edges)     # NaN and under/overflow: in no band
    inside = b >= 0
    alb, sp = np.where(inside, albedo[np.fmax(b, 0)], 0.0), np.where(inside, specular[np.fmax(b, 0)], 1.0)
    refl = inside.copy()
    draws = np.flatnonzero(inside & (alb < 1.0))
    refl[draws] = _philox_block(ids[draws], seed, n_pass, 9)[0] < alb[draws]
    mirror = sp >= 1.0                                         # (a lane that is not reflected: whether Lambert's block is looked at -- ``mu``)
    draws = np.flatnonzero(refl & (sp > 0.0) & (sp < 1.0))
    mirror[draws] = _philox_block(ids[draws], seed, n_pass, _SPECTRAL_MIRROR_WORD)[0] < sp[draws]
    out = _ground_bounce(r, dr, v, hit, p, q_prev, ids, refl, mirror, R2, center, c, seed, n_pass, dtype)
    at = np.flatnonzero(hit)
    out["band"] = np.full(n, -1, dtype=np.int64)
    out["band"][at] = b
    out["mirrored"], out["out_of_band"] = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    out["mirrored"][at[refl & mirror]], out["out_of_band"][at[~inside]] = True, True
    out["reflected_by_band"] = np.bincount(b[refl], minlength=B).astype(np.int64)
    out["absorbed_by_band"] = np.bincount(b[inside & ~refl], minlength=B).astype(np.int64)
    return out


class SpectralSurfaceStep(tally.WriterStep):
    """A ground whose albedo depends on the photon's energy (not in the reference): ``SurfaceReflectStep``'s sphere of ``radius`` about
    ``center`` with, per energy band, the chance that a photon is reflected and the share of the reflected ones that is mirrored --
    vegetation that is dark in the visible and bright in the near infrared, snow the other way round, water, a ground under a
    ``ReemissionStep`` that absorbs nearly all of the infrared coming back down while it reflects a third of the sunlight.

    * ``E_edges``: ``B + 1`` finite, strictly increasing energies in the unit ``E`` is stored in, ``1 <= B <= 1024``:
      ``numpy.histogram``'s bins, the last one closed -- ``PathAbsorptionStep(E_edges=)``'s rule and its lookup, on ``(double)E``.
    * ``albedo``: ``B`` numbers in ``[0, 1]``; ``specular``: one number or ``B`` in ``[0, 1]``, the share of the reflected photons
      that is mirrored; the others leave cosine-weighted about the local vertical.
    * A hit photon whose ``E`` lies in no band (below, above, NaN) is absorbed and counted in ``out_of_band``: the ground stays opaque.

    Who is hit, where, how an absorbed photon is parked (``r`` on the sphere, ``v = 0``, ``dr`` the move up to the hit point,
    ``dv = -v_old``) and how a reflected one flies the rest of its move are ``SurfaceReflectStep``'s, operation for operation; so is the
    placement: LAST in a pass, before a ``ReemissionStep`` or ``RecycleStep``, a ``ShellCrossingMeasureStep`` of the same radius in
    front of it has ``in == reflected + absorbed``.  Plain ``Object``s and particles with a NaN in ``r`` or ``dr`` are never hit.

    The draws a grey ground makes come from the grey ground's Philox blocks: reflect or absorb is word 9 (drawn iff
    ``albedo_b < 1``), the lambertian direction word 8; only mirror-or-Lambert has a word of its own (22, drawn by a reflected photon
    iff ``0 < specular_b < 1``).  With one band that holds every energy and ``specular=0`` the step leaves the store bit for bit as
    ``SurfaceReflectStep(radius, center, albedo, "lambertian")`` does with the same seed, with ``specular=1`` as ``"specular"``.  Because
    words 8 and 9 are shared a simulation holds ONE ground: the first run raises ValueError if the simulation also holds a
    ``SurfaceReflectStep`` or a second ``SpectralSurfaceStep``.  The draws are made on the device with EVERY ``rng=`` setting, and the
    step reads no ``dv`` rule, so it works under ``cl_on=False`` as well.

    After each run ``reflected``, ``absorbed`` (``out_of_band`` among them), ``mirrored`` and ``out_of_band`` hold the pass's counts and
    ``reflected_by_band`` / ``absorbed_by_band`` int64 arrays ``[B]``, global over shards and ranks; ``self.data`` gains the row ``[t,
    reflected, absorbed, mirrored, out_of_band, reflected_by_band, absorbed_by_band]``; ``out_fn`` takes the rows at the end.  The
    rule is written out in include/physicl_hip.h (pcl_step_ground_spectral); ``_spectral_bounce`` restates it with numpy.

    The sweep reads ``E`` and never writes it.  Asking for ``E`` costs a wavelength-dependent scatter step its term cache, which is
    dropped every pass (the library has no read-only access to E) -- what ``PathAbsorptionStep(E_edges=)`` costs it, and a grey
    ``SurfaceReflectStep`` does not.

    One launch per light step: the K-passes-per-launch kernels cannot bounce a photon between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "ground"                                   # (the grey ground's words 8 and 9 (22 is its own))
    _NOTE = "one launch per light step: a SpectralSurfaceStep bounces photons off its sphere behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"
    _writes = ("r", "dr", "v", "dv")

    def __init__(self, radius, albedo, E_edges, center=(0, 0, 0), specular=0.0, out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.radius, self.albedo, self.E_edges, self.center, self.specular = _check_spectral_surface(radius, albedo, E_edges, center, specular)
        self._record_counts(np.zeros(4, dtype=np.int64), np.zeros((2, len(self.albedo)), dtype=np.int64))
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_counts(self, counts, bands):
        for name, x in zip(_SPECTRAL_COUNTS, counts):
            setattr(self, name, int(x))
        bands = np.array(bands, dtype=np.int64).reshape(2, len(self.albedo))
        self.reflected_by_band, self.absorbed_by_band = bands[0].copy(), bands[1].copy()

    def _record_pass(self, sim, reflected, absorbed, mirrored, out_of_band, bands):
        self._record_counts((reflected, absorbed, mirrored, out_of_band), bands)
        self.data.append(tally.object_row([tally._snap(sim.t)] + [getattr(self, name) for name in _SPECTRAL_COUNTS] +
                                          [self.reflected_by_band.copy(), self.absorbed_by_band.copy()]))

    def _refuse(self, sim):                              # words 8 and 9 are the ground's: a simulation holds one ground
        steps = getattr(sim, "steps", None) or {}
        others = [s for s in (steps.values() if hasattr(steps, "values") else steps)
                  if s is not self and isinstance(s, (SurfaceReflectStep, SpectralSurfaceStep))]
        if others:
            raise ValueError("a simulation holds one ground: this SpectralSurfaceStep shares the counter words 8 and 9 with the %s "
                             "that is among the steps as well" % type(others[0]).__name__)

    def _sweep(self, sim, prep):
        counts, refl, gone = sim._dev.ground_spectral(self.radius, self.E_edges, self.albedo, self.specular, self.center,
                                                      _c_h_literals()[0], sim.seed, self._n_pass)
        return [np.asarray(counts, dtype=np.int64), np.stack([np.asarray(refl, dtype=np.int64), np.asarray(gone, dtype=np.int64)])]

    def _host_sweep(self, objs, ids, seed, prep):
        E, photon = tally.photon_energies(objs, PhotonObject)
        new = _spectral_bounce(tally.vec3(objs, "r"), tally.vec3(objs, "dr"), tally.vec3(objs, "v"), E, photon, ids, self.radius,
                               self.center, self.albedo, self.specular, self.E_edges, _c_h_literals()[0], seed, self._n_pass)
        return new, new["hit"], (new["reflected"].sum(), new["absorbed"].sum(), new["mirrored"].sum(), new["out_of_band"].sum(),
                                 np.stack([new["reflected_by_band"], new["absorbed_by_band"]]))

    terminate = tally.TallyStep.terminate                # (a row holds arrays: written as the tally steps write theirs, as plain lists)


# ---------------------------------------------------------------------------------------------- refraction
_REFRACT_WORD = 21                                             # the Fresnel draw's counter word (the header lists the words taken)
_REFRACT_COUNTS = ("in_refracted", "in_reflected", "out_refracted", "out_reflected", "out_total", "overshot")


def _check_refractive(radius, n_inside, n_outside, center):
    """(radius, n_inside, n_outside, centre as 3 float64) of a RefractiveSurfaceStep, or ValueError for everything
    pcl_step_refract_surface would refuse."""
    radius = _radius(radius, "radius", "radius must be a number")
    index = []
    for name, x in (("n_inside", n_inside), ("n_outside", n_outside)):
        x = _scalar(x, name + " must be a number")
        if not (np.isfinite(x) and x > 0):
            raise ValueError("%s must be finite and positive, got %r" % (name, x))
        index.append(x)
    return radius, index[0], index[1], tally.check_center(center)


def _refract_surface(r, dr, v, photon, ids, radius, center, n_inside, n_outside, fresnel, c, seed, n_pass, dtype=np.float64):
    """What pcl_step_refract_surface makes of (n, 3) float64 positions, last moves and velocities, who is a photon and the particles'
    ids, with numpy -- every operation the device's operation in the device's order, one rounding each (include/physicl_hip.h), and
    what is written rounded once to ``dtype``: the device's bit for bit, everywhere (the sweep takes no sin / cos).  A dict: ``r, v,
    dr, dv`` the new state (float64 arrays; rows of particles that do not cross are the arguments', NaN in ``dv``: the sweep does not
    write them), the boolean masks ``inward, outward, crossed, refracted, reflected`` (drawn), ``total`` and ``overshot``, ``counts``
    (int64 [6], the order of the header) and of the crossing particles (NaN elsewhere) ``t``, ``x`` (the hit point about the centre),
    ``N`` (the normal facing the photon), ``mh``, ``dir``, ``eta``, ``ci``, ``ct``, ``rs``, ``rp`` and ``F`` (NaN where total)."""
    r, dr, v = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, dr, v))
    n = len(r)
    center, c, R2 = np.asarray(center, dtype=np.float64), np.float64(c), np.float64(radius) * np.float64(radius)
    eta_in, eta_out = np.float64(n_outside) / np.float64(n_inside), np.float64(n_inside) / np.float64(n_outside)
    with np.errstate(invalid="ignore", over="ignore"):
        d = r - center
        p = d - dr
        q_now, q_prev = _dot3(d, d), _dot3(p, p)
        photon = np.asarray(photon, dtype=bool).reshape(-1)
        inward = (q_now < R2) & (q_prev >= R2) & (q_prev < np.inf) & photon      # the ground's test
        outward = (q_prev < R2) & (q_now >= R2) & (q_now < np.inf) & photon
    at = np.flatnonzero(inward | outward)
    ids = np.asarray(ids).reshape(-1)[at]
    inw = inward[at]
    m, p, vo = dr[at], p[at], v[at]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a, b, cq = _dot3(m, m), _dot3(p, m), q_prev[at] - R2
        sq = np.sqrt(np.fmax(b * b - a * cq, 0.0))
        t = np.where(inw, cq / (sq - b), np.fmin(np.fmax(np.where(b > 0.0, (0.0 - cq) / (sq + b), (sq - b) / a), 0.0), 1.0))
        x = p + t[:, None] * m
        nrm = x / np.sqrt(_dot3(x, x))[:, None]
        sa = np.sqrt(a)
        mh = m / sa[:, None]
        w = (1.0 - t) * sa
        N = np.where(inw[:, None], nrm, -nrm)
        eta = np.where(inw, eta_in, eta_out)
        ci = np.fmax(0.0 - _dot3(mh, N), 0.0)
        k = 1.0 - (eta * eta) * (1.0 - ci * ci)
        total = k < 0.0
        ct = np.where(eta == 1.0, ci, np.sqrt(k))              # no interface: the photon passes
        ec, ect = eta * ci, eta * ct
        rs, rp = (ec - ct) / (ec + ct), (ci - ect) / (ci + ect)
        F = (rs * rs + rp * rp) * 0.5
        drawn = np.zeros(len(at), dtype=bool)
        draws = np.flatnonzero(~total & (F > 0.0)) if fresnel else np.zeros(0, dtype=np.int64)
        drawn[draws] = _philox_block(ids[draws], seed, n_pass, _REFRACT_WORD)[0] < F[draws]
        back = total | drawn
        direction = np.where(back[:, None], mh + (2.0 * ci)[:, None] * N, eta[:, None] * mh + (ec - ct)[:, None] * N)
        v_new = c * direction
        dr_new = w[:, None] * direction
        y = x + dr_new
        r_new = center + y
        dv_new = v_new - vo
        q_new = _dot3(y, y)
        over = np.where(inw != back, q_new >= R2, q_new < R2)  # in refracted and out reflected end inside, the others outside
    out = {"r": r, "v": v, "dr": dr, "dv": np.full((n, 3), np.nan)}
    for name, new in (("r", r_new), ("v", v_new), ("dr", dr_new), ("dv", dv_new)):
        out[name][at] = _stored(new, dtype)
    masks = {"inward": inward, "outward": outward, "crossed": inward | outward, "refracted": ~back, "reflected": drawn, "total": total,
             "overshot": over}
    for name, mask in masks.items():
        if name in ("inward", "outward", "crossed"):
            out[name] = mask
        else:
            out[name] = np.zeros(n, dtype=bool)
            out[name][at] = mask
    F = np.where(total, np.nan, F)
    for name, val in (("t", t), ("x", x), ("N", N), ("mh", mh), ("dir", direction), ("eta", eta), ("ci", ci), ("ct", ct), ("rs", rs),
                      ("rp", rp), ("F", F)):
        out[name] = np.full((n,) + val.shape[1:], np.nan)
        out[name][at] = val
    # an inward total reflection (n_outside > n_inside) is counted as reflected: the header's [1]
    out["counts"] = np.array([(inw & ~back).sum(), (inw & back).sum(), (~inw & ~back).sum(), (~inw & drawn).sum(), (~inw & total).sum(),
                              over.sum()], dtype=np.int64)
    return out


class RefractiveSurfaceStep(tally.WriterStep):
    """A refracting sphere: a dielectric interface (not in the reference) -- an ocean under an atmosphere, a water drop or a glass
    sphere, the top of an atmosphere that is a real change of refractive index.  The medium within the sphere of ``radius`` about
    ``center`` (code units) has the refractive index ``n_inside``, the one around it ``n_outside``.  Every photon whose last move
    crossed the sphere, in EITHER direction, is put onto its new path at the point where the move met the sphere: refracted by Snell's
    law into the medium beyond, or reflected back into the one it came from -- always beyond the critical angle (total internal
    reflection) and, with ``fresnel=True``, with Fresnel's probability ``F`` for unpolarised light below it; ``fresnel=False`` draws
    nothing and refracts every crossing that is not total.  The rest of the move is flown along the new direction.  Equal indices
    are no interface: ``F = 0`` and every photon passes on its way.

    The step changes DIRECTIONS, NOT SPEEDS: the model's photons move ``c*dt`` per pass everywhere, and ``PathAbsorptionStep``
    relies on that, so ``|v| = c`` on both sides of the sphere.  What an index does to the light's speed is not modelled; what it
    does to its path is.

    Put the step where a ground would stand: LAST in a pass, before a ``RecycleStep``, behind the Newton step, the scatter step
    and any measures.  A ``ShellCrossingMeasureStep`` of the same radius and centre placed BEFORE it sees the incoming moves: its
    ``in`` count is this step's ``in_refracted + in_reflected``, its ``out`` count ``out_refracted + out_reflected + out_total``
    (the shell's own rule in float64: a particle exactly on the sphere is outside, every change of side is counted once; a move
    from infinitely far is counted there and left alone here).  A ground (``SurfaceReflectStep``) a little below an ocean's surface
    stands BEFORE this step.  Plain ``Object``s and particles with a NaN in ``r`` or ``dr`` never cross.

    One interaction per photon per pass.  ``overshot`` counts the photons whose remaining move carried them through the sphere
    again (a grazing path whose chord is shorter than the rest of the move): it changes nothing and says that ``c*dt`` is too large
    for the radius.  A total reflection on the way IN (``n_outside > n_inside``: a bubble) is counted in ``in_reflected``.

    After each run ``in_refracted``, ``in_reflected``, ``out_refracted``, ``out_reflected``, ``out_total`` and ``overshot`` hold
    the pass's counts (global over shards and ranks, one collective) and ``self.data`` gains the row ``[t, ...the six...]``;
    ``out_fn`` takes the rows at the end of the run.  The arithmetic is written out in include/physicl_hip.h
    (pcl_step_refract_surface); ``_refract_surface`` restates it with numpy, bit for bit.

    The draw is a Philox block keyed by ``sim.seed``, the photon's id and the step's pass counter ``_n_pass``, in a counter word no
    other kernel uses (21): every other step draws what it draws without this one, and a photon meets the same fate however the run
    is sharded.  It is made on the device with EVERY ``rng=`` setting.  The step reads no ``dv`` rule, so it works under
    ``cl_on=False`` as well.

    One launch per light step: the K-passes-per-launch kernels cannot refract a photon between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "refract"
    _NOTE = "one launch per light step: a RefractiveSurfaceStep refracts photons at its sphere behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"
    _writes = ("r", "dr", "v", "dv")

    def __init__(self, radius, n_inside, n_outside=1.0, center=(0, 0, 0), fresnel=True, out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.radius, self.n_inside, self.n_outside, self.center = _check_refractive(radius, n_inside, n_outside, center)
        self.fresnel = bool(fresnel)
        self._record_counts(np.zeros(6, dtype=np.int64))
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_counts(self, counts):
        for name, x in zip(_REFRACT_COUNTS, counts):
            setattr(self, name, int(x))

    def _record_pass(self, sim, *counts):
        self._record_counts(counts)
        self.data.append(tally.object_row([tally._snap(sim.t)] + [getattr(self, name) for name in _REFRACT_COUNTS]))

    def _sweep(self, sim, prep):
        return [np.asarray(sim._dev.refract_surface(self.radius, self.n_inside, self.n_outside, self.center, self.fresnel,
                                                    _c_h_literals()[0], sim.seed, self._n_pass), dtype=np.int64)]

    def _host_sweep(self, objs, ids, seed, prep):
        new = _refract_surface(tally.vec3(objs, "r"), tally.vec3(objs, "dr"), tally.vec3(objs, "v"), _photons(objs), ids, self.radius,
                               self.center, self.n_inside, self.n_outside, self.fresnel, _c_h_literals()[0], seed, self._n_pass)
        return new, new["crossed"], tuple(new["counts"])


# ---------------------------------------------------------------------------------------------- phase functions
def _check_phase(phase, g):
    """(phase, g as a float) of a PhaseFunctionStep, or ValueError for everything pcl_step_phase_redirect would refuse
    (``g`` is checked for every phase here: a step is built once, and a bad number is a mistake whatever the phase)."""
    from ._hip import PHASE_FUNCTIONS
    if not isinstance(phase, str) or phase not in PHASE_FUNCTIONS:
        raise ValueError("phase must be one of %s, got %r" % (", ".join(repr(k) for k in PHASE_FUNCTIONS), phase))
    return phase, _mean_cosine(g)


def _phase_redirect(v, dv, photon, ids, phase, g, c, seed, n_pass, dtype=np.float64):
    """What pcl_step_phase_redirect makes of (n, 3) float64 velocities and last velocity changes, who is a photon and the
    particles' ids, with numpy -- every operation the device's operation in the device's order, one rounding each
    (include/physicl_hip.h), and what is written rounded once to ``dtype``.  Everything but sin / cos of the azimuth (libm here,
    the library's own on the device) is the device's bit for bit.  A dict: ``v, dv`` the new state (float64 arrays; rows that are
    not re-directed are the arguments'), ``scattered`` (a photon with a non-zero dv) and ``redirected`` (those of them whose old
    velocity has a length that can be worked with) boolean masks, and of the re-directed rows (NaN elsewhere) ``mu``, the cosine
    of the scattering angle, and ``w``, the unit vector of the old direction."""
    v, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (v, dv))
    n = len(v)
    phase, g = _check_phase(phase, g)
    c = np.float64(c)
    with np.errstate(invalid="ignore", over="ignore"):
        scattered = _scattered(dv, photon)
        o_all = v - dv
        oo = _dot3(o_all, o_all)
        go = scattered & _workable(oo)
    at = np.flatnonzero(go)
    ids = np.asarray(ids).reshape(-1)[at]
    out = {"scattered": scattered, "redirected": go, "mu": np.full(n, np.nan), "w": np.full((n, 3), np.nan)}
    o = o_all[at]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = o / np.sqrt(oo[at])[:, None]
        u_a, u_b = _philox_block(ids, seed, n_pass, 10)
        mu = _law_mu(phase, g, None, None, u_a, ids, seed, n_pass)
        v_new = c * _turn_about(w, mu, u_b)
        dv_new = v_new - o
    v[at], dv[at] = _stored(v_new, dtype), _stored(dv_new, dtype)
    out["v"], out["dv"] = v, dv
    out["mu"][at], out["w"][at] = mu, w
    return out


class PhaseFunctionStep(tally.WriterStep):
    """The scattering angle of a pass (not in the reference).  ``ScatterIsotropicStep`` decides who scatters and gives a hit
    photon a direction whose polar angle is uniform about the x axis -- which bunches directions at the poles of x and does not
    depend on where the photon came from.  This step, placed directly BEHIND the scatter step (measures may stand between),
    replaces that direction by one drawn from a phase function about the photon's direction BEFORE the scatter:

    * ``phase="isotropic"``: uniform on the sphere, ``mu = 1 - 2u`` -- what "isotropic" means (the law of
      ``PhotonSource(angular="isotropic")``); ``ScatterIsotropicStep``'s own angles are not;
    * ``phase="hg"``: Henyey-Greenstein with the mean cosine ``g``, ``|g| < 1`` (aerosols and clouds: about 0.85); ``g = 0`` is
      the isotropic law bit for bit.  ``mu`` is the exact inverse of the law's cumulative distribution to 8 ulp(1) for
      ``|g| < 1/2``, down to the smallest ``g``, and to ``32 ulp(1) / (1 - |g|)`` at and above 1/2;
    * ``phase="rayleigh"``: ``3/8 (1 + mu^2)``, a molecular atmosphere.

    "Scattered in this pass" is read off the store: the scatter step leaves ``dv = v' - v_old`` on a hit and ``dv = 0`` on a miss,
    so ``v - dv`` is the old velocity.  A photon whose old velocity is zero or not finite is left alone (and not counted); plain
    ``Object``s are never touched.  After each run ``self.redirected`` holds the pass's count (global over shards and ranks) --
    the scatter step's hit count -- and ``self.data`` gains the row ``[t, redirected]``; ``out_fn`` takes the rows at the end.
    The arithmetic is written out in include/physicl_hip.h (pcl_step_phase_redirect); ``_phase_redirect`` restates it with numpy.

    The draws are Philox blocks keyed by ``sim.seed``, the photon's id and the step's pass counter ``_n_pass``, in counter words no
    other kernel uses: the scatter step draws what it draws without this step, and a photon draws the same numbers however the
    run is sharded.  They are made on the device with every ``rng=`` setting.  Under the reference's Python semantics
    (``cl_on=False``) a hit leaves ``dv = v_old``, the rule above does not hold, and the step raises ``ValueError``.

    One launch per light step: the K-passes-per-launch kernels cannot re-direct a photon between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "phase"                                    # (words 10 and 11, as the layered phase step's)
    _NOTE = "one launch per light step: a PhaseFunctionStep re-directs the scattered photons behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, phase="hg", g=0.0, out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.phase, self.g = _check_phase(phase, g)
        self.redirected = 0
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_pass(self, sim, redirected):
        self.redirected = int(redirected)
        self.data.append(tally.object_row([tally._snap(sim.t), self.redirected]))

    def _refuse(self, sim):
        _dv_rule_refusal(sim, "PhaseFunctionStep", "its direction before the scatter")

    def _sweep(self, sim, prep):
        return [np.array([sim._dev.phase_redirect(self.phase, self.g, _c_h_literals()[0], sim.seed, self._n_pass)], dtype=np.int64)]

    def _reduce(self, sim, parts):
        return [sim._global(parts[0].tolist())]          # the count alone, as ever

    def _host_sweep(self, objs, ids, seed, prep):
        new = _phase_redirect(tally.vec3(objs, "v"), tally.vec3(objs, "dv"), _photons(objs), ids, self.phase, self.g,
                              _c_h_literals()[0], seed, self._n_pass)
        return new, new["redirected"], (new["redirected"].sum(),)


# ---------------------------------------------------------------------------------------------- absorbing media
def _check_absorb(omega0, edges, center, E_bins):
    """(omega0 -- a float without ``edges``, else a float64 array of one value per layer --, edges or None, centre, energy edges or
    None) of an AbsorptionStep, or ValueError for everything pcl_step_absorb_scattered would refuse."""
    from ._hip import ABSORB_MAX_BINS, ABSORB_MAX_CELLS, ABSORB_MAX_LAYERS      # (the header's limits: one place)
    try:
        om = np.array(omega0, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("omega0 must be a number, or with edges one number per layer") from None
    if edges is None:
        if om.shape != ():
            raise ValueError("omega0 must be one number without edges (edges= gives it one value per layer), got shape %r" % (om.shape,))
    else:
        edges = tally.check_edges("edges", edges, ABSORB_MAX_LAYERS, "square")      # (the device compares q with e*e)
        if om.ndim != 1 or len(om) != len(edges) - 1:
            raise ValueError("omega0 must hold one value per layer: edges describe %d layers, omega0 has shape %r" % (len(edges) - 1, om.shape))
    if not np.all((om >= 0.0) & (om <= 1.0)):                 # (False for NaN as well)
        raise ValueError("omega0 must lie in [0, 1], got %r" % (omega0,))
    center = tally.check_center(center)
    rows = 1 if edges is None else len(edges) - 1
    if E_bins is not None:
        E_bins = tally.check_edges("E_bins", E_bins, ABSORB_MAX_BINS)
        cells = 2 + rows * len(E_bins)
        if cells > ABSORB_MAX_CELLS:
            raise ValueError("%d layers x %d E_bins bins are %d tally cells, at most %d are supported" % (rows, len(E_bins) - 1, cells, ABSORB_MAX_CELLS))
    return (float(om) if edges is None else np.ascontiguousarray(om)), edges, center, E_bins


def _absorb_scattered(r, v, dv, E, photon, ids, omega0, edges, center, E_bins, seed, n_pass, dtype=np.float64):
    """What pcl_step_absorb_scattered makes of (n, 3) float64 positions, velocities and last velocity changes, the energies, who is
    a photon and the particles' ids, with numpy -- every operation the device's operation in the device's order, one rounding each
    (include/physicl_hip.h): no transcendental function and no division, so everything is the device's bit for bit.  What is
    written is zero, in any ``dtype``.  A dict: ``v, dv`` the new state (float64 arrays; rows that are not absorbed are the
    arguments'), ``interacted`` (a photon with a non-zero dv) and ``absorbed`` boolean masks, ``layer`` (int64: the layer of every
    interacting row, -1 for a row outside every layer or not interacting) and the tallies ``absorbed_by_layer`` (int64 [L'])
    and ``E_hist`` (int64 [L', bins], None without ``E_bins``)."""
    r, v, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v, dv))
    n = len(v)
    om = np.asarray(omega0, dtype=np.float64).reshape(-1)
    rows = 1 if edges is None else len(edges) - 1
    with np.errstate(invalid="ignore", over="ignore"):
        interacted = _scattered(dv, photon)
        at = np.flatnonzero(interacted)
        layer = np.full(n, -1, dtype=np.int64)
        layer[at] = _layer_of(r[at], edges, center)
    draws = np.flatnonzero(layer >= 0)
    draws = draws[om[layer[draws]] < 1.0]                      # a conservative layer draws nothing
    u = _philox_block(np.asarray(ids).reshape(-1)[draws], seed, n_pass, 12)[0]
    gone = draws[~(u < om[layer[draws]])]                      # the sense of the ground's albedo draw
    absorbed = np.zeros(n, dtype=bool)
    absorbed[gone] = True
    v[gone], dv[gone] = np.zeros(3, dtype=dtype), np.zeros(3, dtype=dtype)
    out = {"v": v, "dv": dv, "interacted": interacted, "absorbed": absorbed, "layer": layer,
           "absorbed_by_layer": np.bincount(layer[gone], minlength=rows).astype(np.int64), "E_hist": None}
    if E_bins is not None:
        nb = len(E_bins) - 1
        eb = _bin_of(np.asarray(E, dtype=np.float64).reshape(-1)[gone], np.asarray(E_bins, dtype=np.float64))
        cell = layer[gone][eb >= 0] * nb + eb[eb >= 0]
        out["E_hist"] = np.bincount(cell, minlength=rows * nb).astype(np.int64).reshape(rows, nb)
    return out


class AbsorptionStep(tally.WriterStep):
    """An absorbing medium (not in the reference): the single-scattering albedo ``omega0``, the chance that an interaction is a
    scatter and not an absorption.  ``ScatterIsotropicStep`` decides who interacts; this step, placed anywhere BEHIND the scatter
    step of a pass and before the next Newton step (before or behind a ``PhaseFunctionStep``; measures may stand between), lets
    each interacting photon be absorbed with probability ``1 - omega0``.

    * ``edges=None``: ``omega0`` is one number in [0, 1] and holds everywhere;
    * ``edges``: ``L + 1`` finite, non-negative, strictly increasing radii about ``center`` (code units, at most 64 layers);
      ``omega0`` is then a sequence of ``L`` numbers in [0, 1].  Layer ``b`` holds a photon iff ``e_b**2 <= q < e_(b+1)**2``, the
      last layer closed as in ``numpy.histogram``, ``q = (d0*d0 + d1*d1) + d2*d2`` the squared distance from ``center`` in
      float64 -- no square root is taken.  A photon outside every layer (or with a NaN in ``q``) is never absorbed: it is counted
      as interacting and left alone.

    "Interacted in this pass" is read off the store by ``PhaseFunctionStep``'s rule: a photon with a non-zero ``dv``.  Plain
    ``Object``s are never touched.  The step is ANALOG: an absorbed photon is parked at rest where it was absorbed, ``v = 0`` and
    ``dv = 0``; ``r``, ``dr``, ``E``, ids and kinds are left alone.  ``E`` is not scaled as a statistical weight -- it is the photon's
    energy, which the wavelength-dependent scatter step reads for its lambda**-4 term: a weight kept there would change the
    photon's colour.  ``dv = 0`` is deliberate and differs from the ground's ``dv = -v_old`` (``SurfaceReflectStep``): the ground
    ends a pass, this step stands in the middle of one, and a ``PhaseFunctionStep`` or a second ``AbsorptionStep`` later in the pass
    must see a photon that did not scatter and leave it at rest -- with ``dv = -v_old`` the phase function would send it off again
    at speed c.  From then on the photon behaves like one the ground absorbed: Newton does not move it, the scatter steps hit it
    only on a draw of exactly 0, and a ``PositionGridMeasureStep`` shows where the energy was left.

    After each run ``self.interacted`` and ``self.absorbed`` hold the pass's counts, ``self.absorbed_by_layer`` an int64 array
    ``[L]`` (``[1]`` without ``edges``) and -- with ``E_bins``, bin edges in the unit E is stored in -- ``self.E_hist`` an int64 array
    ``[max(L, 1), bins]``: the absorbed photons' energies per layer as ``numpy.histogram`` bins them (energies outside the edges are
    not counted).  All of them are global over shards and ranks.  ``self.data`` gains the row ``[t, interacted, absorbed,
    absorbed_by_layer (, E_hist)]``; ``out_fn`` takes the rows at the end.  The arithmetic is written out in include/physicl_hip.h
    (pcl_step_absorb_scattered); ``_absorb_scattered`` restates every bit of it with numpy.

    The draw is a Philox block keyed by ``sim.seed``, the photon's id and the step's pass counter ``_n_pass``, in a counter word no
    other kernel uses: every other step draws what it draws without this one, and a photon draws the same number however the run
    is sharded.  Two ``AbsorptionStep``s of one pass count on through one another (``tally.WriterStep``), so their draws are
    independent.  A layer with ``omega0 == 1`` draws nothing.  The draws are made on the device with every ``rng=`` setting.  Under
    the reference's Python semantics (``cl_on=False``) a hit leaves ``dv = v_old``, the rule above does not hold, and the step
    raises ``ValueError``.

    One launch per light step: the K-passes-per-launch kernels cannot absorb a photon between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "absorb"
    _NOTE = "one launch per light step: an AbsorptionStep absorbs interacting photons behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, omega0=1.0, edges=None, center=(0, 0, 0), E_bins=None, out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.omega0, self.edges, self.center, self.E_bins = _check_absorb(omega0, edges, center, E_bins)
        rows = 1 if self.edges is None else len(self.edges) - 1
        self.interacted = self.absorbed = 0
        self.absorbed_by_layer = np.zeros(rows, dtype=np.int64)
        self.E_hist = None if self.E_bins is None else np.zeros((rows, len(self.E_bins) - 1), dtype=np.int64)
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_pass(self, sim, interacted, absorbed, by_layer, E_hist):
        self.interacted, self.absorbed = int(interacted), int(absorbed)
        self.absorbed_by_layer = np.array(by_layer, dtype=np.int64)
        self.E_hist = None if E_hist is None else np.array(E_hist, dtype=np.int64)
        cells = [self.absorbed_by_layer.copy()] + ([] if self.E_hist is None else [self.E_hist.copy()])
        self.data.append(tally.object_row([tally._snap(sim.t), self.interacted, self.absorbed] + cells))

    def _refuse(self, sim):
        _dv_rule_refusal(sim, "AbsorptionStep", "who interacted in this pass")

    def _sweep(self, sim, prep):
        interacted, absorbed, by_layer, E_hist = sim._dev.absorb_scattered(self.omega0, self.edges, self.center, self.E_bins, sim.seed, self._n_pass)
        return [np.array([interacted, absorbed], dtype=np.int64), np.asarray(by_layer), E_hist]

    def _host_sweep(self, objs, ids, seed, prep):
        E, photon = tally.photon_energies(objs, PhotonObject)
        new = _absorb_scattered(tally.vec3(objs, "r"), tally.vec3(objs, "v"), tally.vec3(objs, "dv"), E, photon, ids,
                                self.omega0, self.edges, self.center, self.E_bins, seed, self._n_pass)
        return new, new["absorbed"], (new["interacted"].sum(), new["absorbed"].sum(), new["absorbed_by_layer"], new["E_hist"])

    terminate = tally.TallyStep.terminate                # (a row holds arrays: written as the tally steps write theirs, as plain lists)


# ---------------------------------------------------------------------------------------------- phase functions by layer
def _check_table_law(j, mu_edges, p, max_bins):
    """(mu, F) of the tabulated law ``laws[j]``: the K + 1 nodes and cumulative values as float64 arrays, or ValueError."""
    try:
        mu, p = np.array(mu_edges, dtype=np.float64), np.array(p, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("laws[%d]: a table's mu_edges and p must be sequences of numbers" % j) from None
    if mu.ndim != 1 or len(mu) < 2:
        raise ValueError("laws[%d]: a table's mu_edges must be a 1-D sequence of at least two values, got shape %r" % (j, mu.shape))
    K = len(mu) - 1
    if K > max_bins:
        raise ValueError("laws[%d]: the table has %d bins, at most %d are supported" % (j, K, max_bins))
    if not (np.all(np.isfinite(mu)) and np.all(np.diff(mu) > 0) and mu[0] == -1.0 and mu[-1] == 1.0):
        raise ValueError("laws[%d]: a table's mu_edges must rise strictly from exactly -1.0 to exactly 1.0" % j)
    if p.shape != (K,):
        raise ValueError("laws[%d]: a table's p must hold one value per bin (%d), got shape %r" % (j, K, p.shape))
    if not (np.all(np.isfinite(p)) and np.all(p > 0)):
        raise ValueError("laws[%d]: a table's p must be finite and > 0 in every bin" % j)
    with np.errstate(over="ignore", invalid="ignore"):
        m = p * (mu[1:] - mu[:-1])
        F = np.concatenate([[0.0], np.cumsum(m) / np.sum(m)])
    F[-1] = 1.0
    if not (np.all(np.isfinite(F)) and np.all(np.diff(F) > 0)):
        raise ValueError("laws[%d]: the table's cumulative distribution is not strictly increasing in float64 (a bin of no weight "
                         "beside its neighbours)" % j)
    return np.ascontiguousarray(mu), np.ascontiguousarray(F)


def _check_layered_phase(laws, weights, edges, center, rows=None):
    """(laws as ``(kind, g, mu, F)`` tuples -- mu and F the nodes and cumulative values of a table, None otherwise --, weights as a
    float64 array [L'][M], their cumulative rows C, edges or None, centre) of a LayeredPhaseStep, or ValueError for everything
    pcl_step_phase_layered would refuse.  ``rows``: how many rows ``weights`` has where they are not one per layer (light_grid: one
    per mixture, without ``edges``)."""
    from ._hip import LPHASE_MAX_LAWS, LPHASE_MAX_LAYERS, LPHASE_MAX_NODES, LPHASE_MAX_TOTAL_NODES      # (the header's limits: one place)
    if isinstance(laws, str) or not isinstance(laws, collections.abc.Sequence):
        raise ValueError("laws must be a sequence of laws: 'isotropic', 'rayleigh', ('hg', g) or ('table', mu_edges, p)")
    M = len(laws)
    if not 1 <= M <= LPHASE_MAX_LAWS:
        raise ValueError("laws must hold 1 to %d laws, got %d" % (LPHASE_MAX_LAWS, M))
    out, total = [], 0
    for j, law in enumerate(laws):
        if isinstance(law, str) and law in ("isotropic", "rayleigh"):
            out.append((law, 0.0, None, None))
        elif isinstance(law, (tuple, list)) and len(law) == 2 and isinstance(law[0], str) and law[0] == "hg":
            out.append(("hg", _mean_cosine(law[1], "laws[%d]: " % j), None, None))
        elif isinstance(law, (tuple, list)) and len(law) == 3 and isinstance(law[0], str) and law[0] == "table":
            mu, F = _check_table_law(j, law[1], law[2], LPHASE_MAX_NODES)
            total += len(mu) - 1
            out.append(("table", 0.0, mu, F))
        else:
            raise ValueError("laws[%d] must be 'isotropic', 'rayleigh', ('hg', g) or ('table', mu_edges, p), got %r" % (j, law))
    if total > LPHASE_MAX_TOTAL_NODES:
        raise ValueError("the tables of laws have %d bins in total, at most %d are supported" % (total, LPHASE_MAX_TOTAL_NODES))
    if edges is not None:
        edges = tally.check_edges("edges", edges, LPHASE_MAX_LAYERS, "square")      # (the device compares q with e*e)
    if rows is None:
        rows = 1 if edges is None else len(edges) - 1
    if weights is None:
        if M > 1:
            raise ValueError("weights may be omitted only with one law, laws holds %d" % M)
        w = np.ones((rows, 1), dtype=np.float64)
    else:
        try:
            w = np.array(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("weights must be numbers: one row per layer, one value per law") from None
        if edges is None and w.shape == (M,):
            w = w.reshape(1, M)
        if w.shape != (rows, M):
            raise ValueError("weights must have the shape [%d][%d] (layers, laws), got %r" % (rows, M, w.shape))
    with np.errstate(over="ignore", invalid="ignore"):
        cs = np.cumsum(w, axis=1)
    if not (np.all(np.isfinite(w)) and np.all(w >= 0) and np.all(np.isfinite(cs)) and np.all(cs[:, -1] > 0)):
        raise ValueError("weights must be finite and >= 0, with a positive sum in every row, got %r" % (weights,))
    cum = cs / cs[:, -1:]
    cum[:, -1] = 1.0
    return out, np.ascontiguousarray(w), np.ascontiguousarray(cum), edges, tally.check_center(center)


def _layered_phase_redirect(r, v, dv, photon, ids, laws, weights, edges, center, c, seed, n_pass, dtype=np.float64):
    """What pcl_step_phase_layered makes of (n, 3) float64 positions, velocities and last velocity changes, who is a photon and the
    particles' ids, with numpy -- every operation the device's operation in the device's order, one rounding each
    (include/physicl_hip.h), and what is written rounded once to ``dtype``.  Everything but sin / cos of the azimuth (libm here, the
    library's own on the device) is the device's bit for bit.  A dict: ``v, dv`` the new state (float64 arrays; rows that are not
    re-directed are the arguments'), the boolean masks ``scattered`` (a photon with a non-zero dv and an old velocity whose length
    can be worked with) and ``redirected`` (those of them inside a layer), per row ``layer`` and ``law`` (int64, -1 for a row that
    is not re-directed), ``mu`` and ``w`` (NaN there), and the tallies ``by_layer`` (int64 [L']) and ``by_law`` (int64 [M])."""
    laws, _, cum, edges, center = _check_layered_phase(laws, weights, edges, center)
    return _layered_phase_apply(r, v, dv, photon, ids, laws, cum, edges, center, c, seed, n_pass, dtype)


def _layered_phase_apply(r, v, dv, photon, ids, laws, cum, edges, center, c, seed, n_pass, dtype=np.float64, row_of=None):
    """``_layered_phase_redirect`` behind its checks: ``laws`` and ``cum`` as ``_check_layered_phase`` returns them.  ``row_of``: None
    -- a photon's row of ``cum`` is its radial layer -- or what gives the rows of the scattered photons from their (k, 3) positions,
    -1 for one that is left alone (light_grid: the mixture of the photon's grid cell); ``layer`` and ``by_layer`` then hold those."""
    r, v, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v, dv))
    n = len(v)
    M, rows = len(laws), len(cum)
    c = np.float64(c)
    with np.errstate(invalid="ignore", over="ignore"):
        o_all = v - dv
        oo = _dot3(o_all, o_all)
        scattered = _scattered(dv, photon) & _workable(oo)
        at = np.flatnonzero(scattered)
        layer = np.full(n, -1, dtype=np.int64)
        layer[at] = _layer_of(r[at], edges, center) if row_of is None else row_of(r[at])
    go = layer >= 0
    at = np.flatnonzero(go)
    ids = np.asarray(ids).reshape(-1)[at]
    b = layer[at]
    pick = np.zeros(len(at), dtype=np.int64)
    if M > 1:                                                  # the first law with u_s < C[b][j]: C does not decrease and ends in 1
        u_s = _philox_block(ids, seed, n_pass, 13)[0]
        pick = (cum[b] <= u_s[:, None]).sum(axis=1).astype(np.int64)
    law = np.full(n, -1, dtype=np.int64)
    law[at] = pick
    out = {"scattered": scattered, "redirected": go, "layer": layer, "law": law, "mu": np.full(n, np.nan), "w": np.full((n, 3), np.nan),
           "by_layer": np.bincount(b, minlength=rows).astype(np.int64), "by_law": np.bincount(pick, minlength=M).astype(np.int64)}
    o = o_all[at]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = o / np.sqrt(oo[at])[:, None]
        u_a, u_b = _philox_block(ids, seed, n_pass, 10)
        mu = np.empty(len(at))
        for j, (kind, g, nodes, F) in enumerate(laws):
            mine = np.flatnonzero(pick == j)
            mu[mine] = _law_mu(kind, g, nodes, F, u_a[mine], ids[mine], seed, n_pass)
        v_new = c * _turn_about(w, mu, u_b)
        dv_new = v_new - o
    v[at], dv[at] = _stored(v_new, dtype), _stored(dv_new, dtype)
    out["v"], out["dv"] = v, dv
    out["mu"][at], out["w"][at] = mu, w
    return out


class LayeredPhaseStep(tally.WriterStep):
    """Phase functions by radial layer, mixed and tabulated (not in the reference).  ``PhaseFunctionStep`` applies one law to the
    whole of space; this step, placed where a ``PhaseFunctionStep`` would stand -- directly BEHIND the scatter step of a pass
    (measures may stand between), before or behind an ``AbsorptionStep`` --, lets the law depend on where the photon stands: a
    Rayleigh atmosphere with a cloud or aerosol layer of another law inside it.

    * ``laws``: 1 to 8 laws, each ``"isotropic"``, ``"rayleigh"``, ``("hg", g)`` with ``|g| < 1``, or ``("table", mu_edges, p)``:
      a piecewise-constant phase function on ``K`` bins (``1 <= K <= 1024``, 2048 bins over all tables of a step) whose ``K + 1``
      edges rise strictly from exactly -1.0 to exactly 1.0, ``p`` the relative density per bin (finite, > 0; the step normalises
      it).  A table whose cumulative distribution is not strictly increasing in float64 is refused.  An ``("hg", g)`` law's
      ``mu`` is as accurate as ``PhaseFunctionStep``'s: 8 ulp(1) for ``|g| < 1/2``, ``32 ulp(1) / (1 - |g|)`` at and above it.
    * ``edges``: None -- one layer that holds everything -- or ``L + 1`` radii about ``center`` by ``AbsorptionStep``'s rule in
      every detail (at most 64 layers; layer ``b`` holds a photon iff ``e_b**2 <= q < e_(b+1)**2``, the last layer closed, no
      square root).
    * ``weights``: shape ``[L][M]`` (``[M]`` is accepted without ``edges``), finite and >= 0 with a positive sum in every row: row
      ``b`` is the probability with which an interaction in layer ``b`` uses each law.  May be omitted with one law.

    "Scattered in this pass" is ``PhaseFunctionStep``'s rule: a photon with ``dv != 0`` whose old velocity ``o = v - dv`` has
    ``0 < o.o < inf``.  Such a photon inside a layer is re-directed about ``o/|o|``; outside every layer (or with a NaN in ``q``) it
    keeps the direction the scatter step gave it and is counted as scattered, not as re-directed.  Plain ``Object``s are never
    touched; ``r``, ``dr``, ``E``, ids and kinds are left alone.  After each run ``self.scattered`` and ``self.redirected`` hold the
    pass's counts and ``self.by_layer`` (int64 ``[L]``, ``[1]`` without edges) and ``self.by_law`` (int64 ``[M]``) the re-directed
    photons by layer and by law, all global over shards and ranks; ``self.data`` gains the row ``[t, scattered, redirected, by_layer,
    by_law]`` and ``out_fn`` takes the rows at the end.  The arithmetic is written out in include/physicl_hip.h
    (pcl_step_phase_layered); ``_layered_phase_redirect`` restates it with numpy.

    The angle is drawn from the Philox blocks ``PhaseFunctionStep`` draws from (counter words 10 and 11), the law from a block of
    this step's own (word 13), keyed by ``sim.seed``, the photon's id and the step's pass counter ``_n_pass``: with one law and no edges
    the step leaves the store bit for bit as ``PhaseFunctionStep`` with that law leaves it.  Sharing the words means A PASS HOLDS
    ONE PHASE STEP: at its first run the step raises ``ValueError`` if the simulation's steps hold another ``PhaseFunctionStep`` or
    ``LayeredPhaseStep``.  Under the reference's Python semantics (``cl_on=False``) a hit leaves ``dv = v_old``, the rule above does
    not hold, and the step raises ``ValueError``.

    One launch per light step: the K-passes-per-launch kernels cannot re-direct a photon between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "phase"                                    # (the phase step's words 10 and 11 (13 is its own))
    _NOTE = "one launch per light step: a LayeredPhaseStep re-directs the scattered photons behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, laws, weights=None, edges=None, center=(0, 0, 0), out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self._laws, self.weights, self.cum, self.edges, self.center = _check_layered_phase(laws, weights, edges, center)
        self.laws = [k if k in ("isotropic", "rayleigh") else ("hg", g) if k == "hg" else ("table", mu, F) for k, g, mu, F in self._laws]
        self.scattered = self.redirected = 0
        self.by_layer = np.zeros(len(self.cum), dtype=np.int64)
        self.by_law = np.zeros(len(self._laws), dtype=np.int64)
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_pass(self, sim, scattered, redirected, by_layer, by_law):
        self.scattered, self.redirected = int(scattered), int(redirected)
        self.by_layer, self.by_law = np.array(by_layer, dtype=np.int64), np.array(by_law, dtype=np.int64)
        self.data.append(tally.object_row([tally._snap(sim.t), self.scattered, self.redirected, self.by_layer.copy(), self.by_law.copy()]))

    def _refuse(self, sim):
        name = type(self).__name__                       # (GridPhaseStep derives from this class)
        _dv_rule_refusal(sim, name, "its direction before the scatter")
        if self._pass == 0:                              # the words 10 and 11 are drawn from once per photon and pass
            steps = getattr(sim, "steps", None) or {}
            for other in (steps.values() if isinstance(steps, dict) else steps):
                if other is not self and isinstance(other, (PhaseFunctionStep, LayeredPhaseStep)):
                    raise ValueError("a pass holds one phase step: the simulation's steps hold a %s beside this %s, and "
                                     "both would draw from the same Philox blocks" % (type(other).__name__, name))

    def _sweep(self, sim, prep):
        scattered, redirected, by_layer, by_law = sim._dev.phase_layered(self._laws, self.cum, self.edges, self.center, _c_h_literals()[0],
                                                                         sim.seed, self._n_pass)
        return [np.array([scattered, redirected], dtype=np.int64), np.asarray(by_layer), np.asarray(by_law)]

    def _host_sweep(self, objs, ids, seed, prep):
        new = _layered_phase_apply(tally.vec3(objs, "r"), tally.vec3(objs, "v"), tally.vec3(objs, "dv"), _photons(objs), ids,
                                   self._laws, self.cum, self.edges, self.center, _c_h_literals()[0], seed, self._n_pass)
        return new, new["redirected"], (new["scattered"].sum(), new["redirected"].sum(), new["by_layer"], new["by_law"])

    terminate = tally.TallyStep.terminate                # (a row holds arrays: written as the tally steps write theirs, as plain lists)


# ---------------------------------------------------------------------------------------------- a continuous source
def _check_recycle(source, top, center, at_rest, spectrum):
    """(source, top or None, centre, at_rest, spectrum as (grid, cdf) float64 arrays or None) of a RecycleStep, or ValueError for
    everything pcl_step_recycle_spent would refuse."""
    from ._hip import RECYCLE_MAX_BINS                        # (the header's limit: one place)
    if not isinstance(source, PhotonSource):
        raise ValueError("source must be a PhotonSource, got %r" % (source,))
    if top is not None:
        top = _radius(top, "top", "top must be None or a number")
    center = tally.check_center(center)
    at_rest = bool(at_rest)
    if not at_rest and top is None:
        raise ValueError("at_rest and top: at least one of the two criteria must be on")
    return source, top, center, at_rest, _check_spectrum(spectrum, RECYCLE_MAX_BINS)


def _check_spectrum(spectrum, max_bins, name="spectrum"):
    """A table to draw energies from as ``(grid, cdf)`` float64 arrays, or None: what RecycleStep(spectrum=) accepts -- None,
    ``(grid, cdf)`` or a PhotonBatch with a table --, or ValueError."""
    if spectrum is None:
        return None
    if isinstance(spectrum, PhotonBatch):
        if spectrum.table is None:
            raise ValueError("%s: this PhotonBatch has no table (make it with generate_photons_bulk(T=...))" % name)
        cdf, grid = spectrum.table                             # (a batch keeps the fill's order)
    else:
        try:
            grid, cdf = spectrum
        except (TypeError, ValueError):
            raise ValueError("%s must be None, (grid, cdf) or a PhotonBatch with a table" % name) from None
    try:
        grid, cdf = np.array(grid, dtype=np.float64), np.array(cdf, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("%s: grid and cdf must be sequences of numbers" % name) from None
    if grid.ndim != 1 or cdf.ndim != 1 or len(grid) != len(cdf) or not 1 <= len(cdf) <= max_bins:
        raise ValueError("%s: grid and cdf must be two sequences of one length between 1 and %d, got shapes %r and %r"
                         % (name, max_bins, grid.shape, cdf.shape))
    if not np.all(np.isfinite(grid)):
        raise ValueError("%s: grid must be finite" % name)
    if np.any(np.isnan(cdf)) or np.any(np.diff(cdf) < 0) or cdf[-1] != 1.0:
        raise ValueError("%s: cdf must not decrease and must end in exactly 1" % name)
    return np.ascontiguousarray(grid), np.ascontiguousarray(cdf)


def _source_emit(ids, source, c, seed, word2, dir_word, pos_word):
    """(v, r) as (n, 3) float64 arrays: what pcl_store_apply_source's arithmetic (include/physicl_hip.h) makes of the Philox blocks
    (id_lo, id_hi, word2, dir_word) and (id_lo, id_hi, word2, pos_word) per id -- every operation the device's, one rounding
    each; sin / cos and the gaussian's log are libm's here, the library's own on the device."""
    ids = np.asarray(ids).reshape(-1)
    n = len(ids)
    c = np.float64(c)
    d, e1, e2, origin = (np.asarray(x, dtype=np.float64) for x in (source.d, source.e1, source.e2, source.origin))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if source.angular == "beam":
            v = np.tile(c * d, (n, 1))
        else:
            u_a, u_b = _philox_block(ids, seed, word2, dir_word)
            if source.angular == "isotropic":
                mu = 1.0 - 2.0 * u_a
            elif source.angular == "cone":
                mu = 1.0 - u_a * (1.0 - np.float64(source.cos_half_angle))
            else:
                mu = np.sqrt(1.0 - u_a)
            v = c * _direction(e1, e2, d, *_polar(mu, u_b), mu)
        if source.spatial == "point":
            r = np.tile(origin, (n, 1))
        else:
            u_c, u_d = _philox_block(ids, seed, word2, pos_word)
            radius = np.float64(source.radius)
            rho = radius * np.sqrt(u_c) if source.spatial == "disc" else radius * np.sqrt(-2.0 * np.log(1.0 - u_c))
            rc, rs = _azimuth(rho, u_d)
            r = origin + (rc[:, None] * e1 + rs[:, None] * e2)
    return v.reshape(n, 3), r.reshape(n, 3)


_RECYCLE_WORDS = (14, 15, 16)                                 # direction, position, energy (the header lists the words taken)


def _recycle_spent(r, v, E, photon, ids, source, top, center, at_rest, spectrum, c, seed, n_pass, dtype=np.float64):
    """What pcl_step_recycle_spent makes of (n, 3) float64 positions and velocities, the energies, who is a photon and the
    particles' ids, with numpy -- every operation the device's operation in the device's order, one rounding each
    (include/physicl_hip.h), and what is written rounded once to ``dtype``.  The rule, a beam, a point and the table look-up are the
    device's bit for bit; sin / cos and the gaussian's log are libm's here.  ``spectrum``: None or ``(grid, cdf)``.  A dict: ``r, v,
    dr, dv, E`` the new state (float64 arrays; rows of particles that are not spent are the arguments', ``dr`` and ``dv`` hold NaN
    there: the sweep does not write them) and the boolean masks ``at_rest``, ``escaped`` and ``spent``."""
    r, v = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v))
    n = len(r)
    E = np.full(n, np.nan) if E is None else np.array(E, dtype=np.float64).reshape(-1)
    photon = np.asarray(photon, dtype=bool).reshape(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        rest = np.zeros(n, dtype=bool)
        if at_rest:
            rest = _at_rest(v)
        gone = np.zeros(n, dtype=bool)
        if top is not None:
            d = r - np.asarray(center, dtype=np.float64)
            gone = ~rest & (_dot3(d, d) > np.float64(top) * np.float64(top))
    rest, gone = rest & photon, gone & photon
    spent = rest | gone
    at = np.flatnonzero(spent)
    ids = np.asarray(ids).reshape(-1)[at]
    v_new, r_new = _source_emit(ids, source, c, seed, n_pass, _RECYCLE_WORDS[0], _RECYCLE_WORDS[1])
    dr, dv = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    r[at], v[at] = _stored(r_new, dtype), _stored(v_new, dtype)
    dr[at], dv[at] = 0.0, 0.0
    if spectrum is not None:
        grid, cdf = (np.asarray(a, dtype=np.float64) for a in spectrum)
        u = _philox_block(ids, seed, n_pass, _RECYCLE_WORDS[2])[0]
        E[at] = _stored(grid[np.searchsorted(cdf, u, side="left")], dtype)                    # the first x with cdf[x] >= u
    return {"r": r, "v": v, "dr": dr, "dv": dv, "E": E, "at_rest": rest, "escaped": gone, "spent": spent}


class RecycleStep(tally.WriterStep):
    """A continuous source (not in the reference): the LAST step of a pass, behind a ``SurfaceReflectStep`` if there is one.  A photon
    the ground or the medium has absorbed stays in the store at rest, one that has left through the top of the atmosphere flies on for
    ever; this step gives the slots of both back to ``source``, a ``PhotonSource``.  The population stays constant
    (``len(sim.objects)`` does not change), the store dense and uniform, and the run converges to the steady state of a lamp that
    keeps emitting: ``self.recycled`` per pass is the source's emission rate.

    * ``at_rest=True``: a photon with ``v == (0, 0, 0)`` is spent (``-0.0`` counts as 0; a NaN in ``v`` is not at rest);
    * ``top``: None, or a positive radius about ``center`` (code units): a photon that is not at rest is spent iff ``q > top*top``,
      ``q = (d0*d0 + d1*d1) + d2*d2`` the squared distance from ``center`` in float64.  Exactly on the sphere is not gone, a NaN in
      ``r`` is not gone, ``q = inf`` is gone.  At least one of ``at_rest`` and ``top`` must be on.
    * ``spectrum=None``: every slot keeps its colour -- a recycled photon keeps its ``E``, and ``E`` is not even asked for, so a
      wavelength-dependent scatter step keeps its term cache.  That is exact for a monochromatic source, or wherever no sink depends
      on ``E``.  With ``wavelength_dep_scattering`` plus an ``AbsorptionStep``, blue slots die and are re-emitted more often, and the
      population drifts blue: give the spectrum.
    * ``spectrum=(grid, cdf)``: two float64 sequences of one length between 1 and 1024, ``cdf`` not decreasing and ending in exactly
      1: a recycled photon gets ``E = grid[x]`` for the first ``x`` with ``cdf[x] >= u`` (the table of ``generate_photons_bulk(T=...)``);
      or the ``PhotonBatch`` such a call returned, whose table is taken.  (After a device run with a spectrum the energies live on the
      device: read them with ``sim.download``.)

    A spent photon is re-emitted the way ``generate_photons_bulk(source=)`` created it (include/physicl_hip.h:
    pcl_store_apply_source), from Philox blocks keyed by ``sim.seed``, its id and the step's pass counter ``_n_pass``, in counter words
    no other kernel uses (14, 15, 16): ``r`` and ``v`` from the source, ``dr = dv = 0`` -- a newborn has not moved and has not scattered.
    Ids and kinds are never written: a slot keeps its id, every re-emission draws new numbers because the pass counter moves, and a
    sharded run recycles the same photons the same way.  Plain ``Object``s are never spent; a particle that is not spent is not
    written at all.  ``_recycle_spent`` restates the sweep with numpy.

    After each run ``self.at_rest``, ``self.escaped`` and ``self.recycled`` (their sum) hold the pass's counts (global over shards and
    ranks) and ``self.data`` gains the row ``[t, at_rest, escaped]``; ``out_fn`` takes the rows at the end of the run.  The step reads
    no ``dv`` rule, so it works under ``cl_on=False`` as well.

    One launch per light step: the K-passes-per-launch kernels cannot re-emit a photon between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "recycle"
    _NOTE = "one launch per light step: a RecycleStep re-emits the spent photons behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, source, top=None, center=(0, 0, 0), at_rest=True, spectrum=None, out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.source, self.top, self.center, self.rest_on, self.spectrum = _check_recycle(source, top, center, at_rest, spectrum)
        self.at_rest = self.escaped = self.recycled = 0
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_pass(self, sim, at_rest, escaped):
        self.at_rest, self.escaped = int(at_rest), int(escaped)
        self.recycled = self.at_rest + self.escaped
        self.data.append(tally.object_row([tally._snap(sim.t), self.at_rest, self.escaped]))

    @property
    def _writes(self):                                   # a recycled photon keeps its E without a spectrum
        return ("r", "dr", "v", "dv") + (() if self.spectrum is None else ("E",))

    def _sweep(self, sim, prep):
        return [np.array(sim._dev.recycle_spent(self.source, _c_h_literals()[0], self.rest_on, self.top, self.center, self.spectrum, sim.seed,
                                                self._n_pass), dtype=np.int64)]

    def _host_sweep(self, objs, ids, seed, prep):
        E, photon = tally.photon_energies(objs, PhotonObject)
        new = _recycle_spent(tally.vec3(objs, "r"), tally.vec3(objs, "v"), E, photon, ids, self.source, self.top,
                             self.center, self.rest_on, self.spectrum, _c_h_literals()[0], seed, self._n_pass)
        return new, new["spent"], (new["at_rest"].sum(), new["escaped"].sum())


# ---------------------------------------------------------------------------------------------- absorption along the path
def _check_path_absorb(k, edges, center, E_edges):
    """(k as a float64 array [max(L, 1)][max(B, 1)], edges or None, centre, energy edges or None) of a PathAbsorptionStep, or
    ValueError for everything pcl_step_absorb_path would refuse."""
    from ._hip import PATH_ABSORB_MAX_BANDS, PATH_ABSORB_MAX_CELLS, PATH_ABSORB_MAX_LAYERS      # (the header's limits: one place)
    try:
        ka = np.array(k, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("k must be a number, or numbers per layer and / or energy band") from None
    if edges is not None:
        edges = tally.check_edges("edges", edges, PATH_ABSORB_MAX_LAYERS, "square")        # (the device compares q with e*e)
    if E_edges is not None:
        E_edges = tally.check_edges("E_edges", E_edges, PATH_ABSORB_MAX_BANDS)
    want = tuple(len(e) - 1 for e in (edges, E_edges) if e is not None)
    if ka.shape != want:
        raise ValueError("k must have the shape %r -- %s -- got %r" % (want, {
            (False, False): "one number without edges and E_edges", (True, False): "one value per layer of edges",
            (False, True): "one value per band of E_edges", (True, True): "layers of edges by bands of E_edges"}[
                (edges is not None, E_edges is not None)], ka.shape))
    if not np.all(np.isfinite(ka) & (ka >= 0.0)):             # (False for NaN as well)
        raise ValueError("k must be finite and not negative, got %r" % (k,))
    rows, cols = (1 if e is None else len(e) - 1 for e in (edges, E_edges))
    if rows * cols > PATH_ABSORB_MAX_CELLS:
        raise ValueError("k: %d layers of edges x %d bands of E_edges are %d cells, at most %d are supported" % (rows, cols, rows * cols, PATH_ABSORB_MAX_CELLS))
    return np.ascontiguousarray(ka.reshape(rows, cols)), edges, tally.check_center(center), E_edges


def _path_probability(k, c, dt):
    """The chance that a photon is absorbed over one pass's move, float64: ``tau = k * (c * dt)``, ``p = -expm1(-tau)`` -- made on the
    host, the device only ever sees ``p``.  ValueError for a ``dt`` that is not finite or is negative."""
    dt = _scalar(dt, "dt must be a number, got %r" % (dt,))
    if not (np.isfinite(dt) and dt >= 0.0):
        raise ValueError("dt must be finite and not negative, got %r" % (dt,))
    with np.errstate(over="ignore"):
        tau = np.asarray(k, dtype=np.float64) * (np.float64(c) * np.float64(dt))
    return -np.expm1(-tau)


_PATH_ABSORB_WORD = 17                                        # the draw's counter word (the header lists the words taken)


def _path_draw(r, v, E, photon, ids, p, edges, center, E_edges, seed, n_pass, word):
    """Who is exposed over the move of a pass and whose draw falls below the cell's probability -- the lines pcl_step_absorb_path and
    pcl_step_scatter_layered share, on (n, 3) float64 ``r`` and ``v``: ``(p as [L'][B'], layer, band, exposed, drawn)``.  ``layer`` and
    ``band``: int64, of every moving photon, -1 for none; ``exposed``: a moving photon with both; ``drawn``: the places whose
    ``u53(w0, w1)`` of the counter ``(id_lo, id_hi, n_pass, word)`` is below ``p[layer][band]`` (a cell with p == 0 draws nothing)."""
    n = len(v)
    rows, cols = (1 if e is None else len(e) - 1 for e in (edges, E_edges))
    p = np.asarray(p, dtype=np.float64).reshape(rows, cols)
    with np.errstate(invalid="ignore", over="ignore"):
        at = np.flatnonzero(~_at_rest(v) & np.asarray(photon, dtype=bool).reshape(-1))
        layer, band = np.full(n, -1, dtype=np.int64), np.full(n, -1, dtype=np.int64)
        layer[at] = _layer_of(r[at], edges, center)
        at = at[layer[at] >= 0]
        if E_edges is None:
            band[at] = 0
        else:                                                  # NaN and under/overflow: in no band
            band[at] = _bin_of(np.asarray(E, dtype=np.float64).reshape(-1)[at], np.asarray(E_edges, dtype=np.float64))
    exposed = band >= 0
    draws = np.flatnonzero(exposed)
    draws = draws[p[layer[draws], band[draws]] > 0.0]          # a cell with p == 0 draws nothing
    u = _philox_block(np.asarray(ids).reshape(-1)[draws], seed, n_pass, word)[0]
    return p, layer, band, exposed, draws[u < p[layer[draws], band[draws]]]


def _absorb_path(r, v, dv, E, photon, ids, p, edges, center, E_edges, seed, n_pass, dtype=np.float64):
    """What pcl_step_absorb_path makes of (n, 3) float64 positions, velocities and last velocity changes, the energies, who is a
    photon and the particles' ids, with numpy -- every operation the device's operation in the device's order, one rounding each
    (include/physicl_hip.h): no transcendental function, no division and no square root, so everything is the device's bit for bit.
    ``p``: the probabilities, max(L, 1) rows of max(B, 1) values.  What is written is zero, in any ``dtype``.  A dict: ``v, dv`` the new
    state (float64 arrays; rows that are not absorbed are the arguments'), the boolean masks ``exposed`` and ``absorbed``, ``layer``
    and ``band`` (int64: of every moving photon, -1 for none) and the tally ``absorbed_by_cell`` (int64 [L', B'])."""
    r, v, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v, dv))
    n = len(v)
    p, layer, band, exposed, gone = _path_draw(r, v, E, photon, ids, p, edges, center, E_edges, seed, n_pass, _PATH_ABSORB_WORD)
    cols = p.shape[1]
    absorbed = np.zeros(n, dtype=bool)
    absorbed[gone] = True
    v[gone], dv[gone] = np.zeros(3, dtype=dtype), np.zeros(3, dtype=dtype)
    cells = np.bincount(layer[gone] * cols + band[gone], minlength=p.size).astype(np.int64).reshape(p.shape)
    return {"v": v, "dv": dv, "exposed": exposed, "absorbed": absorbed, "layer": layer, "band": band, "absorbed_by_cell": cells}


class PathAbsorptionStep(tally.WriterStep):
    """A gas that absorbs without scattering (not in the reference): continuous, Beer-Lambert absorption along the move every photon
    makes in a pass, with a coefficient that depends on the radial layer the photon stands in and on the band its energy falls in --
    ozone above a thin Rayleigh atmosphere, a water-vapour band.  ``AbsorptionStep`` acts on the photons the scatter step made
    interact, and its ``omega0`` is grey; this step needs no scatter step at all.  It stands anywhere BEHIND the Newton step of a pass
    (before or behind the scatter, phase, absorption and ground steps) and before a ``RecycleStep``.  In front of a
    ``SurfaceReflectStep`` let the innermost edge be the ground's radius or above it: the ground decides by ``r`` and ``dr`` alone, so a
    photon parked below it would be bounced off again; one that stands in no layer is left to the ground.

    * ``k``: the absorption coefficient per unit length (code units), finite and not negative: one number; ``[L]`` numbers with
      ``edges`` only; ``[B]`` with ``E_edges`` only; ``[L][B]`` with both.
    * ``edges``: ``L + 1`` finite, non-negative, strictly increasing radii about ``center`` (at most 64 layers), ``AbsorptionStep``'s
      rule exactly: layer ``b`` holds a photon iff ``e_b**2 <= q < e_(b+1)**2``, the last layer closed, ``q = (d0*d0 + d1*d1) + d2*d2``
      in float64; no square root is taken; a NaN is in no layer.
    * ``E_edges``: ``B + 1`` finite, strictly increasing energy edges in the unit E is stored in (at most 1024 bands, and at most 4096
      cells of layers x bands): ``numpy.histogram``'s bins, the last one closed; a NaN or an energy outside the edges is in no band.
      Without ``E_edges`` the gas is grey and E is not even asked for, so a wavelength-dependent scatter step keeps its term cache;
      with them that cache is dropped every pass (the library has no read-only access to E).

    A photon moves ``c*dt`` in every pass -- across a bounce off the ground too --, so the path length is not read from the store:
    per pass the host makes ``tau = k * (c * dt)`` from the simulation's current ``dt`` and ``p = -numpy.expm1(-tau)`` in float64
    (``_path_probability``), and the device only ever sees ``p``.  A ``dt`` that is not finite or is negative is refused.

    Every moving photon with a layer and a band is EXPOSED; a photon at rest (``v == (0, 0, 0)``; ``-0.0`` counts as 0, a NaN moves), a
    plain ``Object`` and a photon in no layer or no band are skipped.  An exposed photon is absorbed iff ``u < p`` (``p == 0`` draws
    nothing, ``p == 1`` absorbs every one), ``u`` from a Philox block keyed by ``sim.seed``, the photon's id and the step's pass counter
    ``_n_pass``, in a counter word no other kernel uses (17): every other step draws what it draws without this one, and a photon
    draws the same number however the run is sharded.  Several ``PathAbsorptionStep``s in one pass -- two gases whose layers and
    bands overlap -- count on through one another (``tally.WriterStep``): their draws are independent, and a photon exposed to both
    survives with ``(1 - p1)(1 - p2)``.  An absorbed photon is parked at rest where it is, ``v = 0`` and ``dv = 0`` --
    ``AbsorptionStep``'s convention and for its reason: a phase or absorption step later in the pass leaves it alone, and
    ``RecycleStep(at_rest=True)`` gives its slot back to the source.  A photon that is not absorbed is not written at all; ``r``,
    ``dr``, ``E``, ids and kinds are never written.  The analog treatment keeps E the photon's colour (it is no statistical weight).

    After each run ``self.exposed`` and ``self.absorbed`` hold the pass's counts and ``self.absorbed_by_cell`` an int64 array
    ``[max(L, 1)][max(B, 1)]`` -- a heating profile by colour --, global over shards and ranks; ``self.data`` gains the row ``[t,
    exposed, absorbed, absorbed_by_cell]``; ``out_fn`` takes the rows at the end.  The rule is written out in include/physicl_hip.h
    (pcl_step_absorb_path); ``_absorb_path`` restates every bit of it with numpy.  The step reads no ``dv`` rule, so it works under
    ``cl_on=False`` as well.

    One launch per light step: the K-passes-per-launch kernels cannot absorb a photon between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "path_absorb"
    _NOTE = "one launch per light step: a PathAbsorptionStep absorbs moving photons behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, k, edges=None, center=(0, 0, 0), E_edges=None, out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.k, self.edges, self.center, self.E_edges = _check_path_absorb(k, edges, center, E_edges)
        self.exposed = self.absorbed = 0
        self.absorbed_by_cell = np.zeros(self.k.shape, dtype=np.int64)
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_pass(self, sim, exposed, absorbed, cells):
        self.exposed, self.absorbed = int(exposed), int(absorbed)
        self.absorbed_by_cell = np.array(cells, dtype=np.int64).reshape(self.k.shape)
        self.data.append(tally.object_row([tally._snap(sim.t), self.exposed, self.absorbed, self.absorbed_by_cell.copy()]))

    def _prepare(self, sim, on_host):                    # p of this pass's dt; a dt that is refused raises here
        return _path_probability(self.k, _c_h_literals()[0], np.asarray(sim.dt) if on_host else sim._dt_code())

    def _sweep(self, sim, p):
        exposed, absorbed, cells = sim._dev.absorb_path(p, self.edges, self.center, self.E_edges, sim.seed, self._n_pass)
        return [np.array([exposed, absorbed], dtype=np.int64), np.asarray(cells, dtype=np.int64)]

    def _host_sweep(self, objs, ids, seed, p):
        E, photon = tally.photon_energies(objs, PhotonObject)
        new = _absorb_path(tally.vec3(objs, "r"), tally.vec3(objs, "v"), tally.vec3(objs, "dv"), E, photon, ids, p,
                           self.edges, self.center, self.E_edges, seed, self._n_pass)
        return new, new["absorbed"], (new["exposed"].sum(), new["absorbed"].sum(), new["absorbed_by_cell"])

    terminate = tally.TallyStep.terminate                # (a row holds arrays: written as the tally steps write theirs, as plain lists)


# ---------------------------------------------------------------------------------------------- scattering by layer and band
_LAYERED_SCATTER_WORDS = (23, 24)                             # the draw, the direction (the header lists the words taken)


def _scatter_layered(r, v, dv, E, photon, ids, p, edges, center, E_edges, first, c, seed, n_pass, dtype=np.float64):
    """What pcl_step_scatter_layered makes of (n, 3) float64 positions, velocities and last velocity changes, the energies, who is a
    photon and the particles' ids, with numpy -- every operation the device's operation in the device's order, one rounding each
    (include/physicl_hip.h), and what is written rounded once to ``dtype``.  Who is exposed, who is hit and every tally are the
    device's bit for bit; sin / cos are libm's here.  ``p``: the probabilities, max(L, 1) rows of max(B, 1) values; ``first``: the
    pass's first scatterer (a photon that is not scattered gets dv = 0) or not (it is not written).  A dict: ``v, dv`` the new state
    (float64 arrays; rows that are not written are the arguments'), the boolean masks ``exposed``, ``scattered`` and ``written``,
    ``layer`` and ``band`` (int64: of every moving photon, -1 for none) and the tally ``scattered_by_cell`` (int64 [L', B'])."""
    r, v, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v, dv))
    n = len(v)
    photon = np.asarray(photon, dtype=bool).reshape(-1)
    p, layer, band, exposed, hit = _path_draw(r, v, E, photon, ids, p, edges, center, E_edges, seed, n_pass, _LAYERED_SCATTER_WORDS[0])
    u_a, u_b = _philox_block(np.asarray(ids).reshape(-1)[hit], seed, n_pass, _LAYERED_SCATTER_WORDS[1])
    with np.errstate(invalid="ignore", over="ignore"):
        v_new = np.float64(c) * _turn_about(np.tile([1.0, 0.0, 0.0], (len(hit), 1)), 1.0 - 2.0 * u_a, u_b)     # uniform on the sphere
        dv[hit] = _stored(v_new - v[hit], dtype)               # the scatter step's mark, from the old velocity
    v[hit] = _stored(v_new, dtype)
    scattered = np.zeros(n, dtype=bool)
    scattered[hit] = True
    written = scattered | (photon & bool(first))
    dv[written & ~scattered] = 0.0                             # first: "did not scatter in this pass"
    cells = np.bincount(layer[hit] * p.shape[1] + band[hit], minlength=p.size).astype(np.int64).reshape(p.shape)
    return {"v": v, "dv": dv, "exposed": exposed, "scattered": scattered, "written": written, "layer": layer, "band": band,
            "scattered_by_cell": cells}


class LayeredScatterStep(tally.WriterStep):
    """Who scatters, by radial layer and energy band (not in the reference): the scattering twin of ``PathAbsorptionStep``.
    ``ScatterIsotropicStep`` decides with ``A * n * |dr|`` -- ``n`` a constant or a closed-form expression, the only colour a
    ``lambda^-4`` --; this step takes a scattering coefficient from a table: a cloud with its own optical depth, an aerosol layer
    with a ``lambda^-1`` spectrum beside the Rayleigh one, a drop or a fog bank in vacuum with no ``ScatterIsotropicStep`` at all.
    It stands BEHIND the Newton step of a pass -- alone, or behind a ``ScatterIsotropicStep`` -- and in front of the phase,
    absorption and ground steps.

    * ``k``: the scattering coefficient per unit length (code units), finite and not negative: one number; ``[L]`` numbers with
      ``edges`` only; ``[B]`` with ``E_edges`` only; ``[L][B]`` with both.
    * ``edges``, ``center``, ``E_edges``: ``PathAbsorptionStep``'s arguments by ``PathAbsorptionStep``'s rules, limits (64 layers, 1024
      bands, 4096 cells) and error messages: layer ``b`` holds a photon iff ``e_b**2 <= q < e_(b+1)**2``, the last layer closed, no
      square root taken; the bands are ``numpy.histogram``'s bins; without ``E_edges`` E is neither read nor asked for, so a
      wavelength-dependent scatter step keeps its term cache.
    * ``first``: True -- this step is the pass's first scatterer and keeps ``ScatterIsotropicStep``'s contract: every photon it does
      not scatter gets ``dv = 0``, exposed or not, at rest or not.  False -- it stands behind another scatterer: a photon that is not
      scattered is not written at all, so the earlier step's mark survives.  None (the default) is decided at the step's first run
      from the simulation's step order: False iff a ``ScatterIsotropicStep``, a ``ScatterSphericalStep``, another
      ``LayeredScatterStep`` or a ``GridScatterStep`` stands earlier in the pass.  A ``ScatterIsotropicStep`` BEHIND this step would wipe its marks: the first
      run raises ``ValueError``.

    Per pass the host makes ``p = -numpy.expm1(-k * (c * dt))`` from the simulation's current ``dt`` (``_path_probability``), and the
    device only ever sees ``p``.  Every moving photon with a layer and a band is EXPOSED (a photon at rest -- ``-0.0`` counts as 0, a
    NaN moves --, a plain ``Object`` and a photon in no layer or no band are skipped); it scatters iff ``u < p`` (``p == 0`` draws
    nothing), ``u`` from a Philox block keyed by ``sim.seed``, the photon's id and the step's pass counter ``_n_pass``, in counter words
    no other kernel uses (23, and 24 for the direction): every other step draws what it draws without this one, and a sharded run
    scatters the same photons the same way.  Several ``LayeredScatterStep``s in one pass count on through one another
    (``tally.WriterStep``): each draws its own hits and its own directions.  The draws are made on the device with every ``rng=``
    setting.  A hit gets a direction
    uniform on the sphere at speed c -- ``ReemissionStep``'s isotropic arithmetic -- and the scatter step's mark: ``v = v'``,
    ``dv = v' - v_old``.  ``r``, ``dr``, ``E``, ids and kinds are never written; plain ``Object``s are never touched.

    What follows from the ``dv`` contract:

    * a ``PhaseFunctionStep`` or ``LayeredPhaseStep`` behind this step re-directs its hits about ``v - dv``, the direction before the
      scatter: that is how a cloud gets both its optical depth and its forward peak;
    * an ``AbsorptionStep`` behind it gives the cloud its own ``omega0``;
    * two scatterers that both hit one photon in one pass are two scatterings, and the phase step turns about the direction after
      the first;
    * a hit whose new direction equals the old one bit for bit reads as a miss -- the same negligible case as in the scatter step.

    After each run ``self.exposed`` and ``self.scattered`` hold the pass's counts and ``self.scattered_by_cell`` an int64 array
    ``[max(L, 1)][max(B, 1)]``, global over shards and ranks; ``self.data`` gains the row ``[t, exposed, scattered,
    scattered_by_cell]``; ``out_fn`` takes the rows at the end.  The rule is written out in include/physicl_hip.h
    (pcl_step_scatter_layered); ``_scatter_layered`` restates it with numpy.  The step writes its own ``dv`` rule and reads none, so it
    works under ``cl_on=False`` -- but not with ``first=False`` there: the Python-semantics scatter step leaves ``dv = v_old``, and
    nothing behind it can use the marks.

    One launch per light step: the K-passes-per-launch kernels cannot scatter a photon by a table between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "scatter_layered"
    _NOTE = "one launch per light step: a LayeredScatterStep scatters moving photons by layer and band behind every pass, which " \
            "the K-passes-per-launch kernels cannot carry"

    def __init__(self, k, edges=None, center=(0, 0, 0), E_edges=None, first=None, out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.k, self.edges, self.center, self.E_edges = _check_path_absorb(k, edges, center, E_edges)
        if first is not None and not isinstance(first, (bool, np.bool_)):
            raise ValueError("first must be None, True or False, got %r" % (first,))
        self.first = None if first is None else bool(first)
        self.exposed = self.scattered = 0
        self.scattered_by_cell = np.zeros(self.k.shape, dtype=np.int64)
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_pass(self, sim, exposed, scattered, cells):
        self.exposed, self.scattered = int(exposed), int(scattered)
        self.scattered_by_cell = np.array(cells, dtype=np.int64).reshape(self.k.shape)
        self.data.append(tally.object_row([tally._snap(sim.t), self.exposed, self.scattered, self.scattered_by_cell.copy()]))

    def _refuse(self, sim):
        first = self.first
        if self._pass == 0:                              # the step order is looked at once, before anything moves
            front, behind = tally.earlier_steps(sim, self)   # (stated once, beside the writer steps' counter rule)
            for other in behind:
                if isinstance(other, ScatterIsotropicStep):
                    raise ValueError("a pass marks its scattered photons once: the simulation's steps hold a %s behind this "
                                     "%s, and it would overwrite the dv of every photon this step has scattered -- "
                                     "put the %s behind it" % (type(other).__name__, type(self).__name__, type(self).__name__))
            if first is None:
                first = not any(isinstance(other, (ScatterIsotropicStep, LayeredScatterStep, GridScatterStep)) for other in front)
        if first is False:
            _dv_rule_refusal(sim, "%s(first=False)" % type(self).__name__, "the earlier scatter step's marks")
        self.first = first

    def _prepare(self, sim, on_host):                    # p of this pass's dt; a dt that is refused raises here
        return _path_probability(self.k, _c_h_literals()[0], np.asarray(sim.dt) if on_host else sim._dt_code())

    def _sweep(self, sim, p):
        exposed, scattered, cells = sim._dev.scatter_layered(p, self.edges, self.center, self.E_edges, self.first, _c_h_literals()[0],
                                                             sim.seed, self._n_pass)
        return [np.array([exposed, scattered], dtype=np.int64), np.asarray(cells, dtype=np.int64)]

    def _host_sweep(self, objs, ids, seed, p):
        E, photon = tally.photon_energies(objs, PhotonObject)
        new = _scatter_layered(tally.vec3(objs, "r"), tally.vec3(objs, "v"), tally.vec3(objs, "dv"), E, photon, ids, p, self.edges,
                               self.center, self.E_edges, self.first, _c_h_literals()[0], seed, self._n_pass)
        return new, new["written"], (new["exposed"].sum(), new["scattered"].sum(), new["scattered_by_cell"])

    terminate = tally.TallyStep.terminate                # (a row holds arrays: written as the tally steps write theirs, as plain lists)


# ---------------------------------------------------------------------------------------------- scattering on a grid of cells
_GRID_SCATTER_WORDS = (25, 26)                                # the draw, the direction (the header lists the words taken)


def _check_grid_scatter(k, axes, edges, center, E_edges):
    """(k as a float64 array of the grid's shape (+ (B,) with E_edges), axes, edges, centre, energy edges or None) of a
    GridScatterStep, or ValueError for everything pcl_step_scatter_grid would refuse.  A single number is broadcast."""
    from ._hip import SCATTER_GRID_MAX_BANDS, SCATTER_GRID_MAX_CELLS      # (the header's limits: one place)
    axes, edges, center = _check_grid(axes, edges, center)
    if E_edges is not None:
        E_edges = tally.check_edges("E_edges", E_edges, SCATTER_GRID_MAX_BANDS)
    try:
        ka = np.array(k, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("k must be a number, or numbers per cell of the grid (and energy band)") from None
    want = tuple(len(e) - 1 for e in edges) + (() if E_edges is None else (len(E_edges) - 1,))
    if ka.shape not in ((), want):
        raise ValueError("k must be one number or have the shape %r -- %s -- got %r" % (
            want, "the grid's cells" + ("" if E_edges is None else " by bands of E_edges"), ka.shape))
    if not np.all(np.isfinite(ka) & (ka >= 0.0)):             # (False for NaN as well)
        raise ValueError("k must be finite and not negative, got %r" % (k,))
    cells = int(np.prod(want))
    if cells > SCATTER_GRID_MAX_CELLS:
        raise ValueError("k: %s are %d cells, at most %d are supported" % (" x ".join(str(n) for n in want), cells, SCATTER_GRID_MAX_CELLS))
    return np.ascontiguousarray(np.broadcast_to(ka, want)), axes, edges, center, E_edges


def _scatter_grid(r, v, dv, E, photon, ids, p, axes, edges, center, E_edges, first, c, seed, n_pass, dtype=np.float64):
    """What pcl_step_scatter_grid makes of (n, 3) float64 positions, velocities and last velocity changes, the energies, who is a
    photon and the particles' ids, with numpy -- every operation the device's operation in the device's order, one rounding each
    (include/physicl_hip.h), and what is written rounded once to ``dtype``.  Who is exposed, who is hit and every tally are the
    device's bit for bit; sin / cos are libm's here.  ``p``: the probabilities, one per cell of the grid (row-major in the order of
    ``axes``) and band; ``first``: the pass's first scatterer (a photon that is not scattered gets dv = 0) or not (it is not written).
    A dict: ``v, dv`` the new state (float64 arrays; rows that are not written are the arguments'), the boolean masks ``exposed``,
    ``scattered`` and ``written``, ``cell`` (int64: cell of the grid times B' plus the band, of every exposed photon, -1 for none)
    and the tally ``scattered_by_cell`` (int64, the grid's shape, with a last dimension of B bands if ``E_edges`` is given)."""
    r, v, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v, dv))
    n = len(v)
    photon = np.asarray(photon, dtype=bool).reshape(-1)
    edges = [np.asarray(e, dtype=np.float64) for e in edges]
    shape = tuple(len(e) - 1 for e in edges) + (() if E_edges is None else (len(E_edges) - 1,))
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    cell = np.full(n, -1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        at = np.flatnonzero(~_at_rest(v) & photon)
        ok, g = _cell_of_positions(r[at], axes, edges, np.asarray(center, dtype=np.float64))
        at, g = at[ok], g[ok]
        if E_edges is not None:                                # NaN and under/overflow: in no band
            Ee = np.asarray(E_edges, dtype=np.float64)
            band = _bin_of(np.asarray(E, dtype=np.float64).reshape(-1)[at], Ee)
            at, g = at[band >= 0], g[band >= 0] * (len(Ee) - 1) + band[band >= 0]
    cell[at] = g
    exposed = cell >= 0
    draws = at[p[g] > 0.0]                                     # a cell with p == 0 draws nothing
    u = _philox_block(np.asarray(ids).reshape(-1)[draws], seed, n_pass, _GRID_SCATTER_WORDS[0])[0]
    hit = draws[u < p[cell[draws]]]
    u_a, u_b = _philox_block(np.asarray(ids).reshape(-1)[hit], seed, n_pass, _GRID_SCATTER_WORDS[1])
    with np.errstate(invalid="ignore", over="ignore"):
        v_new = np.float64(c) * _turn_about(np.tile([1.0, 0.0, 0.0], (len(hit), 1)), 1.0 - 2.0 * u_a, u_b)     # uniform on the sphere
        dv[hit] = _stored(v_new - v[hit], dtype)               # the scatter step's mark, from the old velocity
    v[hit] = _stored(v_new, dtype)
    scattered = np.zeros(n, dtype=bool)
    scattered[hit] = True
    written = scattered | (photon & bool(first))
    dv[written & ~scattered] = 0.0                             # first: "did not scatter in this pass"
    cells = np.bincount(cell[hit], minlength=p.size).astype(np.int64).reshape(shape)
    return {"v": v, "dv": dv, "exposed": exposed, "scattered": scattered, "written": written, "cell": cell, "scattered_by_cell": cells}


class GridScatterStep(LayeredScatterStep):
    """Who scatters, by cell of a 3-D grid and energy band (not in the reference): ``LayeredScatterStep`` with
    ``PositionGridMeasureStep``'s cells in place of the concentric layers -- a cloud of finite width, a broken cloud field, a plume
    or a fog bank over half of the scene, a cloud that shades the ground beside it.  It stands where a ``LayeredScatterStep`` stands:
    BEHIND the Newton step of a pass -- alone, or behind other scatterers -- and in front of the phase, absorption and ground steps.

    * ``axes``, ``edges``, ``center``: ``PositionGridMeasureStep``'s arguments by its rules, limits and error messages: one to three
      distinct names out of ``"x"``, ``"y"``, ``"z"``, ``"r"``, one sequence of bin edges per axis (at most 1024 bins per axis).  The
      cell of a photon is the cell that step would count it in: bins ``[e_b, e_b+1)``, the last one closed; an ``"r"`` axis compares
      ``q = ((x-cx)*(x-cx) + (y-cy)*(y-cy)) + (z-cz)*(z-cz)`` in float64 with the squared edges, no square root is taken; a NaN or a
      position outside any axis's range is in no cell; cells are row-major in the order of ``axes``.
    * ``E_edges``: ``LayeredScatterStep``'s argument by its rule: ``B + 1`` energy edges, ``numpy.histogram``'s bins, at most 1024
      bands.  Without it E is neither read nor asked for, so a wavelength-dependent scatter step keeps its term cache.
    * ``k``: the scattering coefficient per unit length (code units), finite and not negative: one number, or an array of the grid's
      shape (without ``E_edges``) or the grid's shape ``+ (B,)`` (with them).  At most ``2**20`` cells (grid cells times bands).
    * ``first``: ``LayeredScatterStep``'s argument with the same meaning: True -- every photon this step does not scatter gets
      ``dv = 0``; False -- a photon that is not scattered is not written at all, so an earlier scatterer's mark survives (refused
      under ``cl_on=False``); None (the default) is decided at the step's first run: False iff a ``ScatterIsotropicStep``, a
      ``ScatterSphericalStep``, a ``LayeredScatterStep`` or another ``GridScatterStep`` stands earlier in the pass.  A
      ``ScatterIsotropicStep`` BEHIND this step would wipe its marks: the first run raises ``ValueError``.

    Per pass the host makes ``p = -numpy.expm1(-k * (c * dt))`` from the simulation's current ``dt`` (``_path_probability``), and the
    device only ever sees ``p``.  Every moving photon with a cell (and a band, with ``E_edges``) is EXPOSED (a photon at rest --
    ``-0.0`` counts as 0, a NaN moves --, a plain ``Object`` and a photon in no cell or no band are skipped); it scatters iff
    ``u < p`` (``p == 0`` draws nothing), ``u`` from a Philox block keyed by ``sim.seed``, the photon's id and the step's pass counter
    ``_n_pass``, in counter words no other kernel uses (25, and 26 for the direction).  Several ``GridScatterStep``s in one pass count
    on through one another (``tally.WriterStep``).  A hit gets a direction uniform on the sphere at speed c and the scatter step's
    mark, ``v = v'``, ``dv = v' - v_old`` -- ``LayeredScatterStep``'s arithmetic line for line, so a ``PhaseFunctionStep`` or
    ``LayeredPhaseStep`` behind this step re-directs its hits about ``v - dv`` and an ``AbsorptionStep`` gives them an ``omega0``; those
    steps act by radial layer, not by cell -- ``GridPhaseStep`` (light_grid.py) is the phase step that acts by cell, ``GridAbsorptionStep``
    (there, too) the absorption.  ``r``, ``dr``, ``E``, ids and kinds are never written.

    After each run ``self.exposed`` and ``self.scattered`` hold the pass's counts and ``self.scattered_by_cell`` an int64 array of
    ``k``'s broadcast shape, global over shards and ranks; ``self.data`` gains the row ``[t, exposed, scattered,
    scattered_by_cell]``; ``out_fn`` takes the rows at the end.  The rule is written out in include/physicl_hip.h
    (pcl_step_scatter_grid); ``_scatter_grid`` restates it with numpy.

    Cost: up to 4096 cells the table and the tallies live in LDS; above that the kernel reads ``p`` from device memory and adds its
    hits there.  Either way the table goes up over the host link and the tallies come back every pass -- 8 MB each way at ``2**20``
    cells -- and a sharded run all-reduces the tallies in pieces of ``tally.ALLREDUCE_CHUNK``; nothing is cached between passes.

    One launch per light step: the K-passes-per-launch kernels cannot scatter a photon by a table between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "scatter_grid"                             # (words 25 and 26: not the parent's)
    _NOTE = "one launch per light step: a GridScatterStep scatters moving photons by grid cell and band behind every pass, which " \
            "the K-passes-per-launch kernels cannot carry"

    def __init__(self, k, axes, edges, center=(0, 0, 0), E_edges=None, first=None, out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.k, self.axes, self.edges, self.center, self.E_edges = _check_grid_scatter(k, axes, edges, center, E_edges)
        if first is not None and not isinstance(first, (bool, np.bool_)):
            raise ValueError("first must be None, True or False, got %r" % (first,))
        self.first = None if first is None else bool(first)
        self.exposed = self.scattered = 0
        self.scattered_by_cell = np.zeros(self.k.shape, dtype=np.int64)
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _sweep(self, sim, p):
        exposed, scattered, cells = sim._dev.scatter_grid(p, self.axes, self.edges, self.center, self.E_edges, self.first,
                                                          _c_h_literals()[0], sim.seed, self._n_pass)
        return [np.array([exposed, scattered], dtype=np.int64), np.asarray(cells, dtype=np.int64)]

    def _host_sweep(self, objs, ids, seed, p):
        E, photon = tally.photon_energies(objs, PhotonObject)
        new = _scatter_grid(tally.vec3(objs, "r"), tally.vec3(objs, "v"), tally.vec3(objs, "dv"), E, photon, ids, p, self.axes, self.edges,
                            self.center, self.E_edges, self.first, _c_h_literals()[0], seed, self._n_pass)
        return new, new["written"], (new["exposed"].sum(), new["scattered"].sum(), new["scattered_by_cell"])


# ---------------------------------------------------------------------------------------------- the walls of a box
_BOX_WALLS = ("periodic", "mirror", "open")


def _check_box(lo, hi, walls):
    """(lo, hi as 3 float64 each, the three walls -- ``"periodic"``, ``"mirror"``, ``"open"`` or None per axis) of a BoxBoundaryStep, or
    ValueError for everything pcl_step_box_walls would refuse.  One wall stands for all three axes."""
    if walls is None or isinstance(walls, str):
        walls = (walls,) * 3
    try:
        walls = tuple(walls)
    except TypeError:
        raise ValueError("walls must be one of %s or None, or three of them (x, y, z)" % ", ".join(repr(w) for w in _BOX_WALLS)) from None
    if len(walls) != 3 or any(w is not None and (not isinstance(w, str) or w not in _BOX_WALLS) for w in walls):
        raise ValueError("walls must be one of %s or None, or three of them (x, y, z), got %r" % (", ".join(repr(w) for w in _BOX_WALLS), walls))
    if all(w is None for w in walls):
        raise ValueError("walls: a box needs a wall on one axis at least, got None for all three")
    bounds = []
    for name, x in (("lo", lo), ("hi", hi)):
        try:
            x = np.array(x, dtype=np.float64)                   # a Measurement is taken by its stored value, as center is
        except (TypeError, ValueError):
            raise ValueError("%s must be three numbers" % name) from None
        if x.shape != (3,):
            raise ValueError("%s must be three numbers, got %r" % (name, x))
        bounds.append(np.ascontiguousarray(x))
    lo, hi = bounds
    for k, w in enumerate(walls):
        if w is None:                                           # the bounds of an axis without a wall are ignored
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            L = hi[k] - lo[k]
        if not (np.isfinite(lo[k]) and np.isfinite(hi[k]) and np.isfinite(L) and L > 0):
            raise ValueError("axis %s: lo, hi and hi - lo must be finite and hi - lo > 0 on an axis with a wall, got lo = %r, hi = %r" % (
                "xyz"[k], lo[k], hi[k]))
    return lo, hi, walls


def _box_walls(r, v, dr, dv, photon, modes, lo, hi, dtype=np.float64):
    """What pcl_step_box_walls makes of (n, 3) float64 positions, velocities, last moves and last velocity changes and who is a photon,
    with numpy -- every operation the device's operation in the device's order, one rounding each (include/physicl_hip.h), and what is
    written rounded once to ``dtype``: the device's bit for bit, everywhere (add, subtract, multiply, divide, floor, fmin / fmax and
    compares only).  ``modes``: per axis ``"periodic"``, ``"mirror"``, ``"open"`` or None.  A dict: ``r, v, dr, dv`` the new state
    (float64 arrays; what is not written is the arguments'), the boolean masks ``moving``, ``parked``, ``folded`` (outside on an axis
    and not parked), ``multi``, ``written`` (``parked | folded``) and ``outside`` ((n, 3): outside on the axis, whatever becomes of
    it), ``side`` ((n, 3) int: 0 below, 1 above, -1 not outside), ``n`` ((n, 3): the floor of the folded axes, NaN elsewhere),
    ``crossed`` (int64 [3][2]) and ``counts`` (int64 [8]: moving, multi, crossed -- the header's order)."""
    r, v, dr, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v, dr, dv))
    cnt = len(r)
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    photon = np.asarray(photon, dtype=bool).reshape(-1)
    moving = ~_at_rest(v) & photon
    side = np.full((cnt, 3), -1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for a, mode in enumerate(modes):
            if mode is None:
                continue
            x = r[:, a]
            below = x < lo[a]
            above = x >= hi[a] if mode == "periodic" else x > hi[a]
            out = (below | above) & np.isfinite(x) & moving
            side[out, a] = np.where(below[out], 0, 1)
    outside = side >= 0
    is_open = np.array([m == "open" for m in modes], dtype=bool)
    parked = (outside & is_open).any(axis=1)
    folded = outside.any(axis=1) & ~parked
    crossed = np.zeros((3, 2), dtype=np.int64)
    first_open = np.argmax(outside & is_open, axis=1)           # the first open axis a parked photon is outside on
    for a in range(3):
        for sd in range(2):
            crossed[a, sd] = (parked & (first_open == a) & (side[:, a] == sd)).sum() + (folded & (side[:, a] == sd)).sum()
    v[parked] = 0.0
    dv[parked] = 0.0
    n_all = np.full((cnt, 3), np.nan)
    multi = np.zeros(cnt, dtype=bool)
    for a, mode in enumerate(modes):
        at = np.flatnonzero(folded & outside[:, a])
        if mode is None or not len(at):
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            L = hi[a] - lo[a]
            s = r[at, a] - lo[a]
            n = np.floor(s / L)
            f = np.fmin(np.fmax(s - n * L, 0.0), L)
            n_all[at, a] = n
            multi[at] |= (n < -1.0) | (n > 1.0)
            if mode == "periodic":
                y = lo[a] + f
                y = np.where(y < hi[a], y, lo[a])
            else:
                h = n * 0.5
                odd = np.floor(h) != h
                y = np.fmin(np.fmax(np.where(odd, hi[a] - f, lo[a] + f), lo[a]), hi[a])
                for field in (v, dv, dr):                       # an odd number of bounces turns the axis round
                    field[at[odd], a] = -field[at[odd], a]
        r[at, a] = _stored(y, dtype)
    counts = np.concatenate([[moving.sum(), multi.sum()], crossed.reshape(-1)]).astype(np.int64)
    return {"r": r, "v": v, "dr": dr, "dv": dv, "moving": moving, "parked": parked, "folded": folded, "multi": multi,
            "written": parked | folded, "outside": outside, "side": side, "n": n_all, "crossed": crossed, "counts": counts}


class BoxBoundaryStep(tally.WriterStep):
    """The sides of the scene (not in the reference): a box ``[lo, hi]`` with a wall of one kind, or none, per axis.  ``lo`` and ``hi``
    are three numbers each (code units, taken by stored value as ``center`` is); ``walls`` is one of ``"periodic"``, ``"mirror"``,
    ``"open"`` and None, or three of them for x, y, z.  On an axis with a wall ``lo``, ``hi`` and ``L = hi - lo`` (float64, rounded
    once) must be finite and ``L > 0``; on an axis with None the bounds are ignored; None on all three raises ``ValueError``.

    * ``"periodic"``: a photon that has left through one side comes back in through the other -- the horizontal boundary condition of
      a cloud field, without which domain-averaged fluxes mean nothing.  The box is ``[lo, hi)``; only ``r`` of the axis is written, so
      ``r - dr`` is the image of where the photon came from.
    * ``"mirror"``: the whole move is folded back at the walls, exact for any number of bounces: ``r`` of the axis is the image, and an
      odd number of bounces turns ``v``, ``dv`` and ``dr`` of the axis round.  ``|v|`` does not change.  On the wall is inside.
    * ``"open"``: a photon outside is parked as ``PathAbsorptionStep`` parks -- ``v = 0``, ``dv = 0``, ``r`` and ``dr`` left alone -- and
      counted once, for the first open axis it is outside on (x, y, z order).  It is at rest from then on, no later pass counts it, and a
      ``RecycleStep(at_rest=True)`` behind the step hands its slot back to the source.  Open walls come first: a photon parked through
      one is not folded on any other axis.

    Only moving photons are looked at (the sibling sweeps' test: some ``v_k != 0``; ``-0.0`` counts as 0, a NaN moves); plain
    ``Object``s, photons at rest and a position that is not finite on an axis are left alone.  A photon that crosses nothing is not
    written at all; ``E``, ids and kinds are never written.

    Put the step LAST in a pass: behind the ground or the interface, if there is one, and in front of a ``ReemissionStep`` or a
    ``RecycleStep``.  A tally placed BEHIND it in the same pass sees image positions -- a plane or shell crossing read off ``r - dr``
    there is the image's, not the move's; nothing refuses that placement.  The step changes nothing in any other step.

    After each run ``moving`` and ``multi`` hold the pass's counts, ``crossed`` an int64 ``[3][2]`` array (axis; below, above) and
    ``parked`` the sum of ``crossed`` over the open axes, global over shards and ranks (one collective); ``self.data`` gains the row
    ``[t, moving, multi, crossed]``; ``out_fn`` takes the rows at the end.  ``multi`` counts the photons folded more than once on
    some axis (``n < -1`` or ``n > 1``): it changes nothing and says that ``c*dt`` is too large for the box, as
    ``RefractiveSurfaceStep.overshot`` does for a sphere.  The rule is written out in include/physicl_hip.h (pcl_step_box_walls);
    ``_box_walls`` restates it with numpy, bit for bit.

    The sweep is deterministic: no draw, no id, no seed.  It works with every ``rng=`` setting and, reading no ``dv`` rule, under
    ``cl_on=False`` as well.  One launch per light step: the K-passes-per-launch kernels cannot fold a photon between two of their
    passes, and ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is
    made with numpy."""
    _STREAM = "box_walls"                                # (it draws nothing: its pass counter is handed to nobody)
    _NOTE = "one launch per light step: a BoxBoundaryStep folds or parks the photons that have left its box behind every pass, " \
            "which the K-passes-per-launch kernels cannot carry"
    _writes = ("r", "dr", "v", "dv")

    def __init__(self, lo, hi, walls="periodic", out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.lo, self.hi, self.walls = _check_box(lo, hi, walls)
        self._record_counts(np.zeros(8, dtype=np.int64))
        self._pass = 0                                   # runs so far (tally.WriterStep)

    def _record_counts(self, counts):
        counts = np.asarray(counts, dtype=np.int64).reshape(8)
        self.moving, self.multi = int(counts[0]), int(counts[1])
        self.crossed = counts[2:].reshape(3, 2).copy()
        self.parked = int(sum(self.crossed[a].sum() for a, w in enumerate(self.walls) if w == "open"))

    def _record_pass(self, sim, *counts):
        self._record_counts(counts)
        self.data.append(tally.object_row([tally._snap(sim.t), self.moving, self.multi, self.crossed]))

    def _sweep(self, sim, prep):
        return [np.asarray(sim._dev.box_walls(self.walls, self.lo, self.hi), dtype=np.int64)]

    def _host_sweep(self, objs, ids, seed, prep):
        new = _box_walls(tally.vec3(objs, "r"), tally.vec3(objs, "v"), tally.vec3(objs, "dr"), tally.vec3(objs, "dv"), _photons(objs),
                         self.walls, self.lo, self.hi)
        return new, new["written"], tuple(new["counts"])

    terminate = tally.TallyStep.terminate                # (a row holds an array: written as the tally steps write theirs, as a plain list)


# ---------------------------------------------------------------------------------------------- re-emission in place
def _check_reemission(spectra, edges, center, eta, angular):
    """(tables -- per layer None or (grid, cdf) float64 arrays --, edges or None, centre, eta as a float64 array [L'], angular as a
    tuple of L' names) of a ReemissionStep, L' = max(layers, 1), or ValueError for everything pcl_step_reemit_parked would refuse."""
    from ._hip import REEMIT_LAWS, REEMIT_MAX_BINS, REEMIT_MAX_LAYERS, REEMIT_MAX_TOTAL_BINS      # (the header's limits: one place)
    if edges is not None:
        edges = tally.check_edges("edges", edges, REEMIT_MAX_LAYERS, "square")               # (the device compares q with e*e)
    rows = 1 if edges is None else len(edges) - 1
    center = tally.check_center(center)
    try:
        et = np.array(eta, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("eta must be a number, or one number per layer") from None
    if et.shape not in ((), (rows,)):
        raise ValueError("eta must be one number or one per layer (%d), got shape %r" % (rows, et.shape))
    if not np.all((et >= 0.0) & (et <= 1.0)):                  # (False for NaN as well)
        raise ValueError("eta must lie in [0, 1], got %r" % (eta,))
    et = np.ascontiguousarray(np.broadcast_to(et, (rows,)))
    laws = (angular,) * rows if isinstance(angular, str) else angular
    try:
        laws = tuple(laws)
    except TypeError:
        raise ValueError("angular must be 'isotropic' or 'lambertian', or one of them per layer, got %r" % (angular,)) from None
    if len(laws) != rows or not all(isinstance(a, str) and a in REEMIT_LAWS for a in laws):
        raise ValueError("angular must be 'isotropic' or 'lambertian', or one of them per layer (%d), got %r" % (rows, angular))
    one = spectra is None or isinstance(spectra, PhotonBatch)
    if not one:                                                # (grid, cdf): two sequences of numbers, not two spectra
        try:
            one = len(spectra) == 2 and all(x is not None and not isinstance(x, PhotonBatch)
                                            and np.array(x, dtype=np.float64).ndim == 1 for x in spectra)
        except (TypeError, ValueError):
            one = False
    if one:
        tables = [_check_spectrum(spectra, REEMIT_MAX_BINS, "spectra")] * rows
    else:
        try:
            given = list(spectra)
        except TypeError:
            raise ValueError("spectra must be None, one spectrum or one per layer, got %r" % (spectra,)) from None
        if len(given) != rows:
            raise ValueError("spectra must hold one entry per layer (%d), got %d" % (rows, len(given)))
        tables = [_check_spectrum(s, REEMIT_MAX_BINS, "spectra[%d]" % b) for b, s in enumerate(given)]
    total = sum(len(t[1]) for t in tables if t is not None)
    if total > REEMIT_MAX_TOTAL_BINS:
        raise ValueError("spectra: the tables of all layers hold %d entries, at most %d are supported" % (total, REEMIT_MAX_TOTAL_BINS))
    return tables, edges, center, et, laws


_REEMIT_WORDS = (18, 19, 20)                                  # the draw, the direction, the energy (the header lists the words taken)


def _reemit_parked(r, v, E, photon, ids, eta, angular, tables, edges, center, c, seed, n_pass, dtype=np.float64):
    """What pcl_step_reemit_parked makes of (n, 3) float64 positions and velocities, the energies, who is a photon and the particles'
    ids, with numpy -- every operation the device's operation in the device's order, one rounding each (include/physicl_hip.h), and
    what is written rounded once to ``dtype``.  The rule, the draw and the table look-up are the device's bit for bit; sin / cos are
    libm's here.  ``eta``, ``angular`` and ``tables`` (None, or per layer None or ``(grid, cdf)``): one value, or one per layer.  A
    dict: ``r, v, dr, dv, E`` the new state (float64 arrays; ``r`` is the argument's, and so is every row of a particle that is not
    re-emitted -- ``dr`` and ``dv`` hold NaN there: the sweep does not write them), the boolean masks ``parked`` and ``reemitted``,
    ``layer`` (int64: of every photon at rest, -1 for none) and the tally ``by_layer`` (int64 [L'])."""
    r, v = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v))
    n = len(v)
    E = np.full(n, np.nan) if E is None else np.array(E, dtype=np.float64).reshape(-1)
    ids = np.asarray(ids).reshape(-1)
    rows = 1 if edges is None else len(edges) - 1
    eta = np.broadcast_to(np.asarray(eta, dtype=np.float64).reshape(-1), (rows,))
    lam = np.array([a == "lambertian" for a in ((angular,) * rows if isinstance(angular, str) else angular)], dtype=bool)
    tables = [None] * rows if tables is None else list(tables)
    center, c = np.asarray(center, dtype=np.float64), np.float64(c)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        at = np.flatnonzero(_at_rest(v) & np.asarray(photon, dtype=bool).reshape(-1))
        layer = np.full(n, -1, dtype=np.int64)
        layer[at] = _layer_of(r[at], edges, center)
        parked = layer >= 0
        draws = np.flatnonzero(parked)
        draws = draws[eta[layer[draws]] > 0.0]                 # a layer that holds what it absorbed draws nothing
        go = draws[_philox_block(ids[draws], seed, n_pass, _REEMIT_WORDS[0])[0] < eta[layer[draws]]]
        d = r[go] - center
        q = _dot3(d, d)
        ok = ~lam[layer[go]] | ((q > 0.0) & (q < np.inf))      # no vertical at the centre (or with a NaN): parked only
        go, d, q = go[ok], d[ok], q[ok]
        up = lam[layer[go]]
        u_a, u_b = _philox_block(ids[go], seed, n_pass, _REEMIT_WORDS[1])
        w, mu = np.tile([1.0, 0.0, 0.0], (len(go), 1)), 1.0 - 2.0 * u_a
        w[up] = d[up] / np.sqrt(q[up])[:, None]                # the local vertical
        mu[up] = np.sqrt(1.0 - u_a[up])                        # cosine-weighted about it
        v_new = c * _turn_about(w, mu, u_b)
    reemitted = np.zeros(n, dtype=bool)
    reemitted[go] = True
    dr, dv = np.full((n, 3), np.nan), np.full((n, 3), np.nan)
    v[go] = _stored(v_new.reshape(len(go), 3), dtype)
    dr[go], dv[go] = 0.0, 0.0
    for b, table in enumerate(tables):
        if table is not None:
            grid, cdf = (np.asarray(a, dtype=np.float64) for a in table)
            sel = go[layer[go] == b]
            u = _philox_block(ids[sel], seed, n_pass, _REEMIT_WORDS[2])[0]
            E[sel] = _stored(grid[np.searchsorted(cdf, u, side="left")], dtype)               # the first x with cdf[x] >= u
    return {"r": r, "v": v, "dr": dr, "dv": dv, "E": E, "parked": parked, "reemitted": reemitted, "layer": layer,
            "by_layer": np.bincount(layer[go], minlength=rows).astype(np.int64)}


class ReemissionStep(tally.WriterStep):
    """Absorbed photons re-emitted in place (not in the reference).  Every sink of a pass -- ``AbsorptionStep``,
    ``PathAbsorptionStep``, a ``SurfaceReflectStep`` with an albedo -- parks the photon at rest where it was absorbed; from there it
    either stays for ever or a ``RecycleStep`` hands its slot back to the lamp.  This step puts the energy back WHERE it was absorbed:
    a ground that absorbs sunlight and radiates in the infrared, a gas layer that absorbs a band and returns it isotropically (the
    greenhouse return flux a ``ShellCrossingMeasureStep`` counts inward at the ground), fluorescence with a lifetime.  It stands
    anywhere behind the steps of a pass that park photons, and before a ``RecycleStep`` if there is one: the lamp then takes what this
    step left at rest.

    * ``edges``: ``L + 1`` finite, non-negative, strictly increasing radii about ``center`` (at most 64 layers), ``AbsorptionStep``'s
      rule exactly: layer ``b`` holds a photon iff ``e_b**2 <= q < e_(b+1)**2``, the last layer closed, ``q = (d0*d0 + d1*d1) + d2*d2``
      in float64; no square root is taken; a NaN is in no layer.  Without ``edges`` one layer holds everything and ``r`` is not read,
      unless that layer is lambertian.  A photon parked in no layer stays parked.  Below, ``L' = max(L, 1)``.
    * ``eta``: one number in [0, 1] or ``L'`` of them: the chance per pass that a photon parked in the layer is re-emitted in this
      pass.  1 re-emits at once; below 1 the photon stays parked and draws again next pass -- a lifetime of ``dt / eta``; 0 draws nothing.
    * ``angular``: ``"isotropic"`` or ``"lambertian"``, one name or ``L'`` of them.  Lambertian is cosine-weighted about the local
      vertical ``(r - center)/|r - center|``: a ground shell radiating upward.  The ground parks photons on its sphere up to rounding,
      so give the ground a thin shell of its own, for example ``R*(1 - 1e-6) .. R*(1 + 1e-6)`` -- wide enough for an fp32 store.  A
      photon exactly at ``center`` has no vertical: it is counted as parked and left alone.
    * ``spectra``: None (a re-emitted photon keeps its ``E``), one spectrum for every layer, or a sequence of ``L'`` entries, each
      None, ``(grid, cdf)`` or a ``PhotonBatch`` with a table -- what ``RecycleStep(spectrum=)`` accepts, by the same checks: a table has
      at most 1024 entries, all tables of a step together at most 2048.  The new ``E`` does not look at the old one.  If no layer has
      a table ``E`` is neither written nor asked for, so a wavelength-dependent scatter step keeps its term cache.

    A re-emitted photon gets ``v`` at speed c along the drawn direction and ``dr = dv = 0``: later steps of the pass see a photon that
    has neither moved nor scattered.  ``r``, ids and kinds are never written; a particle that is not re-emitted is not written at
    all; plain ``Object``s are never touched.  The draws are Philox blocks keyed by ``sim.seed``, the photon's id and the step's pass counter
    ``_n_pass``, in counter words no other kernel uses (18, 19, 20): every other step draws what it draws without this one, and a
    sharded run re-emits the same photons the same way; several ``ReemissionStep``s in one pass count on through one another
    (``tally.WriterStep``), so each draws for itself.  The rule is written out in include/physicl_hip.h
    (pcl_step_reemit_parked); ``_reemit_parked`` restates it with numpy.  The step reads no ``dv`` rule, so it works under
    ``cl_on=False`` as well.

    After each run ``self.parked`` (the photons at rest that have a layer), ``self.reemitted`` and ``self.by_layer`` (int64 ``[L']``:
    the re-emitted per layer) hold the pass's tallies, global over shards and ranks; ``self.data`` gains the row ``[t, parked,
    reemitted, by_layer]``; ``out_fn`` takes the rows at the end.

    One launch per light step: the K-passes-per-launch kernels cannot re-emit a photon between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "reemit"
    _NOTE = "one launch per light step: a ReemissionStep re-emits the parked photons behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, spectra=None, edges=None, center=(0, 0, 0), eta=1.0, angular="isotropic", out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.spectra, self.edges, self.center, self.eta, self.angular = _check_reemission(spectra, edges, center, eta, angular)
        self.parked = self.reemitted = 0
        self.by_layer = np.zeros(len(self.eta), dtype=np.int64)
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_pass(self, sim, parked, reemitted, *by_layer):
        self.parked, self.reemitted = int(parked), int(reemitted)
        self.by_layer = np.array(by_layer, dtype=np.int64).reshape(-1)
        self.data.append(tally.object_row([tally._snap(sim.t), self.parked, self.reemitted, self.by_layer.copy()]))

    @property
    def _writes(self):                                   # r goes back as it came; without a table a re-emitted photon keeps its E
        return ("r", "dr", "v", "dv") + (("E",) if any(t is not None for t in self.spectra) else ())

    def _sweep(self, sim, prep):
        parked, reemitted, by_layer = sim._dev.reemit_parked(_c_h_literals()[0], self.eta, self.angular, self.spectra, self.edges,
                                                             self.center, sim.seed, self._n_pass)
        return [np.concatenate([[parked, reemitted], by_layer]).astype(np.int64)]

    def _host_sweep(self, objs, ids, seed, prep):
        E, photon = tally.photon_energies(objs, PhotonObject)
        new = _reemit_parked(tally.vec3(objs, "r"), tally.vec3(objs, "v"), E, photon, ids, self.eta, self.angular, self.spectra,
                             self.edges, self.center, _c_h_literals()[0], seed, self._n_pass)
        return new, new["reemitted"], (new["parked"].sum(), new["reemitted"].sum(), *new["by_layer"])

    terminate = tally.TallyStep.terminate                # (a row holds an array: written as the tally steps write theirs, as plain lists)


def _DEFAULT_ID_INFO(x):
    """The reference's default ``lambda x: str(type(x))`` (light.py:438), recognised by identity.  The label goes into the trace
    table's first column: this package's own classes read as the reference's (``<class 'physicl.light.PhotonObject'>``, what a
    trace file written by the reference holds -- tests/golden/g5_trace.npz), anybody else's class as it is."""
    return str(type(x)).replace("<class 'physicl_amd.", "<class 'physicl.", 1)


_PHOTON_LABEL = "<class 'physicl.light.PhotonObject'>"


class _Col:
    """The positions of tracked particle ``j`` over the first ``n`` logged passes: column j of the blocks the device returned
    ((passes, tracked, 4) arrays), made into vectors when somebody looks at them."""
    __slots__ = ("blocks", "j", "n")

    def __init__(self, blocks, j, n):
        self.blocks, self.j, self.n = blocks, j, n

    def __len__(self):
        return self.n

    def __iter__(self):
        left = self.n
        for b in self.blocks:
            if left <= 0:
                break
            k = min(left, len(b))
            yield from b[:k, self.j, :3]
            left -= k


class _Lazy(collections.abc.MutableSequence):
    """A list whose elements are made when somebody looks at them: the concatenation of ``parts`` (lists, or 2-D arrays whose
    rows are the elements).  The trace of 1000 photons over 500 passes is half a million position vectors; kept as the blocks
    the device returned, ``terminate`` costs a millisecond instead of a tenth of a second -- as long as the run itself
    (physicl/__init__.py:519-524 stops the run's clock after the steps' terminate).  Behaves like the reference's plain
    lists (``pos_dict[i]["pos"]``, the rows of ``data``) for everything a script does with them."""

    def __init__(self, parts=()):
        self._parts, self._list = list(parts), None

    def _all(self):
        if self._list is None:
            self._list = [x for part in self._parts for x in part]
            self._parts = None
        return self._list

    def __len__(self):
        return len(self._list) if self._list is not None else sum(len(part) for part in self._parts)

    def __getitem__(self, i):
        return self._all()[i]

    def __setitem__(self, i, x):
        self._all()[i] = x

    def __delitem__(self, i):
        del self._all()[i]

    def insert(self, i, x):
        self._all().insert(i, x)

    def append(self, x):
        self.extend([x])

    def extend(self, seq):
        if self._list is not None:
            self._list.extend(seq)
        elif self._parts and type(self._parts[-1]) is list and type(seq) is list:
            self._parts[-1].extend(seq)
        else:
            self._parts.append(seq)

    def __iter__(self):
        return iter(self._all())

    def __eq__(self, other):
        return list(self) == list(other)

    def __repr__(self):
        return repr(self._all())


class TracePathMeasureStep(MeasureStep):
    """Records objects' positions at every step (physicl/light.py:433-483).

    Two ways of running:

    * **tracked subset, on the device** -- when the step sits behind a light step in a fused group ([Newton][ScatterIsotropic |
      ScatterDelete][measures / this step]) and the run uses the device RNG: the positions of the tracked particles over
      the next launch's passes are worked out ahead of the launch by one thread per tracked particle
      (``pcl_store_trace_ahead``; photons do not interact and their random streams are keyed by their ids, so a particle's
      history is a function of its own state) -- nothing is downloaded per step, no Python object is built, the K-passes-
      per-launch schedule stays, and it works for a ``PhotonBatch`` of 1e8 photons and for sharded runs.  Which particles:
      ``trace_ids=[...]`` (ids = positions in the object list at upload, or photon numbers of a PhotonBatch), ``track=K``
      (the first K), default: every object of an explicit-object run (up to 65536), the first 1000 photons of a
      PhotonBatch.  The reference traces every object (O(N*T) host memory): with explicit objects that is the default here too.
    * **host plugin** otherwise (host-drawn randoms, ``cl_on=False``, a step list that is not fused): the first time an
      object is seen it is looked at as a Python object (``id_info_fn(obj)``, exactly as in the reference); after that, while
      the particles live on the device, a step costs three array downloads (ids, r, dv)."""
    _reads_only = True
    _fuse_role = "trace"
    MAX_TRACKED = 65536          # == PCL_TRACE_MAX (include/physicl_hip.h)

    def __init__(self, out_fn, trace_type=Object, id_info_fn=_DEFAULT_ID_INFO, trace_dv=False, track=None, trace_ids=None):
        super().__init__(out_fn)
        self.trace_type, self.id_info_fn, self.trace_dv = trace_type, id_info_fn, trace_dv
        self.track, self.trace_ids = track, trace_ids
        self.id_counter = 0
        self.id_dict, self.pos_dict = {}, {}
        self._tid_map, self._map_gen, self._log = None, None, []
        self._ahead_ids, self._ahead_gen, self._ahead_log, self._ahead_tids, self._ahead_objs = None, None, [], None, None

    # fused-group protocol of the counting measures (core.Simulation._build_plan): no planes, no counter row
    def _n_planes(self):
        return 0

    def _plane_rows(self):
        return []

    # ------------------------------------------------------------------ tracked subset, ahead of the launch
    def _ahead_set(self, sim):
        """The tracked ids (ascending int64) if this run can be traced on the device, else None."""
        if sim._py_semantics() or sim._dev is None or sim._rng_mode() != sim._hip.RNG_PHILOX:
            return None
        if self._ahead_ids is not None and self._ahead_gen == sim._upload_gen:
            return self._ahead_ids
        if self._ahead_ids is not None:
            self._flush_ahead(sim)                        # a new upload: file what the old population left
        n_all = sim._batch.n if sim._batch is not None else len(sim._objects._items) if isinstance(sim._uploaded, list) else None
        if n_all is None:
            return None                                   # (a materialised batch that went back up: host plugin)
        if self.trace_ids is not None:
            ids = np.unique(np.asarray(self.trace_ids, dtype=np.int64))
        else:
            k = self.track if self.track is not None else (1000 if sim._batch is not None else n_all)
            ids = np.arange(min(int(k), n_all), dtype=np.int64)
        ids = ids[(ids >= 0) & (ids < n_all)]
        if len(ids) > self.MAX_TRACKED:
            if self.track is None and self.trace_ids is None:
                return None                               # every object of a big explicit-object run: the host plugin, as before
            raise ValueError("TracePathMeasureStep tracks at most %d particles on the device, %d asked for" % (self.MAX_TRACKED, len(ids)))
        self._ahead_ids, self._ahead_gen = ids, sim._upload_gen
        self._ahead_tids = None
        # explicit objects: the objects behind the ids NOW (device id == place in the list that was just uploaded) -- by the time the
        # rows are filed the list may have lost its removed photons (a host visit) or been uploaded again
        explicit = sim._batch is None and isinstance(sim._uploaded, list)
        self._ahead_objs = [sim._objects._items[i] for i in ids.tolist()] if explicit else None
        return ids

    def _ahead_record(self, sim, ts, rows):
        """``rows`` = (len(ts), n_tracked, 4) of pcl_store_trace_ahead for the passes whose times are ``ts``."""
        if not self._ahead_log:
            self._ahead_t0 = _snap_t(ts[0])
        self._ahead_log.append(rows[:len(ts)])        # (a view of the launch's own array: nobody else writes it)

    def _assign_tids(self, sim, t0, present):
        """First sight of the tracked particles (light.py:450-455): a trace id each, in object order, unless the object
        already carries one (the host plugin saw it earlier, or an earlier upload of the same objects was traced).  A
        particle that is gone before the step first runs is never seen (``present``): no id, no row -- as in the reference."""
        explicit = self._ahead_objs is not None
        tids = np.full(len(self._ahead_ids), -1, dtype=np.int64)
        for j, i in enumerate(self._ahead_ids.tolist()):
            obj = self._ahead_objs[j] if explicit else None
            tid = obj.__dict__.get("__trace_path_id") if explicit else (self._uid_tid or {}).get(i)
            if tid is None and present[j]:
                tid = self.id_counter
                self.id_counter += 1
                if explicit:
                    obj.__dict__["__trace_path_id"] = tid
                    self.id_dict[tid] = self.id_info_fn(obj)
                else:
                    self.id_dict[tid] = _PHOTON_LABEL if self.id_info_fn is _DEFAULT_ID_INFO else self.id_info_fn(_batch_photon(sim, i))
                self.pos_dict[tid] = {"start": t0, "pos": _Lazy()}
                if self.trace_dv:
                    self.pos_dict[tid]["freq"] = 0
            if tid is not None:
                tids[j] = tid
        return tids

    def _flush_ahead(self, sim=None):
        """File the device rows under the trace ids (a photon's list ends where it was removed).  The blocks are not taken
        apart: a particle's positions are a view of its column (_Col) -- terminate() belongs to the run's clock."""
        if not self._ahead_log:
            return
        blocks, self._ahead_log = self._ahead_log, []
        comm = getattr(sim, "comm", None)
        if comm is not None and comm.world > 1:
            blocks = [_merge_shards(comm, np.concatenate(blocks, axis=0))]
        n_there = np.zeros(blocks[0].shape[1], dtype=np.int64)               # removal is for good: a prefix of the passes
        freq = np.zeros(blocks[0].shape[1], dtype=np.int64)
        first = None
        for blk in blocks:
            there = ~np.isnan(blk[:, :, 0])
            if first is None:
                first = there[0]
            n_there += there.sum(axis=0)
            if self.trace_dv:
                freq += ((blk[:, :, 3] != 0) & there).sum(axis=0)
        if self._ahead_tids is None:
            self._ahead_tids = self._assign_tids(sim, self._ahead_t0, first)
        n_there, freq = n_there.tolist(), freq.tolist()
        for j, tid in enumerate(self._ahead_tids.tolist()):
            if tid < 0 or not n_there[j]:
                continue
            entry = self.pos_dict[tid]
            entry["pos"].extend(_Col(blocks, j, n_there[j]))
            if self.trace_dv:
                entry["freq"] += freq[j]

    # ------------------------------------------------------------------ host plugin
    def _device_rows(self, sim):
        """(trace ids, positions, moved flags) of the resident particles straight from the device, or None when some
        particle has not been seen as an object yet / the state is not on the device / the run is sharded."""
        dev = getattr(sim, "_dev", None)
        if dev is None or sim._batch is not None or sim.comm is not None or sim._residency == "host" or not isinstance(sim._uploaded, list) or not sim._uploaded:
            return None
        if self._tid_map is None or self._map_gen != sim._upload_gen:
            self._tid_map = np.array([o.__dict__.get("__trace_path_id", -1) for o in sim._uploaded], dtype=np.int64)
            self._map_gen = sim._upload_gen
        with sim._dev_lock:
            n = dev.count
            idx = dev.download_ids(n) - sim._upload_lo
            if n and (idx.min() < 0 or idx.max() >= len(self._tid_map)):
                return None
            tids = self._tid_map[idx]
            if n and tids.min() < 0:
                return None
            hip = sim._hip
            r = np.stack([dev.download(f, n) for f in (hip.R0, hip.R1, hip.R2)], 1) if n else np.zeros((0, 3))
            moved = None
            if self.trace_dv:
                moved = np.zeros(n, dtype=bool)
                for f in (hip.DV0, hip.DV1, hip.DV2):
                    moved |= dev.download(f, n) != 0
        return tids, r, moved

    def _flush(self, sim):
        self._flush_ahead(sim)
        for tids, r, moved in self._log:
            for k, tid in enumerate(tids.tolist()):
                self.pos_dict[tid]["pos"].append(r[k])
            if moved is not None:
                for tid in tids[moved].tolist():
                    self.pos_dict[tid]["freq"] += 1
        self._log = []

    def run(self, sim):
        if self._ahead_ids is not None:
            # the tracked subset has been traced on the device so far: the objects the host plugin is about to walk carry
            # those trace ids on (explicit objects; a PhotonBatch's photons are looked up by their uid)
            self._flush(sim)
            self._adopt_ahead(sim)
        rows = self._device_rows(sim)
        if rows is not None:
            self._log.append(rows)
            return
        self._flush(sim)
        self._tid_map = None
        for obj in sim.objects:
            tid = obj.__dict__.get("__trace_path_id")
            if tid is None and self._uid_tid:
                tid = self._uid_tid.get(obj.__dict__.get("uid"))
                if tid is not None:
                    obj.__dict__["__trace_path_id"] = tid
            if tid is None:
                tid = obj.__dict__["__trace_path_id"] = self.id_counter
                self.id_dict[tid] = self.id_info_fn(obj)
                self.pos_dict[tid] = {"start": copy.deepcopy(sim.t), "pos": []}
                if self.trace_dv:
                    self.pos_dict[tid]["freq"] = 0
                self.id_counter += 1
            self.pos_dict[tid]["pos"].append(copy.deepcopy(obj.r))
            if self.trace_dv and np.any(np.asarray(obj.dv) != 0):
                self.pos_dict[tid]["freq"] += 1

    _uid_tid = None

    def _adopt_ahead(self, sim):
        """The run leaves the device-traced schedule (a host plugin joined, the objects were taken back, ...): from here on the
        particles are walked as Python objects, which must find the trace ids the device rows were filed under -- explicit
        objects carry them (_assign_tids), a PhotonBatch's photons are looked up by their uid."""
        ids, tids, explicit = self._ahead_ids, self._ahead_tids, self._ahead_objs is not None
        self._ahead_ids = self._ahead_gen = self._ahead_tids = self._ahead_objs = None
        if tids is not None and not explicit:
            self._uid_tid = dict(self._uid_tid or {}, **{int(i): int(t) for i, t in zip(ids, tids) if t >= 0})

    def terminate(self, sim):
        """data[0] = ["t", t0, t1, ...]; data[1+i] = [id info, (freq,) NaN-padded positions of object i]."""
        self._flush(sim)
        cols = len(sim.ts)
        table = [["t"] + copy.deepcopy(sim.ts)]
        for i in range(len(self.id_dict)):
            entry = self.pos_dict[i]
            head = [self.id_dict[i]]
            if self.trace_dv:
                head.append(entry["freq"])
            before = sim.ts.index(entry["start"])
            after = cols - len(entry["pos"])                                 # (as the reference counts it, light.py:477)
            table.append(_Lazy([head, [np.nan, np.nan, np.nan] * before, entry["pos"], [np.nan, np.nan, np.nan] * after]))
        self.data = table


def _snap_t(t):
    return t if isinstance(t, (int, float, np.generic)) else copy.deepcopy(t)


def _batch_photon(sim, i):
    """Photon ``i`` of a PhotonBatch as generate_photons would have made it (physicl/light.py:126-128), for id_info_fn."""
    # (the energy is looked up while the store still holds every photon at its own index; afterwards it is not known here;
    #  a sourced batch's r and v are the store's at that moment -- behind the launch whose rows are being filed -- under the
    #  same condition, NaN otherwise)
    known = sim.comm is None and sim._dev.is_uniform() and i < sim._dev.count
    E = sim._dev.download(sim._hip.E, 1, int(i)) if known else np.nan
    o = PhotonObject.__new__(PhotonObject)
    Object.__init__(o, E=np.double(np.asarray(E).reshape(-1)[0]), v=Measurement._from_code([float(np.asarray(c)), 0, 0], units="m**1 s**-1"),
                    uid=int(i))
    if getattr(sim._batch, "source", None) is not None:      # a sourced batch: r and v are the store's, known when E is
        get = lambda fids: [float(sim._dev.download(f, 1, int(i))[0]) if known else np.nan for f in fids]     # noqa: E731
        o.r = Measurement._from_code(get(sim._hip.FIELD_GROUPS["r"]), units="m**1")
        o.v = Measurement._from_code(get(sim._hip.FIELD_GROUPS["v"]), units="m**1 s**-1")
    return o


def _merge_shards(comm, rows):
    """Every rank traced the same ids and holds NaN rows for the particles of other shards: one int64 sum all-reduce of the
    bit patterns (zeros where a rank has nothing) + of the "I have it" flags puts the table together on every rank."""
    mine = ~np.isnan(rows[:, :, 0])
    bits = np.where(mine[:, :, None], rows, 0.0).view(np.int64)
    tot = comm.allreduce_sum(np.concatenate([bits.reshape(-1), mine.astype(np.int64).reshape(-1)]))
    got = tot[:bits.size].reshape(rows.shape).view(np.float64).copy()
    owners = tot[bits.size:].reshape(mine.shape)
    got[owners != 1] = np.nan
    return got


# GridPhaseStep and GridAbsorptionStep stand in light_grid.py, which builds on this module and hands the classes to this module's names
# at its end (``from physicl_amd.light import *`` and ``phys.light.GridPhaseStep`` find them, whichever of the two modules is imported first).
from . import light_grid  # noqa: E402,F401
