"""The light steps that act by cell of a grid behind the scatter: ``GridPhaseStep``, the phase law by grid cell, and
``GridAbsorptionStep``, absorption along the path and at the interaction by grid cell with the heating field -- and the tally that goes
with them, ``PlaneFluxMapStep``, the up and down fluxes through planes as maps --, each with the numpy restatement of its sweep.  Built on
light.py -- ``LayeredPhaseStep``'s laws, draws and turn, ``PositionGridMeasureStep``'s cells -- and re-exported there:
``phys.light.GridPhaseStep``, ``phys.light.GridAbsorptionStep``, ``phys.light.PlaneFluxMapStep``."""
import numpy as np

from . import light, tally
from .core import MeasureStep


def _check_grid_phase(laws, weights, axes, edges, mixture, outside, center):
    """(laws as ``(kind, g, mu, F)`` tuples, weights as a float64 array [K][M], their cumulative rows C, axes, edges, the mixture map
    as an int64 array of the grid's shape, outside as None or an int, centre) of a GridPhaseStep, or ValueError for everything
    pcl_step_phase_grid would refuse: the laws and the rows of weights by ``light._check_layered_phase``, the grid by
    ``light._check_grid``."""
    from ._hip import PHASE_GRID_LDS_BYTES, PHASE_GRID_MAX_MIXTURES, phase_grid_lds_bytes      # (the header's limits: one place)
    K = 1
    if weights is not None:
        try:
            shape = np.array(weights, dtype=np.float64).shape
        except (TypeError, ValueError):
            raise ValueError("weights must be numbers: one row per mixture, one value per law") from None
        K = shape[0] if len(shape) == 2 else 1                 # ([M] is one mixture; any other shape is refused with the rows' checks)
    if not 1 <= K <= PHASE_GRID_MAX_MIXTURES:
        raise ValueError("weights must hold 1 to %d mixtures (rows), got %d" % (PHASE_GRID_MAX_MIXTURES, K))
    laws, w, cum, _, _ = light._check_layered_phase(laws, weights, None, (0, 0, 0), rows=K)
    axes, edges, center = light._check_grid(axes, edges, center)
    shape = tuple(len(e) - 1 for e in edges)
    if mixture is None:
        if K != 1:
            raise ValueError("mixture may be omitted only with one mixture, weights holds %d rows" % K)
        mix = np.zeros(shape, dtype=np.int64)
    else:
        try:
            mix = np.asarray(mixture)
        except (TypeError, ValueError):
            raise ValueError("mixture must be an array of integers of the grid's shape %r" % (shape,)) from None
        if mix.dtype.kind not in "iu":
            raise ValueError("mixture must hold integers (a row of weights per cell, -1: left alone), got dtype %s" % mix.dtype)
        if mix.shape != shape:
            raise ValueError("mixture must have the grid's shape %r, got %r" % (shape, mix.shape))
        mix = np.ascontiguousarray(mix, dtype=np.int64)
        if not np.all((mix >= -1) & (mix < K)):
            raise ValueError("mixture must hold values from -1 (left alone) to %d (the last row of weights), got %d .. %d"
                             % (K - 1, mix.min(), mix.max()))
    if outside is not None:
        if isinstance(outside, (bool, np.bool_)) or not isinstance(outside, (int, np.integer)) or not 0 <= outside < K:
            raise ValueError("outside must be None or a row of weights, 0 to %d, got %r" % (K - 1, outside))
        outside = int(outside)
    n_edges, n_nodes = sum(len(e) for e in edges), sum(len(mu) for _, _, mu, _ in laws if mu is not None)
    need = phase_grid_lds_bytes(K, len(laws), n_edges, n_nodes)
    if need > PHASE_GRID_LDS_BYTES:
        raise ValueError("the tables of laws (%d nodes, %d bytes) and the edges of the grid (%d edges, %d bytes) do not fit the "
                         "workgroup's local memory together: %d bytes with the weights and the counters, at most %d"
                         % (n_nodes, 24 * n_nodes, n_edges, 8 * n_edges, need, PHASE_GRID_LDS_BYTES))
    return laws, w, cum, axes, edges, mix, outside, center


def _grid_phase_redirect(r, v, dv, photon, ids, laws, weights, axes, edges, mixture, outside, center, c, seed, n_pass, dtype=np.float64):
    """What pcl_step_phase_grid makes of (n, 3) float64 positions, velocities and last velocity changes, who is a photon and the
    particles' ids, with numpy -- every operation the device's operation in the device's order, one rounding each
    (include/physicl_hip.h), and what is written rounded once to ``dtype``.  Everything but sin / cos of the azimuth (libm here, the
    library's own on the device) is the device's bit for bit.  ``light._layered_phase_redirect``'s dict with ``mixture`` (per row, the
    row of weights it was re-directed with, -1 for a row that is not re-directed) and ``by_mixture`` (int64 [K]) in place of ``layer``
    and ``by_layer``."""
    laws, _, cum, axes, edges, mixture, outside, center = _check_grid_phase(laws, weights, axes, edges, mixture, outside, center)
    return _grid_phase_apply(r, v, dv, photon, ids, laws, cum, axes, edges, mixture, outside, center, c, seed, n_pass, dtype)


def _grid_phase_apply(r, v, dv, photon, ids, laws, cum, axes, edges, mixture, outside, center, c, seed, n_pass, dtype=np.float64):
    """``_grid_phase_redirect`` behind its checks: the arguments as ``_check_grid_phase`` returns them.  The body is
    ``light._layered_phase_apply``'s, handed the mixture of each scattered photon's cell as its row of ``cum``."""
    by_cell, none = mixture.reshape(-1), -1 if outside is None else outside

    def row_of(positions):
        ok, cell = light._cell_of_positions(positions, axes, edges, center)
        return np.where(ok, by_cell[np.where(ok, cell, 0)], none)

    out = light._layered_phase_apply(r, v, dv, photon, ids, laws, cum, None, center, c, seed, n_pass, dtype, row_of=row_of)
    out["mixture"], out["by_mixture"] = out.pop("layer"), out.pop("by_layer")
    return out


class GridPhaseStep(light.LayeredPhaseStep):
    """Phase functions by cell of a grid (not in the reference): ``LayeredPhaseStep`` with ``PositionGridMeasureStep``'s cells in
    place of the concentric layers -- cloud droplets' forward peak in the cloudy columns of a broken cloud field, Rayleigh in the clear
    air between and around them.  ``GridScatterStep`` decides WHERE photons scatter in such a field; this step, placed where a
    ``LayeredPhaseStep`` would stand -- directly BEHIND the scatter steps of a pass (measures may stand between), before or behind an
    ``AbsorptionStep`` --, decides HOW.

    * ``laws``: ``LayeredPhaseStep``'s argument with its checks, limits and error messages: 1 to 8 laws, each ``"isotropic"``,
      ``"rayleigh"``, ``("hg", g)`` or ``("table", mu_edges, p)``; at most 1024 bins per table and 2048 over all tables.
    * ``weights``: shape ``[K][M]``, ``1 <= K <= 64``; each row is a MIXTURE: row ``m`` is the probability with which an interaction
      in a cell of mixture ``m`` uses each law (finite and >= 0 with a positive sum, as ``LayeredPhaseStep``'s rows).  ``[M]`` is
      accepted as ``K = 1``, None with one law.
    * ``axes``, ``edges``, ``center``: ``PositionGridMeasureStep``'s arguments by its rules, limits and error messages (at most 1024
      bins per axis and ``2**20`` cells).  A photon's cell is the cell that step would count it in.
    * ``mixture``: an integer array of the grid's shape: ``m`` in ``[0, K)`` names the cell's row of ``weights``; ``-1``: a scattered
      photon in the cell keeps the direction the scatter step gave it (counted as scattered, not as re-directed).  None is allowed
      with ``K == 1`` only: every cell uses row 0.
    * ``outside``: None or a row in ``[0, K)``, for a scattered photon in no cell (outside some axis's range, or with a NaN position):
      with a row it is re-directed with that row -- Rayleigh everywhere round the field without a grid that spans the world --, with
      None it is left alone, as outside ``LayeredPhaseStep``'s layers.

    Everything else is ``LayeredPhaseStep``'s: who was scattered (``dv != 0`` and ``0 < o.o < inf`` for ``o = v - dv``), the turn about
    ``o/|o|``, what is written (``v`` and ``dv`` only), the ``cl_on=False`` refusal, one launch per light step, host-resident objects.
    The angle is drawn from the phase family's Philox blocks (counter words 10 and 11), the law from word 13, only where the row is
    not one-hot; no new counter word is taken.  A PASS HOLDS ONE PHASE STEP: the first run raises ``ValueError`` beside a
    ``PhaseFunctionStep``, a ``LayeredPhaseStep`` or a second ``GridPhaseStep``.  Sharing the words gives two equivalences, bit for bit:
    with ``axes=("r",)``, ``edges=[e]``, ``mixture=arange(L)`` and ``outside=None`` the store and the tallies are those of
    ``LayeredPhaseStep(laws, weights, e, center)``; one cell, one law and ``outside=0`` leave the store as ``PhaseFunctionStep`` with
    that law does.

    After each run ``self.scattered`` and ``self.redirected`` hold the pass's counts and ``self.by_mixture`` (int64 ``[K]``) and
    ``self.by_law`` (int64 ``[M]``) the re-directed photons by mixture and by law, all global over shards and ranks; ``self.data``
    gains the row ``[t, scattered, redirected, by_mixture, by_law]`` and ``out_fn`` takes the rows at the end.  There is no tally by
    cell: ``GridScatterStep.scattered_by_cell`` says where the scatterings happen.  The rule is written out in
    include/physicl_hip.h (pcl_step_phase_grid); ``_grid_phase_redirect`` restates it with numpy.

    Cost: the weights, the laws' tables and the grid's edges sit in the workgroup's local memory, 64 KiB at the most -- the largest
    tables and the largest edge arrays together do not fit, and the constructor says so; the mixture map goes up every pass as one byte
    per cell and stays in device memory, where a scattered photon reads its byte."""
    _NOTE = "one launch per light step: a GridPhaseStep re-directs the scattered photons behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, laws, weights, axes, edges, mixture=None, outside=None, center=(0, 0, 0), out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self._laws, self.weights, self.cum, self.axes, self.edges, self.mixture, self.outside, self.center = \
            _check_grid_phase(laws, weights, axes, edges, mixture, outside, center)
        self.laws = [k if k in ("isotropic", "rayleigh") else ("hg", g) if k == "hg" else ("table", mu, F) for k, g, mu, F in self._laws]
        self.scattered = self.redirected = 0
        self.by_mixture = np.zeros(len(self.cum), dtype=np.int64)
        self.by_law = np.zeros(len(self._laws), dtype=np.int64)
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_pass(self, sim, scattered, redirected, by_mixture, by_law):
        self.scattered, self.redirected = int(scattered), int(redirected)
        self.by_mixture, self.by_law = np.array(by_mixture, dtype=np.int64), np.array(by_law, dtype=np.int64)
        self.data.append(tally.object_row([tally._snap(sim.t), self.scattered, self.redirected, self.by_mixture.copy(), self.by_law.copy()]))

    def _sweep(self, sim, prep):
        scattered, redirected, by_mixture, by_law = sim._dev.phase_grid(self._laws, self.cum, self.axes, self.edges, self.center,
                                                                        self.mixture, self.outside, light._c_h_literals()[0], sim.seed,
                                                                        self._n_pass)
        return [np.array([scattered, redirected], dtype=np.int64), np.asarray(by_mixture), np.asarray(by_law)]

    def _host_sweep(self, objs, ids, seed, prep):
        new = _grid_phase_apply(tally.vec3(objs, "r"), tally.vec3(objs, "v"), tally.vec3(objs, "dv"), light._photons(objs), ids,
                                self._laws, self.cum, self.axes, self.edges, self.mixture, self.outside, self.center,
                                light._c_h_literals()[0], seed, self._n_pass)
        return new, new["redirected"], (new["scattered"].sum(), new["redirected"].sum(), new["by_mixture"], new["by_law"])


light.GridPhaseStep = GridPhaseStep                      # phys.light.GridPhaseStep, and ``from physicl_amd.light import *``


# ---------------------------------------------------------------------------------------------- absorption on a grid of cells
_GRID_ABSORB_WORDS = (27, 28)                                 # along the path, at the interaction (the header lists the words taken)


def _check_grid_absorb(k, omega0, axes, edges, center, E_edges):
    """(k and omega0, each None or a float64 array of the grid's shape (+ (B,) with E_edges), axes, edges, centre, energy edges or
    None) of a GridAbsorptionStep, or ValueError for everything pcl_step_absorb_grid would refuse.  A single number is broadcast."""
    from ._hip import ABSORB_GRID_MAX_BANDS, ABSORB_GRID_MAX_CELLS      # (the header's limits: one place)
    axes, edges, center = light._check_grid(axes, edges, center)
    if E_edges is not None:
        E_edges = tally.check_edges("E_edges", E_edges, ABSORB_GRID_MAX_BANDS)
    if k is None and omega0 is None:
        raise ValueError("k and omega0 are both None: give an absorption coefficient, a single-scattering albedo, or both")
    want = tuple(len(e) - 1 for e in edges) + (() if E_edges is None else (len(E_edges) - 1,))
    cells = int(np.prod(want))
    out = []
    for name, x in (("k", k), ("omega0", omega0)):
        if x is None:
            out.append(None)
            continue
        try:
            xa = np.array(x, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("%s must be a number, or numbers per cell of the grid (and energy band)" % name) from None
        if xa.shape not in ((), want):
            raise ValueError("%s must be one number or have the shape %r -- %s -- got %r" % (
                name, want, "the grid's cells" + ("" if E_edges is None else " by bands of E_edges"), xa.shape))
        if name == "k" and not np.all(np.isfinite(xa) & (xa >= 0.0)):             # (False for NaN as well)
            raise ValueError("k must be finite and not negative, got %r" % (x,))
        if name == "omega0" and not np.all((xa >= 0.0) & (xa <= 1.0)):
            raise ValueError("omega0 must lie in [0, 1], got %r" % (x,))
        if cells > ABSORB_GRID_MAX_CELLS:
            raise ValueError("%s: %s are %d cells, at most %d are supported" % (name, " x ".join(str(n) for n in want), cells,
                                                                                ABSORB_GRID_MAX_CELLS))
        out.append(np.ascontiguousarray(np.broadcast_to(xa, want)))
    return out[0], out[1], axes, edges, center, E_edges


def _grid_absorb(r, v, dv, E, photon, ids, p, omega0, axes, edges, center, E_edges, seed, n_pass, dtype=np.float64):
    """What pcl_step_absorb_grid makes of (n, 3) float64 positions, velocities and last velocity changes, the energies, who is a
    photon and the particles' ids, with numpy -- the rule of include/physicl_hip.h: no transcendental function, no division and no
    square root, so everything is the device's bit for bit.  ``p`` and ``omega0``: None, or one value per cell of the grid (row-major
    in the order of ``axes``) and band, not both None.  What is written is zero, in any ``dtype``.  A dict: ``v, dv`` the new state
    (float64 arrays; rows that are not absorbed are the arguments'), the boolean masks ``exposed``, ``interacted``, ``absorbed_path``,
    ``absorbed_hit`` and ``absorbed`` (either), ``cell`` (int64: cell of the grid times B' plus the band, of every exposed photon, -1
    for none) and the tally ``absorbed_by_cell`` (int64, the grid's shape, with a last dimension of B bands if ``E_edges`` is given)."""
    r, v, dv = (np.array(a, dtype=np.float64).reshape(-1, 3) for a in (r, v, dv))
    n = len(v)
    photon = np.asarray(photon, dtype=bool).reshape(-1)
    ids = np.asarray(ids).reshape(-1)
    edges = [np.asarray(e, dtype=np.float64) for e in edges]
    shape = tuple(len(e) - 1 for e in edges) + (() if E_edges is None else (len(E_edges) - 1,))
    p, omega0 = (None if t is None else np.asarray(t, dtype=np.float64).reshape(-1) for t in (p, omega0))
    cell = np.full(n, -1, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):        # the cell and the band: light._scatter_grid's lines
        at = np.flatnonzero(~light._at_rest(v) & photon)
        ok, g = light._cell_of_positions(r[at], axes, edges, np.asarray(center, dtype=np.float64))
        at, g = at[ok], g[ok]
        if E_edges is not None:                                # NaN and under/overflow: in no band
            Ee = np.asarray(E_edges, dtype=np.float64)
            band = light._bin_of(np.asarray(E, dtype=np.float64).reshape(-1)[at], Ee)
            at, g = at[band >= 0], g[band >= 0] * (len(Ee) - 1) + band[band >= 0]
    cell[at] = g
    exposed = cell >= 0
    gone_path, gone_hit = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    interacted = exposed & light._scattered(dv, photon) if omega0 is not None else np.zeros(n, dtype=bool)
    if p is not None:
        draws = at[p[g] > 0.0]                                 # a transparent cell draws nothing
        u = light._philox_block(ids[draws], seed, n_pass, _GRID_ABSORB_WORDS[0])[0]
        gone_path[draws[u < p[cell[draws]]]] = True
    if omega0 is not None:
        draws = np.flatnonzero(interacted & ~gone_path)
        draws = draws[omega0[cell[draws]] < 1.0]               # a conservative cell draws nothing
        u = light._philox_block(ids[draws], seed, n_pass, _GRID_ABSORB_WORDS[1])[0]
        gone_hit[draws[~(u < omega0[cell[draws]])]] = True     # AbsorptionStep's sense of the draw
    absorbed = gone_path | gone_hit
    v[absorbed], dv[absorbed] = np.zeros(3, dtype=dtype), np.zeros(3, dtype=dtype)        # parked
    cells = np.bincount(cell[absorbed], minlength=int(np.prod(shape))).astype(np.int64).reshape(shape)
    return {"v": v, "dv": dv, "exposed": exposed, "interacted": interacted, "absorbed_path": gone_path, "absorbed_hit": gone_hit,
            "absorbed": absorbed, "cell": cell, "absorbed_by_cell": cells}


class GridAbsorptionStep(tally.WriterStep):
    """Absorption and heating rates by cell of a grid (not in the reference): ``PathAbsorptionStep`` (Beer-Lambert along the move) and
    ``AbsorptionStep`` (the single-scattering albedo at an interaction) with ``PositionGridMeasureStep``'s cells in place of the
    concentric layers, both in ONE sweep -- a smoke plume or a water-vapour column of finite width, droplets that absorb only where the
    clouds of a broken cloud field are -- and the product a 3-D radiative-transfer run exists for: the absorbed photons by cell and
    colour, the heating field.  It stands where those two steps stand: BEHIND the scatter and phase steps of a pass
    (``GridScatterStep``, ``GridPhaseStep``), in front of the ground, the walls and a ``RecycleStep``.

    * ``axes``, ``edges``, ``center``: ``PositionGridMeasureStep``'s arguments by its rules, limits and error messages (at most 1024
      bins per axis).  A photon's cell is the cell that step would count it in; cells are row-major in the order of ``axes``.
    * ``E_edges``: ``GridScatterStep``'s argument by its rule: ``B + 1`` energy edges, ``numpy.histogram``'s bins, at most 1024 bands.
      Without it E is neither read nor asked for.
    * ``k``: the absorption coefficient per unit length (code units), finite and not negative: one number, or an array of the grid's
      shape (``+ (B,)`` with ``E_edges``).  Per pass the host makes ``p = -numpy.expm1(-k * (c * dt))`` (``light._path_probability``)
      and the device only ever sees ``p``.
    * ``omega0``: the single-scattering albedo, every value in ``[0, 1]``, with the same shapes as ``k``.
    * At least one of ``k`` and ``omega0`` must be given; cells times bands may be at most ``2**20``.

    Every moving photon with a cell (and a band) is EXPOSED -- a photon at rest (``-0.0`` counts as 0, a NaN moves), a plain ``Object``
    and a photon in no cell or no band are skipped -- and, with ``omega0``, INTERACTED iff its ``dv`` is not zero (the scatter steps'
    mark).  With ``k`` and ``p > 0`` in its cell it is absorbed along the path iff ``u < p``; otherwise, if it interacted and ``omega0
    < 1`` there, it is absorbed at the interaction iff ``not (u < omega0)`` (``AbsorptionStep``'s sense of the draw).  The two ``u`` come
    from Philox blocks keyed by ``sim.seed``, the photon's id and the step's pass counter ``_n_pass``, in counter words no other kernel
    uses (27 and 28); several ``GridAbsorptionStep``s in one pass count on through one another (``tally.WriterStep``), so their draws
    are independent.  An absorbed photon is parked as the older steps park it, ``v = 0`` and ``dv = 0``; a photon that is not absorbed
    is not written at all; ``r``, ``dr``, ``E``, ids and kinds are never written.  With ``omega0`` the step reads the ``dv`` rule and
    raises ``ValueError`` under ``cl_on=False``, as ``AbsorptionStep`` does; with ``k`` alone it works there too.

    After each run ``self.exposed``, ``self.interacted`` (0 without ``omega0``), ``self.absorbed_path``, ``self.absorbed_hit`` and
    ``self.absorbed`` (their sum) hold the pass's counts and ``self.absorbed_by_cell`` an int64 array of the tables' shape, both kinds
    together: the heating field.  All are global over shards and ranks; ``self.data`` gains the row ``[t, exposed, interacted,
    absorbed_path, absorbed_hit, absorbed_by_cell]``; ``out_fn`` takes the rows at the end.  The rule is written out in
    include/physicl_hip.h (pcl_step_absorb_grid); ``_grid_absorb`` restates every bit of it with numpy.

    Cost: up to 4096 cells, and while the edges, the tables given (8 B a cell each) and the tallies (4 B a cell) stay within 64 KiB,
    tables and tallies live in LDS -- 16 x 16 x 16 cells with one table, not with two; above that the kernel reads the tables from
    device memory and adds what it absorbed there.  Either way the tables go up and the tallies come back every pass.

    One launch per light step: the K-passes-per-launch kernels cannot absorb a photon between two of their passes, and
    ``sim.launch_note`` says so.  On host-resident objects (``step.run(sim)`` outside a device loop) the same state is made with
    numpy, the ids being the places in the object list."""
    _STREAM = "absorb_grid"                              # (words 27 and 28: nobody else's)
    _NOTE = "one launch per light step: a GridAbsorptionStep absorbs photons by grid cell and band behind every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, axes, edges, k=None, omega0=None, center=(0, 0, 0), E_edges=None, out_fn=None):
        MeasureStep.__init__(self, out_fn)
        self.k, self.omega0, self.axes, self.edges, self.center, self.E_edges = _check_grid_absorb(k, omega0, axes, edges, center, E_edges)
        self.exposed = self.interacted = self.absorbed_path = self.absorbed_hit = self.absorbed = 0
        self.absorbed_by_cell = np.zeros((self.k if self.k is not None else self.omega0).shape, dtype=np.int64)
        self._pass = 0                                   # runs so far; the sweep is handed _n_pass (tally.WriterStep)

    def _record_pass(self, sim, exposed, interacted, absorbed_path, absorbed_hit, cells):
        self.exposed, self.interacted = int(exposed), int(interacted)
        self.absorbed_path, self.absorbed_hit = int(absorbed_path), int(absorbed_hit)
        self.absorbed = self.absorbed_path + self.absorbed_hit
        self.absorbed_by_cell = np.array(cells, dtype=np.int64).reshape(self.absorbed_by_cell.shape)
        self.data.append(tally.object_row([tally._snap(sim.t), self.exposed, self.interacted, self.absorbed_path, self.absorbed_hit,
                                           self.absorbed_by_cell.copy()]))

    def _refuse(self, sim):
        if self.omega0 is not None:
            light._dv_rule_refusal(sim, "GridAbsorptionStep with omega0", "who interacted in this pass")

    def _prepare(self, sim, on_host):                    # p of this pass's dt; a dt that is refused raises here
        if self.k is None:
            return None
        return light._path_probability(self.k, light._c_h_literals()[0], np.asarray(sim.dt) if on_host else sim._dt_code())

    def _sweep(self, sim, p):
        counts, cells = sim._dev.absorb_grid(p, self.omega0, self.axes, self.edges, self.center, self.E_edges, sim.seed, self._n_pass)
        return [np.asarray(counts, dtype=np.int64), np.asarray(cells, dtype=np.int64)]

    def _host_sweep(self, objs, ids, seed, p):
        E, photon = tally.photon_energies(objs, light.PhotonObject)
        new = _grid_absorb(tally.vec3(objs, "r"), tally.vec3(objs, "v"), tally.vec3(objs, "dv"), E, photon, ids, p, self.omega0, self.axes,
                           self.edges, self.center, self.E_edges, seed, self._n_pass)
        return new, new["absorbed"], (new["exposed"].sum(), new["interacted"].sum(), new["absorbed_path"].sum(),
                                      new["absorbed_hit"].sum(), new["absorbed_by_cell"])

    terminate = tally.TallyStep.terminate                # (a row holds arrays: written as the tally steps write theirs, as plain lists)


light.GridAbsorptionStep = GridAbsorptionStep            # phys.light.GridAbsorptionStep, and ``from physicl_amd.light import *``


# ---------------------------------------------------------------------------------------------- flux maps of planes
_PLANE_AXES = {"x": (0, 1, 2), "y": (1, 0, 2), "z": (2, 0, 1)}  # the normal, then (u, v): the remaining two in x, y, z order


def _check_plane_flux(axis, levels, edges, E_bins=None):
    """(axis, levels, [u edges, v edges], band edges or None) of a PlaneFluxMapStep as float64 arrays, or ValueError for everything
    pcl_step_plane_flux would refuse."""
    from ._hip import PLANE_FLUX_MAX_BANDS, PLANE_FLUX_MAX_BINS, PLANE_FLUX_MAX_CELLS, PLANE_FLUX_MAX_LEVELS      # (the header's limits: one place)
    if not isinstance(axis, str) or axis not in _PLANE_AXES:
        raise ValueError('axis must be one of "x", "y", "z" (the normal of the planes), got %r' % (axis,))
    try:
        levels = np.array(levels, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("levels must be a 1-D sequence of numbers (coordinates along %s)" % axis) from None
    if levels.ndim != 1 or not 1 <= len(levels) <= PLANE_FLUX_MAX_LEVELS:
        raise ValueError("levels must be a 1-D sequence of 1 to %d coordinates, got shape %r" % (PLANE_FLUX_MAX_LEVELS, levels.shape))
    if not np.all(np.isfinite(levels)) or not np.all(np.diff(levels) > 0):
        raise ValueError("levels must be finite and strictly increasing, got %r" % (levels,))
    try:
        n_seq = len(edges)
    except TypeError:
        n_seq = -1
    if n_seq != 2:
        raise ValueError("edges must be two sequences of bin edges, for u and for v (the axes other than %s, in x, y, z order)" % axis)
    names = ["xyz"[k] for k in _PLANE_AXES[axis][1:]]
    edges = [tally.check_edges("edges[%d] (%s)" % (k, names[k]), edges[k], PLANE_FLUX_MAX_BINS) for k in range(2)]
    E_bins = None if E_bins is None else tally.check_edges("E_bins", E_bins, PLANE_FLUX_MAX_BANDS)
    S, B, n_u, n_v = len(levels), 0 if E_bins is None else len(E_bins) - 1, len(edges[0]) - 1, len(edges[1]) - 1
    cells = 2 * S * max(B, 1) * n_u * n_v
    if cells > PLANE_FLUX_MAX_CELLS:
        raise ValueError("2 directions x %d levels x %d bands x %d x %d bins are %d map cells, at most %d are supported"
                         % (S, max(B, 1), n_u, n_v, cells, PLANE_FLUX_MAX_CELLS))
    return axis, np.ascontiguousarray(levels), edges, E_bins


def _bin_scaled(e, H, D):
    """pcl_sweep::bin_of(e, n, H, D) for arrays: the bin b with ``e_b * D <= H < e_(b+1) * D``, the last one closed -- the device's
    binary search, probe by probe (the caller has checked that H is inside)."""
    lo, hi = np.zeros(len(H), dtype=np.int64), np.full(len(H), len(e) - 1, dtype=np.int64)
    while True:
        open_ = hi - lo > 1
        if not open_.any():
            return lo
        mid = (lo + hi) >> 1
        with np.errstate(invalid="ignore", over="ignore"):
            below = e[mid] * D <= H
        lo, hi = np.where(open_ & below, mid, lo), np.where(open_ & ~below, mid, hi)


def _plane_flux_maps(r, dr, E, photon, axis, levels, edges, E_edges=None):
    """What pcl_step_plane_flux answers, from (n, 3) float64 positions and last moves, the energies and who is a photon, with numpy --
    every operation the device's operation, one rounding each (include/physicl_hip.h): (counts int64[2, S], maps int64[2, S, max(bands,
    1), n_u, n_v]), [0] up, [1] down."""
    r, dr = np.asarray(r, dtype=np.float64).reshape(-1, 3), np.asarray(dr, dtype=np.float64).reshape(-1, 3)
    a, tu, tv = _PLANE_AXES[axis]
    levels = np.asarray(levels, dtype=np.float64).reshape(-1)
    ue, ve = (np.asarray(e, dtype=np.float64).reshape(-1) for e in edges)
    S, n_u, n_v, nE = len(levels), len(ue) - 1, len(ve) - 1, 0 if E_edges is None else len(E_edges) - 1
    nB = max(nE, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        now, m = r[:, a], dr[:, a]
        prev = now - m
        cross = np.stack([(prev < levels[:, None]) & (now >= levels[:, None]),          # up: on the plane is above
                          (prev >= levels[:, None]) & (now < levels[:, None])])         # down; NaN: neither
    counts = cross.sum(axis=2).astype(np.int64)
    hit = np.flatnonzero(cross.any(axis=(0, 1)))                                        # the maps look at these only
    n_map = 2 * S * nB * n_u * n_v
    maps = np.zeros(n_map, dtype=np.int64)
    band = np.zeros(len(hit), dtype=np.int64)
    if nE:                                                        # numpy.histogram's bins; what is no photon or outside the bands: in no cell
        e, v = np.asarray(E_edges, dtype=np.float64), np.asarray(E, dtype=np.float64).reshape(-1)[hit]
        with np.errstate(invalid="ignore"):
            ok = (v >= e[0]) & (v <= e[-1]) & np.asarray(photon, dtype=bool).reshape(-1)[hit]
        hit, band = hit[ok], np.clip(np.searchsorted(e, v, side="right") - 1, 0, nE - 1)[ok]
    with np.errstate(invalid="ignore", over="ignore"):
        D = np.abs(m[hit])
        ok = D < np.inf
        hit, band, D = hit[ok], band[ok], D[ok]
        du, dv = dr[hit, tu], dr[hit, tv]
        pu, pv = r[hit, tu] - du, r[hit, tv] - dv                                       # where the move began
        for s in range(S):
            for d in range(2):
                w = np.flatnonzero(cross[d, s, hit])
                G = np.abs(levels[s] - prev[hit[w]])
                Hu, Hv = pu[w] * D[w] + du[w] * G, pv[w] * D[w] + dv[w] * G             # the crossing point times D
                ok = (np.abs(Hu) < np.inf) & (np.abs(Hv) < np.inf) & (Hu >= ue[0] * D[w]) & (Hu <= ue[-1] * D[w]) \
                    & (Hv >= ve[0] * D[w]) & (Hv <= ve[-1] * D[w])
                w, Hu, Hv = w[ok], Hu[ok], Hv[ok]
                iu, iv = _bin_scaled(ue, Hu, D[w]), _bin_scaled(ve, Hv, D[w])
                maps += np.bincount((((d * S + s) * nB + band[w]) * n_u + iu) * n_v + iv, minlength=n_map)
    return counts, maps.reshape(2, S, nB, n_u, n_v)


class PlaneFluxMapStep(tally.TallyStep):
    """The irradiance field (not in the reference): what passed up and down through horizontal levels in the last move, resolved by
    column -- the shadow a cloud field throws on the ground beside it, the reflected flux above a broken deck.  ``axis`` (``"x"``,
    ``"y"`` or ``"z"``) is the normal of the planes, ``levels`` 1 to 16 finite, strictly increasing coordinates along it (code units),
    and ``edges`` the bin edges of the two transverse axes ``(u, v)`` -- the remaining two in x, y, z order: ``"x"`` gives (y, z), ``"y"``
    gives (x, z), ``"z"`` gives (x, y) --, at most 1024 bins each.  With ``E_bins`` (band edges in the unit E is stored in, at most 1024
    bands) only photons whose energy lies inside the bands reach the maps, one plane per band as ``numpy.histogram`` bins them; a plain
    ``Object`` or another energy is counted and lands in no cell.  ``2 * S * max(B, 1) * n_u * n_v`` may be at most ``2**20``.

    Every run records the row ``[t, N, up, down]`` (no ``N`` with ``measure_n=False``), ``up[s]`` / ``down[s]`` the particles whose last
    move took them up / down through ``levels[s]``, int64 arrays of ``len(levels)``; with ``frames=True`` the row goes on with the pass's
    ``up_map`` and ``down_map``, each int64 ``[S][max(B, 1)][n_u][n_v]``.  ``step.up`` and ``step.down`` are the last pass's counts;
    ``step.up_map`` and ``step.down_map`` are exposures, the sum over all passes so far, as ``DetectorMeasureStep.image`` is.

    A crossing is a change of side between the end points of the move, a particle exactly on the plane being above: up iff ``prev < X
    <= now``, down iff ``now < X <= prev``, with ``prev = r_a - dr_a`` in float64; a NaN crosses nothing.  Every change of side is
    counted exactly once, so ``cumsum(up - down)`` per level is the change of the population at or above it.  The column is where the
    straight move met the plane, compared without a division as ``e_b * D <= H < e_(b+1) * D`` with ``D = |dr_a|``, ``G = |X - prev|``
    and ``H_t = (r_t - dr_t) * D + dr_t * G``, the last bin closed; a photon that crosses several levels in one move is tallied at each
    of them.  A crossing whose ``D`` or ``H`` is not finite, or whose point lies outside the edges, is counted and lands in no cell.  No
    division and no square root is taken anywhere, so numpy restates every cell exactly (``light_grid._plane_flux_maps``); the rule is
    written out in include/physicl_hip.h (pcl_step_plane_flux).

    The step reads ``r`` and ``dr`` of the last move, so it stands IN FRONT of the steps that rewrite them -- the ground and the
    refracting interface, which fly the rest of the move along the new direction, and the walls --, where a
    ``ShellCrossingMeasureStep`` of the ground's radius stands.

    The tally is made on the device in one read-only sweep of the resident store and adds, so sharded runs all-reduce ``[N, counts,
    maps]`` in one collective per pass.  Cost: up to 4096 cells the maps are tallied in the workgroups' local memory and the sweep costs
    what a one-shell ``ShellCrossingMeasureStep`` costs; above that the crossing photons add to device memory with 64-bit atomics, which
    serialise where many photons cross into few cells in one pass (CHANGELOG.md has the times).  The maps come back from the device every pass (8 B a cell), and on the library's own
    communicator, which carries 2048 values a call, a ``2**20``-cell map is 513 calls per pass -- keep the map small where ranks are
    many, or hand the simulation a communicator that takes the payload whole.  A flux needs every pass, which the K-passes-per-launch
    kernels cannot carry: a loop with this step runs one launch per light step, as with ``ShellCrossingMeasureStep``, and
    ``sim.launch_note`` says so.  E is asked for only with bands.  On host-resident objects (hence under ``cl_on=False``) the same row
    is made with numpy; the step draws nothing and works with every ``rng=`` setting."""
    _fuse_role = None
    _NOTE = "one launch per light step: a PlaneFluxMapStep tallies the last move of every pass, which the " \
            "K-passes-per-launch kernels cannot carry"

    def __init__(self, out_fn, axis, levels, edges, E_bins=None, frames=False, measure_n=True):
        MeasureStep.__init__(self, out_fn)
        self.axis, self.levels, self.edges, self.E_bins = _check_plane_flux(axis, levels, edges, E_bins)
        self.frames, self.measure_n = bool(frames), measure_n
        shape = (len(self.levels), 1 if self.E_bins is None else len(self.E_bins) - 1, len(self.edges[0]) - 1, len(self.edges[1]) - 1)
        self.up_map, self.down_map = np.zeros(shape, dtype=np.int64), np.zeros(shape, dtype=np.int64)
        self.up, self.down = np.zeros(shape[0], dtype=np.int64), np.zeros(shape[0], dtype=np.int64)

    def _device_run(self, sim):
        if getattr(sim, "launch_note", self._NOTE) is None and sim._k_wanted() > 1:      # (a device run only: the host path says nothing)
            sim.launch_note = self._NOTE
        tally.TallyStep._device_run(self, sim)

    def _sweep(self, dev):
        return list(dev.plane_flux(self.axis, self.levels, self.edges, self.E_bins))

    def _host_parts(self, objs):
        return list(_plane_flux_maps(tally.vec3(objs, "r"), tally.vec3(objs, "dr"), *tally.photon_energies(objs, light.PhotonObject),
                                     self.axis, self.levels, self.edges, self.E_bins))

    def _cells(self, parts):                           # (counts, maps), global: the exposures go on
        counts, maps = (np.asarray(x, dtype=np.int64) for x in parts)
        maps = maps.reshape((2,) + self.up_map.shape)
        self.up, self.down = counts.reshape(2, -1)[0].copy(), counts.reshape(2, -1)[1].copy()
        self.up_map, self.down_map = self.up_map + maps[0], self.down_map + maps[1]
        return [self.up.copy(), self.down.copy()] + ([maps[0].copy(), maps[1].copy()] if self.frames else [])


light.PlaneFluxMapStep = PlaneFluxMapStep                # phys.light.PlaneFluxMapStep, and ``from physicl_amd.light import *``
