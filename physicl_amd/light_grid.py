"""The light steps that act by cell of a grid behind the scatter: ``GridPhaseStep``, the phase law by grid cell, and the numpy
restatement of its sweep.  Built on light.py -- ``LayeredPhaseStep``'s laws, draws and turn, ``PositionGridMeasureStep``'s cells --
and re-exported there: ``phys.light.GridPhaseStep``."""
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
