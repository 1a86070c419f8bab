"""The host side of a tally measure step, once -- the counterpart of csrc/pcl_sweep.h: the bin-edge and centre checks, the
state of host-resident Python objects as arrays, the one collective of a pass, and ``TallyStep``, the base class that turns
"one sweep of the store -> one collective -> one object row" into three hooks -- and ``WriterStep``, the same for the steps
whose sweep writes the store.  The steps themselves, and the numpy
restatements of their sweeps that the host-plugin path answers with, are in light.py.  NumPy only."""
import numpy as np

from .core import DeviceStep, MeasureStep, _snap
from .units import Measurement

ALLREDUCE_CHUNK = 2048       # values one pcl_comm_allreduce_sum_i64 call takes (physicl_amd.comm.NativeCounterComm)


# ---------------------------------------------------------------------------------------------- checks
def check_edges(name, edges, max_bins, transform=None):
    """The bin edges ``name`` as a contiguous float64 array, or ValueError -- the rule of pcl_sweep::check_edges: a 1-D
    sequence of 2 to ``max_bins + 1`` finite, strictly increasing numbers.  ``transform`` is what the device compares with:
    None (the edges), "square" (e*e: a radius, which must not be negative) or "signed_square" (e*|e|: a cosine); the
    transformed edges must be finite and strictly increasing as well (1e200 squares to inf, +-1e-200 to +-0: a tie)."""
    try:
        e = np.array(edges, dtype=np.float64)                 # a Measurement is taken by its stored value
    except (TypeError, ValueError):
        raise ValueError("%s must be a 1-D sequence of numbers (bin edges)" % name) from None
    if e.ndim != 1 or len(e) < 2:
        raise ValueError("%s must be a 1-D sequence of at least two bin edges, got shape %r" % (name, e.shape))
    if len(e) - 1 > max_bins:
        raise ValueError("%s describes %d bins, at most %d are supported" % (name, len(e) - 1, max_bins))
    if transform == "square" and not np.all(e >= 0):          # (False for NaN as well)
        raise ValueError("%s: radius edges must not be negative" % name)
    with np.errstate(over="ignore"):
        w = e if transform is None else e * (e if transform == "square" else np.abs(e))
    for x, what in ((e, ""), (w, " (also as the device compares them: %s)" % transform)):
        if not np.all(np.isfinite(x)) or not np.all(np.diff(x) > 0):
            raise ValueError("%s must be finite and strictly increasing%s" % (name, what))
    return np.ascontiguousarray(e)


def check_center(center):
    """``center`` as three finite float64, or ValueError."""
    try:
        center = np.array(center, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("center must be three numbers") from None
    if center.shape != (3,) or not np.all(np.isfinite(center)):
        raise ValueError("center must be three finite numbers, got %r" % (center,))
    return np.ascontiguousarray(center)


# ---------------------------------------------------------------------------------------------- host-resident objects
def host_resident(sim):
    """Whether a step is called as a host plugin on host-resident Python objects: they hold the state."""
    return getattr(sim, "_residency", None) == "host" and getattr(sim, "_batch", None) is None \
        and (sim.comm is None or sim.comm.world == 1)


def vec3(objs, attr):
    """``obj.<attr>`` of every object as an (n, 3) float64 array."""
    return np.array([np.asarray(getattr(o, attr), dtype=np.float64).reshape(3) for o in objs], dtype=np.float64).reshape(len(objs), 3)


def photon_energies(objs, photon_type):
    """(E as float64, NaN for what is no photon; who is a photon) -- exactly ``photon_type``, as the light steps decide it."""
    photon = np.array([type(o) is photon_type for o in objs], dtype=bool)
    return np.array([float(np.asarray(o.E)) if ph else np.nan for o, ph in zip(objs, photon)], dtype=np.float64), photon


# ---------------------------------------------------------------------------------------------- the collective
def reduce_parts(sim, parts):
    """(N, parts) summed over all shards in ONE payload: ``[sim._dev.count] + parts`` flattened in this order (``parts``: int64
    arrays, None where a tally was not asked for; the answer has the same shapes).  The library's own communicator takes 2048
    values per call, so a longer payload goes through ``sim._global`` in consecutive pieces of that size -- cut by position
    alone, so every rank cuts alike.  Every rank must call this, also with an empty shard."""
    flat = np.concatenate([[sim._dev.count]] + [x.reshape(-1) for x in parts if x is not None]).astype(np.int64, copy=False)
    if len(flat) <= ALLREDUCE_CHUNK:
        glob = np.asarray(sim._global(flat), dtype=np.int64)
    else:
        glob = np.concatenate([np.asarray(sim._global(flat[at:at + ALLREDUCE_CHUNK]), dtype=np.int64)
                               for at in range(0, len(flat), ALLREDUCE_CHUNK)])
    out, at = [], 1
    for x in parts:
        out.append(None if x is None else glob[at:at + x.size].reshape(x.shape))
        at += 0 if x is None else x.size
    return int(glob[0]), out


# ---------------------------------------------------------------------------------------------- rows
def object_row(cells):
    """The cells as one object-dtype row (cell by cell: numpy must not look into the arrays and lists among them)."""
    out = np.empty(len(cells), dtype=object)
    for k, x in enumerate(cells):
        out[k] = x
    return out


# ---------------------------------------------------------------------------------------------- the writer steps' streams
N_PASS_MAX = 0xFFFFFFFF      # n_pass is one 32-bit counter word


def writer_family(step):
    """The name of the Philox stream ``step`` draws from, which its class states (``_STREAM``, ``WriterStep``): steps of one name
    share counter words and are a family."""
    stream = type(step)._STREAM
    if stream is None:
        raise TypeError("%s states no _STREAM: a class below WriterStep names the Philox stream it draws from" % type(step).__name__)
    return stream


def earlier_steps(sim, step):
    """(the steps in front of ``step`` in the simulation's pass, those behind it), in the order the pass runs them."""
    steps = getattr(sim, "steps", None) or {}
    steps = list(steps.values() if isinstance(steps, dict) else steps)
    at = next((k for k, s in enumerate(steps) if s is step), len(steps))
    return steps[:at], steps[at + 1:]


class TallyStep(DeviceStep, MeasureStep):
    """A measure step whose row is ``[t, N, cells...]``, the cells made of integer tallies that add over shards.  A subclass
    sets ``measure_n`` and supplies three things:

    * ``_sweep(dev)``: the tallies of the resident store, one device sweep -- a sequence of int64 arrays (None: not asked for);
    * ``_host_parts(objs)``: the same sequence from the Python objects, with numpy;
    * ``_cells(parts)``: the row's cells behind ``[t, N]``.

    ``_device_run(sim)`` asks the simulation for ``t``, ``_dev`` and ``_global`` and nothing else (the CPU tests drive it
    with stand-ins that have no more).  ``_take`` is the name core.py calls behind a launch on a "snapshot" step."""

    def _sweep(self, dev):
        raise NotImplementedError

    def _host_parts(self, objs):
        raise NotImplementedError

    def _cells(self, parts):
        raise NotImplementedError

    def _due(self):
        """Whether this run of the step records (a step that records every n-th run counts here)."""
        return True

    def _clock(self, sim):
        return _snap(sim.t)                            # (a clock with units advances in place: the row keeps its own copy)

    def _record_tally(self, sim, n, parts):
        self.data.append(object_row([self._clock(sim)] + ([int(n)] if self.measure_n else []) + self._cells(parts)))

    def _take(self, sim):
        """One sweep of the store, then ONE collective for the whole row (every rank issues it, also with an empty shard)."""
        self._record_tally(sim, *reduce_parts(sim, self._sweep(sim._dev)))

    def _device_run(self, sim):
        if self._due():
            self._take(sim)

    def run(self, sim):
        if host_resident(sim):
            # called as a host plugin on host-resident objects: they hold the state, so nothing is uploaded for a
            # measurement.  float64 on both sides (core.py allocates no other store), so the row does not depend on where
            # the objects reside
            if self._due():
                objs = list(sim.objects)
                self._record_tally(sim, len(objs), self._host_parts(objs))
            return None
        return DeviceStep.run(self, sim)

    def terminate(self, sim):
        if self.out_fn is None:
            return
        with open(self.out_fn, "w") as f:              # an array cell is written as a list cell is: a (nested) plain list of integers
            for row in self.data:
                f.write(", ".join(str(x.tolist() if isinstance(x, np.ndarray) else x) for x in list(row)) + "\n")


class WriterStep(DeviceStep, MeasureStep):
    """A step that WRITES the store in one sweep behind a pass, draws from Philox blocks keyed by a pass counter of its own and
    records the sweep's tallies.  "refuse -> prepare -> move ``_pass`` -> one sweep -> one collective -> ``_record_pass``", on the
    device and -- with numpy, float64 -- on host-resident objects, is here once.

    Two counters.  ``_pass`` is the number of runs so far.  ``_n_pass`` is the Philox counter word the run's sweep and its numpy
    restatement are handed -- what a subclass passes on, readable after each run.  Steps whose draws share a counter word (a
    FAMILY: the classes that state the same ``_STREAM``) would draw the same number for the same photon if their
    counters moved in lock-step -- two gases absorbing in one pass would absorb the same photons.  So at its first run a step takes
    from the simulation's step list how many members ``m`` its family has in the pass and its place ``j`` among them in pass order,
    and from then on ``_n_pass = (_pass - 1) * m + j + 1``: the members' counters interleave and never meet.  With one member (and
    for a stand-in ``sim`` without ``steps``) that is ``_pass``.  Every rank of a sharded run holds the same step list, so nothing
    is communicated.  A counter beyond 2**32 - 1 is refused (ValueError) before ``_pass`` moves: it would wrap.

    A subclass sets
    ``_STREAM`` (every class directly below this one states it in its body: the name of the Philox stream it draws from -- the name of
    another class's where the two share counter words, as the two grounds do; what derives from the class inherits it, or states a
    name of its own where its draws have words of their own; a class that states none is refused at its first run, TypeError),
    ``_NOTE`` (what ``sim.launch_note`` says: the K-passes-per-launch kernels cannot carry the step) and ``_writes`` (which of
    ``r``, ``dr``, ``v``, ``dv``, ``E`` the host path writes back), keeps its own ``__init__`` and ``_record_pass``, and supplies:

    * ``_refuse(sim)`` and ``_prepare(sim, on_host)`` (both optional): raise what the step cannot run under, and work out what a
      pass needs ahead of its sweep; both run before ``_pass`` moves, so a refused call leaves the step as it was;
    * ``_sweep(sim, prep)``: the device sweep, its tallies as a list of int64 arrays (None: not asked for), the scalar counts
      together in the first;
    * ``_host_sweep(objs, ids, seed, prep)``: the numpy restatement on the Python objects -- ``(new, mask, record)``: the new
      state by field name, who is written back, and ``_record_pass``'s arguments behind ``sim``.

    ``_reduce(sim, parts)`` is the pass's ONE collective (every rank issues it, also with an empty shard)."""
    _fuse_role = None
    _STREAM = None
    _NOTE = None
    _writes = ("v", "dv")
    _pass = _n_pass = 0
    _family = None                                       # (members in the pass, this step's place among them): the first run's

    def _place(self, sim):
        """(m, j): how many steps of this step's family the simulation's pass holds and this step's place among them."""
        mine = writer_family(self)
        front, behind = earlier_steps(sim, self)
        same = lambda others: sum(1 for s in others if isinstance(s, WriterStep) and writer_family(s) == mine)   # noqa: E731
        return same(front) + 1 + same(behind), same(front)

    def _next_pass(self, sim):
        """Move ``_pass`` and set ``_n_pass`` for the run that begins, or ValueError with the step as it was."""
        place = self._family or self._place(sim)
        n_pass = self._pass * place[0] + place[1] + 1
        if n_pass > N_PASS_MAX:
            raise ValueError("%s: the Philox pass counter would pass 2**32 - 1 (run %d of member %d of %d that share a counter "
                             "word): it would wrap and repeat earlier draws" % (type(self).__name__, self._pass + 1, place[1] + 1, place[0]))
        self._family, self._pass, self._n_pass = place, self._pass + 1, n_pass

    def _refuse(self, sim):
        pass

    def _prepare(self, sim, on_host):
        return None

    def _sweep(self, sim, prep):
        raise NotImplementedError

    def _host_sweep(self, objs, ids, seed, prep):
        raise NotImplementedError

    def _reduce(self, sim, parts):
        # one payload, cut where it is longer than one call of the library's own communicator carries
        return reduce_parts(sim, parts)[1]

    def _device_run(self, sim):
        self._refuse(sim)
        prep = self._prepare(sim, False)
        self._next_pass(sim)                             # (may refuse, too: before anything is said)
        if getattr(sim, "launch_note", self._NOTE) is None and sim._k_wanted() > 1:      # (a device run only: the host path says nothing)
            sim.launch_note = self._NOTE
        parts = self._sweep(sim, prep)
        sim._scattered = True                            # velocities were replaced on the device
        parts = self._reduce(sim, parts)
        self._record_pass(sim, *parts[0], *parts[1:])

    def run(self, sim):
        self._refuse(sim)
        if not host_resident(sim):
            return DeviceStep.run(self, sim)
        prep = self._prepare(sim, True)
        objs = list(sim.objects)
        self._next_pass(sim)
        new, mask, record = self._host_sweep(objs, np.arange(len(objs)), getattr(sim, "seed", 0), prep)
        for k in np.flatnonzero(mask).tolist():
            o = objs[k]
            if "r" in self._writes:
                o.r = Measurement._from_code(new["r"][k], like=o.r, units="m**1")
                o.dr = Measurement._from_code(new["dr"][k], units="m**1")
            o.v, o.dv = np.array(new["v"][k], dtype=np.double), np.array(new["dv"][k], dtype=np.double)   # plain arrays, as a scatter leaves them
            if "E" in self._writes:
                o.E = Measurement._from_code(new["E"][k], like=o.E, units="J**1") if isinstance(o.E, Measurement) else np.double(new["E"][k])
        self._record_pass(sim, *record)
        return None
