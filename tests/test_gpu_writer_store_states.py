"""GPU: the six sweeps that write the store -- the ground, the phase function, absorption, the layered phase function, recycling,
absorption along the path (pcl_surface.hip) -- on the states the hot path leaves the store in, at the level of the C ABI
(``_hip.Device``).

A writer cannot be checked the way the read-only sweeps are (download, sweep, restate): the download itself makes the store
dense and dr / dv real.  So every case runs TWIN devices through one history with one set of seeds (Philox is keyed by id and
step, the tallies are integer atomics: the runs are deterministic):

* A: the sweep meets the store as the hot path left it;
* B: ``download_state()`` first -- the "before" state, and a store that is dense and real -- then the sweep;
* Q: as A, and nothing is downloaded until the very end;
* C: B's state after the sweep, uploaded into a fresh store and stepped on with ``lazy=False``: the plain path.

Required: A's and B's answers are equal; their stores after the sweep are equal bit for bit (thirteen rows, ids, kinds, count);
B's "after" is the numpy restatement of B's "before" under the bounds of tests/writer_reference.py (counts exact, untouched rows
bit-identical, absorption exact everywhere); and after what the loop does next -- a lazy fused step with a scatter and a lazy
delete body, or for S3 delete bodies until a compaction has happened -- A, B, Q and C hold the same store bit for bit.

The states (tests/writer_reference.py: ``reach``), each in f64 and f32, reached as tests/test_gpu_shell.py reaches them, from
``fill_photons`` + ``apply_source`` of an isotropic gaussian spot off the centre:

* S1  dr and dv implicit: two ``step_fused(lazy=True)`` with a scatter (A*n*|dr| = 0.45);
* S2  S1 and one ``step_fused_delete(lazy=True)`` body: an alive mask (``slots > count``), ids of their own after ``densify``;
* S3  a delete-only chain from a fresh fill: dv known to be zero; delete bodies behind the sweep until ``slots`` has dropped --
      the survivors' dv must be what the ground wrote; the phase function and absorption find nobody and change nothing;
* S4  one ``step_fused_multi`` with K = 4;
* S5  S1 with every 7th particle a plain Object and ids in scrambled order: kinds and ids are staged behind a lazy store.

The sphere, the layers and omega0 were chosen on the CPU (the oracle's steps and the restatements on source_reference's
population) so that every sweep has work in every state it is asked to act in; the counts are asserted, not assumed.

The ground, the phase function, absorption and path absorption run on all four devices and every state (``FOUR``).  The layered
phase function and recycling run as A and B alone, on S1, S2 and S4 (``TWIN``): the answers are equal, the stores are equal bit
for bit behind the sweep and behind one lazy fused step and delete body, and B's "after" is the restatement of B's "before".

* layered phase: the three-layer mixture (Rayleigh | 0.3 Rayleigh + 0.7 Henyey-Greenstein | Henyey-Greenstein) about the source;
  tallies exact, rows that are not re-directed bit-identical, re-directed rows within the phase function's bounds;
* recycle: the top is the outer edge of the second layer about the source: the photons that never scattered stand beyond it, the
  random walkers inside.  Nobody is at rest on these states (that count is 0); a spectrum is given, so E is written as well;
* path absorption: the gas has the three layers about the source -- the middle one transparent -- and the eight energy bands of
  ``W.E_EDGES`` (the energies reach from 1 to 3: some photons are in no band); everybody moves in these states, the restatement
  holds without a tolerance, and on S3 the sweep writes dv = 0 on the photons it absorbs, and the survivors carry it.
"""
import numpy as np
import pytest

import writer_reference as W
from layered_phase_reference import MIX_LAWS, MIX_WEIGHTS, check_layered
from path_absorb_reference import check_path_absorb
from physicl_amd import light
from recycle_reference import CDF, GRID, check_recycle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def devs(hip):
    made = [hip.Device(0) for _ in range(4)]
    yield made
    for d in made:
        d.close()


class Ground:
    touched = "hit"                                                    # the restatement's mask of the rows the sweep acted on

    def __init__(self, mode):
        self.mode, self.name = mode, "ground " + mode

    def call(self, dev, state):
        radius, center = W.sphere(state)
        return tuple(dev.surface_reflect(radius, center, 0.5, self.mode, W.C, W.SEED, W.N_PASS))

    def check(self, before, after, answer, state, what):
        radius, center = W.sphere(state)
        ref = W.check_surface(before, after, answer, radius, center, 0.5, self.mode, W.C, W.SEED, W.N_PASS, W.W_MAX, what)
        print("%s: reflected %d, absorbed %d" % (what, answer[0], answer[1]))
        assert answer[0] > 0 and answer[1] > 0, what                   # albedo 0.5: both happen, in every state
        return ref

    def survivors(self, final, ref, at, what):
        kept = ref["hit"][at]
        print("%s: %d of the survivors carry the ground's dv" % (what, int(kept.sum())))
        assert kept.sum() > 0 and np.stack(final["dv"], 1)[kept].any(axis=1).all(), what


class Phase:
    touched = "redirected"

    def __init__(self, phase, g):
        self.phase, self.g, self.name = phase, g, "phase " + phase

    def call(self, dev, state):
        return (dev.phase_redirect(self.phase, self.g, W.C, W.SEED, W.N_PASS),)

    def check(self, before, after, answer, state, what):
        ref = W.check_phase(before, after, answer[0], self.phase, self.g, W.C, W.SEED, W.N_PASS, what)
        print("%s: redirected %d" % (what, answer[0]))
        assert (answer[0] == 0) if state == "S3" else (answer[0] > 0), what
        return ref


class Absorb:
    name, touched = "absorb layers", "interacted"

    def call(self, dev, state):
        interacted, absorbed, by_layer, E_hist = dev.absorb_scattered(W.OMEGA0, W.layer_edges(state), W.Source.origin, W.E_EDGES, W.SEED, W.N_PASS)
        return interacted, absorbed, by_layer.tolist(), E_hist.tolist()

    def check(self, before, after, answer, state, what):
        ref = W.check_absorb(before, after, answer, W.OMEGA0, W.layer_edges(state), W.Source.origin, W.E_EDGES, W.SEED, W.N_PASS, what)
        interacted, absorbed, by_layer, E_hist = answer
        print("%s: interacted %d, absorbed %d, by layer %s, in the energy bins %d" % (what, interacted, absorbed, by_layer, int(np.sum(E_hist))))
        if state == "S3":                                              # dv is zero: nobody interacted
            assert interacted == 0 and absorbed == 0 and not any(by_layer) and not np.any(E_hist), what
        else:                                                          # the grey and the black-ish layer absorb, the conservative one does not
            assert by_layer[0] > 0 and by_layer[1] == 0 and by_layer[2] > 0 and interacted > absorbed and np.sum(E_hist) > 0, what
        return ref


class PathAbsorb:
    name, touched = "path absorb", "exposed"
    P_GAS = np.array([np.linspace(0.1, 0.45, 8), np.zeros(8), np.linspace(0.9, 0.2, 8)])      # grey-ish, transparent, black-ish

    def call(self, dev, state):
        exposed, absorbed, cells = dev.absorb_path(self.P_GAS, W.layer_edges(state), W.Source.origin, W.E_EDGES, W.SEED, W.N_PASS)
        return exposed, absorbed, cells.tolist()

    def check(self, before, after, answer, state, what):
        ref = check_path_absorb(before, after, answer, self.P_GAS, W.layer_edges(state), np.asarray(W.Source.origin), W.E_EDGES, W.SEED,
                                W.N_PASS, what)
        exposed, absorbed, cells = answer
        by_layer = np.asarray(cells).sum(axis=1)
        print("%s: exposed %d, absorbed %d, by layer %s" % (what, exposed, absorbed, by_layer.tolist()))
        assert 0 < absorbed < exposed < before["count"] and by_layer[1] == 0 and by_layer[2] > 0, what      # some energies are in no band
        assert state == "S3" or by_layer[0] > 0, what                  # (S3: nobody has scattered, next to nobody stands that far in)
        return ref

    def survivors(self, final, ref, at, what):                         # the dv the sweep left there: zeros
        for k in range(3):
            assert not final["dv"][k].any(), (what, "dv", k)
        parked = ref["absorbed"][at]
        assert parked.sum() > 0 and not np.stack(final["v"], 1)[parked].any(), what          # a parked photon stays parked


class Layered:
    name = "layered phase"

    def call(self, dev, state):
        laws, _, cum, edges, center = light._check_layered_phase(MIX_LAWS, MIX_WEIGHTS, W.layer_edges(state), W.Source.origin)
        scattered, redirected, by_layer, by_law = dev.phase_layered(laws, cum, edges, center, W.C, W.SEED, W.N_PASS)
        return scattered, redirected, by_layer.tolist(), by_law.tolist()

    def check(self, before, after, answer, state, what):
        scattered, redirected, by_layer, by_law = answer
        assert min(by_layer) > 0 and min(by_law) > 0 and sum(by_layer) == sum(by_law) == redirected, what  # every layer and law has work
        check_layered(before, after, answer, MIX_LAWS, MIX_WEIGHTS, W.layer_edges(state), W.Source.origin, W.C, W.SEED, W.N_PASS, what)


class Recycle:
    name = "recycle"

    def call(self, dev, state):
        top = float(W.layer_edges(state)[2])
        return dev.recycle_spent(W.Source, W.C, True, top, W.Source.origin, (GRID, CDF), W.SEED, W.N_PASS)

    def check(self, before, after, answer, state, what):
        top = float(W.layer_edges(state)[2])
        ref = check_recycle(before, after, answer, W.Source, top, np.asarray(W.Source.origin), True, (GRID, CDF), W.SEED, W.N_PASS,
                            what, W.photons(before))
        assert W.same_bits(before["kind"], after["kind"]) and before["count"] == after["count"], what
        assert answer[0] == 0 and 0 < answer[1] < before["count"], what    # some but not all photons are outside, nobody is at rest
        assert int(ref["spent"].sum()) == answer[1], what


FOUR = [Ground("lambertian"), Ground("specular"), Phase(*W.LAWS[0]), Phase(*W.LAWS[1]), Absorb(), PathAbsorb()]
TWIN = [Layered(), Recycle()]
by_sweep = lambda sweeps: pytest.mark.parametrize("sweep", sweeps, ids=[s.name.replace(" ", "_") for s in sweeps])      # noqa: E731


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", W.STATES)
@by_sweep(FOUR)
def test_a_writer_sweep_on_the_store_the_hot_path_left(hip, devs, sweep, state, dtype):
    a, b, c, q = devs
    what = "%s %s %s" % (sweep.name, state, dtype)
    step = W.reach(hip, a, state, dtype)
    assert W.reach(hip, b, state, dtype) == step and W.reach(hip, q, state, dtype) == step
    if state in ("S2", "S3"):                                          # the alive mask is really there
        assert a.slots > a.count and b.slots > b.count and a.slots == b.slots and a.count == b.count, what
        print("%s: slots %d > count %d before the sweep" % (what, a.slots, a.count))
    before = W.snapshot(b)                                             # makes B dense and real
    got_a, got_b, got_q = sweep.call(a, state), sweep.call(b, state), sweep.call(q, state)
    assert got_a == got_b == got_q, what
    after_a, after_b = W.snapshot(a), W.snapshot(b)
    W.assert_same_state(after_a, after_b, what + ": A and B behind the sweep")
    assert a.is_uniform() == (state in ("S1", "S4")), what             # S2, S3: ids of their own behind densify; S5: staged ids and kinds
    ref = sweep.check(before, after_b, got_b, state, what)
    if state == "S5":
        assert not ref[sweep.touched][::7].any(), what                 # plain Objects are never touched

    # what the loop does next
    W.upload_plain(c, after_b, b.capacity, dtype)
    slots0 = a.slots
    bodies = W.aftermath(hip, a, state, step, lazy=True)
    if state == "S3":
        assert a.slots < slots0 and a.slots == a.count, what           # a compaction has happened
        print("%s: slots dropped from %d to %d behind %d delete bodies" % (what, slots0, a.slots, bodies))
    for dev, lazy in ((b, True), (q, True), (c, False)):
        assert W.aftermath(hip, dev, state, step, lazy=lazy, bodies=bodies) == bodies
    final = W.snapshot(a)
    assert 0 < final["count"] < after_b["count"], what
    for dev, name in ((b, "B"), (q, "Q"), (c, "C (lazy=False)")):
        W.assert_same_state(W.snapshot(dev), final, "%s: %s and A behind the aftermath" % (what, name))
    if state == "S3":                                                  # the survivors' dv is what the sweep left there
        at = np.searchsorted(after_b["id"], final["id"])
        assert np.array_equal(after_b["id"][at], final["id"]), what
        for k in range(3):
            assert W.same_bits(final["dv"][k], after_b["dv"][k][at]), (what, "dv", k)
        if hasattr(sweep, "survivors"):
            sweep.survivors(final, ref, at, what)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", ["S1", "S2", "S4"])
@by_sweep(TWIN)
def test_a_writer_sweep_on_twin_devices(hip, devs, sweep, state, dtype):
    a, b = devs[:2]
    what = "%s %s %s" % (sweep.name, state, dtype)
    step = W.reach(hip, a, state, dtype)
    assert W.reach(hip, b, state, dtype) == step
    if state == "S2":                                                  # the alive mask is really there
        assert a.slots > a.count and b.slots > b.count and a.slots == b.slots and a.count == b.count, what
    before = W.snapshot(b)                                             # makes B dense and real
    got_a, got_b = sweep.call(a, state), sweep.call(b, state)
    assert got_a == got_b, what
    after_a, after_b = W.snapshot(a), W.snapshot(b)
    W.assert_same_state(after_a, after_b, what + ": A and B behind the sweep")
    sweep.check(before, after_b, got_b, state, what)                   # B's "after" is the restatement of B's "before"

    # what the loop does next: a lazy fused step with a scatter and a lazy delete body
    assert W.aftermath(hip, a, state, step, lazy=True) == W.aftermath(hip, b, state, step, lazy=True) == 1
    final = W.snapshot(a)
    assert 0 < final["count"] < after_b["count"], what
    W.assert_same_state(W.snapshot(b), final, what + ": A and B behind the aftermath")
