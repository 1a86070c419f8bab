"""GPU: PathAbsorptionStep's sweep (pcl_step_absorb_path) on every state the hot path leaves the store in, at the level of the C ABI.

The twin-device scheme of tests/test_gpu_writer_store_states.py, with its helpers (tests/writer_reference.py: ``reach``,
``aftermath``, ``upload_plain``): device A meets the store as the hot path left it, B downloads first -- the "before" state, and a
store that is dense and real --, Q as A with nothing downloaded until the very end, C is B's state after the sweep in a fresh store,
stepped on with ``lazy=False``.  Required: the answers are equal; A's and B's stores are equal bit for bit behind the sweep; B's
"after" is the numpy restatement of B's "before" without a tolerance (tests/path_absorb_reference.py: ``check_path_absorb``); and
behind what the loop does next A, B, Q and C hold the same store bit for bit.

The states: S1 (two lazy fused steps: dr and dv implicit), S2 (plus a lazy delete body: an alive mask), S3 (a delete-only chain: dv
known to be zero -- the sweep writes dv = 0 on the photons it absorbs, and the survivors carry it), S4 (one K = 4 launch) and S5
(every 7th particle a plain Object, ids in scrambled order), f64 and f32.  The gas has the three layers of the writer tests about the
source -- the middle one transparent -- and the eight energy bands of ``W.E_EDGES`` (the energies reach from 1 to 3: some photons
are in no band).  Everybody moves in these states.
"""
import numpy as np
import pytest

import writer_reference as W
from path_absorb_reference import check_path_absorb

pytestmark = pytest.mark.gpu

P_GAS = np.array([np.linspace(0.1, 0.45, 8), np.zeros(8), np.linspace(0.9, 0.2, 8)])          # grey-ish, transparent, black-ish


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


def sweep(dev, state):
    exposed, absorbed, cells = dev.absorb_path(P_GAS, W.layer_edges(state), W.Source.origin, W.E_EDGES, W.SEED, W.N_PASS)
    return exposed, absorbed, cells.tolist()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", W.STATES)
def test_the_sweep_on_the_store_the_hot_path_left(hip, devs, state, dtype):
    a, b, c, q = devs
    what = "path absorb %s %s" % (state, dtype)
    step = W.reach(hip, a, state, dtype)
    assert W.reach(hip, b, state, dtype) == step and W.reach(hip, q, state, dtype) == step
    if state in ("S2", "S3"):                                          # the alive mask is really there
        assert a.slots > a.count and b.slots > b.count and a.slots == b.slots and a.count == b.count, what
    before = W.snapshot(b)                                             # makes B dense and real
    got_a, got_b, got_q = sweep(a, state), sweep(b, state), sweep(q, state)
    assert got_a == got_b == got_q, what
    after_a, after_b = W.snapshot(a), W.snapshot(b)
    W.assert_same_state(after_a, after_b, what + ": A and B behind the sweep")
    assert a.is_uniform() == (state in ("S1", "S4")), what

    # B's "after" is the restatement of B's "before"
    ref = check_path_absorb(before, after_b, got_b, P_GAS, W.layer_edges(state), np.asarray(W.Source.origin), W.E_EDGES, W.SEED, W.N_PASS, what)
    exposed, absorbed, cells = got_b
    by_layer = np.asarray(cells).sum(axis=1)
    print("%s: exposed %d, absorbed %d, by layer %s" % (what, exposed, absorbed, by_layer.tolist()))
    assert 0 < absorbed < exposed < before["count"] and by_layer[1] == 0 and by_layer[2] > 0, what      # some energies are in no band
    assert state == "S3" or by_layer[0] > 0, what                      # (S3: nobody has scattered, next to nobody stands that far in)
    if state == "S5":
        assert not ref["exposed"][::7].any(), what                     # plain Objects are never touched

    # what the loop does next
    W.upload_plain(c, after_b, b.capacity, dtype)
    slots0 = a.slots
    bodies = W.aftermath(hip, a, state, step, lazy=True)
    if state == "S3":
        assert a.slots < slots0 and a.slots == a.count, what           # a compaction has happened
    for dev, lazy in ((b, True), (q, True), (c, False)):
        assert W.aftermath(hip, dev, state, step, lazy=lazy, bodies=bodies) == bodies
    final = W.snapshot(a)
    assert 0 < final["count"] < after_b["count"], what
    for dev, name in ((b, "B"), (q, "Q"), (c, "C (lazy=False)")):
        W.assert_same_state(W.snapshot(dev), final, "%s: %s and A behind the aftermath" % (what, name))
    if state == "S3":                                                  # the survivors' dv is what the sweep left there: zeros
        at = np.searchsorted(after_b["id"], final["id"])
        assert np.array_equal(after_b["id"][at], final["id"]), what
        for k in range(3):
            assert W.same_bits(final["dv"][k], after_b["dv"][k][at]) and not final["dv"][k].any(), (what, "dv", k)
        parked = ref["absorbed"][at]
        assert parked.sum() > 0 and not np.stack(final["v"], 1)[parked].any(), what          # a parked photon stays parked
