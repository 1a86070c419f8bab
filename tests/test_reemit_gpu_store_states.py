"""GPU: the re-emission sweep (pcl_step_reemit_parked) on the states the hot path leaves the store in, at the level of the C ABI
(``_hip.Device``) -- tests/test_gpu_writer_store_states.py's scheme for the seventh writer.

Nobody is at rest in the states of tests/writer_reference.py (``reach``: S1 .. S5), so a gas parks photons first
(``Device.absorb_path``, the grey-ish / transparent / black-ish gas of that file in the three layers about the source), on every
device alike.  Then, with one history and one set of seeds:

* A: the sweep meets the store as the hot path and the gas left it;
* B: ``download_state()`` first -- the "before" state, and a store that is dense and real -- then the sweep;
* C: B's state after the sweep, uploaded into a fresh store and stepped on with ``lazy=False``: the plain path.

Required: A's and B's answers are equal; their stores behind the sweep are equal bit for bit (thirteen rows, ids, kinds, count);
B's "after" is the numpy restatement of B's "before" (tests/reemit_reference.py: ``check_reemit``); and after what the loop does
next (``aftermath``) A, B and C hold the same store bit for bit.

The sweep has the gas's layers: the first re-emits at once, isotropically, from a table; the second (where the gas parks nobody)
has neither; the third is lambertian about the local vertical, holds every other photon back and has a table.
"""
import numpy as np
import pytest

import writer_reference as W
from reemit_reference import CDF_B, GRID_B, check_reemit

pytestmark = pytest.mark.gpu

P_GAS = np.array([np.linspace(0.1, 0.45, 8), np.zeros(8), np.linspace(0.9, 0.2, 8)])      # tests/test_gpu_writer_store_states.py's
GAS_PASS = W.N_PASS + 100


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def devs(hip):
    made = [hip.Device(0) for _ in range(3)]
    yield made
    for d in made:
        d.close()


def config(state):
    return dict(eta=np.array([1.0, 1.0, 0.5]), angular=("isotropic", "isotropic", "lambertian"),
                tables=[(GRID_B, CDF_B), None, (GRID_B, CDF_B)], edges=W.layer_edges(state), center=np.asarray(W.Source.origin))


def park(dev, state):
    return dev.absorb_path(P_GAS, W.layer_edges(state), W.Source.origin, W.E_EDGES, W.SEED, GAS_PASS)[1]


def sweep(dev, cfg):
    parked, reemitted, by_layer = dev.reemit_parked(W.C, cfg["eta"], cfg["angular"], cfg["tables"], cfg["edges"], cfg["center"], W.SEED, W.N_PASS)
    return parked, reemitted, by_layer.tolist()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", W.STATES)
def test_the_sweep_on_the_store_the_hot_path_left(hip, devs, state, dtype):
    a, b, c = devs
    what = "reemit %s %s" % (state, dtype)
    cfg = config(state)
    step = W.reach(hip, a, state, dtype)
    assert W.reach(hip, b, state, dtype) == step
    gone = park(a, state)
    assert park(b, state) == gone > 0, what
    before = W.snapshot(b)                                             # makes B dense and real
    got_a, got_b = sweep(a, cfg), sweep(b, cfg)
    assert got_a == got_b, what
    after_a, after_b = W.snapshot(a), W.snapshot(b)
    W.assert_same_state(after_a, after_b, what + ": A and B behind the sweep")
    assert W.same_bits(before["kind"], after_b["kind"]) and before["count"] == after_b["count"], what
    ref = check_reemit(before, after_b, got_b, cfg, W.SEED, W.N_PASS, what, W.photons(before), W.C)
    parked, reemitted, by_layer = got_b
    assert parked == gone and 0 < reemitted < parked and by_layer[1] == 0 and by_layer[2] > 0, what    # everybody parked stands in a layer
    assert state == "S3" or by_layer[0] > 0, what                      # (S3: nobody has scattered, next to nobody stands that far in)
    if state == "S5":
        assert not ref["parked"][::7].any(), what                      # plain Objects are never touched

    # what the loop does next
    W.upload_plain(c, after_b, b.capacity, dtype)
    bodies = W.aftermath(hip, a, state, step, lazy=True)
    for dev, lazy in ((b, True), (c, False)):
        assert W.aftermath(hip, dev, state, step, lazy=lazy, bodies=bodies) == bodies
    final = W.snapshot(a)
    assert 0 < final["count"] < after_b["count"], what
    for dev, name in ((b, "B"), (c, "C (lazy=False)")):
        W.assert_same_state(W.snapshot(dev), final, "%s: %s and A behind the aftermath" % (what, name))
