"""GPU: the scattering sweep by layer and band (pcl_step_scatter_layered) on the states the hot path leaves the store in, at the level
of the C ABI (``_hip.Device``) -- tests/test_gpu_writer_store_states.py's scheme for this writer.

The states are tests/writer_reference.py's (``reach``: S1 a lazy fused step with implicit dr / dv, S2 behind an alive mask after a
delete body, S3 a large store whose aftermath compacts, S4 behind a K-pass launch, S5 scrambled ids and plain Objects).  With one
history and one set of seeds:

* A: the sweep meets the store as the hot path left it;
* B: ``download_state()`` first -- the "before" state, and a store that is dense and real -- then the sweep;
* C: B's state after the sweep, uploaded into a fresh store and stepped on with ``lazy=False``: the plain path.

Required: A's and B's answers are equal; their stores behind the sweep are equal bit for bit (thirteen rows, ids, kinds, count); B's
"after" is the numpy restatement of B's "before" (tests/scatter_layered_reference.py: ``check_scatter_layered``); and after what the
loop does next (``aftermath``) A, B and C hold the same store bit for bit.

The sweep has three layers about the source and eight bands over the fill's energies (some fall outside); the middle layer is clear.
``first`` is 0 (behind the fused scatter whose marks the store carries) and 1.
"""
import numpy as np
import pytest

import writer_reference as W
from scatter_layered_reference import check_scatter_layered

pytestmark = pytest.mark.gpu

P_CLOUD = np.array([np.linspace(0.1, 0.45, 8), np.zeros(8), np.linspace(0.9, 0.2, 8)])


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


def sweep(dev, state, first):
    exposed, scattered, cells = dev.scatter_layered(P_CLOUD, W.layer_edges(state), W.Source.origin, W.E_EDGES, first, W.C, W.SEED, W.N_PASS)
    return exposed, scattered, cells.tolist()


@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", W.STATES)
def test_the_sweep_on_the_store_the_hot_path_left(hip, devs, state, dtype, first):
    a, b, c = devs
    what = "layered scatter %s %s first=%d" % (state, dtype, first)
    step = W.reach(hip, a, state, dtype)
    assert W.reach(hip, b, state, dtype) == step
    before = W.snapshot(b)                                             # makes B dense and real
    got_a, got_b = sweep(a, state, first), sweep(b, state, first)
    assert got_a == got_b, what
    after_a, after_b = W.snapshot(a), W.snapshot(b)
    W.assert_same_state(after_a, after_b, what + ": A and B behind the sweep")
    assert W.same_bits(before["kind"], after_b["kind"]) and before["count"] == after_b["count"], what
    ref = check_scatter_layered(before, after_b, (got_b[0], got_b[1], np.asarray(got_b[2])), P_CLOUD, W.layer_edges(state),
                                np.asarray(W.Source.origin), W.E_EDGES, first, W.C, W.SEED, W.N_PASS, what)
    exposed, scattered, cells = got_b
    assert 0 < scattered < exposed < before["count"] and not np.asarray(cells)[1].any() and np.asarray(cells)[2].sum() > 0, what
    if state == "S5":
        assert not ref["written"][::7].any(), what                     # plain Objects are never touched

    # what the loop does next
    W.upload_plain(c, after_b, b.capacity, dtype)
    bodies = W.aftermath(hip, a, state, step, lazy=True)
    for dev, lazy in ((b, True), (c, False)):
        assert W.aftermath(hip, dev, state, step, lazy=lazy, bodies=bodies) == bodies
    final = W.snapshot(a)
    assert 0 < final["count"] < after_b["count"], what
    for dev, name in ((b, "B"), (c, "C (lazy=False)")):
        W.assert_same_state(W.snapshot(dev), final, "%s: %s and A behind the aftermath" % (what, name))
