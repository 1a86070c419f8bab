"""GPU: RecycleStep's sweep (pcl_step_recycle_spent) on the states the hot path leaves the store in, at the level of the C ABI.

The twin-device scheme of tests/test_layered_phase_gpu_store_states.py, with its helpers (tests/writer_reference.py: ``reach``,
``aftermath``): device A meets the store as the hot path left it, device B downloads first -- the "before" state, and a store
that is dense and real.  Required: the answers are equal; the stores are equal bit for bit behind the sweep and behind what the
loop does next; and B's "after" is the numpy restatement of B's "before" (tests/recycle_reference.py: ``check_recycle``).

The top is the outer edge of the second layer about the source: the photons that never scattered stand beyond it, the random
walkers inside.  Nobody is at rest on these states (that count is 0); a spectrum is given, so E is written as well.  S1 (two lazy
fused steps: dr and dv implicit), S2 (plus a lazy delete body: an alive mask) and S4 (one K = 4 launch), f64 and f32.
"""
import numpy as np
import pytest

import writer_reference as W
from recycle_reference import CDF, GRID, check_recycle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def devs(hip):
    made = [hip.Device(0) for _ in range(2)]
    yield made
    for d in made:
        d.close()


def top_of(state):
    return float(W.layer_edges(state)[2])


def sweep(dev, state):
    return dev.recycle_spent(W.Source, W.C, True, top_of(state), W.Source.origin, (GRID, CDF), W.SEED, W.N_PASS)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", ["S1", "S2", "S4"])
def test_the_sweep_on_the_store_the_hot_path_left(hip, devs, state, dtype):
    a, b = devs
    what = "recycle %s %s" % (state, dtype)
    step = W.reach(hip, a, state, dtype)
    assert W.reach(hip, b, state, dtype) == step
    if state == "S2":                                                  # the alive mask is really there
        assert a.slots > a.count and b.slots > b.count and a.slots == b.slots and a.count == b.count, what
    before = W.snapshot(b)                                             # makes B dense and real
    got_a, got_b = sweep(a, state), sweep(b, state)
    assert got_a == got_b, what
    after_a, after_b = W.snapshot(a), W.snapshot(b)
    W.assert_same_state(after_a, after_b, what + ": A and B behind the sweep")

    # B's "after" is the restatement of B's "before"
    ref = check_recycle(before, after_b, got_b, W.Source, top_of(state), np.asarray(W.Source.origin), True, (GRID, CDF), W.SEED, W.N_PASS,
                        what, W.photons(before))
    assert W.same_bits(before["kind"], after_b["kind"]) and before["count"] == after_b["count"], what
    assert got_b[0] == 0 and 0 < got_b[1] < before["count"], what      # some but not all photons are outside, nobody is at rest
    assert int(ref["spent"].sum()) == got_b[1], what

    # what the loop does next: a lazy fused step with a scatter and a lazy delete body
    assert W.aftermath(hip, a, state, step, lazy=True) == W.aftermath(hip, b, state, step, lazy=True) == 1
    final = W.snapshot(a)
    assert 0 < final["count"] < after_b["count"], what
    W.assert_same_state(W.snapshot(b), final, what + ": A and B behind the aftermath")
