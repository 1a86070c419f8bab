"""GPU: LayeredPhaseStep's sweep (pcl_step_phase_layered) on the states the hot path leaves the store in, at the level of the C ABI.

The twin-device scheme of tests/test_gpu_writer_store_states.py, with its helpers (tests/writer_reference.py: ``reach``,
``aftermath``): device A meets the store as the hot path left it, device B downloads first -- the "before" state, and a store
that is dense and real.  Required: the answers are equal; the stores are equal bit for bit behind the sweep and behind what the
loop does next; and B's "after" is the numpy restatement of B's "before" (tallies exact, rows that are not re-directed
bit-identical, re-directed rows within the phase function's bounds of writer_reference).

The three-layer mixture (Rayleigh | 0.3 Rayleigh + 0.7 Henyey-Greenstein | Henyey-Greenstein) about the source, on
S1 (two lazy fused steps: dr and dv implicit), S2 (plus a lazy delete body: an alive mask) and S4 (one K = 4 launch), f64 and f32.
"""
import numpy as np
import pytest

import writer_reference as W
from layered_phase_reference import MIX_LAWS, MIX_WEIGHTS
from physicl_amd import light

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


def sweep(dev, state):
    laws, _, cum, edges, center = light._check_layered_phase(MIX_LAWS, MIX_WEIGHTS, W.layer_edges(state), W.Source.origin)
    scattered, redirected, by_layer, by_law = dev.phase_layered(laws, cum, edges, center, W.C, W.SEED, W.N_PASS)
    return scattered, redirected, by_layer.tolist(), by_law.tolist()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", ["S1", "S2", "S4"])
def test_the_sweep_on_the_store_the_hot_path_left(hip, devs, state, dtype):
    a, b = devs
    what = "layered phase %s %s" % (state, dtype)
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
    bw, aw = W.wide(before), W.wide(after_b)
    T = np.asarray(before["E"]).dtype.type
    ref = light._layered_phase_redirect(bw["r"], bw["v"], bw["dv"], W.photons(before), before["id"], MIX_LAWS, MIX_WEIGHTS,
                                        W.layer_edges(state), W.Source.origin, W.C, W.SEED, W.N_PASS, T)
    scattered, redirected, by_layer, by_law = got_b
    print("%s: scattered %d, redirected %d, by layer %s, by law %s" % (what, scattered, redirected, by_layer, by_law))
    assert (scattered, redirected) == (int(ref["scattered"].sum()), int(ref["redirected"].sum())), what
    assert by_layer == ref["by_layer"].tolist() and by_law == ref["by_law"].tolist(), what
    assert min(by_layer) > 0 and min(by_law) > 0 and sum(by_layer) == sum(by_law) == redirected, what      # every layer and law has work
    go = ref["redirected"]
    for f in set(before) - set(W.FIELDS) - {"count"}:                  # E, ids, kinds
        assert W.same_bits(before[f], after_b[f]), (what, f)
    for f in W.FIELDS:                                                 # not re-directed: bit-identical; r and dr: everybody
        assert W.same_bits(aw[f][~go], bw[f][~go]), (what, f)
    assert W.same_bits(aw["r"], bw["r"]) and W.same_bits(aw["dr"], bw["dr"]), what
    v_unit, v_bound = (W.ulp(W.C), W.DIR_ULP) if T is np.float64 else (W.ulp(W.C, np.float32), W.DIR_ULP + 0.5)
    v_err = np.max(np.abs(aw["v"][go] - ref["v"][go])) / v_unit
    dv_err = np.max(np.abs(aw["dv"][go] - ref["dv"][go])) / v_unit
    print("%s: v %.3g ulp(c) (bound %g), dv %.3g ulp(c) (bound %g)" % (what, v_err, v_bound, dv_err, v_bound + 1))
    assert v_err <= v_bound and dv_err <= v_bound + 1.0, what

    # what the loop does next: a lazy fused step with a scatter and a lazy delete body
    assert W.aftermath(hip, a, state, step, lazy=True) == W.aftermath(hip, b, state, step, lazy=True) == 1
    final = W.snapshot(a)
    assert 0 < final["count"] < after_b["count"], what
    W.assert_same_state(W.snapshot(b), final, what + ": A and B behind the aftermath")
