"""GPU: the absorption sweep on a grid (pcl_step_absorb_grid) on the states the hot path leaves the store in, at the level of the C
ABI (``_hip.Device``) -- tests/test_scatter_grid_gpu_store_states.py's scheme, its twin devices and its states, for this writer.

The states are tests/writer_reference.py's (``reach``: S1 a lazy fused step with implicit dr / dv, S2 behind an alive mask after a
delete body, S3 a large store whose aftermath compacts and whose dv is known to be zero, S4 behind a K-pass launch, S5 scrambled ids
and plain Objects).  With one history and one set of seeds:

* A: the sweep meets the store as the hot path left it;
* B: ``download_state()`` first -- the "before" state, and a store that is dense and real -- then the sweep;
* C: B's state after the sweep, uploaded into a fresh store and stepped on with ``lazy=False``: the plain path.

Required: A's and B's answers are equal; their stores behind the sweep are equal bit for bit; B's "after" is the restatement of B's
"before" (grid_absorb_reference.check_grid_absorb, without tolerance); and after what the loop does next (``aftermath``) A, B and C
hold the same store bit for bit.

The grid is tests/test_scatter_grid_gpu_store_states.py's box about the source: 4 x 4 x 4 cells by eight bands with both tables in the
LDS form, 17 x 16 x 16 cells in the global form with k alone and with omega0 alone.  The slab along x just below the source is
transparent and conservative.
"""
import numpy as np
import pytest

import writer_reference as W
from grid_absorb_reference import check_grid_absorb
from test_scatter_grid_gpu_store_states import AXES, FORMS, clear_slab

pytestmark = pytest.mark.gpu


def field(form, which):
    bins, E_edges = FORMS[form]
    edges = [W.Source.origin[k] + np.linspace(-5.0, 5.0, b + 1) * W.STEP for k, b in enumerate(bins)]
    shape = bins + (() if E_edges is None else (len(E_edges) - 1,))
    p = np.broadcast_to(np.linspace(0.1, 0.6, shape[-1]), shape).copy()
    om = np.broadcast_to(np.linspace(0.2, 0.9, shape[-1]), shape).copy()
    p[clear_slab(form)], om[clear_slab(form)] = 0.0, 1.0
    return (p if which != "omega0" else None), (om if which != "k" else None), edges, E_edges


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


def sweep(dev, form, which):
    p, om, edges, E_edges = field(form, which)
    counts, cells = dev.absorb_grid(p, om, AXES, edges, None, E_edges, W.SEED, W.N_PASS)
    return counts.tolist(), cells.tolist()


@pytest.mark.parametrize("form, which", [("lds", "both"), ("global", "k"), ("global", "omega0")])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", W.STATES)
def test_the_sweep_on_the_store_the_hot_path_left(hip, devs, state, dtype, form, which):
    a, b, c = devs
    what = "grid absorb %s %s %s %s" % (state, dtype, form, which)
    step = W.reach(hip, a, state, dtype)
    assert W.reach(hip, b, state, dtype) == step
    before = W.snapshot(b)                                             # makes B dense and real
    got_a, got_b = sweep(a, form, which), sweep(b, form, which)
    assert got_a == got_b, what
    after_a, after_b = W.snapshot(a), W.snapshot(b)
    W.assert_same_state(after_a, after_b, what + ": A and B behind the sweep")
    assert W.same_bits(before["kind"], after_b["kind"]) and before["count"] == after_b["count"], what
    p, om, edges, E_edges = field(form, which)
    ref = check_grid_absorb(before, after_b, (got_b[0], np.asarray(got_b[1])), p, om, AXES, edges, np.zeros(3), E_edges, W.SEED, W.N_PASS, what)
    exposed, interacted, n_path, n_hit = got_b[0]
    size = (p if p is not None else om).size
    slab = ref["cell"] // (size // FORMS[form][0][0])                   # the cell's place along x (-1: not exposed)
    assert n_path + n_hit < exposed <= before["count"] and not np.asarray(got_b[1])[clear_slab(form)].any(), what
    assert (slab[ref["exposed"]] == clear_slab(form)).sum() > 100, what  # the clear slab is not empty: its photons drew nothing
    if state != "S3":                                                  # (S3's dv is known to be zero: there nobody has interacted)
        assert n_path + n_hit > 0 and (which == "k" or 0 < n_hit <= interacted <= exposed), what
    elif which != "omega0":
        assert n_path > 0, what
    if state == "S5":
        assert not ref["absorbed"][::7].any() and not ref["exposed"][::7].any(), what      # plain Objects are never touched

    # what the loop does next
    W.upload_plain(c, after_b, b.capacity, dtype)
    bodies = W.aftermath(hip, a, state, step, lazy=True)
    for dev, lazy in ((b, True), (c, False)):
        assert W.aftermath(hip, dev, state, step, lazy=lazy, bodies=bodies) == bodies
    final = W.snapshot(a)
    assert 0 < final["count"] < after_b["count"], what
    for dev, name in ((b, "B"), (c, "C (lazy=False)")):
        W.assert_same_state(W.snapshot(dev), final, "%s: %s and A behind the aftermath" % (what, name))
