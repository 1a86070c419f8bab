"""GPU: the scattering sweep on a grid (pcl_step_scatter_grid) on the states the hot path leaves the store in, at the level of the C
ABI (``_hip.Device``) -- tests/test_scatter_layered_gpu_store_states.py's scheme, its twin devices and its states, for this writer.

The states are tests/writer_reference.py's (``reach``: S1 a lazy fused step with implicit dr / dv, S2 behind an alive mask after a
delete body, S3 a large store whose aftermath compacts and whose dv is known to be zero, S4 behind a K-pass launch, S5 scrambled ids
and plain Objects).  With one history and one set of seeds:

* A: the sweep meets the store as the hot path left it;
* B: ``download_state()`` first -- the "before" state, and a store that is dense and real -- then the sweep;
* C: B's state after the sweep, uploaded into a fresh store and stepped on with ``lazy=False``: the plain path.

Required: A's and B's answers are equal; their stores behind the sweep are equal bit for bit (thirteen rows, ids, kinds, count); B's
"after" is the restatement of B's "before" (tests/scatter_grid_reference.py: ``check_scatter_grid`` -- with light._scatter_grid, the
numpy restatement, for S3's size; tests/test_scatter_grid_cpu.py holds that one bit for bit to the independent loop on Python
integers, and tests/test_scatter_grid_gpu.py compares the device with the loop directly); and after what the loop does
next (``aftermath``) A, B and C hold the same store bit for bit.

The grid is a box of ten moves' width about the source: 4 x 4 x 4 cells by eight bands over the fill's energies (some fall outside)
in the LDS form, with ``first`` 0 (behind the fused scatter whose marks the store carries) and 1; 17 x 16 x 16 cells without bands in
the global form, with ``first`` 0.  The cells of the slab along x just below the source (``clear_slab``) are clear.
"""
import numpy as np
import pytest

import writer_reference as W
from scatter_grid_reference import check_scatter_grid

pytestmark = pytest.mark.gpu

AXES = ("x", "y", "z")
FORMS = {"lds": ((4, 4, 4), W.E_EDGES), "global": ((17, 16, 16), None)}


def field(form):
    bins, E_edges = FORMS[form]
    edges = [W.Source.origin[k] + np.linspace(-5.0, 5.0, b + 1) * W.STEP for k, b in enumerate(bins)]
    shape = bins + (() if E_edges is None else (len(E_edges) - 1,))
    p = np.broadcast_to(np.linspace(0.15, 0.9, shape[-1]), shape).copy()
    p[clear_slab(form)] = 0.0
    return p, edges, E_edges


def clear_slab(form):
    return FORMS[form][0][0] // 2 - 1


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


def sweep(dev, form, first):
    p, edges, E_edges = field(form)
    exposed, scattered, cells = dev.scatter_grid(p, AXES, edges, None, E_edges, first, W.C, W.SEED, W.N_PASS)
    return exposed, scattered, cells.tolist()


@pytest.mark.parametrize("form, first", [("lds", 0), ("lds", 1), ("global", 0)])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", W.STATES)
def test_the_sweep_on_the_store_the_hot_path_left(hip, devs, state, dtype, form, first):
    a, b, c = devs
    what = "grid scatter %s %s %s first=%d" % (state, dtype, form, first)
    step = W.reach(hip, a, state, dtype)
    assert W.reach(hip, b, state, dtype) == step
    before = W.snapshot(b)                                             # makes B dense and real
    got_a, got_b = sweep(a, form, first), sweep(b, form, first)
    assert got_a == got_b, what
    after_a, after_b = W.snapshot(a), W.snapshot(b)
    W.assert_same_state(after_a, after_b, what + ": A and B behind the sweep")
    assert W.same_bits(before["kind"], after_b["kind"]) and before["count"] == after_b["count"], what
    p, edges, E_edges = field(form)
    ref = check_scatter_grid(before, after_b, (got_b[0], got_b[1], np.asarray(got_b[2])), p, AXES, edges, np.zeros(3), E_edges, first, W.C,
                             W.SEED, W.N_PASS, what)
    exposed, scattered, cells = got_b
    slab = ref["cell"] // (p.size // p.shape[0])                        # the cell's place along x (-1: not exposed)
    assert 0 < scattered < exposed <= before["count"] and not np.asarray(cells)[clear_slab(form)].any(), what
    assert (slab[ref["exposed"]] == clear_slab(form)).sum() > 100, what  # the clear slab is not empty: its photons drew nothing
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
