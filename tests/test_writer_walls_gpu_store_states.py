"""GPU: the walls' sweep (pcl_step_box_walls) on the states the hot path leaves the store in, at the level of the C ABI
(``_hip.Device``) -- tests/test_scatter_grid_gpu_store_states.py's scheme, its twin devices and its states, for this writer.

The states are tests/writer_reference.py's (``reach``: S1 a lazy fused step with implicit dr / dv, S2 behind an alive mask after a
delete body, S3 a large store whose aftermath compacts and whose dv is known to be zero, S4 behind a K-pass launch, S5 scrambled ids
and plain Objects).  With one history and one set of seeds:

* A: the sweep meets the store as the hot path left it;
* B: ``download_state()`` first -- the "before" state, and a store that is dense and real -- then the sweep;
* C: B's state after the sweep, uploaded into a fresh store and stepped on with ``lazy=False``: the plain path.

Required: A's and B's counts are equal; their stores behind the sweep are equal bit for bit (thirteen rows, ids, kinds, count); B's
"after" is the restatement of B's "before" (tests/box_walls_reference.py: ``check_box_walls`` -- with light._box_walls, the numpy
restatement, for S3's size; tests/test_writer_walls_cpu.py holds that one bit for bit to the independent loop); and after what the loop
does next (``aftermath``) A, B and C hold the same store bit for bit.

The box is three moves wide about the source, so the photons that never scattered stand outside it: mixed walls ("periodic",
"mirror", "open": r alone, all four groups, and v and dv are written -- an implicit dr and dv have to be real) and mirrors alone.
"""
import numpy as np
import pytest

import writer_reference as W
from box_walls_reference import WALLS, check_box_walls
from physicl_amd import light

pytestmark = pytest.mark.gpu

LO = [W.Source.origin[k] - 1.5 * W.STEP for k in range(3)]
HI = [W.Source.origin[k] + 1.5 * W.STEP for k in range(3)]


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


@pytest.mark.parametrize("walls", ["mixed", "mirror"])
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", W.STATES)
def test_the_sweep_on_the_store_the_hot_path_left(hip, devs, state, dtype, walls):
    a, b, c = devs
    modes = WALLS[walls]
    what = "box walls %s %s %s" % (state, dtype, walls)
    step = W.reach(hip, a, state, dtype)
    assert W.reach(hip, b, state, dtype) == step
    before = W.snapshot(b)                                             # makes B dense and real
    got_a, got_b = a.box_walls(modes, LO, HI), b.box_walls(modes, LO, HI)
    assert got_a.tolist() == got_b.tolist(), what
    after_a, after_b = W.snapshot(a), W.snapshot(b)
    W.assert_same_state(after_a, after_b, what + ": A and B behind the sweep")
    assert W.same_bits(before["kind"], after_b["kind"]) and before["count"] == after_b["count"], what
    ref = check_box_walls(before, after_b, got_b, modes, LO, HI, what, restate=light._box_walls)
    crossed = got_b[2:].reshape(3, 2)
    assert 0 < crossed.sum() and 0 < got_b[0] <= before["count"] and ref["written"].sum() > 100, what
    assert (crossed.sum(axis=1) > 0).all() and 0 < (ref["moving"] & ~ref["written"]).sum(), what
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
