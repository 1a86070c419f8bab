"""GPU: the spectral ground's sweep (pcl_step_ground_spectral) on the states the hot path leaves the store in, at the level of the C ABI
(``_hip.Device``) -- tests/test_gpu_writer_store_states.py's scheme, as tests/test_writer_refract_gpu_store_states.py has it.

The states are those of tests/writer_reference.py (``reach``: S1 .. S5 -- implicit dr and dv, behind an alive mask, a delete-only
chain, what a K-pass launch leaves, scrambled ids with plain Objects among the photons), the sphere the one the ground's tests put
in the photons' way there (``sphere``), the bands in the style of its ``E_EDGES``: eight bands between 1.4 and 2.6 -- the fill's
energies reach from 1 to 3, so four in ten of the photons that are hit lie in no band (the sphere is hit by a hundred photons or
so: every outcome needs its share).  With one history and one set of seeds:

* A: the sweep meets the store as the hot path left it;
* B: ``download_state()`` first -- the "before" state, and a store that is dense and real -- then the sweep;
* C: B's state after the sweep, uploaded into a fresh store and stepped on with ``lazy=False``: the plain path.

Required: A's and B's tallies are equal; their stores behind the sweep are equal bit for bit (thirteen rows, ids, kinds, count);
B's "after" is the numpy restatement of B's "before" (tests/spectral_surface_reference.py: ``check_spectral`` -- exact but for the
lambertian lanes, which keep writer_reference's bounds); and after what the loop does next (``aftermath``) A, B and C hold the same
store bit for bit.
"""
import numpy as np
import pytest

import writer_reference as W
from spectral_surface_reference import assert_every_outcome, check_spectral

pytestmark = pytest.mark.gpu

E_EDGES = np.linspace(1.4, 2.6, 9)
ALBEDO = np.array([0.5, 1.0, 0.5, 0.0, 0.4, 0.6, 0.5, 0.5])
SPECULAR = np.array([1.0, 0.5, 0.0, 0.5, 0.5, 0.5, 0.5, 0.5])


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


def sweep(dev, cfg):
    return dev.ground_spectral(cfg["radius"], cfg["E_edges"], cfg["albedo"], cfg["specular"], cfg["center"], W.C, W.SEED, W.N_PASS)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("state", W.STATES)
def test_the_sweep_on_the_store_the_hot_path_left(hip, devs, state, dtype):
    a, b, c = devs
    what = "spectral %s %s" % (state, dtype)
    radius, center = W.sphere(state)
    cfg = dict(radius=radius, center=center, E_edges=E_EDGES, albedo=ALBEDO, specular=SPECULAR)
    step = W.reach(hip, a, state, dtype)
    assert W.reach(hip, b, state, dtype) == step
    before = W.snapshot(b)                                             # makes B dense and real
    got_a, got_b = sweep(a, cfg), sweep(b, cfg)
    for x, y in zip(got_a, got_b):
        assert x.tolist() == y.tolist(), what
    after_a, after_b = W.snapshot(a), W.snapshot(b)
    W.assert_same_state(after_a, after_b, what + ": A and B behind the sweep")
    assert W.same_bits(before["kind"], after_b["kind"]) and before["count"] == after_b["count"], what
    ref = check_spectral(before, after_b, got_b, cfg, W.SEED, W.N_PASS, what, W.photons(before), W.C, W.W_MAX)
    # the sphere stands in the photons' way; the shares need the device's history, so they are printed, not recorded
    print(what, assert_every_outcome(ref, what))
    if state == "S5":
        assert not ref["hit"][::7].any(), what                         # plain Objects are never hit

    # what the loop does next
    W.upload_plain(c, after_b, b.capacity, dtype)
    bodies = W.aftermath(hip, a, state, step, lazy=True)
    for dev, lazy in ((b, True), (c, False)):
        assert W.aftermath(hip, dev, state, step, lazy=lazy, bodies=bodies) == bodies
    final = W.snapshot(a)
    assert 0 < final["count"] < after_b["count"], what
    for dev, name in ((b, "B"), (c, "C (lazy=False)")):
        W.assert_same_state(W.snapshot(dev), final, "%s: %s and A behind the aftermath" % (what, name))
