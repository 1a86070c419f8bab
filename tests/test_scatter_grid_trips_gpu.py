"""GPU: the scattering on a grid (k_scatter_grid) past its first trip -- tests/test_writer_trips_gpu.py's scheme for this sweep.

A sweep's grid is capped at the resident workgroups, so a store of more than ``CAP = compute_units * 8 * 256`` slots sends every
workgroup through the loop's body again: the second trip is the first in which the wave-wide ballots at the head of the body run
behind a divergent ``continue`` and in which the run of hits a wave carries from trip to trip (one add for a run in one cell) is
carried at all.  Both forms -- the LDS form on 4 x 4 x 4 cells, the global form on 17 x 16 x 16, just above the switch -- at
``N2 = CAP + 2049 + 13`` slots (two trips, a ragged last wave) in f64 and f32 and at ``N3 = 2 * CAP + 77`` (three trips, workgroups
whose trip counts differ by one) in f64, every slot against the restatement (tests/scatter_grid_reference.py).

The scene is the edge scene with mixed probabilities: about a third of the exposed photons are hit.  ``has_work`` (the conditions of
tests/test_writer_trips_gpu.py, on the restatement's own mask of the hit slots: the lanes that stay in the body) is held from CAP on:
between 10 % and 90 % are hit, there are waves hit in part below CAP and from there on, with lane 0 idle beside a hit and with lane 0
hit beside an idle lane.  tests/test_scatter_grid_cpu.py needs no device to see that this file names the case.

In that scene the hit lanes of a wave hardly ever share a cell, so every hit is added by its own lane.  What the kernel has beyond its
siblings -- a wave whose hit lanes all stand in ONE cell adds their count once, and carries cell and count from trip to trip until the
cell changes or the loop ends -- is held by ``test_runs_of_hits_carried_across_trips``: p = 1 in every cell but one (Z, p = 0), every
slot placed in one of three cells A, B, Z, both forms, the same sizes.  ``PATTERNS``: every slot in A (that cell's tally is N, from
one add per wave for the whole sweep); the slots below CAP in A and those from CAP on in B; by trip A, Z, A (``stride_of`` restates
pcl_sweep::balanced_grid: a wave's slots in consecutive trips lie one stride apart), so a run waits through a trip without a hit and
is taken up again; and a cell drawn per 64 slots out of A, B, Z with a tenth of the lanes at rest, so that whatever the stride is
every wave is in one cell per trip and runs end, wait and go on in every order with some lanes of the wave left out.  ``sequences``
asserts from the pattern alone (tests/test_scatter_grid_cpu.py does it without a device, for 256 CUs) that waves go A -> B, A -> Z and,
with three trips, A -> Z -> A.  The tallies, the counts and every slot are the restatement's.

The restatement these cases are compared with is light._scatter_grid, the numpy one, for their size; tests/test_scatter_grid_cpu.py
holds it bit for bit to the independent loop on Python integers (tests/scatter_grid_reference.py: ``scatter_grid_loop``) on the edge
scene, and tests/test_scatter_grid_gpu.py compares the device with that loop directly.
"""
import numpy as np
import pytest

import writer_reference as W
from scatter_grid_reference import C, CENTER, ID_BASE, SEED, check_scatter_grid, grid_edges, probabilities, scene
from test_writer_trips_gpu import has_work, slots

pytestmark = pytest.mark.gpu

AXES = ("x", "y", "z")
FORMS = {"lds": (4, 4, 4), "global": (17, 16, 16)}                     # 64 cells; 4352 cells, above the 4096 of the switch


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def cap(dev):
    return dev.info()["compute_units"] * 8 * 256


@pytest.mark.parametrize("size, dtype", [("N2", "f64"), ("N2", "f32"), ("N3", "f64")])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_both_forms_past_one_trip(dev, cap, form, size, dtype):
    n, bins = slots(cap, size), FORMS[form]
    edges = grid_edges(AXES, bins)
    p = probabilities(bins)
    state = dict(scene(n, AXES, edges, np.float32 if dtype == "f32" else np.float64), id_base=ID_BASE)
    dev.store_alloc(n, dtype)
    dev.upload_state(state)
    before = W.snapshot(dev)
    for first, n_pass in ((1, 3), (0, 4)):                             # the second call on what the first left
        what = "grid scatter trips %s %s %s first=%d" % (form, size, dtype, first)
        answer = dev.scatter_grid(p, AXES, edges, CENTER, None, first, C, SEED, n_pass)
        after = W.snapshot(dev)
        ref = check_scatter_grid(before, after, answer, p, AXES, edges, CENTER, None, first, C, SEED, n_pass, what)
        has_work(ref["scattered"], cap, what)
        assert 0 < ref["exposed"][cap:].mean() < 0.9, what             # and lanes that are not exposed
        assert (np.asarray(answer[2]) > 0).sum() > 0.4 * p.size and not np.asarray(answer[2])[p == 0.0].any(), what
        before = after


# ------------------------------------------------------------------------------------------------ runs of hits, from trip to trip
SPOTS = {"A": (0.3, -0.6, 1.1), "B": (-1.3, 0.7, -0.4), "Z": (1.7, 1.7, -1.7)}     # three cells of either grid; Z is clear
PATTERNS = ("one_cell", "below_and_above_cap", "by_trip", "per_wave")


def stride_of(n, compute_units):
    """The slots between a wave's consecutive trips: pcl_sweep::balanced_grid's workgroups (8 resident per CU with these small LDS
    needs) times 256."""
    blocks, most = -(-n // 256), compute_units * 8
    trips = -(-blocks // most)
    return -(-blocks // trips) * 256


def pattern(name, n, cap, stride):
    """(the letter of every slot's cell, who is at rest)"""
    i = np.arange(n)
    rest = np.zeros(n, dtype=bool)
    if name == "one_cell":
        where = np.full(n, "A")
    elif name == "below_and_above_cap":
        where = np.where(i < cap, "A", "B")
    elif name == "by_trip":
        where = np.array(["A", "Z", "A"])[(i // stride) % 3]
    else:
        rng = np.random.RandomState(n)
        where = rng.choice(["A", "B", "Z"], size=-(-n // 64))[i // 64]
        rest = rng.uniform(size=n) < 0.1
    return where, rest


def sequences(where, stride):
    """The cells a wave stands in, trip by trip, as a set of strings like "AZA" over all waves with a slot in every trip."""
    n = len(where)
    trips = -(-n // stride)
    first = np.arange(0, stride, 64)
    first = first[first + (trips - 1) * stride < n]
    return set("".join(t) for t in zip(*(where[first + t * stride] for t in range(trips)))), trips


def runs_scene(name, n, cap, stride, dtype):
    where, rest = pattern(name, n, cap, stride)
    rng = np.random.RandomState(7)
    u = rng.normal(size=(n, 3))
    v = C * u / np.sqrt((u * u).sum(axis=1))[:, None]
    v[rest] = 0.0
    spots = np.array([SPOTS[k] for k in "ABZ"])
    state = {"r": spots[np.searchsorted(np.array(["A", "B", "Z"]), where)], "v": v, "dr": np.zeros((n, 3)), "dv": rng.normal(size=(n, 3)),
             "E": np.full(n, 2.0)}
    return {k: a.astype(dtype).astype(np.float64) for k, a in state.items()}, where, rest


def cell_of(edges, spot):
    return tuple(int(np.searchsorted(e, x, side="right")) - 1 for e, x in zip(edges, spot))


@pytest.mark.parametrize("size, dtype", [("N2", "f64"), ("N2", "f32"), ("N3", "f64")])
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_runs_of_hits_carried_across_trips(dev, cap, form, name, size, dtype):
    n, bins = slots(cap, size), FORMS[form]
    stride = stride_of(n, cap // (8 * 256))
    edges = grid_edges(AXES, bins)
    at = {k: cell_of(edges, SPOTS[k]) for k in SPOTS}
    assert len(set(at.values())) == 3
    p = np.ones(bins)
    p[at["Z"]] = 0.0
    state, where, rest = runs_scene(name, n, cap, stride, np.float32 if dtype == "f32" else np.float64)
    seen, trips = sequences(where, stride)
    assert trips == {"N2": 2, "N3": 3}[size]
    if name == "by_trip":
        assert seen == {"AZA"[:trips]}
    if name == "below_and_above_cap":
        assert any("AB" in q for q in seen) and len(seen) >= 2         # some waves change cell between two trips, some do not
    if name == "per_wave":
        assert {"AB", "AZ", "ZA", "BA", "AA"} <= {q[:2] for q in seen} and (trips == 2 or {"AZA", "ABA", "AAB", "ZAB"} <= seen)
    dev.store_alloc(n, dtype)
    dev.upload_state(dict(state, id_base=ID_BASE))
    before = W.snapshot(dev)
    what = "grid scatter runs %s %s %s %s" % (form, name, size, dtype)
    answer = dev.scatter_grid(p, AXES, edges, CENTER, None, 1, C, SEED, 5)
    ref = check_scatter_grid(before, W.snapshot(dev), answer, p, AXES, edges, CENTER, None, 1, C, SEED, 5, what)
    got = np.asarray(answer[2])
    want = {k: int(((where == k) & ~rest).sum()) for k in "AB"}         # p = 1: every moving photon of A and B is hit
    assert (int(got[at["A"]]), int(got[at["B"]]), int(got[at["Z"]])) == (want["A"], want["B"], 0), what
    assert answer[1] == want["A"] + want["B"] == int(got.sum()) and answer[0] == int((~rest).sum()), what
    if name == "one_cell":
        assert int(got[at["A"]]) == n == answer[1], what
