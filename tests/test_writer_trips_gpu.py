"""GPU: every store sweep past its first trip ("Trips").

A sweep's grid is capped at the resident workgroups -- ``pcl_sweep::balanced_grid``: 8 workgroups of 256 slots per CU, fewer with
large LDS tables --, so a store of more than ``CAP = compute_units * 8 * 256`` slots sends every workgroup through the loop's body
again.  The second trip is the first in which the wave-wide ballots at the head of the body run behind a divergent ``continue``, in
which a value computed once outside the loop is used a second time, in which a tile index passes ``gridDim * 256``, and -- with a
third -- in which neighbouring workgroups take different numbers of trips.  ``TRIP_CASES`` names, for every kernel of
``build.ADDONS``, the test that compares it slot by slot at such a size (tests/test_writer_trips_cpu.py holds the
table against the build's); the seven that had none are in this file.

* the five writers (the ground, the phase function, absorption, the layered phase function, re-emission) through the ``Device`` call,
  the scene builder and the comparison of their own test files, in the configuration with the most branches: ``N2 = CAP + 2049 + 13``
  slots (two trips, a ragged last wave, a last tile that is not full) in f64 and f32, ``N3 = 2 * CAP + 77`` (three trips,
  workgroups whose trip counts differ by one) in f64, N2 with scrambled explicit ids and plain Objects among the photons, and at
  N2 in f64 a second pass on the state the first left behind;
* the detector's image (an aperture with bands, 33 x 17) and the source (a cone from a gaussian spot) at the same sizes.

No case passes on nothing (``has_work``, on the restatement's own mask of the slots the kernel works on): (a) between 10 % and
90 % of the slots from CAP on work; (b) below CAP and from CAP on there are waves of which some but not all lanes work; (c) from
CAP on there is a wave whose lane 0 is idle while another lane works, and one whose lane 0 works while another lane is idle.  The
source writes every slot: for it the slots from CAP on are written and are the restatement's.

The ground's population is surface_reference.cloud's in a shuffled order (there every even slot is hit, and lane 0 of every wave
with them).  The ground's second pass finds only those of the photons it parked on the sphere that rounding left a hair inside
(a twelfth of the slots: a photon that bounced stands outside): it is held to (b), (c) and somebody at work from CAP on, without
the 10 % of (a); the other writers' second passes meet (a)-(c) in full.  Absorption's population is made on the device (its own
test file's builder: a source, a Newton step, a scatter step), so its conditions are only known once the case runs.  Re-emission
with a third at rest is held to (a)-(c) on the parked, who take the ballots, and to (b), (c) and somebody at work on the
re-emitted, the lanes that stay in the body.  Bounds are tests/writer_reference.py's; nothing here has a tolerance of its own.
"""
import numpy as np
import pytest

import writer_reference as W
from layered_phase_reference import C, SEED, cases as layered_cases, check_layered
from phase_reference import cloud as phase_cloud
from physicl_amd import light
from reemit_reference import LAYERED, check_reemit
from surface_reference import CENTER as GROUND_CENTER, RADIUS, cloud as ground_cloud

pytestmark = pytest.mark.gpu

# kernel -> (file, test) of the case that takes it past one trip and compares every slot (tests/test_writer_trips_cpu.py)
HERE = "test_writer_trips_gpu.py"
TRIP_CASES = {
    "k_plane_spectra": ("test_gpu_spectrum.py", "test_spectra_equal_histogram_of_the_lists_after_a_newton_step"),     # 1 000 000 slots
    "k_apply_source": (HERE, "test_the_source_past_one_trip"),
    "k_shell_crossings": ("test_gpu_shell.py", "test_tallies_equal_the_restatement"),                                  # 600 011 slots
    "k_detector_image": (HERE, "test_the_detector_s_image_past_one_trip"),
    "k_position_grid": ("test_gpu_snapshot_grid.py", "test_grid_equals_the_restatement_on_a_spread_cloud"),            # 1 000 000 slots
    "k_surface_reflect": (HERE, "test_a_writer_past_one_trip"),
    "k_phase_redirect": (HERE, "test_a_writer_past_one_trip"),
    "k_absorb_scattered": (HERE, "test_a_writer_past_one_trip"),
    "k_phase_layered": (HERE, "test_a_writer_past_one_trip"),
    "k_recycle_spent": ("test_recycle_gpu.py", "test_a_workgroup_takes_more_than_one_trip"),
    "k_absorb_path": ("test_path_absorb_gpu.py", "test_a_workgroup_takes_more_than_one_trip"),
    "k_reemit_parked": (HERE, "test_a_writer_past_one_trip"),
    "k_refract_surface": ("test_writer_refract_gpu.py", "test_past_the_grid_s_first_stride"),
    "k_ground_spectral": ("test_spectral_surface_gpu.py", "test_past_the_first_trip"),
    "k_scatter_layered": ("test_scatter_layered_gpu.py", "test_just_past_the_first_trip_of_the_balanced_grid"),
    "k_scatter_grid": ("test_scatter_grid_trips_gpu.py", "test_both_forms_past_one_trip"),
    "k_box_walls": ("test_writer_walls_trips_gpu.py", "test_the_walls_past_one_trip"),
}

ID_BASE = W.ID_BASE                                                    # above 2^32
ROOM = 300                                                             # capacity beyond N
N_PASS = 3
SHUFFLE_SEED = 17                                                      # the ground's population, out of its even / odd order
SIZES = [("N2", "f64"), ("N2", "f32"), ("N3", "f64")]
assert C == W.C and ID_BASE > 2 ** 32


def slots(cap, size):
    return {"N2": cap + 2049 + 13, "N3": 2 * cap + 77}[size]


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
    """The slots of a sweep's first trip at the most: the grid's cap of resident workgroups, from the device."""
    return dev.info()["compute_units"] * 8 * 256


def has_work(mask, cap, what, floor=0.1):
    """Conditions (a)-(c) of the module's docstring on a kernel's work mask.  ``floor``: the lower end of (a); a mask that is
    sparse for a stated reason is held to ``floor=0.0`` -- somebody from ``cap`` on works, and (b) and (c) in full.  Returns the
    working fraction from ``cap`` on."""
    mask = np.asarray(mask, dtype=bool)
    assert cap % 64 == 0 and len(mask) >= cap + 128, what
    first, later = (m[:len(m) // 64 * 64].reshape(-1, 64) for m in (mask[:cap], mask[cap:]))      # whole waves
    fraction = float(mask[cap:].mean())
    partial = [int((w.any(axis=1) & ~w.all(axis=1)).sum()) for w in (first, later)]
    lane0_idle = int((~later[:, 0] & later[:, 1:].any(axis=1)).sum())
    lane0_works = int((later[:, 0] & ~later[:, 1:].all(axis=1)).sum())
    print("%s: %.4f of the slots from %d on work; waves in part: %d below, %d from there on; lane 0 idle beside work in %d, at work beside "
          "idle lanes in %d" % (what, fraction, cap, partial[0], partial[1], lane0_idle, lane0_works))
    assert 0.0 < fraction and floor <= fraction <= 0.9, what           # (a)
    assert partial[0] > 0 and partial[1] > 0, what                     # (b)
    assert lane0_idle > 0 and lane0_works > 0, what                    # (c)
    return fraction


def np_type(dtype):
    return np.float32 if dtype == "f32" else np.float64


# ------------------------------------------------------------------------------------------------ the five writers
class Ground:
    name, touched, also = "ground", "hit", ()
    # A photon that bounced stands outside the sphere, so a second pass re-hits only those of the photons the first parked on the
    # sphere (albedo 0.5: a quarter of the slots) whose rounded position lies a hair inside it: too few for the 10 % of (a).
    second_pass_floor = 0.0

    def state(self, hip, dev, n, dtype, mixed):
        r, dr, v = ground_cloud(n, seed=1 + n, dtype=np_type(dtype))
        order = np.random.RandomState(SHUFFLE_SEED).permutation(n)
        rng = np.random.RandomState(n)
        return {"r": r[order], "v": v[order], "dr": dr[order], "dv": rng.normal(size=(n, 3)), "E": 1.0 + rng.uniform(size=n)}

    def call(self, dev, n_pass):
        return tuple(dev.surface_reflect(RADIUS, GROUND_CENTER, 0.5, "lambertian", C, SEED, n_pass))

    def check(self, before, after, answer, n_pass, what):
        from test_gpu_surface import W_MAX
        return W.check_surface(before, after, answer, RADIUS, GROUND_CENTER, 0.5, "lambertian", C, SEED, n_pass, W_MAX, what)


class Phase:
    name, touched, also, second_pass_floor = "phase", "redirected", (), 0.1

    def state(self, hip, dev, n, dtype, mixed):
        v, dv = phase_cloud(n, seed=1 + n, dtype=np_type(dtype))
        rng = np.random.RandomState(n)
        return {"r": rng.normal(size=(n, 3)), "v": v, "dr": rng.normal(size=(n, 3)), "dv": dv, "E": 1.0 + rng.uniform(size=n)}

    def call(self, dev, n_pass):
        return dev.phase_redirect("hg", 0.85, C, SEED, n_pass)

    def check(self, before, after, answer, n_pass, what):
        return W.check_phase(before, after, answer, "hg", 0.85, C, SEED, n_pass, what)


class Absorb:
    name, touched, also, second_pass_floor = "absorb", "interacted", (), 0.1

    def case(self):
        from test_gpu_scatter_absorb import CASES, CENTER
        omega0, edges, E_bins = CASES["layers3_E"]
        return omega0, edges, CENTER, E_bins

    def state(self, hip, dev, n, dtype, mixed):
        from test_gpu_scatter_absorb import GROUPS, scattered_state
        s = scattered_state(dev, hip, n, dtype)                        # a source, a Newton step and a scatter step, on the device
        up = {g: np.stack(s[g], 1) for g in GROUPS}
        up["E"] = s["E"]
        return up

    def call(self, dev, n_pass):
        omega0, edges, center, E_bins = self.case()
        return dev.absorb_scattered(omega0, edges, center, E_bins, SEED, n_pass)

    def check(self, before, after, answer, n_pass, what):
        omega0, edges, center, E_bins = self.case()
        ref = W.check_absorb(before, after, answer, omega0, edges, center, E_bins, SEED, n_pass, what)
        assert 0 < answer[1] < answer[0] and np.sum(answer[3]) > 0, what
        return ref


class Layered:
    name, touched, also, second_pass_floor = "layered", "redirected", (), 0.1
    laws, weights, edges = layered_cases()["table+rayleigh"]           # a table and a law mixed in one layer, the law alone in another

    def state(self, hip, dev, n, dtype, mixed):
        from test_layered_phase_gpu import state_of
        return state_of(n, dtype)

    def call(self, dev, n_pass):
        from absorb_reference import CENTER
        checked, _, cum, edges, center = light._check_layered_phase(self.laws, self.weights, self.edges, CENTER)
        return dev.phase_layered(checked, cum, edges, center, C, SEED, n_pass)

    def check(self, before, after, answer, n_pass, what):
        from absorb_reference import CENTER
        ref = check_layered(before, after, answer, self.laws, self.weights, self.edges, CENTER, C, SEED, n_pass, what)
        assert min(answer[2]) > 0 and min(answer[3]) > 0 and answer[1] < answer[0], what       # every layer and law; some in no layer
        return ref


class Reemit:
    second_pass_floor = 0.1

    def __init__(self, population, touched, also=()):
        self.population, self.touched, self.also, self.name = population, touched, also, "reemit_" + population

    def state(self, hip, dev, n, dtype, mixed):
        from test_reemit_gpu import state_of
        return state_of(n, dtype, self.population, mixed)[0]           # (mixed: the scene's own scrambled ids and plain Objects)

    def call(self, dev, n_pass):
        from test_reemit_gpu import call
        return call(dev, LAYERED, n_pass)

    def check(self, before, after, answer, n_pass, what):
        ref = check_reemit(before, after, answer, LAYERED, SEED, n_pass, what, W.photons(before))
        assert W.same_bits(before["kind"], after["kind"]) and 0 < answer[1] < answer[0], what
        return ref


# Re-emission's mask.  With a third at rest: the parked, who take the ballots -- and, without the 10 % of (a), the re-emitted, the
# lanes that stay in the body behind ``if (!go) continue`` (a second pass re-emits a twenty-fifth of the slots: the layers of eta 1
# are empty by then).  With everybody at rest: the re-emitted.
WRITERS = [Ground(), Phase(), Absorb(), Layered(), Reemit("every_third", "parked", also=("reemitted",))]
by_writer = pytest.mark.parametrize("sweep", WRITERS, ids=[s.name for s in WRITERS])


def sweep_and_check(hip, dev, cap, sweep, n, dtype, mixed=False, passes=1):
    """``passes`` consecutive sweeps of ``sweep``'s population of ``n`` slots, each against the restatement of the state downloaded
    before it.  The working fractions from ``cap`` on, pass by pass."""
    assert n > cap
    up = dict(sweep.state(hip, dev, n, dtype, mixed), id_base=ID_BASE)
    if mixed and "id" not in up:                                       # ids in scrambled order, every 7th a plain Object: both are staged
        up["id"] = ID_BASE + np.random.RandomState(5).permutation(n).astype(np.int64)
        up["kind"] = np.where(np.arange(n) % 7 == 0, hip.KIND_OBJECT, hip.KIND_PHOTON).astype(np.uint8)
    dev.store_alloc(n + ROOM, dtype)
    dev.upload_state(up)
    assert dev.is_uniform() == (not mixed) and dev.count == n and dev.capacity > n
    before, fractions = W.snapshot(dev), []
    for n_pass in range(N_PASS, N_PASS + passes):
        what = "%s n=%d %s%s pass %d" % (sweep.name, n, dtype, " mixed" if mixed else "", n_pass)
        answer = sweep.call(dev, n_pass)
        after = W.snapshot(dev)
        ref = sweep.check(before, after, answer, n_pass, what)
        assert dev.count == n, what
        mask = ref[sweep.touched]
        if mixed:
            assert not mask[np.asarray(before["kind"]) == hip.KIND_OBJECT].any(), what         # plain Objects are never touched
        fractions.append(has_work(mask, cap, what, 0.1 if n_pass == N_PASS else sweep.second_pass_floor))
        for other in sweep.also:                                       # (b), (c) and somebody at work, whatever their share
            has_work(ref[other], cap, "%s [%s]" % (what, other), floor=0.0)
        before = after
    return fractions


@pytest.mark.parametrize("size, dtype", SIZES)
@by_writer
def test_a_writer_past_one_trip(hip, dev, cap, sweep, size, dtype):
    """N2: two trips, a ragged last wave, a last tile that is not full -- and in f64 a second pass on what the first left behind:
    the first pass's writes of a later trip are the second's inputs.  N3: three trips, workgroups whose trip counts differ."""
    sweep_and_check(hip, dev, cap, sweep, slots(cap, size), dtype, passes=2 if (size, dtype) == ("N2", "f64") else 1)


@by_writer
def test_a_writer_past_one_trip_with_staged_ids_and_kinds(hip, dev, cap, sweep):
    """Scrambled explicit ids and plain Objects among the photons: the ``ids`` and ``kind`` arrays are read past one trip."""
    sweep_and_check(hip, dev, cap, sweep, slots(cap, "N2"), "f64", mixed=True)


def test_reemission_past_one_trip_with_everybody_at_rest(hip, dev, cap):
    sweep_and_check(hip, dev, cap, Reemit("all", "reemitted"), slots(cap, "N2"), "f64")


# ------------------------------------------------------------------------------------------------ the detector's image
@pytest.mark.parametrize("size, dtype", SIZES)
def test_the_detector_s_image_past_one_trip(hip, cap, size, dtype):
    from detector_reference import configs, scene
    from test_tally_detector_gpu import check, uploaded
    name = "aligned_33x17_bands"
    cfg, n = configs()[name], slots(cap, size)
    st = scene(n, dtype, name)
    what = "detector %s n=%d %s" % (name, n, dtype)
    seen = light._detector_seen(st[0], st[1], cfg["position"], cfg["frame"], cfg["radius"], cfg["x_edges"], cfg["y_edges"])[1]
    has_work(seen, cap, what)
    d = uploaded(hip, st, dtype, capacity=n + ROOM)
    try:
        counts, image = check(d, st, cfg, what)                        # the two counts and every cell of the image, equal
        assert counts[1] == seen.sum() and 0 < image.sum() < counts[1] and np.count_nonzero(image) > image.size // 2, what
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ the source
@pytest.mark.parametrize("size, dtype", SIZES)
def test_the_source_past_one_trip(hip, dev, cap, size, dtype):
    """The sweep writes every slot: those from CAP on are written, and are the restatement's like all the others."""
    from test_gpu_source import C as C_SOURCE, GEOMETRY, SEED as SEED_SOURCE, check_source, fill, src_of
    geometry, n = "oblique_far", slots(cap, size)
    origin, direction, radius = GEOMETRY[geometry]
    src = src_of("cone", "gaussian", origin, direction, radius)
    dev.store_alloc(n + ROOM, dtype)
    fill(dev, hip, n, ID_BASE)
    dev.apply_source(src, C_SOURCE, SEED_SOURCE)
    assert dev.count == n and dev.is_uniform()
    r, v = check_source(dev, src, ID_BASE, "cone", "gaussian", geometry, dtype)
    assert len(r) == n and r[cap:].any(axis=1).all() and v[cap:, 1:].any(axis=1).all()      # the fill left r = 0 and v = (c, 0, 0)
