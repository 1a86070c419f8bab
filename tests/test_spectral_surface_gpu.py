"""GPU: SpectralSurfaceStep (pcl_step_ground_spectral, light.SpectralSurfaceStep).

* ``Device.ground_spectral`` against the numpy restatement (light._spectral_bounce): a state that is uploaded explicitly
  (tests/spectral_surface_reference.py: ``scene`` -- tests/surface_reference.py's cloud, every even slot's move ending inside the
  sphere, energies between 1 and 3 with the special ones on and beside the bands' edges), downloaded before and after the call.
  Decisions, the four counts, both rows by band, parked lanes and mirrored lanes WITHOUT A TOLERANCE; lambertian lanes within
  writer_reference's bounds for the project's sin / cos (DIR_ULP, lambertian_position_bound), nothing looser.  N at the wave and tile
  edges, fp64 and fp32 stores, 1, 3 and 1024 bands, two consecutive passes.
* the grey ground on the device: one band that holds every energy, specular 0 and 1, against ``Device.surface_reflect`` on a copy of
  the same store -- r, v, dr, dv and E identical bits.
* scrambled ids and plain Objects; one size past the grid's first trip (``CAP + 2049 + 13``) with a second pass; the refusals; an
  empty store; no store; a device group of two shards; the step through ``Simulation`` with a shell tally in front, cl_on=True and
  cl_on=False.

Every case of 64 slots or more asserts on the restatement's masks that somebody reflects diffusely, somebody is mirrored, somebody
is absorbed in a band, somebody is out of band and somebody is not hit.  The scene's seed is 1 (the scene draws from ``seed + n``
and ``seed + 7 n``), the draws' SEED 0x5EED5A7F; a uniform store's ids are ``ID_BASE + slot``, a mixed store's the scene's scrambled
ones.  The restatement alone (no device) gives, as shares of all slots (diffuse / mirrored / absorbed in a band / out of band / not
hit), with the ids of a uniform store and pass 1:

    n = 64     B = 1: .078 .047 .109 .188 .578    B = 3: .109 .016 .109 .188 .578    B = 1024: .016 .031 .188 .188 .578
    n = 65     B = 1: .077 .092 .077 .185 .569    B = 3: .092 .031 .123 .185 .569    B = 1024: .046 .046 .154 .185 .569
    n = 2047   B = 1: .079 .077 .119 .155 .570    B = 3: .101 .043 .130 .155 .570    B = 1024: .059 .041 .175 .155 .570
    n = 2048   B = 1: .080 .078 .112 .160 .570    B = 3: .097 .048 .125 .160 .570    B = 1024: .052 .040 .179 .160 .570
    n = 2049   B = 1: .074 .078 .111 .167 .570    B = 3: .087 .043 .133 .167 .570    B = 1024: .055 .047 .161 .167 .570
    n = 4097   B = 1: .079 .080 .111 .161 .570    B = 3: .089 .044 .136 .161 .570    B = 1024: .051 .051 .167 .161 .570

(the fp32 scene gives the same shares to three digits; .016 of 64 is one photon).  Three bands elsewhere: the mixed stores, scrambled
ids and pass 6, .108 .031 .092 .169 .600 at 65 slots and .077 .043 .123 .160 .597 at 2049; the unsharded store of the group case, 6221
slots and pass 4, .087 .056 .134 .154 .570; the trip case, 526 350 slots and pass 3, .091 .050 .132 .157 .570.  The store-state cases
(tests/test_spectral_surface_gpu_store_states.py) and the ``Simulation`` case need a history on the device, so their shares cannot be
worked out without one: they assert the same on the restatement of the state they download (the ``Simulation`` case: of the pass in
which most photons come down), and the run prints the shares.  The two-rank case keeps no state in its workers and reads the five
outcomes off the all-reduced counts.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import light
from spectral_surface_reference import (BAD_CALLS, C, CENTER, COUNTS, FIELDS, ID_BASE, RADIUS, SEED, abi_args, assert_every_outcome,
                                        check_spectral, config, scene)
from writer_reference import same_bits

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 2047, 2048, 2049, 4097]                        # wave and tile edges
BANDS = [1, 3, 1024]
ROOM = 300                                                             # capacity beyond N


@pytest.fixture(scope="module")
def hip():
    from physicl_amd import _hip
    return _hip


@pytest.fixture(scope="module")
def dev(hip):
    d = hip.Device(0)
    yield d
    d.close()


def np_type(dtype):
    return np.float32 if dtype == "f32" else np.float64


def upload(dev, n, dtype, B=3, mixed=False, special=True):
    """The scene in a fresh store; ``mixed``: its scrambled ids and plain Objects as well.  (the downloaded state, who is a photon)"""
    s = scene(n, np_type(dtype), B=B, special=special)
    up = {f: s[f] for f in FIELDS}
    up.update(E=s["E"], id_base=ID_BASE)
    photon = None
    if mixed:
        up.update(id=s["id"], kind=s["photon"].astype(np.uint8))
        photon = s["photon"]
    dev.store_alloc(n + ROOM, dtype)
    dev.upload_state(up)
    return dev.download_state(), photon


def call(dev, cfg, n_pass, seed=SEED):
    return dev.ground_spectral(cfg["radius"], cfg["E_edges"], cfg["albedo"], cfg["specular"], cfg["center"], C, seed, n_pass)


def sweep_and_check(dev, before, cfg, n_pass, what, photon=None):
    answer = call(dev, cfg, n_pass)
    after = dev.download_state()
    return answer, after, check_spectral(before, after, answer, cfg, SEED, n_pass, what, photon)


@pytest.mark.parametrize("B", BANDS)
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_every_slot_against_the_numpy_restatement(dev, n, dtype, B):
    cfg = config(B)
    before, _ = upload(dev, n, dtype, B)
    for n_pass in (1, 2):                                              # two consecutive passes: the pass counter moves
        what = "spectral n=%d %s B=%d pass %d" % (n, dtype, B, n_pass)
        (counts, by_refl, by_gone), before, ref = sweep_and_check(dev, before, cfg, n_pass, what)
        assert dev.count == n and dev.is_uniform()
        assert len(by_refl) == len(by_gone) == B and by_refl.sum() == counts[0] and by_gone.sum() == counts[1] - counts[3]
        if n >= 64 and n_pass == 1:
            assert_every_outcome(ref, what)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("n", [65, 2049])
def test_a_store_that_is_not_uniform(dev, hip, n, dtype):
    cfg = config(3)
    before, photon = upload(dev, n, dtype, mixed=True)
    what = "spectral mixed n=%d %s" % (n, dtype)
    (counts, _, _), after, ref = sweep_and_check(dev, before, cfg, 6, what, photon)
    assert not dev.is_uniform() and counts[0] > 0
    obj = dev.download_kind() == hip.KIND_OBJECT
    assert np.array_equal(obj, np.arange(n) % 17 == 0) and not ref["hit"][obj].any()       # kinds are never written, Objects never hit
    assert_every_outcome(ref, what)                                    # (both sizes hold 64 slots or more)
    # the draws follow the ids: the same state with ids in store order decides otherwise
    upload(dev, n, dtype)
    other = call(dev, cfg, 6)
    assert not same_bits(np.stack(dev.download_state()["v"], 1), np.stack(after["v"], 1)) and other[0][0] > 0


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_past_the_first_trip(dev, dtype):
    """``CAP + 2049 + 13`` slots: two trips, a ragged last wave, a last tile that is not full; then a second pass, the pass counter
    advanced, on what the first left behind."""
    cap = dev.info()["compute_units"] * 8 * 256
    n = cap + 2049 + 13
    cfg = config(3)
    before, _ = upload(dev, n, dtype)
    what = "spectral past one trip n=%d %s" % (n, dtype)
    (counts, by_refl, by_gone), after, ref = sweep_and_check(dev, before, cfg, 3, what)
    assert_every_outcome(ref, what)
    tail = slice(cap, None)                                            # the second trip had work of every kind
    assert ref["hit"][tail].sum() > 500 and ref["mirrored"][tail].sum() > 50 and ref["out_of_band"][tail].sum() > 50
    assert (ref["reflected"] & ~ref["mirrored"])[tail].sum() > 50 and min(by_refl) > 0
    assert by_gone[0] > 0 and by_gone[1] == 0 and by_gone[2] > 0       # (the second band's albedo is 1)
    sweep_and_check(dev, after, cfg, 4, what + ", second pass")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("albedo", [1.0, 0.4, 0.0])
@pytest.mark.parametrize("specular, mode", [(0.0, "lambertian"), (1.0, "specular")])
def test_one_band_that_holds_every_energy_is_the_grey_ground_bit_for_bit(dev, specular, mode, albedo, dtype):
    n, n_pass = 4097, 5
    s = scene(n, np_type(dtype), special=False)
    up = {f: s[f] for f in FIELDS}
    up.update(E=s["E"], id_base=ID_BASE)
    states, answers = [], []
    for spectral in (False, True):                                     # the same store twice, the same seed and pass
        dev.store_alloc(n + ROOM, dtype)
        dev.upload_state(up)
        if spectral:
            counts, by_refl, by_gone = dev.ground_spectral(RADIUS, [0.5, 3.5], [albedo], [specular], CENTER, C, SEED, n_pass)
            assert counts[3] == 0 and counts[2] == (counts[0] if mode == "specular" else 0)
            assert by_refl.tolist() == [counts[0]] and by_gone.tolist() == [counts[1]]
            answers.append((int(counts[0]), int(counts[1])))
        else:
            answers.append(tuple(dev.surface_reflect(RADIUS, CENTER, albedo, mode, C, SEED, n_pass)))
        states.append(dev.download_state())
    assert answers[0] == answers[1] and sum(answers[0]) == (n + 1) // 2
    assert (answers[0][1] == 0) if albedo == 1.0 else (answers[0][0] == 0) if albedo == 0.0 else min(answers[0]) > 500
    for f in FIELDS:
        for k in range(3):
            assert same_bits(states[0][f][k], states[1][f][k]), (f, k)
    assert same_bits(states[0]["E"], states[1]["E"]) and np.array_equal(states[0]["id"], states[1]["id"])


def test_refused_calls_an_empty_store_and_no_store(dev, hip):
    before, _ = upload(dev, 300, "f64")
    for kw in BAD_CALLS:
        keep, args, counts, bands = abi_args(**kw)
        assert dev.lib.pcl_step_ground_spectral(dev.ctx, *args) == -2, kw
        assert (counts is None or (counts == -7).all()) and (bands is None or (bands == -7).all()), kw
    after = dev.download_state()
    for f in FIELDS:
        for k in range(3):
            assert same_bits(after[f][k], before[f][k]), f
    keep, good, counts, bands = abi_args()                             # four counts and two rows of three, no more
    assert dev.lib.pcl_step_ground_spectral(dev.ctx, *good) == 0 and (counts[:4] >= 0).all() and counts[4:].tolist() == [-7, -7]
    assert (bands[:6] >= 0).all() and bands[6:].tolist() == [-7, -7] and counts[0] + counts[1] > 0
    assert bands[:3].sum() == counts[0] and bands[3:6].sum() == counts[1] - counts[3]
    dev.set_count(0, 0)
    counts, by_refl, by_gone = call(dev, config(3), 1)
    assert counts.tolist() == [0] * 4 and by_refl.tolist() == by_gone.tolist() == [0] * 3
    bare = hip.Device(0)
    with pytest.raises(hip.HipError) as e:
        call(bare, config(3), 1)
    assert e.value.code == -3
    bare.close()


def test_device_group_gives_the_unsharded_store(dev, hip):
    n = 3 * 2048 + 77
    cfg = config(3)
    before, _ = upload(dev, n, "f64")
    whole, _, ref = sweep_and_check(dev, before, cfg, 4, "spectral unsharded n=%d" % n)    # the unsharded store is the restatement's
    assert_every_outcome(ref, "spectral group n=%d" % n)
    with hip.DeviceGroup([0, 0]) as g:
        g.store_alloc(n)
        g.fill_photons(n, ID_BASE, C, 1.0, 2.0, SEED)
        for i in range(2):                                             # the shards' rows through their own contexts
            lo, hi = g.shard(n, i)
            ctx = hip.c_void_p()
            hip.check(g.lib.pcl_group_ctx(g.g, i, hip.byref(ctx)))
            rows = [(f, before[name][f - hip.FIELD_GROUPS[name][0]]) for name in FIELDS for f in hip.FIELD_GROUPS[name]] + [(hip.E, before["E"])]
            for f, row in rows:
                col = np.ascontiguousarray(row[lo:hi])
                hip.check(g.lib.pcl_store_upload(ctx, f, col.ctypes.data, 0, hi - lo))
        got = call(g, cfg, 4)
        for a, b in zip(got, whole):                                   # the same photons meet the same fate, and the rows add
            assert a.tolist() == b.tolist()
        assert min(whole[0]) > 0 and min(whole[1]) > 0 and whole[2].tolist()[1] == 0 < min(whole[2][[0, 2]])    # (the second band's albedo is 1)
        for f in range(hip.E + 1):                                     # the union of the shards is the unsharded run, bit for bit
            assert same_bits(g.download(f), dev.download(f)), f
        with pytest.raises(hip.HipError) as e:
            call(g, dict(cfg, albedo=[0.5, 1.5, 0.5]), 4)
        assert e.value.code == -2


# ------------------------------------------------------------------------------------------------ through Simulation
N_SIM, PASSES = 5000, 16               # no medium: a lamp one unit above the ground, whose light comes down within ten moves
STEP = 0.5                             # length of a move, in units of which the sphere has radius 10
DT = STEP / C
EDGES = [1.25, 1.75, 2.25, 2.75]       # the photons' energies reach from 1 to 3


ALBEDO_SIM, SPECULAR_SIM = [0.05, 1.0, 0.5], [1.0, 0.5, 0.0]


class BeforeTheGround(phys.DeviceStep):
    """In front of the ground: the store as the ground will meet it, pass by pass."""
    _fuse_role = None

    def __init__(self):
        self.states = []

    def _device_run(self, sim):
        self.states.append({f: sim.download(f) for f in ("r", "dr", "v", "E", "id")})


def ground_sim(cl_on):
    """tests/test_gpu_surface.py's scene over a spectral ground: the rows of the step and of the shell in front of it, the final
    state, the launch note, the step, and the states the ground met."""
    sim = phys.Simulation(cl_on=cl_on, rng="philox", seed=7, exit=lambda s: len(s.ts) >= PASSES)
    src = phys.light.PhotonSource(origin=CENTER + [RADIUS + 1.0, 0.0, 0.0], angular="isotropic")
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    shell = phys.light.ShellCrossingMeasureStep(None, [RADIUS], center=CENTER)
    step = phys.light.SpectralSurfaceStep(RADIUS, ALBEDO_SIM, EDGES, CENTER, specular=SPECULAR_SIM)
    look = BeforeTheGround()
    sim.add_step(3, shell)
    sim.add_step(4, look)
    sim.add_step(5, step)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    rows = [[int(x) for x in list(row)[1:5]] + [row[5].tolist(), row[6].tolist()] for row in step.data]
    came_in = [int(row[3][0]) for row in shell.data]
    state = {f: sim.download(f) for f in ("r", "v", "dr", "dv", "E")}
    note = sim.launch_note
    sim.close(download=False)
    return rows, came_in, state, note, step, look.states


def test_the_shell_in_front_counts_what_the_ground_decides():
    rows, came_in, state, note, step, met = ground_sim(True)
    assert len(rows) == PASSES == step._pass == len(met)
    # the restatement of every pass, on the store the ground met: its counts and rows are the step's, and in the pass in which most
    # photons come down somebody reflects diffusely, is mirrored, is absorbed in a band, is out of band and is not hit
    busiest = int(np.argmax(came_in))
    for k, (s, row) in enumerate(zip(met, rows)):
        ref = light._spectral_bounce(s["r"], s["dr"], s["v"], s["E"], np.ones(N_SIM, dtype=bool), s["id"], RADIUS, CENTER, ALBEDO_SIM,
                                     SPECULAR_SIM, EDGES, light._c_h_literals()[0], 7, 1 + k)
        assert [int(ref[name].sum()) for name in COUNTS] == row[:4], k
        assert ref["reflected_by_band"].tolist() == row[4] and ref["absorbed_by_band"].tolist() == row[5], k
        if k == busiest:
            print("pass %d:" % (1 + k), assert_every_outcome(ref, "Simulation, pass %d" % (1 + k)))
    for (refl, gone, mirrored, none, by_refl, by_gone), inn in zip(rows, came_in):
        assert inn == refl + gone and sum(by_refl) == refl and sum(by_gone) == gone - none and mirrored <= refl
        assert by_gone[1] == 0                                         # albedo 1: nobody is absorbed in the second band
    sums = np.sum([row[:4] for row in rows], axis=0)
    print("the spectral ground's counts over %d passes:" % PASSES, dict(zip(COUNTS, sums.tolist())))
    assert sums[0] > 100 and sums[1] > 100 and 0 < sums[2] < sums[0] and 0 < sums[3] < sums[1]
    assert "one launch per light step" in note and ("SpectralSurfaceStep" in note or "ShellCrossingMeasureStep" in note)
    assert [getattr(step, name) for name in COUNTS] == rows[-1][:4]
    d = state["r"] - CENTER
    assert np.min((d * d).sum(axis=1)) >= RADIUS * RADIUS * (1 - 1e-12)                    # nobody is left inside the sphere
    assert int(np.sum(~state["v"].any(axis=1))) == sums[1]                                 # the absorbed stay, at rest
    # the same script under the reference's Python semantics: the step reads no dv rule
    rows_py, came_in_py, state_py, _, _, _ = ground_sim(False)
    assert rows_py == rows and came_in_py == came_in
    for f in state:
        assert same_bits(state_py[f], state[f]), f


@pytest.mark.filterwarnings("ignore::pytest.PytestUnhandledThreadExceptionWarning")     # (the simulation's thread keeps the error and ends on it)
def test_a_device_resident_simulation_with_two_grounds_is_refused():
    """Words 8 and 9 are the ground's: the first pass raises, on the device path as on the host path, before anything is swept."""
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, exit=lambda s: len(s.ts) >= 2)
    src = phys.light.PhotonSource(origin=CENTER + [RADIUS + 1.0, 0.0, 0.0], angular="isotropic")
    sim.add_objs(phys.light.generate_photons_bulk(256, min=1.0, max=3.0, seed=7, source=src))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(DT)))
    sim.add_step(1, phys.newton.NewtonianKinematicsStep())
    grey = phys.light.SurfaceReflectStep(2 * RADIUS, center=CENTER)
    step = phys.light.SpectralSurfaceStep(RADIUS, ALBEDO_SIM, EDGES, CENTER, specular=SPECULAR_SIM)
    sim.add_step(3, grey)
    sim.add_step(4, step)
    sim.start()
    sim.join()
    assert isinstance(sim.error, ValueError) and "one ground" in str(sim.error) and "SurfaceReflectStep" in str(sim.error)
    assert step._pass == 0 and step.data == []
    sim.close(download=False)
