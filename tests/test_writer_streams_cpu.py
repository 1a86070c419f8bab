"""CPU: the Philox streams of the writer steps (tally.WriterStep and its twelve steps in light.py).

Every writer sweep draws from the Philox4x32-10 block with the counter ``(id_lo, id_hi, n_pass, word)`` and the key ``(seed_lo,
seed_hi)``; ``word`` is a constant per kind of draw.  Three things are held here:

* ``light._philox_block`` -- the block every numpy restatement draws from -- against a Philox on Python integers
  (scatter_layered_reference.philox) and the three published known answers of Philox4x32-10, over ids, seeds and pass counters that
  use every bit of their words, in every counter word include/physicl_hip.h lists as taken;
* the counter rule: steps that share a counter word (a family) in one pass get the counters ``(_pass - 1) * m + j + 1``: disjoint
  over the family's members, ``_pass`` itself for a member alone, refused before it wraps;
* independence: two steps of one kind in one pass, on host-resident objects of a ``Simulation``.  Among the ``n`` photons the
  second step finds exposed and the first left untouched, its hits ``k`` are binomial(n, p2): ``|k - n p2| <= 5 sqrt(n p2 (1 - p2))``
  (five standard deviations of the binomial law: nothing measured).  With counters in lock-step both steps drew the same number for
  a photon, and a photon the first missed (u >= p1) was hit by the second iff p1 <= u < p2: never with p2 <= p1.  For the two
  steps that draw a direction, among the photons both hit no direction is repeated bit for bit, and with ``mu = 1 - 2u`` uniform
  on [-1, 1] (variance 1/3) the mean of ``mu1 * mu2`` over n photons has the standard deviation ``1 / (3 sqrt(n))``: five of them.
  The seeds are such that the Python-integer Philox alone meets each bound, which is checked before the steps are looked at.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
from physicl_amd import light, tally
from scatter_layered_reference import philox

C = light._c_h_literals()[0]
TAKEN_WORDS = [0, 1, 2, 3, 4, 5] + list(range(8, 25))                  # include/physicl_hip.h: scatter 0 and 1, fill and source 2..5, 8..24
IDS = [0, 1, 2**32 - 1, 2**32, 7_000_000_001, 2**63 - 1]
SEEDS = [0, 2**32 - 1, 2**32, 0x5EED5A7F + (0xC0FFEE << 40), 2**64 - 1]
N_PASSES = [0, 1, 2**31 - 1, 2**31, 2**32 - 1]
N = 16385
DT = 0.5 / C


# ------------------------------------------------------------------------------------------------ the block
def u53(a, b):
    """include/physicl_hip.h (pcl_store_apply_source): 53 bits of two words as a double in [0, 1)."""
    return float((a >> 5) * (1 << 26) + (b >> 6)) * (1.0 / 9007199254740992.0)


KNOWN = [  # (counter, key, the block): the known answers of the Random123 distribution (kat_vectors, philox4x32 10)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter, key, block", KNOWN)
def test_the_published_known_answers(counter, key, block):
    want = (u53(block[0], block[1]), u53(block[2], block[3]))
    id_, seed = counter[0] | (counter[1] << 32), key[0] | (key[1] << 32)
    assert philox(id_, seed, counter[2], counter[3]) == want
    got = light._philox_block(np.array([id_], dtype=np.uint64), seed, counter[2], counter[3])
    assert (float(got[0][0]), float(got[1][0])) == want


def test_the_numpy_block_is_the_integer_block_at_full_width():
    ids = np.array(IDS, dtype=np.uint64)
    for seed in SEEDS:
        for n_pass in N_PASSES:
            for word in TAKEN_WORDS:
                a, b = light._philox_block(ids, seed, n_pass, word)
                want = [philox(i, seed, n_pass, word) for i in IDS]
                assert [(float(x), float(y)) for x, y in zip(a, b)] == want, (seed, n_pass, word)
    a, _ = light._philox_block(np.array(IDS, dtype=np.int64), SEEDS[3], 7, 17)          # ids as the store holds them: int64
    assert a.tolist() == [philox(i, SEEDS[3], 7, 17)[0] for i in IDS]


@pytest.mark.parametrize("word", TAKEN_WORDS)
def test_the_upper_half_of_the_key_and_the_top_bit_of_the_pass_counter_are_used(word):
    ids = np.array(IDS, dtype=np.uint64)
    for seed in (0, 0x5EED5A7F, 2**32 - 1, 7 << 32):
        for n_pass in (0, 1, 7, 2**31 - 1):
            base = np.stack(light._philox_block(ids, seed, n_pass, word))
            hi_key = np.stack(light._philox_block(ids, seed + 2**32, n_pass, word))
            hi_pass = np.stack(light._philox_block(ids, seed, n_pass + 2**31, word))
            assert (base != hi_key).all() and (base != hi_pass).all() and (hi_key != hi_pass).all(), (seed, n_pass)


# ------------------------------------------------------------------------------------------------ the counter rule
def photon_objects(r, v, dv, E, dr=None):
    out = []
    for k in range(len(E)):
        o = phys.light.PhotonObject(E=np.double(E[k]), v=phys.light.c * [1, 0, 0])
        o.r = phys.Measurement(np.array(r[k]), "m**1")
        o.v, o.dv = np.array(v[k]), np.array(dv[k])
        o.dr = phys.Measurement(np.array(np.zeros(3) if dr is None else dr[k]), "m**1")
        out.append(o)
    return out


def a_few(n=12):
    rng = np.random.RandomState(3)
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    return photon_objects(2.0 * d, C * d, C * d, rng.uniform(1.0, 3.0, size=n), dr=0.5 * d)


class HostSim:                                                         # what the host path asks of a simulation (no device here)
    _residency, _batch, comm, launch_note = "host", None, None, None
    t, seed, dt = 0.25, 7, np.double(DT)

    def __init__(self, objs, steps=None):
        self.objects = objs
        if steps is not None:
            self.steps = dict(enumerate(steps))

    def _py_semantics(self):
        return False

    def _dt_code(self):                                                # (the device path asks for these two ahead of its sweep)
        return float(self.dt)

    def _k_wanted(self):
        return 32


def gas():
    return phys.light.PathAbsorptionStep(0.01 / (C * DT))


@pytest.mark.parametrize("members", [1, 2, 3])
def test_the_members_of_a_family_count_through_one_another(members):
    steps = [gas() for _ in range(members)]
    others = [phys.light.AbsorptionStep(0.9), phys.light.ReemissionStep(eta=0.5), phys.light.LayeredScatterStep(0.5)]   # not of the family
    order = [x for pair in zip(steps, others) for x in pair]
    sim = HostSim(a_few(), [phys.newton.NewtonianKinematicsStep()] + order)
    seen = [[] for _ in steps]
    for _ in range(8):
        for s in order:
            s.run(sim)
        for k, s in enumerate(steps):
            seen[k].append(s._n_pass)
    assert all(s._pass == 8 and s._family == (members, k) for k, s in enumerate(steps))
    assert all(s._n_pass == s._pass == 8 for s in order if s not in steps)          # alone in their families
    for k, mine in enumerate(seen):
        assert mine == [p * members + k + 1 for p in range(8)]
        for other in seen[k + 1:]:
            assert not set(mine) & set(other)
    assert sorted(x for mine in seen for x in mine) == list(range(1, 8 * members + 1))   # no counter is skipped either
    if members == 1:
        assert seen[0] == list(range(1, 9))


def test_a_step_without_a_step_list_counts_its_runs():
    class Bare:                                                        # a stand-in without ``steps``
        _residency, _batch, comm, launch_note = "host", None, None, None
        t, seed, dt, objects = 0.25, 7, np.double(DT), a_few()

        def _py_semantics(self):
            return False
    for step in (gas(), phys.light.SurfaceReflectStep(2.0, albedo=0.5), phys.light.LayeredScatterStep(0.5 / (C * DT))):
        for p in range(1, 9):
            step.run(Bare())
            assert (step._pass, step._n_pass, step._family) == (p, p, (1, 0))
    loose = gas()                                                      # a step the simulation's list does not hold
    loose.run(HostSim(a_few(), [gas(), gas()]))
    assert (loose._pass, loose._n_pass) == (1, 3) and loose._family == (3, 2)            # counted behind those it holds: no counter is shared


def twelve():
    """One step of every writer class of light.py, by a short name, in one order."""
    L = phys.light
    return {"ground": L.SurfaceReflectStep(2.0), "spectral": L.SpectralSurfaceStep(2.0, [0.5, 0.5], [1.0, 2.0, 3.0]),
            "phase": L.PhaseFunctionStep("hg", 0.5), "layered": L.LayeredPhaseStep(["rayleigh"]), "absorb": L.AbsorptionStep(0.5),
            "glass": L.RefractiveSurfaceStep(2.0, 1.5), "lamp": L.RecycleStep(L.PhotonSource()), "gas": gas(), "cloud": L.LayeredScatterStep(1.0),
            "grid": L.GridScatterStep(1.0, ("x",), [[-4.0, 0.0, 4.0]]), "box": L.BoxBoundaryStep((-4, -4, -4), (4, 4, 4)),
            "glow": L.ReemissionStep()}


def below(cls):
    return [c for sub in cls.__subclasses__() for c in [sub] + below(sub)]


def test_families_are_the_steps_that_share_a_counter_word():
    L = phys.light
    made = twelve()
    fam = {k: tally.writer_family(s) for k, s in made.items()}
    assert fam["ground"] == fam["spectral"] and fam["phase"] == fam["layered"]
    rest = [k for k in made if k not in ("spectral", "layered")]
    assert len(made) == 12 and len({fam[k] for k in rest}) == len(rest) == 10       # the others pairwise distinct: ten families
    assert fam["grid"] != fam["cloud"] and fam["box"] != fam["glass"]
    assert sorted(type(s).__name__ for s in made.values()) == sorted(c.__name__ for c in below(tally.WriterStep) if c.__module__ == light.__name__)
    assert all("_STREAM" in vars(c) for c in tally.WriterStep.__subclasses__() if c.__module__ == light.__name__)    # stated, not inherited

    class Haze(L.PathAbsorptionStep):                                  # a subclass draws from its parent's stream
        pass

    class Plume(L.GridScatterStep):
        pass
    assert tally.writer_family(Haze(0.5)) == fam["gas"] and tally.writer_family(Plume(1.0, ("x",), [[-4.0, 0.0, 4.0]])) == fam["grid"]


def test_a_writer_class_that_states_no_stream_is_refused_at_its_first_run():
    class Nameless(tally.WriterStep):
        def __init__(self):
            phys.MeasureStep.__init__(self, None)

        def _host_sweep(self, objs, ids, seed, prep):
            raise AssertionError("nothing is swept")
    step = Nameless()
    assert tally.WriterStep._STREAM is None
    with pytest.raises(TypeError, match="_STREAM"):
        step.run(HostSim(a_few(), [step]))
    assert (step._pass, step._n_pass, step._family) == (0, 0, None)

    class Named(Nameless):
        _STREAM = "named"
    assert tally.writer_family(Named()) == "named"


# (members of the family in the pass, the step's place among them) behind the first run of two steps of every class in one pass, in
# the order of twelve() twice: the two grounds share a stream and so do the two phase steps, every other class has its own
FAMILY_OF = {"ground": [(4, 0), (4, 2)], "spectral": [(4, 1), (4, 3)], "phase": [(4, 0), (4, 2)], "layered": [(4, 1), (4, 3)]}
# a second ground refuses a spectral one its run, a second phase step a layered one: their place is what the counter rule alone gives
REFUSED = {"spectral": "a simulation holds one ground", "layered": "a pass holds one phase step"}


def test_two_steps_of_every_class_in_one_pass_take_their_places():
    first, second = twelve(), twelve()
    order = [(k, j, s) for j, made in enumerate((first, second)) for k, s in made.items()]
    sim = HostSim(a_few(), [phys.newton.NewtonianKinematicsStep()] + [s for _, _, s in order])
    for k, j, s in order:
        if k in REFUSED:
            with pytest.raises(ValueError, match=REFUSED[k]):
                s.run(sim)
            assert (s._pass, s._family) == (0, None)
            s._next_pass(sim)                                          # what run() does behind the refusal
        else:
            s.run(sim)
    for k, j, s in order:
        assert s._family == FAMILY_OF.get(k, [(2, 0), (2, 1)])[j], (k, j)
        assert (s._pass, s._n_pass) == (1, s._family[1] + 1), (k, j)


@pytest.mark.parametrize("kind", ["ground", "glass"])
def test_a_pair_of_grounds_and_a_pair_of_glass_spheres_get_distinct_counters(kind):
    make = (lambda: phys.light.SurfaceReflectStep(1.5, albedo=0.5)) if kind == "ground" else (lambda: phys.light.RefractiveSurfaceStep(1.5, 1.5))
    a, b = make(), make()
    sim = HostSim(a_few(), [a, phys.light.AbsorptionStep(0.5), b])
    seen = []
    for _ in range(8):
        a.run(sim)
        b.run(sim)
        seen.append((a._n_pass, b._n_pass))
    assert seen == [(2 * p + 1, 2 * p + 2) for p in range(8)] and a._pass == b._pass == 8


def test_a_counter_that_would_wrap_is_refused_and_the_step_is_as_it_was():
    step = gas()
    sim = HostSim(a_few(), [step])
    step._pass = 2**32 - 2
    step.run(sim)                                                      # the last counter there is
    assert (step._pass, step._n_pass, len(step.data)) == (2**32 - 1, 2**32 - 1, 1)
    v = tally.vec3(sim.objects, "v")
    kept = (step.exposed, step.absorbed, step.absorbed_by_cell.tolist())
    for run in (lambda: step.run(sim), lambda: step._device_run(sim)):
        with pytest.raises(ValueError, match=r"2\*\*32 - 1"):
            run()
        assert (step._pass, step._n_pass, len(step.data)) == (2**32 - 1, 2**32 - 1, 1)
        assert kept == (step.exposed, step.absorbed, step.absorbed_by_cell.tolist()) and sim.launch_note is None
        assert np.array_equal(tally.vec3(sim.objects, "v"), v)
    a, b = gas(), gas()                                                # two members: the second reaches the end one run earlier
    sim = HostSim(a_few(), [a, b])
    a._pass = b._pass = 2**31 - 1
    a.run(sim)
    assert (a._pass, a._n_pass) == (2**31, 2**32 - 1)
    with pytest.raises(ValueError, match="member 2 of 2"):
        b.run(sim)
    assert (b._pass, b._n_pass, b.data) == (2**31 - 1, 0, [])


# ------------------------------------------------------------------------------------------------ independence
def five_sigma(n, p):
    return 5.0 * np.sqrt(n * p * (1.0 - p))


def cloud_of_photons(seed):
    """N moving photons about the origin: radii from 1 to 4, energies from 1 to 3, dv != 0 (they have interacted)."""
    rng = np.random.RandomState(seed)
    d, w = rng.normal(size=(N, 3)), rng.normal(size=(N, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    w /= np.sqrt((w * w).sum(axis=1))[:, None]
    return dict(r=rng.uniform(1.0, 4.0, size=N)[:, None] * d, v=C * w, dv=C * (w - d), E=rng.uniform(1.0, 3.0, size=N))


def simulation(seed, state, steps):
    """A ``Simulation`` with host-resident objects and no device: one is opened with ``cl_on=True`` only, and the steps that read the
    dv rule refuse the Python semantics ``cl_on=False`` stands for -- so the flag is set behind the constructor.  The steps run as
    host plugins (``step.run(sim)``), which never ask for the device."""
    sim = phys.Simulation(cl_on=False, seed=seed)
    sim.cl_on = True
    sim.add_objs(photon_objects(state["r"], state["v"], state["dv"], state["E"]))
    sim.dt = np.double(DT)
    for k, s in enumerate(steps):
        sim.add_step(k, s)
    return sim


def state_of(sim):
    objs = list(sim.objects)
    return dict(r=tally.vec3(objs, "r"), v=tally.vec3(objs, "v"), dv=tally.vec3(objs, "dv"), E=tally.photon_energies(objs, phys.light.PhotonObject)[0])


def run_in_order(sim, steps):
    """The states in front of the first step and behind every step."""
    states = [state_of(sim)]
    for s in steps:
        s.run(sim)
        states.append(state_of(sim))
    return states


def moving(state):
    return state["v"].any(axis=1)


def check_binomial(what, who, hit, p2, seed, n_pass, word, below=True, part=False):
    """``who``: the photons a step found exposed (``part``: some of them, picked by what the step in front did to them); ``hit``: the
    step's hits; ``below``: a hit is ``u < p2`` (or the absorber's ``not u < 1 - p2``).  The Python-integer Philox alone first: the
    seed is one for which the law holds."""
    at = np.flatnonzero(who)
    n = len(at)
    u = np.array([philox(int(i), seed, n_pass, word)[0] for i in at])
    k_ref = int(((u < p2) if below else ~(u < 1.0 - p2)).sum())
    k, bound = int(hit[at].sum()), five_sigma(n, p2)
    print("%s: n = %d, k = %d (the integer Philox: %d), n p2 = %.1f, bound %.1f" % (what, n, k, k_ref, n * p2, bound))
    assert n > N // 8, what
    assert abs(k_ref - n * p2) <= bound, (what, "the seed")
    assert k == k_ref and abs(k - n * p2) <= bound, what
    assert part or not hit[~who].any(), what
    return n, k


def check_directions(what, both, v1, v2):
    n = int(both.sum())
    same = (v1[both] == v2[both]).all(axis=1)
    mu1, mu2 = v1[both, 0] / C, v2[both, 0] / C                        # the direction is turned about (1, 0, 0): its x is mu = 1 - 2 u_a
    corr, bound = float(np.mean(mu1 * mu2)), 5.0 / (3.0 * np.sqrt(n))
    print("%s: hit by both %d, repeated directions %d, mean(mu1 mu2) = %.4f (bound %.4f)" % (what, n, same.sum(), corr, bound))
    assert n > N // 8 and not same.any(), what
    assert abs(corr) <= bound, what


def test_two_gases_absorb_independently():
    """Overlapping layers, bands that differ and overlap: p1 = 0.5 in every cell of the first gas, p2 = 0.75 in every cell of the second."""
    seed = 7
    k1, k2 = -np.log(0.5) / (C * DT), -np.log(0.25) / (C * DT)
    a = phys.light.PathAbsorptionStep(np.full((2, 2), k1), [1.0, 2.0, 3.5], (0, 0, 0), [1.0, 2.0, 2.6])
    b = phys.light.PathAbsorptionStep(np.full((2, 2), k2), [1.5, 3.0, 4.0], (0, 0, 0), [1.4, 2.2, 3.0])
    sim = simulation(seed, cloud_of_photons(1), [phys.newton.NewtonianKinematicsStep(), a, b])
    s0, s1, s2 = run_in_order(sim, [a, b])
    assert (a._n_pass, b._n_pass, a._pass, b._pass) == (1, 2, 1, 1)
    p1, p2 = (float(light._path_probability(k, C, DT)) for k in (k1, k2))
    assert abs(p1 - 0.5) < 1e-15 and abs(p2 - 0.75) < 1e-15
    ids = np.arange(N)
    ref1 = light._absorb_path(s0["r"], s0["v"], s0["dv"], s0["E"], np.ones(N, bool), ids, np.full((2, 2), p1), a.edges, a.center, a.E_edges, seed, 1)
    ref2 = light._absorb_path(s1["r"], s1["v"], s1["dv"], s1["E"], np.ones(N, bool), ids, np.full((2, 2), p2), b.edges, b.center, b.E_edges, seed, 2)
    gone1, gone2 = moving(s0) & ~moving(s1), moving(s1) & ~moving(s2)
    assert np.array_equal(gone1, ref1["absorbed"]) and np.array_equal(gone2, ref2["absorbed"])
    assert (a.exposed, a.absorbed, b.exposed, b.absorbed) == (ref1["exposed"].sum(), gone1.sum(), ref2["exposed"].sum(), gone2.sum())
    check_binomial("gas 1", ref1["exposed"], gone1, p1, seed, 1, 17)
    check_binomial("gas 2, everybody it exposed", ref2["exposed"], gone2, p2, seed, 2, 17)
    shared = ref1["exposed"] & ref2["exposed"]                         # exposed to both: the first missed them (they still move)
    assert not gone1[shared].any() and (ref2["exposed"] & ~ref1["exposed"]).sum() > N // 8
    check_binomial("gas 2, exposed to both", shared, gone2, p2, seed, 2, 17, part=True)


def test_two_gases_of_equal_strength():
    """p1 = p2 = 0.5, everybody exposed to both: in lock-step the second gas absorbed nobody."""
    seed = 7
    k = -np.log(0.5) / (C * DT)
    a, b = phys.light.PathAbsorptionStep(k), phys.light.PathAbsorptionStep(k)
    sim = simulation(seed, cloud_of_photons(2), [a, b])
    s0, s1, s2 = run_in_order(sim, [a, b])
    gone1, gone2 = moving(s0) & ~moving(s1), moving(s1) & ~moving(s2)
    assert a.exposed == N and b.exposed == N - a.absorbed == int(moving(s1).sum())
    check_binomial("equal gas 1", moving(s0), gone1, 0.5, seed, 1, 17)
    check_binomial("equal gas 2", moving(s1), gone2, 0.5, seed, 2, 17)
    assert abs((N - a.absorbed - b.absorbed) - N * 0.25) <= five_sigma(N, 0.25)          # survival (1 - p1)(1 - p2)


def test_two_absorbers_absorb_independently():
    """omega0 = 0.5, then 0.25: an interaction is an absorption with 1 - omega0 (the draw's sense: absorbed iff not u < omega0)."""
    seed = 11
    a, b = phys.light.AbsorptionStep(0.5), phys.light.AbsorptionStep(0.25)
    sim = simulation(seed, cloud_of_photons(3), [phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)), a, b])
    s0, s1, s2 = run_in_order(sim, [a, b])
    assert (a._n_pass, b._n_pass) == (1, 2)
    gone1, gone2 = moving(s0) & ~moving(s1), moving(s1) & ~moving(s2)
    assert a.interacted == N and b.interacted == N - a.absorbed and (a.absorbed, b.absorbed) == (gone1.sum(), gone2.sum())
    check_binomial("absorber 1", moving(s0), gone1, 0.5, seed, 1, 12, below=False)
    check_binomial("absorber 2", moving(s1), gone2, 0.75, seed, 2, 12, below=False)


def test_two_clouds_scatter_independently():
    """p = 0.5 each, everybody exposed; ``first`` is resolved by the steps: True, then False."""
    seed = 7
    k = -np.log(0.5) / (C * DT)
    a, b = phys.light.LayeredScatterStep(k), phys.light.LayeredScatterStep(k)
    sim = simulation(seed, cloud_of_photons(4), [phys.newton.NewtonianKinematicsStep(), a, b])
    s0, s1, s2 = run_in_order(sim, [a, b])
    assert (a.first, b.first, a._n_pass, b._n_pass) == (True, False, 1, 2) and a.exposed == b.exposed == N
    hit1, hit2 = (s0["v"] != s1["v"]).any(axis=1), (s1["v"] != s2["v"]).any(axis=1)
    assert (a.scattered, b.scattered) == (hit1.sum(), hit2.sum())
    check_binomial("cloud 1", np.ones(N, bool), hit1, 0.5, seed, 1, 23)
    check_binomial("cloud 2, whom cloud 1 missed", ~hit1, hit2, 0.5, seed, 2, 23, part=True)
    check_binomial("cloud 2, whom cloud 1 hit", hit1, hit2, 0.5, seed, 2, 23, part=True)
    check_directions("clouds", hit1 & hit2, s1["v"], s2["v"])
    at = np.flatnonzero(hit1 & hit2)[:64]                              # and x / c is the integer Philox's mu = 1 - 2 u_a, word 24
    for i in at:
        assert abs(s2["v"][i, 0] / C - (1.0 - 2.0 * philox(int(i), seed, 2, 24)[0])) < 1e-15
    assert not s1["dv"][~hit1].any() and np.array_equal(s2["dv"][~hit2], s1["dv"][~hit2])      # first: dv = 0 on a miss; not first: not written


def test_two_reemitters_draw_independently():
    """eta = 0.5 each, everybody parked in front of either: a black gas (p == 1) parks everybody again between the two, so both
    can hit one photon in one pass."""
    seed = 11
    a, b = phys.light.ReemissionStep(eta=0.5), phys.light.ReemissionStep(eta=0.5)
    park = phys.light.PathAbsorptionStep(1e3 / (C * DT))
    state = cloud_of_photons(5)
    state["v"], state["dv"] = np.zeros((N, 3)), np.zeros((N, 3))
    sim = simulation(seed, state, [a, park, b])
    s0, s1, sp, s2 = run_in_order(sim, [a, park, b])
    assert (a._n_pass, b._n_pass, park._n_pass) == (1, 2, 1) and not moving(s0).any() and not moving(sp).any()
    assert a.parked == b.parked == N and park.absorbed == a.reemitted
    go1, go2 = moving(s1), moving(s2)
    assert (a.reemitted, b.reemitted) == (go1.sum(), go2.sum())
    check_binomial("re-emitter 1", np.ones(N, bool), go1, 0.5, seed, 1, 18)
    check_binomial("re-emitter 2, whom 1 left parked", ~go1, go2, 0.5, seed, 2, 18, part=True)
    check_binomial("re-emitter 2, whom 1 re-emitted", go1, go2, 0.5, seed, 2, 18, part=True)
    check_directions("re-emitters", go1 & go2, s1["v"], s2["v"])
