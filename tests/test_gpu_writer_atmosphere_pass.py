"""GPU: the step list of examples/point_source_atmosphere.py --ground --phase --omega0 --shells in ONE pass, through ``Simulation``:

    UpdateTimeStep, Newton, ScatterIsotropicStep, AbsorptionStep(layers, E_bins), PhaseFunctionStep("hg", 0.85),
    ShellCrossingMeasureStep(radii with the ground's), SurfaceReflectStep(R, albedo 0.5), PositionGridMeasureStep

The ground, the phase function and absorption all read "interacted in this pass" off ``dv != 0``, and the ground ends a pass with
``dv = v' - v_old`` on a reflected photon and ``dv = -v_old`` on an absorbed one: only the next pass's scatter step, writing dv on
every miss, keeps the phase function from sending a ground-absorbed photon off again at speed c.  Probes (plain DeviceSteps that
download r, v, dr, dv, E and the ids) stand in front of the absorption step, behind it, behind the phase step and behind the
ground; for every pass

* each of the three steps is replayed with its numpy restatement from the device's own probed state in front of it (nothing
  accumulates), with the step's own pass counter and ``sim.seed``, and compared with the probed state behind it under the bounds of
  tests/writer_reference.py; its recorded row is compared exactly;
* ``phase.redirected == medium.interacted - medium.absorbed``; the shell's inward count at the ground's radius is
  ``floor.reflected + floor.absorbed``; the census ``N == moving + absorbed by the medium so far + absorbed by the ground so far``;
* a parked photon stays parked: in every later pass it stands in front of the absorption step with dv == 0, v == 0 and r
  unchanged, and is neither among the medium's interacting rows nor among the phase function's re-directed ones;
* in front of the absorption step dv is zero for everybody whose velocity is what the last pass left, ``v - v_old`` for the
  others -- a ground-reflected photon carries dv == 0 unless the scatter step hit it.

Variants: no probes at all (the probes make dr / dv real in every pass: the run without them gives the same rows and the same
final store); two contexts on one GPU; a ``Newton, ScatterDeleteStep`` group in front (ids with gaps, a shrinking store);
``omega0 = 1`` everywhere with ``albedo = 1`` (nobody is ever parked).

Every check is an equality, a counting identity or one of the derived bounds: no number here comes from the code under test.
"""
import numpy as np
import pytest

import physicl as phys
import physicl.light
import physicl.newton
import writer_reference as W
from physicl_amd import light

pytestmark = pytest.mark.gpu

N_SIM, PASSES = 4097, 8
STEP = 0.5                                           # length of a move: A*n*|dr| = 0.5, about half interact per pass
DT = STEP / W.C
RADIUS = 4.0
CENTER = np.array([3.0, -2.0, 1.25])
ORIGIN = CENTER + [RADIUS + 0.3, 0.2, -0.1]          # the source: just above the ground, off the sphere's axes
LAYERS = RADIUS + np.array([0.0, 0.5, 1.2, 6.0])     # the source stands in the first; nobody gets beyond the last in 8 passes
OMEGA0 = (0.5, 1.0, 0.2)
E_BINS = np.linspace(1.2, 2.8, 5)                    # the photons' energies reach from 1 to 3: some fall outside
SHELLS = [RADIUS + 1.2, RADIUS, RADIUS + 0.5]        # the ground's radius among them, in no order
GROUND_SHELL = 1
W_MAX = 1.001 * STEP                                 # the longest move: |v| dt with |v| = c to a few ulp
STATE = ("r", "v", "dr", "dv", "E", "id")


class Look(phys.DeviceStep):
    """The store as it stands, pass by pass."""
    _fuse_role = None

    def __init__(self):
        self.states = []

    def _device_run(self, sim):
        self.states.append({f: sim.download(f) for f in STATE})


class Run:
    pass


def atmosphere(devices=None, probes=True, removal=False, conservative=False):
    sim = phys.Simulation(cl_on=True, rng="philox", seed=7, devices=devices, exit=lambda s: len(s.ts) >= PASSES)
    src = phys.light.PhotonSource(origin=ORIGIN, angular="isotropic")
    sim.add_objs(phys.light.generate_photons_bulk(N_SIM, min=1.0, max=3.0, seed=7, source=src))
    run = Run()
    run.medium = phys.light.AbsorptionStep((1.0, 1.0, 1.0) if conservative else OMEGA0, edges=LAYERS, center=CENTER, E_bins=E_BINS)
    run.phase = phys.light.PhaseFunctionStep("hg", 0.85)
    run.shell = phys.light.ShellCrossingMeasureStep(None, SHELLS, center=CENTER)
    run.floor = phys.light.SurfaceReflectStep(RADIUS, center=CENTER, albedo=1.0 if conservative else 0.5)
    run.grid = phys.light.PositionGridMeasureStep(None, ("r",), [LAYERS], center=CENTER)
    run.looks = [Look() for _ in range(4)] if probes else [None] * 4
    steps = [phys.UpdateTimeStep(lambda s: np.double(DT))]
    if removal:                                      # 2 % of the moving photons per pass
        steps += [phys.newton.NewtonianKinematicsStep(), phys.light.ScatterDeleteStep(n=np.double(1.0), A=np.double(0.04))]
    steps += [phys.newton.NewtonianKinematicsStep(), phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)),
              run.looks[0], run.medium, run.looks[1], run.phase, run.looks[2], run.shell, run.floor, run.looks[3], run.grid]
    for k, s in enumerate(x for x in steps if x is not None):
        sim.add_step(k, s)
    sim.start()
    sim.join()
    assert sim.error is None, sim.error
    run.final = {f: sim.download(f) for f in STATE}
    run.note, run.schedule, run.n_objects, run.seed = sim.launch_note, dict(sim.schedule), len(sim.objects), sim.seed
    sim.close(download=False)
    return run


def rows(run):
    """Every step's rows as plain lists."""
    return {name: [[np.asarray(x).tolist() for x in row] for row in getattr(run, name).data] for name in ("medium", "phase", "shell", "floor", "grid")}


def sorted_by_id(state):
    order = np.argsort(state["id"], kind="stable")
    return {f: state[f][order] for f in STATE}


def places(ids, wanted):
    """Where the ids ``wanted`` stand among ``ids`` (all of them must be there)."""
    order = np.argsort(ids, kind="stable")
    at = order[np.minimum(np.searchsorted(ids[order], wanted), len(ids) - 1)] if len(ids) else np.zeros(0, dtype=np.int64)
    assert len(at) == len(wanted) and np.array_equal(ids[at], wanted)
    return at


def check_run(run, removal=False, conservative=False):
    """The replays and the invariants of the module's docstring, pass by pass.  Returns the totals seen."""
    c_lit = light._c_h_literals()[0]
    assert all(len(look.states) == PASSES for look in run.looks)
    assert all(len(getattr(run, name).data) == PASSES for name in ("medium", "phase", "shell", "floor", "grid"))
    assert run.medium._pass == run.phase._pass == run.floor._pass == PASSES
    parked_ids, parked_r = np.zeros(0, dtype=np.int64), np.zeros((0, 3))
    gone_medium = gone_floor = 0
    seen = dict(reflected=0, absorbed_floor=0, interacted=0, absorbed_medium=0, redirected=0, bounced_then_hit=0, bounced_then_missed=0)
    by_layer = np.zeros(len(OMEGA0), dtype=np.int64)
    for p in range(PASSES):
        s0, s1, s2, s3 = (look.states[p] for look in run.looks)
        what = "pass %d" % (p + 1)
        assert all(W.same_bits(s0["id"], s["id"]) for s in (s1, s2, s3)), what
        medium, phase, shell, floor, grid = (getattr(run, name).data[p] for name in ("medium", "phase", "shell", "floor", "grid"))
        omega0 = (1.0, 1.0, 1.0) if conservative else OMEGA0
        ref_a = W.check_absorb(s0, s1, (medium[1], medium[2], medium[3], medium[4]), omega0, LAYERS, CENTER, E_BINS, run.seed, p + 1, what + " absorb")
        ref_p = W.check_phase(s1, s2, phase[1], "hg", 0.85, c_lit, run.seed, p + 1, what + " phase")
        ref_g = W.check_surface(s2, s3, (floor[1], floor[2]), RADIUS, CENTER, 1.0 if conservative else 0.5, "lambertian", c_lit, run.seed, p + 1,
                                W_MAX, what + " ground")
        # the counting identities
        assert int(phase[1]) == int(medium[1]) - int(medium[2]), what
        assert int(shell[3][GROUND_SHELL]) == int(floor[1]) + int(floor[2]), what
        assert int(grid[1]) == len(s3["id"]), what
        # a parked photon stays parked
        if len(parked_ids):
            at = places(s0["id"], parked_ids)                          # still in the store: a photon at rest is never removed
            assert not s0["dv"][at].any() and not s0["v"][at].any() and W.same_bits(s0["r"][at], parked_r), what
            assert not ref_a["interacted"][at].any() and not ref_p["redirected"][at].any() and not ref_g["hit"][at].any(), what
            assert not s3["v"][at].any() and W.same_bits(s3["r"][at], parked_r), what
        # dv in front of the absorption step: zero on a miss, v - v_old on a hit -- whatever the ground left there
        if p > 0:
            last = run.looks[3].states[p - 1]
            at = places(last["id"], s0["id"])                          # everybody here was there (a delete group only removes)
            v_old = last["v"][at]
            missed = (s0["v"] == v_old).all(axis=1)
            assert not s0["dv"][missed].any(), what
            assert np.array_equal(s0["dv"][~missed], s0["v"][~missed] - v_old[~missed]), what
            bounced = np.isin(s0["id"], last["id"][reflected_last])
            seen["bounced_then_hit"] += int((bounced & ~missed).sum())
            seen["bounced_then_missed"] += int((bounced & missed).sum())
            assert last["dv"][at][bounced].any(axis=1).all(), what     # (the ground did leave a dv on them)
        reflected_last = ref_g["reflected"]
        # the census
        for ref, state, n in ((ref_a, s1, int(medium[2])), (ref_g, s3, int(floor[2]))):
            assert int(ref["absorbed"].sum()) == n
            parked_ids = np.concatenate([parked_ids, state["id"][ref["absorbed"]]])
            parked_r = np.concatenate([parked_r, state["r"][ref["absorbed"]]])
        gone_medium, gone_floor = gone_medium + int(medium[2]), gone_floor + int(floor[2])
        at_rest = ~s3["v"].any(axis=1)
        assert len(s3["id"]) == int((~at_rest).sum()) + gone_medium + gone_floor, what
        assert len(np.unique(parked_ids)) == len(parked_ids) == gone_medium + gone_floor, what      # nobody is absorbed twice
        assert np.array_equal(np.sort(s3["id"][at_rest]), np.sort(parked_ids)), what
        assert (len(s3["id"]) == N_SIM) if not removal else (len(s3["id"]) <= N_SIM - p), what
        seen["reflected"] += int(floor[1]); seen["absorbed_floor"] += int(floor[2]); seen["interacted"] += int(medium[1])
        seen["absorbed_medium"] += int(medium[2]); seen["redirected"] += int(phase[1])
        by_layer += np.asarray(medium[3])
    seen["by_layer"], seen["left"] = by_layer.tolist(), len(run.final["id"])
    for f in STATE:                                                    # nothing moves behind the last probe
        assert W.same_bits(run.final[f], run.looks[3].states[-1][f]), f
    assert "one launch per light step" in run.note and not run.schedule.get("fused_multi") and run.schedule["fused"] == PASSES
    assert run.n_objects == len(run.final["id"])
    print("atmosphere pass (removal %s, conservative %s): %s" % (removal, conservative, seen))
    return seen


@pytest.fixture(scope="module")
def base():
    return atmosphere()


def test_every_step_replays_from_the_probed_state_and_the_counts_add_up(base):
    seen = check_run(base)
    assert base.n_objects == N_SIM
    assert seen["reflected"] > 0 and seen["absorbed_floor"] > 0 and seen["redirected"] > 0            # every step had work
    assert seen["by_layer"][0] > 0 and seen["by_layer"][1] == 0 and seen["by_layer"][2] > 0 and seen["interacted"] > seen["absorbed_medium"]
    assert seen["bounced_then_hit"] > 0 and seen["bounced_then_missed"] > 0
    assert N_SIM * PASSES // 4 < seen["interacted"] < N_SIM * PASSES * 3 // 4                          # about half interact per pass, until they are parked


def test_the_probes_do_not_disturb_the_run(base):
    """The probes download dr and dv, which makes them real in every pass; without probes the sweeps meet them implicit."""
    bare = atmosphere(probes=False)
    assert rows(bare) == rows(base) and bare.note == base.note and bare.schedule == base.schedule
    for f in STATE:
        assert W.same_bits(bare.final[f], base.final[f]), f


def test_two_contexts_on_one_gpu_give_the_unsharded_run(base):
    both = atmosphere(devices=[0, 0])
    assert rows(both) == rows(base) and "one launch per light step" in both.note and both.n_objects == N_SIM
    got, want = sorted_by_id(both.final), sorted_by_id(base.final)
    for f in STATE:
        assert W.same_bits(got[f], want[f]), f


def test_behind_a_delete_group_ids_have_gaps_and_the_store_shrinks():
    run = atmosphere(removal=True)
    seen = check_run(run, removal=True)
    assert run.schedule["fused_delete"] == PASSES
    counts = [len(s["id"]) for s in run.looks[0].states]
    assert counts[0] < N_SIM and all(a > b for a, b in zip(counts, counts[1:])) and run.n_objects == counts[-1]   # every pass removes somebody
    ids = run.final["id"]
    assert not np.array_equal(ids, ids[0] + np.arange(len(ids)))       # gaps
    assert seen["reflected"] > 0 and seen["absorbed_floor"] > 0 and seen["redirected"] > 0 and seen["absorbed_medium"] > 0
    assert seen["bounced_then_hit"] > 0 and seen["bounced_then_missed"] > 0


def test_a_conservative_medium_over_a_white_ground_parks_nobody():
    run = atmosphere(conservative=True)
    seen = check_run(run, conservative=True)
    assert seen["absorbed_floor"] == 0 and seen["absorbed_medium"] == 0 and seen["by_layer"] == [0, 0, 0]
    assert seen["reflected"] > 0 and seen["redirected"] == seen["interacted"] > 0
    assert all(s["v"].any(axis=1).all() for look in run.looks for s in look.states)
