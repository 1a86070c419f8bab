"""GPU: the six writer steps -- SurfaceReflectStep, PhaseFunctionStep, AbsorptionStep, LayeredPhaseStep, RecycleStep and
PathAbsorptionStep -- each on a sharded run of two processes.

2 processes sharing device 0, gloo for the all-reduce (the launcher of tests/test_gpu_shell_dist.py): after the case's passes
the photons of the two shards, by id, and the per-pass rows of the step are those of the single-process run: a photon draws the
same numbers however the run is sharded, and the counts and tallies are all-reduced.  N = 4097 is two 2048-particle tiles plus
one, so the shard boundary falls inside a tile (the ground's run keeps its 3001).

A case of ``CASES`` gives what is a step's own: the lines between the simulation and ``sim.run()`` (objects, steps), what a rank
records besides ids and note (a dict, evaluated in the worker), which of its keys every rank must hold as the single-process run
holds them, the fields compared by id, the step's name where the launch note carries it, and ``check(one, two, N)``: the asserts
on the rows themselves, so that the comparison is not one of empty runs.

* surface: 10 passes, with the shell tally before the ground: every crossing inward is reflected or absorbed;
* phase: 3 passes; absorb: 3 passes, per-layer rows and energy histograms; layered_phase: 3 passes, by layer and by law;
* recycle: 8 passes of the absorbing atmosphere over a black ground: the same ids are re-emitted the same way;
* path_absorb: 8 passes of the recycling atmosphere with a gas of two layers and two bands.
"""
import os

import pytest

import rank_world

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import physicl as phys, physicl.light, physicl.newton
from physicl_amd.dist import CounterComm
comm = CounterComm.from_env(backend="gloo")
C = 299792458.0
sim = phys.Simulation(cl_on=True, device=0, comm=comm if comm.world > 1 else None, seed=21, rng="philox", exit=lambda s: len(s.ts) >= %(passes)d)
%(steps)s
sim.run()
assert sim.error is None, sim.error
out = {"rank": comm.rank, "ids": sim.download("id").tolist(), "note": sim.launch_note}
out.update({f: sim.download(f).tolist() for f in %(fields)r})
out.update(%(record)s)
print(json.dumps(out))
comm.close()
"""

ISOTROPIC = """\
sim.add_objs(phys.light.generate_photons_bulk(%(N)d, min=1.0, max=3.0, seed=21, source=phys.light.PhotonSource(angular="isotropic")))
sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.5 / C)))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
"""
DISC = """\
src = phys.light.PhotonSource(origin=(2.0, 0.0, 0.0), angular="isotropic", spatial="disc", radius=0.25)
sim.add_objs(phys.light.generate_photons_bulk(%(N)d, min=1.0, max=3.0, seed=21, source=src))
sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.5 / C)))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
"""


def check_surface(one, two, N):
    assert [a + b for a, b in one["ground"]] == one["in"] and sum(one["in"]) > 100
    assert any(a for a, _ in one["ground"]) and any(b for _, b in one["ground"])


def check_phase(one, two, N):
    assert len(one["redirected"]) == 3 and min(one["redirected"]) > N // 3 and one["redirected"][-1] == one["hits"]


def check_absorb(one, two, N):
    assert len(one["counts"]) == 3 and one["counts"][-1][0] == one["hits"] and min(c[0] for c in one["counts"]) > N // 8
    for (interacted, absorbed), layers, hist in zip(one["counts"], one["layers"], one["E_hist"]):
        assert 0 < absorbed < interacted and sum(layers) == absorbed and sum(sum(row) for row in hist) == absorbed
        assert [sum(row) for row in hist] == layers
    assert sum(x > 0 for x in one["layers"][-1]) >= 2                  # by the third pass more than one layer has absorbed somebody


def check_layered_phase(one, two, N):
    assert len(one["rows"]) == 3 and min(row[0] for row in one["rows"]) > N // 3 and one["rows"][-1][0] == one["hits"]
    for row in one["rows"]:                                                                 # layers and laws were all in use
        assert 0 < row[1] <= row[0] and sum(row[2:5]) == sum(row[5:8]) == row[1] and min(row[5:8]) > 0
    assert one["rows"][-1][1] < one["rows"][-1][0]                                          # some photons have left the layers
    assert all(sum(row[2 + b] for row in one["rows"]) > 0 for b in range(3))                # and every layer had work


def check_recycle(one, two, N):
    assert len(one["rows"]) == 8 and min(row[0] for row in one["rows"]) > 0 and sum(row[1] for row in one["rows"]) > 0
    recycled = sum(e in (1.25, 1.5, 2.0, 2.75) for e in one["E"])
    assert recycled > N // 2                                                                # most slots have been re-emitted by then


def check_path_absorb(one, two, N):
    assert len(one["rows"]) == 8 and min(row[1] for row in one["rows"]) > 0
    for exposed, absorbed, cells in one["rows"]:
        assert 0 < absorbed < exposed <= N and sum(map(sum, cells)) == absorbed and cells[0][1] == 0 and len(cells) == 2 == len(cells[0])


CASES = [
    dict(name="surface", N=3001, passes=10, fields=("r", "v"), rows=("ground", "in"), note="", check=check_surface, steps="""\
C, R, CENTER = 299792458.0, 10.0, np.array([3.0, -2.0, 1.25])
src = phys.light.PhotonSource(origin=CENTER + [R + 1.0, 0.0, 0.0], angular="isotropic")
sim.add_objs(phys.light.generate_photons_bulk(%(N)d, min=1.0, max=3.0, seed=21, source=src))
sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.5 / C)))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(0.6), n=np.double(1.0)))
tally = phys.light.ShellCrossingMeasureStep(None, [R], center=CENTER)
floor = phys.light.SurfaceReflectStep(R, center=CENTER, albedo=0.5)
sim.add_step(3, tally)
sim.add_step(4, floor)
""", record='{"ground": [[int(x) for x in row[1:]] for row in floor.data], "in": [int(row[3][0]) for row in tally.data]}'),
    dict(name="phase", N=4097, passes=3, fields=("v",), rows=("redirected", "hits"), note="PhaseFunctionStep", check=check_phase,
         steps=ISOTROPIC + """\
step = phys.light.PhaseFunctionStep("hg", 0.85)
sim.add_step(3, step)
""", record='{"redirected": [int(row[1]) for row in step.data], "hits": sim.hits}'),
    dict(name="absorb", N=4097, passes=3, fields=("v",), rows=("counts", "layers", "E_hist", "hits"), note="AbsorptionStep",
         check=check_absorb, steps=ISOTROPIC + """\
step = phys.light.AbsorptionStep((0.5, 0.5, 0.2), edges=(0.0, 0.6, 1.1, 1.4), E_bins=np.linspace(1.0, 3.0, 5))
sim.add_step(3, step)
""", record='{"counts": [[int(row[1]), int(row[2])] for row in step.data], "layers": [row[3].tolist() for row in step.data], '
            '"E_hist": [row[4].tolist() for row in step.data], "hits": sim.hits}'),
    dict(name="layered_phase", N=4097, passes=3, fields=("v",), rows=("rows", "hits"), note="LayeredPhaseStep", check=check_layered_phase,
         steps=ISOTROPIC + """\
edges = np.linspace(-1.0, 1.0, 65)
table = ("table", edges, 1.0 / (1.7225 - 1.7 * 0.5 * (edges[1:] + edges[:-1])) ** 1.5)
step = phys.light.LayeredPhaseStep(["rayleigh", ("hg", 0.85), table], [[1, 0, 0], [0.3, 0.3, 0.4], [0, 0, 1]], edges=[0.0, 0.45, 0.6, 1.2])
sim.add_step(3, step)
""", record='{"rows": [[int(row[1]), int(row[2])] + row[3].tolist() + row[4].tolist() for row in step.data], "hits": sim.hits}'),
    dict(name="recycle", N=4097, passes=8, fields=("r", "v", "E"), rows=("rows",), note="", check=check_recycle, steps=DISC + """\
sim.add_step(3, phys.light.AbsorptionStep(omega0=0.5))
sim.add_step(4, phys.light.SurfaceReflectStep(1.0, albedo=0.0))
step = phys.light.RecycleStep(src, top=3.0, spectrum=([1.25, 1.5, 2.0, 2.75], [0.1, 0.4, 0.8, 1.0]))
sim.add_step(5, step)
""", record='{"rows": [[int(row[1]), int(row[2])] for row in step.data]}'),
    dict(name="path_absorb", N=4097, passes=8, fields=("r", "v", "E"), rows=("rows",), note="", check=check_path_absorb, steps=DISC + """\
step = phys.light.PathAbsorptionStep([[0.4, 0.0], [0.1, 0.8]], [1.0, 2.0, 3.0], (0, 0, 0), [1.0, 2.0, 3.0])
sim.add_step(3, step)
sim.add_step(4, phys.light.SurfaceReflectStep(1.0, albedo=0.5))
sim.add_step(5, phys.light.RecycleStep(src, top=3.0))
""", record='{"rows": [[int(row[1]), int(row[2]), np.asarray(row[3]).tolist()] for row in step.data]}'),
]


def run_world(case, world):
    steps = (case["steps"] % {"N": case["N"]}).rstrip()
    return rank_world.run_world(WORKER % dict(case, root=ROOT, steps=steps), world)


@pytest.mark.parametrize("case", CASES, ids=[case["name"] for case in CASES])
def test_two_shards_hold_the_single_process_run_s_photons(case):
    N, fields = case["N"], case["fields"]
    one = run_world(case, 1)[0]
    two = run_world(case, 2)
    for rank in two:
        for key in case["rows"]:
            assert rank[key] == one[key], key                          # every rank records the GLOBAL counts and tallies
        assert "one launch per light step" in rank["note"] and case["note"] in rank["note"]
    case["check"](one, two, N)
    by_id = {i: row for rank in two for i, *row in zip(rank["ids"], *(rank[f] for f in fields))}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, *row in zip(one["ids"], *(one[f] for f in fields)):
        assert by_id[i] == row, i
