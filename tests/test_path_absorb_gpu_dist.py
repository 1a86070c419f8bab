"""GPU: PathAbsorptionStep on a sharded run of two processes.

2 processes sharing device 0, gloo for the all-reduce (the launcher of tests/test_gpu_shell_dist.py): after 8 passes of the recycling
atmosphere with a gas of two layers and two bands the positions, velocities and energies of the two shards, by id, and the per-pass
tallies of the step -- exposed, absorbed, absorbed by cell -- are those of the single-process run: a photon draws the same number
however the run is sharded, and the tallies are all-reduced.
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
sim = phys.Simulation(cl_on=True, device=0, comm=comm if comm.world > 1 else None, seed=21, rng="philox", exit=lambda s: len(s.ts) >= 8)
src = phys.light.PhotonSource(origin=(2.0, 0.0, 0.0), angular="isotropic", spatial="disc", radius=0.25)
sim.add_objs(phys.light.generate_photons_bulk(%(N)d, min=1.0, max=3.0, seed=21, source=src))
sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.5 / C)))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
step = phys.light.PathAbsorptionStep([[0.4, 0.0], [0.1, 0.8]], [1.0, 2.0, 3.0], (0, 0, 0), [1.0, 2.0, 3.0])
sim.add_step(3, step)
sim.add_step(4, phys.light.SurfaceReflectStep(1.0, albedo=0.5))
sim.add_step(5, phys.light.RecycleStep(src, top=3.0))
sim.run()
assert sim.error is None, sim.error
print(json.dumps({"rank": comm.rank, "ids": sim.download("id").tolist(), "v": sim.download("v").tolist(), "r": sim.download("r").tolist(),
                  "E": sim.download("E").tolist(), "rows": [[int(row[1]), int(row[2]), np.asarray(row[3]).tolist()] for row in step.data],
                  "note": sim.launch_note}))
comm.close()
"""


def run_world(world, N):
    return rank_world.run_world(WORKER % {"root": ROOT, "N": N}, world)


def test_two_shards_absorb_the_single_process_run_s_photons():
    N = 4097
    one = run_world(1, N)[0]
    two = run_world(2, N)
    for rank in two:
        assert rank["rows"] == one["rows"]                                                  # every rank records the GLOBAL tallies
        assert "one launch per light step" in rank["note"]                                  # (the first writer of the pass says it)
    assert len(one["rows"]) == 8 and min(row[1] for row in one["rows"]) > 0
    for exposed, absorbed, cells in one["rows"]:
        assert 0 < absorbed < exposed <= N and sum(map(sum, cells)) == absorbed and cells[0][1] == 0 and len(cells) == 2 == len(cells[0])
    by_id = {i: (r, v, e) for rank in two for i, r, v, e in zip(rank["ids"], rank["r"], rank["v"], rank["E"])}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, r, v, e in zip(one["ids"], one["r"], one["v"], one["E"]):
        assert by_id[i] == (r, v, e), i
