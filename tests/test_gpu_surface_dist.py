"""GPU: SurfaceReflectStep on a sharded run of two processes.

2 processes sharing device 0, gloo for the all-reduce (the launcher of tests/test_gpu_shell_dist.py): after 10 passes the
photons of the two shards -- r and v, sorted by id -- and the per-pass counts of the step and of the shell tally before it are
those of the single-process run: a photon draws the same numbers however the run is sharded, and the counts are all-reduced.
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
C, R, CENTER = 299792458.0, 10.0, np.array([3.0, -2.0, 1.25])
sim = phys.Simulation(cl_on=True, device=0, comm=comm if comm.world > 1 else None, seed=21, rng="philox", exit=lambda s: len(s.ts) >= 10)
src = phys.light.PhotonSource(origin=CENTER + [R + 1.0, 0.0, 0.0], angular="isotropic")
sim.add_objs(phys.light.generate_photons_bulk(%(N)d, min=1.0, max=3.0, seed=21, source=src))
sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.5 / C)))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(0.6), n=np.double(1.0)))
tally = phys.light.ShellCrossingMeasureStep(None, [R], center=CENTER)
floor = phys.light.SurfaceReflectStep(R, center=CENTER, albedo=0.5)
sim.add_step(3, tally)
sim.add_step(4, floor)
sim.run()
assert sim.error is None, sim.error
print(json.dumps({"rank": comm.rank, "ids": sim.download("id").tolist(), "r": sim.download("r").tolist(), "v": sim.download("v").tolist(),
                  "ground": [[int(x) for x in row[1:]] for row in floor.data], "in": [int(row[3][0]) for row in tally.data],
                  "note": sim.launch_note}))
comm.close()
"""


def run_world(world, N):
    return rank_world.run_world(WORKER % {"root": ROOT, "N": N}, world)


def test_two_shards_hold_the_single_process_run_s_photons():
    N = 3001
    one = run_world(1, N)[0]
    two = run_world(2, N)
    for rank in two:
        assert rank["ground"] == one["ground"] and rank["in"] == one["in"]      # every rank records the GLOBAL counts
        assert "one launch per light step" in rank["note"]
    assert [a + b for a, b in one["ground"]] == one["in"] and sum(one["in"]) > 100
    assert any(a for a, _ in one["ground"]) and any(b for _, b in one["ground"])
    by_id = {i: (r, v) for rank in two for i, r, v in zip(rank["ids"], rank["r"], rank["v"])}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, r, v in zip(one["ids"], one["r"], one["v"]):
        assert by_id[i] == (r, v), i
