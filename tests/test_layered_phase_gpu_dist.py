"""GPU: LayeredPhaseStep on a sharded run of two processes.

2 processes sharing device 0, gloo for the all-reduce (the launcher of tests/test_gpu_shell_dist.py): after 3 passes the
velocities of the two shards, by id, and the per-pass tallies of the step -- scattered, re-directed, by layer and by law -- are
those of the single-process run: a photon draws the same numbers however the run is sharded, and the tallies are all-reduced.
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
sim = phys.Simulation(cl_on=True, device=0, comm=comm if comm.world > 1 else None, seed=21, rng="philox", exit=lambda s: len(s.ts) >= 3)
sim.add_objs(phys.light.generate_photons_bulk(%(N)d, min=1.0, max=3.0, seed=21, source=phys.light.PhotonSource(angular="isotropic")))
sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.5 / C)))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(1.0), n=np.double(1.0)))
edges = np.linspace(-1.0, 1.0, 65)
table = ("table", edges, 1.0 / (1.7225 - 1.7 * 0.5 * (edges[1:] + edges[:-1])) ** 1.5)
step = phys.light.LayeredPhaseStep(["rayleigh", ("hg", 0.85), table], [[1, 0, 0], [0.3, 0.3, 0.4], [0, 0, 1]], edges=[0.0, 0.45, 0.6, 1.2])
sim.add_step(3, step)
sim.run()
assert sim.error is None, sim.error
print(json.dumps({"rank": comm.rank, "ids": sim.download("id").tolist(), "v": sim.download("v").tolist(),
                  "rows": [[int(row[1]), int(row[2])] + row[3].tolist() + row[4].tolist() for row in step.data], "hits": sim.hits,
                  "note": sim.launch_note}))
comm.close()
"""


def run_world(world, N):
    return rank_world.run_world(WORKER % {"root": ROOT, "N": N}, world)


def test_two_shards_hold_the_single_process_run_s_photons():
    N = 4097
    one = run_world(1, N)[0]
    two = run_world(2, N)
    for rank in two:
        assert rank["rows"] == one["rows"] and rank["hits"] == one["hits"]                  # every rank records the GLOBAL tallies
        assert "one launch per light step" in rank["note"] and "LayeredPhaseStep" in rank["note"]
    assert len(one["rows"]) == 3 and min(row[0] for row in one["rows"]) > N // 3 and one["rows"][-1][0] == one["hits"]
    for row in one["rows"]:                                                                 # layers and laws were all in use
        assert 0 < row[1] <= row[0] and sum(row[2:5]) == sum(row[5:8]) == row[1] and min(row[5:8]) > 0
    assert one["rows"][-1][1] < one["rows"][-1][0]                                          # some photons have left the layers
    assert all(sum(row[2 + b] for row in one["rows"]) > 0 for b in range(3))                # and every layer had work
    by_id = {i: v for rank in two for i, v in zip(rank["ids"], rank["v"])}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, v in zip(one["ids"], one["v"]):
        assert by_id[i] == v, i
