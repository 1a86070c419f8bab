"""GPU: AbsorptionStep on a sharded run of two processes.

2 processes sharing device 0, gloo for the all-reduce (the launcher of tests/test_gpu_shell_dist.py): after 3 passes the
per-pass counts, per-layer rows and energy histograms of the step are those of the single-process run on every rank, and so are
the velocities of the two shards, by id: a photon draws the same number however the run is sharded, and the tallies are
all-reduced.
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
step = phys.light.AbsorptionStep((0.5, 0.5, 0.2), edges=(0.0, 0.6, 1.1, 1.4), E_bins=np.linspace(1.0, 3.0, 5))
sim.add_step(3, step)
sim.run()
assert sim.error is None, sim.error
print(json.dumps({"rank": comm.rank, "ids": sim.download("id").tolist(), "v": sim.download("v").tolist(),
                  "counts": [[int(row[1]), int(row[2])] for row in step.data], "layers": [row[3].tolist() for row in step.data],
                  "E_hist": [row[4].tolist() for row in step.data], "hits": sim.hits, "note": sim.launch_note}))
comm.close()
"""


def run_world(world, N):
    return rank_world.run_world(WORKER % {"root": ROOT, "N": N}, world)


def test_two_shards_hold_the_single_process_run_s_counts_and_photons():
    N = 4097
    one = run_world(1, N)[0]
    two = run_world(2, N)
    for rank in two:                                                   # every rank records the GLOBAL tallies
        assert rank["counts"] == one["counts"] and rank["layers"] == one["layers"] and rank["E_hist"] == one["E_hist"]
        assert rank["hits"] == one["hits"]
        assert "one launch per light step" in rank["note"] and "AbsorptionStep" in rank["note"]
    assert len(one["counts"]) == 3 and one["counts"][-1][0] == one["hits"] and min(c[0] for c in one["counts"]) > N // 8
    for (interacted, absorbed), layers, hist in zip(one["counts"], one["layers"], one["E_hist"]):
        assert 0 < absorbed < interacted and sum(layers) == absorbed and sum(sum(row) for row in hist) == absorbed
        assert [sum(row) for row in hist] == layers
    assert sum(x > 0 for x in one["layers"][-1]) >= 2                  # by the third pass more than one layer has absorbed somebody
    by_id = {i: v for rank in two for i, v in zip(rank["ids"], rank["v"])}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, v in zip(one["ids"], one["v"]):
        assert by_id[i] == v, i
