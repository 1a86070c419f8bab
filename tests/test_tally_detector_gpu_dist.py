"""GPU: DetectorMeasureStep on a sharded run of two processes.

2 processes sharing device 0, gloo for the all-reduce (the launcher of tests/test_gpu_spectrum_dist.py): the rows of a sharded
Simulation -- [N, through, seen, image] all-reduced in one collective per pass, 1 + 2 + 2 x 40 x 32 = 2563 values, i.e. two pieces
of at most 2048 -- and the exposure are those of the single-process run, on every rank; also when one rank's shard is empty.
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
N = %(N)d
sim = phys.Simulation(cl_on=True, device=0, comm=comm if comm.world > 1 else None, seed=21, rng="philox", exit=lambda s: s.t >= 0.0065)
sim.add_objs(phys.light.generate_photons_bulk(N, min=1.0, max=3.0, seed=21, source=phys.light.PhotonSource(origin=(1e5, 0.0, 0.0), angular="isotropic")))
sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.001)))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(0.001), n=np.double(0.001), wavelength_dep_scattering=False))
cam = phys.light.DetectorMeasureStep(None, position=(7e5, 1.5e5, -1e5), normal=(-1.0, -0.2, 0.1), radius=5e5, pixels=(32, 40), fov=(1.0, 1.2),
                                     E_bins=[1.0, 2.0, 3.0], frames=True)
sim.add_step(3, cam)
sim.run()
assert sim.error is None, sim.error
print(json.dumps({"rank": comm.rank, "rows": [[x.tolist() if isinstance(x, np.ndarray) else float(x) for x in r] for r in cam.data],
                  "image": cam.image.tolist(), "last": [cam.through, cam.seen], "local": int(sim._dev.count), "note": sim.launch_note}))
comm.close()
"""


def run_world(world, N):
    return rank_world.run_world(WORKER % {"root": ROOT, "N": N}, world)


@pytest.mark.parametrize("N", [20001, 1], ids=["payload_2563", "empty_shard"])
def test_two_shards_reproduce_the_single_process_rows(N):
    one = run_world(1, N)[0]
    two = run_world(2, N)
    for rank in two:
        assert rank["rows"] == one["rows"]                   # every rank records the GLOBAL rows
        assert rank["image"] == one["image"] and rank["last"] == one["last"]
        assert "DetectorMeasureStep" in rank["note"]
    assert two[0]["local"] + two[1]["local"] == one["local"] == N
    if N == 1:
        assert two[0]["local"] == 0                          # rank 0 holds nothing and still joins every collective
    rows = one["rows"]
    assert len(rows) >= 5 and all(len(r) == 5 and r[1] == N and len(r[4]) == 2 and len(r[4][0]) == 40 and len(r[4][0][0]) == 32 for r in rows)
    total = [[[sum(r[4][b][y][x] for r in rows) for x in range(32)] for y in range(40)] for b in range(2)]
    assert one["image"] == total                             # the exposure is the sum of the passes' frames
    if N > 1:
        through, seen, lit = sum(r[2] for r in rows), sum(r[3] for r in rows), sum(v > 0 for band in total for line in band for v in line)
        assert 0 < sum(map(sum, total[0])) + sum(map(sum, total[1])) <= seen <= through and lit >= 2
