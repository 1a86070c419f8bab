"""GPU: a sourced PhotonBatch on a sharded run -- 2 processes sharing device 0, gloo for the all-reduce (the launcher of
tests/test_gpu_spectrum_dist.py).  Each rank fills its block ``[lo, hi)`` with ``id_base = lo`` and applies the source to it: the
initial positions and velocities of the two ranks, put one behind the other, are the single process's bit for bit, and so are the
counter rows of the run (sign counts and plane crossings, all-reduced) on every rank.
"""
import os

import numpy as np
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
src = phys.light.PhotonSource(origin=(6371000.0, 5.0, -3.0), direction=(1, -2, 0.5), angular=%(angular)r, spatial=%(spatial)r,
                              half_angle=0.3 if %(angular)r == "cone" else None, radius=None if %(spatial)r == "point" else 1e4)
sim = phys.Simulation(cl_on=True, device=0, comm=comm if comm.world > 1 else None, seed=21, rng="philox", exit=lambda s: len(s.ts) >= 12)
sim.add_objs(phys.light.generate_photons_bulk(N, min=1.0, max=2.0, seed=21, source=src))
sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(1e-5)))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(0.01), n=np.double(0.01)))
sign = phys.light.ScatterSignMeasureStep(None, True)
m = phys.light.ScatterMeasureStep(None, True, [[6371000.0 + 9000.0, np.nan, np.nan], [np.nan, 0.0, np.nan]])
sim.add_step(3, sign)
sim.add_step(4, m)
sim.prepare()
dev = sim._dev
first = {"id": dev.download_ids().tolist()}
for g, fids in (("r", (0, 1, 2)), ("v", (3, 4, 5))):
    first[g] = [dev.download(f).view(np.int64).tolist() for f in fids]       # bit patterns
sim.run()
assert sim.error is None, sim.error
print(json.dumps({"rank": comm.rank, "first": first, "rows": [[float(x) for x in r] for r in sign.data + m.data], "local": int(dev.count)}))
comm.close()
"""


def run_world(world, N, angular, spatial):
    return rank_world.run_world(WORKER % {"root": ROOT, "N": N, "angular": angular, "spatial": spatial}, world)


@pytest.mark.parametrize("N,angular,spatial", [(3 * 2048 + 77, "lambertian", "gaussian"), (3 * 2048 + 77, "cone", "disc"), (1, "isotropic", "point")],
                         ids=["lambertian_gaussian", "cone_disc", "empty_shard"])
def test_two_ranks_start_from_the_single_process_s_photons(N, angular, spatial):
    one = run_world(1, N, angular, spatial)[0]
    two = run_world(2, N, angular, spatial)
    assert two[0]["local"] + two[1]["local"] == one["local"] == N
    assert two[0]["first"]["id"] + two[1]["first"]["id"] == one["first"]["id"] == list(range(N))
    for g in ("r", "v"):
        for k in range(3):
            assert two[0]["first"][g][k] + two[1]["first"][g][k] == one["first"][g][k], (g, k)
    for rank in two:
        assert rank["rows"] == one["rows"]                   # every rank records the GLOBAL rows
    assert len(one["rows"]) == 24
    if N > 1:
        v0 = np.array(one["first"]["v"][0], dtype=np.int64).view(np.float64)
        assert len(np.unique(v0)) > N // 2 and two[0]["local"] > 0
    else:
        assert two[0]["local"] == 0                          # rank 0 holds nothing and still joins every collective
