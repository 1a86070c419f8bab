"""GPU: ShellCrossingMeasureStep on a sharded run of two processes.

2 processes sharing device 0, gloo for the all-reduce (the launcher of tests/test_gpu_spectrum_dist.py): the rows of a sharded
Simulation -- [N, counts, histograms] all-reduced in one collective per pass, 1 + 2 x 4 x (1 + 256 + 64) = 2569 values, i.e. two
pieces of at most 2048 -- are the rows of the single-process run, on every rank; also when one rank's shard is empty.
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
m = phys.light.ScatterMeasureStep(None, True, [[6e5, np.nan, np.nan]])
s = phys.light.ShellCrossingMeasureStep(None, [2.5e5, 7e5, 1.2e6, 4e5], E_bins=np.linspace(1.0, 3.0, 257), mu_bins=np.linspace(-1, 1, 65))
sim.add_step(3, m)
sim.add_step(4, s)
sim.run()
assert sim.error is None, sim.error
print(json.dumps({"rank": comm.rank, "rows": [[x.tolist() if isinstance(x, np.ndarray) else float(x) for x in r] for r in s.data],
                  "local": int(sim._dev.count), "note": sim.launch_note}))
comm.close()
"""


def run_world(world, N):
    return rank_world.run_world(WORKER % {"root": ROOT, "N": N}, world)


@pytest.mark.parametrize("N", [150001, 1], ids=["payload_2569", "empty_shard"])
def test_two_shards_reproduce_the_single_process_rows(N):
    one = run_world(1, N)[0]
    two = run_world(2, N)
    for rank in two:
        assert rank["rows"] == one["rows"]                   # every rank records the GLOBAL rows
        assert "ShellCrossingMeasureStep" in rank["note"]
    assert two[0]["local"] + two[1]["local"] == one["local"] == N
    if N == 1:
        assert two[0]["local"] == 0                          # rank 0 holds nothing and still joins every collective
    rows = one["rows"]
    assert len(rows) >= 5 and all(len(r) == 8 and r[1] == N and len(r[2]) == 4 and len(r[4][0]) == 256 and len(r[6][0]) == 64 for r in rows)
    assert sum(sum(r[2]) for r in rows) > 0                  # something went out
    if N > 1:
        assert sum(sum(r[3]) for r in rows) > 0 and sum(sum(map(sum, r[4])) for r in rows) > 0 and sum(sum(map(sum, r[7])) for r in rows) > 0
