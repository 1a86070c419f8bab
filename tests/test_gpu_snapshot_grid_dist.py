"""GPU: PositionGridMeasureStep on sharded runs.

* 2 processes sharing device 0, gloo for the all-reduce (the launcher of tests/test_gpu_dist.py): the rows of a sharded
  Simulation -- [N, cells] all-reduced once per recorded pass, 1 + 64 x 64 values, i.e. three collectives of at most 2048 -- are
  the rows of the single-process run, on every rank, with the K-pass launches kept; also when one rank's shard is empty (a
  single photon).
* the library's own RCCL communicator (physicl_amd.comm.NativeCounterComm) with the world of one a one-GPU box allows: the same
  payload goes through the real pcl_comm_allreduce_sum_i64, which takes 2048 values per call, and gives the plain rows.
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
S = 299792458.0 * 0.001
sim = phys.Simulation(cl_on=True, device=0, comm=comm if comm.world > 1 else None, seed=21, rng="philox", exit=lambda s: s.t >= 0.0405)
sim.add_objs(phys.light.generate_photons_bulk(N, min=1.0, max=2.0, seed=21, source=phys.light.PhotonSource(origin=(S, 0, 0), angular="isotropic")))
sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.001)))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(0.001), n=np.double(0.0001), wavelength_dep_scattering=False))
m = phys.light.PositionGridMeasureStep(None, ("r", "z"), [np.linspace(0, 40 * S, 65), np.linspace(-30 * S, 30 * S, 65)], center=(S, 0, 0), every=8)
sim.add_step(3, m)
sim.run()
assert sim.error is None, sim.error
print(json.dumps({"rank": comm.rank, "rows": [[x.tolist() if isinstance(x, np.ndarray) else float(x) for x in r] for r in m.data],
                  "local": int(sim._dev.count), "schedule": dict(sim.schedule)}))
comm.close()
"""


def run_world(world, N):
    return rank_world.run_world(WORKER % {"root": ROOT, "N": N}, world)


@pytest.mark.parametrize("N", [150001, 1], ids=["payload_4097", "empty_shard"])
def test_two_shards_reproduce_the_single_process_grids(N):
    one = run_world(1, N)[0]
    two = run_world(2, N)
    for rank in two:
        assert rank["rows"] == one["rows"]                   # every rank records the GLOBAL rows
        assert rank["schedule"] == one["schedule"] == {"fused_multi": 6}     # 41 passes, every=8: five launches of 8 and one of 1
    assert two[0]["local"] + two[1]["local"] == one["local"] == N
    if N == 1:
        assert two[0]["local"] == 0                          # rank 0 holds nothing and still joins every collective
    rows = one["rows"]
    assert len(rows) == 5 and all(len(r) == 3 and r[1] == N and np.array(r[2]).shape == (64, 64) for r in rows)
    assert all(np.sum(r[2]) == N for r in rows[:3])          # nobody has left the grid after 24 passes
    if N > 1:
        assert np.count_nonzero(rows[-1][2]) > 300


def grid_run(native):
    import physicl_amd as phys
    import physicl_amd.light as light
    import physicl_amd.newton as newton
    from physicl_amd.comm import NativeCounterComm
    S = 299792458.0 * 0.001
    comm = NativeCounterComm(0, 1, exchange=lambda ident: ident) if native else None
    sim = phys.Simulation(exit=lambda s: len(s.ts) >= 16, seed=3, rng="philox", comm=comm)
    sim.add_objs(light.generate_photons_bulk(50_000, min=1.0, max=2.0, seed=3, source=light.PhotonSource(angular="isotropic")))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.001)))
    sim.add_step(1, newton.NewtonianKinematicsStep())
    sim.add_step(2, light.ScatterIsotropicStep(A=np.double(0.001), n=np.double(0.0001)))
    m = light.PositionGridMeasureStep(None, ("x", "y", "z"), [np.linspace(-20 * S, 20 * S, 17)] * 3, every=4)   # 1 + 4096 values per record
    sim.add_step(3, m)
    sim.start()
    sim.join()
    err = sim.error
    reduces = None
    if comm is not None:                                     # the communicator lives on the simulation's context: it goes first
        assert comm.info()["ranks_seen"] == 1 and comm.rccl_version
        reduces = comm.info().get("reduces")
        comm.close()
    schedule = dict(sim.schedule)
    sim.close(download=False)
    return err, [[x.tolist() if isinstance(x, np.ndarray) else x for x in r] for r in m.data], schedule, reduces


def test_grid_step_runs_on_the_library_s_rccl_communicator():
    err, plain, schedule, _ = grid_run(False)
    assert err is None and len(plain) == 4 and schedule == {"fused_multi": 4}
    err, native, schedule_n, reduces = grid_run(True)
    assert err is None, err
    assert native == plain and schedule_n == schedule and all(np.sum(r[2]) == 50_000 for r in plain)
    assert np.count_nonzero(plain[-1][2]) > 200
