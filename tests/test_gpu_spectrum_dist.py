"""GPU: a binned ScatterMeasureStep on sharded runs.

* 2 processes sharing device 0, gloo for the all-reduce (the launcher of tests/test_gpu_dist.py): the rows of a sharded
  Simulation -- counts and histograms all-reduced, 4 planes x 1024 bins = 4101 values, i.e. three collectives of at most 2048
  -- are the rows of the single-process run, on every rank; also when one rank's shard is empty (a single photon).
* the library's own RCCL communicator (physicl_amd.comm.NativeCounterComm) with the world of one a one-GPU box allows (two ranks
  on one device are refused by RCCL, tests/test_gpu_comm.py): the same payload goes through the real
  pcl_comm_allreduce_sum_i64, which takes 2048 values per call, and gives the plain rows; the list form raises there.
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
N, n_bins = %(N)d, %(n_bins)d
lo, hi = float(np.asarray(phys.light.E_from_wavelength(700e-9))), float(np.asarray(phys.light.E_from_wavelength(200e-9)))
sim = phys.Simulation(cl_on=True, device=0, comm=comm if comm.world > 1 else None, seed=21, rng="philox", exit=lambda s: s.t >= 0.0065)
sim.add_objs(phys.light.generate_photons_bulk(N, min=lo, max=hi, seed=21))
sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.001)))
sim.add_step(1, phys.newton.NewtonianKinematicsStep())
sim.add_step(2, phys.light.ScatterIsotropicStep(A=np.double(0.001), n=np.double(0.001), wavelength_dep_scattering=False))
m = phys.light.ScatterMeasureStep(None, True, [[6e5, np.nan, np.nan], [np.nan, 0.0, np.nan], [np.nan, np.nan, 1e5], [9e5, np.nan, np.nan]],
                                  measure_E=True, E_bins=np.linspace(lo * 1.05, hi * 0.95, n_bins + 1))
sim.add_step(3, m)
sim.run()
assert sim.error is None, sim.error
print(json.dumps({"rank": comm.rank, "rows": [[x.tolist() if isinstance(x, np.ndarray) else float(x) for x in r] for r in m.data],
                  "local": int(sim._dev.count)}))
comm.close()
"""


def run_world(world, N, n_bins):
    return rank_world.run_world(WORKER % {"root": ROOT, "N": N, "n_bins": n_bins}, world)


@pytest.mark.parametrize("N,n_bins", [(150001, 1024), (150001, 50), (1, 1024)], ids=["payload_4101", "payload_205", "empty_shard"])
def test_two_shards_reproduce_the_single_process_binned_rows(N, n_bins):
    one = run_world(1, N, n_bins)[0]
    two = run_world(2, N, n_bins)
    for rank in two:
        assert rank["rows"] == one["rows"]                   # every rank records the GLOBAL rows
    assert two[0]["local"] + two[1]["local"] == one["local"] == N
    if N == 1:
        assert two[0]["local"] == 0                          # rank 0 holds nothing and still joins every collective
    rows = one["rows"]
    assert len(rows) >= 5 and all(len(r) == 10 and len(r[3]) == n_bins for r in rows)
    assert sum(r[2] + r[4] + r[6] + r[8] for r in rows) > 0
    if N > 1:
        assert sum(sum(r[3]) for r in rows) > 0              # photons were binned, not only counted


def planck_like(native, E_bins):
    import physicl_amd as phys
    import physicl_amd.light as light
    import physicl_amd.newton as newton
    from physicl_amd.comm import NativeCounterComm
    comm = NativeCounterComm(0, 1, exchange=lambda ident: ident) if native else None
    sim = phys.Simulation(exit=lambda s: len(s.ts) >= 8, seed=3, rng="philox", comm=comm)
    sim.add_objs(light.generate_photons_bulk(50_000, min=1.0, max=2.0, seed=3))
    sim.add_step(0, phys.UpdateTimeStep(lambda s: np.double(0.001)))
    sim.add_step(1, newton.NewtonianKinematicsStep())
    sim.add_step(2, light.ScatterIsotropicStep(A=np.double(0.001), n=np.double(0.001)))
    m = light.ScatterMeasureStep(None, True, [[6e5, np.nan, np.nan], [np.nan, 0.0, np.nan], [np.nan, np.nan, 1e5], [9e5, np.nan, np.nan]],
                                 measure_E=True, E_bins=E_bins)
    sim.add_step(3, m)
    sim.start()
    sim.join()
    err = sim.error
    if comm is not None:                                     # the communicator lives on the simulation's context: it goes first
        assert comm.info()["ranks_seen"] == 1 and comm.rccl_version
        comm.close()
    sim.close(download=False)
    return err, [[x.tolist() if isinstance(x, np.ndarray) else x for x in r] for r in m.data]


def test_binned_step_runs_on_the_library_s_rccl_communicator_where_the_list_form_raises():
    edges = np.linspace(1.05, 1.95, 1025)                    # 1 + 4 + 4 x 1024 values per pass: more than one call takes
    err, plain = planck_like(False, edges)
    assert err is None and len(plain) == 8
    err, native = planck_like(True, edges)
    assert err is None, err
    assert native == plain and sum(sum(r[3]) for r in plain) > 0
    err, _ = planck_like(True, None)                         # the list form: lists do not sum
    assert isinstance(err, NotImplementedError)
