"""GPU: PlaneFluxMapStep on a sharded run of two processes.

2 processes sharing device 0, gloo for the all-reduce (tests/rank_world.py): the rows of a sharded Simulation -- [N, up, down, up_map,
down_map] all-reduced in one collective per pass, 1 + 2 x 3 + 2 x 3 x 2 x 16 x 12 = 2311 values, i.e. two pieces of at most 2048 -- and the
exposures are those of the single-process run, on every rank; also when one rank's shard is empty.
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
flux = phys.light.PlaneFluxMapStep(None, "x", [-4e5, 2.5e5, 9e5], [np.linspace(-2e6, 2e6, 17), np.linspace(-2e6, 2e6, 13)], E_bins=[1.0, 2.0, 3.0], frames=True)
sim.add_step(3, flux)
sim.run()
assert sim.error is None, sim.error
print(json.dumps({"rank": comm.rank, "rows": [[x.tolist() if isinstance(x, np.ndarray) else float(x) for x in r] for r in flux.data],
                  "up_map": flux.up_map.tolist(), "down_map": flux.down_map.tolist(), "last": [flux.up.tolist(), flux.down.tolist()],
                  "local": int(sim._dev.count), "note": sim.launch_note}))
comm.close()
"""


def run_world(world, N):
    return rank_world.run_world(WORKER % {"root": ROOT, "N": N}, world)


@pytest.mark.parametrize("N", [20001, 1], ids=["payload_2311", "empty_shard"])
def test_two_shards_reproduce_the_single_process_rows(N):
    import numpy as np
    one = run_world(1, N)[0]
    two = run_world(2, N)
    for rank in two:
        assert rank["rows"] == one["rows"]                   # every rank records the GLOBAL rows
        assert rank["up_map"] == one["up_map"] and rank["down_map"] == one["down_map"] and rank["last"] == one["last"]
        assert "PlaneFluxMapStep" in rank["note"]
    assert two[0]["local"] + two[1]["local"] == one["local"] == N
    if N == 1:
        assert two[0]["local"] == 0                          # rank 0 holds nothing and still joins every collective
    rows = one["rows"]
    assert len(rows) >= 5 and all(len(r) == 6 and r[1] == N and np.shape(r[4]) == np.shape(r[5]) == (3, 2, 16, 12) for r in rows)
    assert np.array_equal(one["up_map"], np.sum([r[4] for r in rows], axis=0))              # the exposure is the sum of the passes' frames
    assert np.array_equal(one["down_map"], np.sum([r[5] for r in rows], axis=0))
    if N > 1:
        up, down = np.sum([r[2] for r in rows], axis=0), np.sum([r[3] for r in rows], axis=0)
        assert up[1:].min() > 0 and down.sum() > 0 and 0 < np.sum(one["up_map"]) <= up.sum() and np.count_nonzero(one["up_map"]) > 100
