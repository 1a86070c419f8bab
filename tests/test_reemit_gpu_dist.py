"""GPU: ReemissionStep on a sharded run of two processes -- tests/test_gpu_writers_dist.py's pattern, its worker and its comparison,
for the seventh writer step.

2 processes sharing device 0, gloo for the all-reduce: after the case's passes the photons of the two shards, by id, and the
per-pass rows of the step are those of the single-process run: a photon draws the same numbers however the run is sharded, and
the 2 + L' counts are all-reduced.  N = 4097 is two 2048-particle tiles plus one, so the shard boundary falls inside a tile.

8 passes of an atmosphere with a grey gas in two layers over a black ground: the ground's thin shell re-emits upward (lambertian)
from a table with a lifetime of two passes, the lower gas layer at once and isotropically from another table, the upper one keeps
its photons' energies.
"""
import pytest

from test_gpu_writers_dist import DISC, run_world

pytestmark = pytest.mark.gpu

CASE = dict(name="reemit", N=4097, passes=8, fields=("r", "v", "E"), rows=("rows", "absorbed"), note="", steps=DISC + """\
gas = phys.light.PathAbsorptionStep([0.4, 0.2], [1.0, 2.0, 3.0])
sim.add_step(3, gas)
sim.add_step(4, phys.light.SurfaceReflectStep(1.0, albedo=0.0))
step = phys.light.ReemissionStep([([0.25, 0.5], [0.5, 1.0]), ([0.75, 0.875], [0.25, 1.0]), None], [1.0 - 1e-6, 1.0 + 1e-6, 2.0, 3.0],
                                 eta=[0.5, 1.0, 1.0], angular=["lambertian", "isotropic", "isotropic"])
sim.add_step(5, step)
""", record='{"rows": [[int(row[1]), int(row[2]), np.asarray(row[3]).tolist()] for row in step.data], '
            '"absorbed": [int(row[2]) for row in gas.data]}')


def test_two_shards_hold_the_single_process_run_s_photons():
    N, fields = CASE["N"], CASE["fields"]
    one = run_world(CASE, 1)[0]
    two = run_world(CASE, 2)
    for rank in two:
        for key in CASE["rows"]:
            assert rank[key] == one[key], key                          # every rank records the GLOBAL counts and tallies
        assert "one launch per light step" in rank["note"]
    assert len(one["rows"]) == 8
    for parked, reemitted, by_layer in one["rows"]:
        assert 0 < reemitted <= parked <= N and sum(by_layer) == reemitted and len(by_layer) == 3
    assert all(sum(row[2][b] for row in one["rows"]) > 0 for b in range(3))                 # the ground and both gas layers had work
    assert sum(e in (0.25, 0.5, 0.75, 0.875) for e in one["E"]) > N // 4                    # many slots carry a re-emitted energy by then
    by_id = {i: row for rank in two for i, *row in zip(rank["ids"], *(rank[f] for f in fields))}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, *row in zip(one["ids"], *(one[f] for f in fields)):
        assert by_id[i] == row, i
