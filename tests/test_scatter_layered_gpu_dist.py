"""GPU: LayeredScatterStep on a sharded run of two processes -- tests/test_gpu_writers_dist.py's pattern, its worker and its
comparison, for this writer step.

2 processes sharing device 0, gloo for the all-reduce: after the case's passes the photons of the two shards, by id, and the
per-pass rows of the step are those of the single-process run: a photon draws the same numbers however the run is sharded, and the
two counts and the cells are all-reduced.  N = 4097 is two 2048-particle tiles plus one, so the shard boundary falls inside a tile.

8 passes of a cloud of two layers and two bands behind the clear air's scatter step (``first`` resolves to False on every rank), with
a forward-peaked phase function in the cloud, an absorbing medium and a grey ground behind it.
"""
import pytest

from test_gpu_writers_dist import DISC, run_world

pytestmark = pytest.mark.gpu

CASE = dict(name="scatter_layered", N=4097, passes=8, fields=("r", "v", "E"), rows=("rows", "first", "redirected"), note="LayeredScatterStep",
            steps=DISC + """\
step = phys.light.LayeredScatterStep([[1.2, 0.0], [0.2, 0.6]], [1.0, 2.0, 3.0], (0, 0, 0), [1.0, 2.0, 3.0])
sim.add_step(3, step)
phase = phys.light.LayeredPhaseStep(["rayleigh", ("hg", 0.85)], [[0.2, 0.8], [1.0, 0.0]], edges=[1.0, 2.0, 3.0])
sim.add_step(4, phase)
sim.add_step(5, phys.light.AbsorptionStep((0.9, 1.0), edges=[1.0, 2.0, 3.0]))
sim.add_step(6, phys.light.SurfaceReflectStep(1.0, albedo=0.5))
""", record='{"rows": [[int(row[1]), int(row[2]), np.asarray(row[3]).tolist()] for row in step.data], "first": step.first, '
            '"redirected": [int(row[2]) for row in phase.data]}')


def test_two_shards_hold_the_single_process_run_s_photons():
    N, fields = CASE["N"], CASE["fields"]
    one = run_world(CASE, 1)[0]
    two = run_world(CASE, 2)
    for rank in two:
        for key in CASE["rows"]:
            assert rank[key] == one[key], key                          # every rank records the GLOBAL counts and tallies
        assert "one launch per light step" in rank["note"] and CASE["note"] in rank["note"]
    assert len(one["rows"]) == 8 and one["first"] is False
    for (exposed, scattered, cells), redirected in zip(one["rows"], one["redirected"]):
        assert 0 < scattered < exposed <= N and sum(map(sum, cells)) == scattered and cells[0][1] == 0 and len(cells) == 2 == len(cells[0])
        assert redirected > 0
    assert all(sum(row[2][b][e] for row in one["rows"]) > 0 for b, e in ((0, 0), (1, 0), (1, 1)))
    by_id = {i: row for rank in two for i, *row in zip(rank["ids"], *(rank[f] for f in fields))}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, *row in zip(one["ids"], *(one[f] for f in fields)):
        assert by_id[i] == row, i
