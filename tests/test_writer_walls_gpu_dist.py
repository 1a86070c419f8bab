"""GPU: BoxBoundaryStep on a sharded run of two processes -- tests/test_gpu_writers_dist.py's pattern, its worker and its comparison,
for this writer step.

2 processes sharing device 0, gloo for the all-reduce: after the case's passes the photons of the two shards, by id, and the
per-pass rows of the step are those of the single-process run: the rule reads no id, so a photon meets the same wall however the run
is sharded, and the eight counts are all-reduced.  N = 4097 is two 2048-particle tiles plus one, so the shard boundary falls inside a
tile.

8 passes of the clear air's scatter step in a box two moves wide about the source: periodic in x, mirrors in y, open in z.
"""
import pytest

from test_gpu_writers_dist import DISC, run_world

pytestmark = pytest.mark.gpu

CASE = dict(name="box_walls", N=4097, passes=8, fields=("r", "v", "E"), rows=("rows", "parked"), note="BoxBoundaryStep",
            steps=DISC + """\
step = phys.light.BoxBoundaryStep((1.0, -1.0, -1.0), (3.0, 1.0, 1.0), ("periodic", "mirror", "open"))
sim.add_step(3, step)
""", record='{"rows": [[int(row[1]), int(row[2]), np.asarray(row[3]).tolist()] for row in step.data], "parked": step.parked}')


def test_two_shards_hold_the_single_process_run_s_photons():
    N, fields = CASE["N"], CASE["fields"]
    one = run_world(CASE, 1)[0]
    two = run_world(CASE, 2)
    for rank in two:
        for key in CASE["rows"]:
            assert rank[key] == one[key], key                          # every rank records the GLOBAL counts
        assert "one launch per light step" in rank["note"] and CASE["note"] in rank["note"]
    assert len(one["rows"]) == 8
    moving = [row[0] for row in one["rows"]]
    total = [[sum(row[2][a][s] for row in one["rows"]) for s in range(2)] for a in range(3)]
    assert moving[0] == N and all(a >= b for a, b in zip(moving, moving[1:])) and moving[-1] < N     # what leaves through z is parked
    assert all(n > 0 for line in total for n in line) and N - moving[-1] + one["parked"] == sum(total[2])
    assert all(row[1] == 0 for row in one["rows"])                     # a move is a quarter of the box
    by_id = {i: row for rank in two for i, *row in zip(rank["ids"], *(rank[f] for f in fields))}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, *row in zip(one["ids"], *(one[f] for f in fields)):
        assert by_id[i] == row, i
