"""GPU: GridScatterStep on a sharded run of two processes -- tests/test_gpu_writers_dist.py's pattern, its worker and its comparison,
for this writer step.

2 processes sharing device 0, gloo for the all-reduce: after the case's passes the photons of the two shards, by id, and the
per-pass rows of the step are those of the single-process run: a photon draws the same numbers however the run is sharded, and the
two counts and the cells are all-reduced.  N = 4097 is two 2048-particle tiles plus one, so the shard boundary falls inside a tile.

6 passes of a field of 17 x 16 x 16 = 4352 cells -- the kernel's global form, and a row of three pieces of
``tally.ALLREDUCE_CHUNK`` for the collective -- behind the clear air's scatter step (``first`` resolves to False on every rank), with a
forward-peaked phase function behind it.  The cloudy columns are a checkerboard in x and y.
"""
import pytest

from test_gpu_writers_dist import DISC, run_world

pytestmark = pytest.mark.gpu

CASE = dict(name="scatter_grid", N=4097, passes=6, fields=("r", "v", "E"), rows=("rows", "first", "redirected"), note="GridScatterStep",
            steps=DISC + """\
ix, iy, iz = np.indices((17, 16, 16))
k = np.where((ix + iy) %% 2 == 0, 1.5, 0.0)
step = phys.light.GridScatterStep(k, ("x", "y", "z"), [np.linspace(0.0, 4.0, 18), np.linspace(-2.0, 2.0, 17), np.linspace(-2.0, 2.0, 17)])
sim.add_step(3, step)
phase = phys.light.PhaseFunctionStep("hg", 0.85)
sim.add_step(4, phase)
""", record='{"rows": [[int(row[1]), int(row[2]), np.asarray(row[3]).tolist()] for row in step.data], "first": step.first, '
            '"redirected": [int(row[1]) for row in phase.data]}')


def test_two_shards_hold_the_single_process_run_s_photons():
    N, fields = CASE["N"], CASE["fields"]
    one = run_world(CASE, 1)[0]
    two = run_world(CASE, 2)
    for rank in two:
        for key in CASE["rows"]:
            assert rank[key] == one[key], key                          # every rank records the GLOBAL counts and tallies
        assert "one launch per light step" in rank["note"] and CASE["note"] in rank["note"]
    assert len(one["rows"]) == 6 and one["first"] is False
    for (exposed, scattered, cells), redirected in zip(one["rows"], one["redirected"]):
        flat = [n for plane in cells for line in plane for n in line]
        assert 0 < scattered < exposed <= N and sum(flat) == scattered and len(flat) == 4352 and redirected >= scattered
        assert not any(cells[x][y][z] for x in range(17) for y in range(16) for z in range(16) if (x + y) % 2)
    by_id = {i: row for rank in two for i, *row in zip(rank["ids"], *(rank[f] for f in fields))}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, *row in zip(one["ids"], *(one[f] for f in fields)):
        assert by_id[i] == row, i
