"""GPU: RefractiveSurfaceStep on a sharded run of two processes -- tests/test_gpu_writers_dist.py's pattern, its worker and its
comparison, as tests/test_reemit_gpu_dist.py has them.

2 processes sharing device 0, gloo for the all-reduce: after the case's passes the photons of the two shards, by id, and the
per-pass rows of the step are those of the single-process run: a photon meets the same fate however the run is sharded, and the
six counts are all-reduced.  N = 4097 is two 2048-particle tiles plus one, so the shard boundary falls inside a tile.

10 passes of a scattering medium about a glass sphere of radius 1.5 that the lamp stands just outside of, with the shell tally of
the same radius in front of the step: random walkers cross it both ways, pass after pass.
"""
import pytest

from test_gpu_writers_dist import DISC, run_world

pytestmark = pytest.mark.gpu

CASE = dict(name="refract", N=4097, passes=10, fields=("r", "v", "dr", "dv"), rows=("rows", "shell"), note="", steps=DISC + """\
tally = phys.light.ShellCrossingMeasureStep(None, [1.5])
step = phys.light.RefractiveSurfaceStep(1.5, 1.5)
sim.add_step(3, tally)
sim.add_step(4, step)
""", record='{"rows": [[int(x) for x in list(row)[1:]] for row in step.data], '
            '"shell": [[int(row[2][0]), int(row[3][0])] for row in tally.data]}')


def test_two_shards_hold_the_single_process_run_s_photons():
    N, fields = CASE["N"], CASE["fields"]
    one = run_world(CASE, 1)[0]
    two = run_world(CASE, 2)
    for rank in two:
        for key in CASE["rows"]:
            assert rank[key] == one[key], key                          # every rank records the GLOBAL counts
        assert "one launch per light step" in rank["note"]
    assert len(one["rows"]) == 10
    for (i_t, i_r, o_t, o_r, o_tot, over), (out, inn) in zip(one["rows"], one["shell"]):
        assert inn == i_t + i_r and out == o_t + o_r + o_tot           # the shell in front counts the same crossings
    sums = [sum(row[k] for row in one["rows"]) for k in range(6)]
    assert min(sums[:5]) > 0 and sums[0] > N // 8, sums                # both directions, all three outcomes
    by_id = {i: row for rank in two for i, *row in zip(rank["ids"], *(rank[f] for f in fields))}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, *row in zip(one["ids"], *(one[f] for f in fields)):
        assert by_id[i] == row, i
