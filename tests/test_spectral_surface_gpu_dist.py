"""GPU: SpectralSurfaceStep on a sharded run of two processes -- tests/test_gpu_writers_dist.py's pattern, its worker and its
comparison, as tests/test_writer_refract_gpu_dist.py has them.

2 processes sharing device 0, gloo for the all-reduce: after the case's passes the photons of the two shards, by id, and the
per-pass rows of the step are those of the single-process run: a photon meets the same fate however the run is sharded, and the
four counts and both rows by band are all-reduced -- the rows add.  N = 4097 is two 2048-particle tiles plus one, so the shard
boundary falls inside a tile.

10 passes of a scattering medium about a ground of radius 1 that the lamp stands one radius above, with the shell tally of the same
radius in front of the step: random walkers come down on it pass after pass.  Three bands between 1.25 and 2.75; the photons'
energies reach from 1 to 3.
"""
import pytest

from test_gpu_writers_dist import DISC, run_world

pytestmark = pytest.mark.gpu

CASE = dict(name="spectral", N=4097, passes=10, fields=("r", "v", "dr", "dv", "E"), rows=("rows", "in"), note="", steps=DISC + """\
tally = phys.light.ShellCrossingMeasureStep(None, [1.0])
step = phys.light.SpectralSurfaceStep(1.0, [0.05, 1.0, 0.5], [1.25, 1.75, 2.25, 2.75], specular=[1.0, 0.5, 0.0])
sim.add_step(3, tally)
sim.add_step(4, step)
""", record='{"rows": [[int(x) for x in list(row)[1:5]] + [row[5].tolist(), row[6].tolist()] for row in step.data], '
            '"in": [int(row[3][0]) for row in tally.data]}')


def test_two_shards_hold_the_single_process_run_s_photons():
    N, fields = CASE["N"], CASE["fields"]
    one = run_world(CASE, 1)[0]
    two = run_world(CASE, 2)
    for rank in two:
        for key in CASE["rows"]:
            assert rank[key] == one[key], key                          # every rank records the GLOBAL counts and rows
        assert "one launch per light step" in rank["note"]
    assert len(one["rows"]) == 10
    for (refl, gone, mirrored, none, by_refl, by_gone), inn in zip(one["rows"], one["in"]):
        assert inn == refl + gone and sum(by_refl) == refl and sum(by_gone) == gone - none     # the shell in front counts the same photons
    sums = [sum(row[k] for row in one["rows"]) for k in range(4)]
    # every outcome, read off the global counts (a worker keeps no state for a restatement: tests/test_spectral_surface_gpu.py
    # restates a Simulation's passes): diffuse = reflected - mirrored, mirrored, absorbed in a band = absorbed - out_of_band,
    # out_of_band, and in every pass somebody who is not hit
    diffuse, mirrored, in_band, none = sums[0] - sums[2], sums[2], sums[1] - sums[3], sums[3]
    assert sums[0] > 100 and min(diffuse, mirrored, in_band, none) > 0 and max(one["in"]) < N, sums
    by_id = {i: row for rank in two for i, *row in zip(rank["ids"], *(rank[f] for f in fields))}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, *row in zip(one["ids"], *(one[f] for f in fields)):
        assert by_id[i] == row, i
