"""GPU: GridAbsorptionStep on a sharded run of two processes -- tests/test_gpu_writers_dist.py's pattern, its worker and its
comparison, as tests/test_writers_grid_phase_gpu_dist.py uses them.

2 processes sharing device 0, gloo for the all-reduce: after the case's passes the photons of the two shards, by id, and the per-pass
rows of the step are those of the single-process run: a photon draws the same numbers however the run is sharded, and the four counts
and the heating field -- 4352 cells, more than one piece of the collective -- are all-reduced.  N = 4097 is two 2048-particle tiles
plus one, so the shard boundary falls inside a tile.

6 passes of the broken cloud field of 17 x 16 x 16 = 4352 cells -- cloudy columns on a checkerboard in x and y -- behind the clear
air's scatter step: a GridScatterStep decides where the droplets scatter, the GridAbsorptionStep behind it gives the cloudy cells an
omega0 of 0.8 and one column of cells an absorption coefficient.
"""
import pytest

from test_gpu_writers_dist import DISC, run_world

pytestmark = pytest.mark.gpu

CASE = dict(name="absorb_grid", N=4097, passes=6, fields=("r", "v", "E"), rows=("rows", "cells", "scattered"),
            note="GridScatterStep",                                    # (the pass's first writer step is the one the note names)
            steps=DISC + """\
ix, iy, iz = np.indices((17, 16, 16))
cloudy = (ix + iy) %% 2 == 0
grid = [np.linspace(0.0, 4.0, 18), np.linspace(-2.0, 2.0, 17), np.linspace(-2.0, 2.0, 17)]
cloud = phys.light.GridScatterStep(np.where(cloudy, 1.5, 0.0), ("x", "y", "z"), grid)
sim.add_step(3, cloud)
step = phys.light.GridAbsorptionStep(("x", "y", "z"), grid, k=np.where((ix == 9) & (iy == 8), 1.0, 0.0), omega0=np.where(cloudy, 0.8, 1.0))
sim.add_step(4, step)
""", record='{"rows": [[int(x) for x in row[1:5]] for row in step.data], "cells": [row[5].sum(axis=2).tolist() for row in step.data], '
            '"scattered": [int(row[2]) for row in cloud.data]}')


def test_two_shards_hold_the_single_process_run_s_photons():
    N, fields = CASE["N"], CASE["fields"]
    one = run_world(CASE, 1)[0]
    two = run_world(CASE, 2)
    for rank in two:
        for key in CASE["rows"]:
            assert rank[key] == one[key], key                          # every rank records the GLOBAL counts and tallies
        assert "one launch per light step" in rank["note"] and CASE["note"] in rank["note"]
    assert len(one["rows"]) == 6
    for (exposed, interacted, on_path, at_hit), columns in zip(one["rows"], one["cells"]):
        assert 0 < interacted <= exposed <= N and sum(map(sum, columns)) == on_path + at_hit
    assert sum(row[2] for row in one["rows"]) > 0 and sum(row[3] for row in one["rows"]) > 0
    by_id = {i: row for rank in two for i, *row in zip(rank["ids"], *(rank[f] for f in fields))}
    assert len(by_id) == N == len(one["ids"]) and len(two[0]["ids"]) + len(two[1]["ids"]) == N
    for i, *row in zip(one["ids"], *(one[f] for f in fields)):
        assert by_id[i] == row, i
