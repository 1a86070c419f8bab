"""CPU: the one bin-edge check and the one centre check of physicl_amd/tally.py, through every constructor that uses them --
``E_bins`` of the binned spectrum, ``E_bins`` / ``mu_bins`` of the shell step, a Cartesian and a radius axis of the grid.
Every kind of bad input is a ValueError whose text names the offending argument (and the limit, where one is exceeded); the
inputs that only a transform makes bad (square for a radius, signed square for a cosine) are fine everywhere else."""
import numpy as np
import pytest

from physicl_amd import _hip, light, tally

NAN, INF = float("nan"), float("inf")

ENTRY = {                                                  # name in the message, constructor, transform
    "spectrum E_bins": ("E_bins", lambda e: light.ScatterMeasureStep(None, measure_E=True, E_bins=e), None),
    "shell E_bins": ("E_bins", lambda e: light.ShellCrossingMeasureStep(None, [1.0], E_bins=e), None),
    "shell mu_bins": ("mu_bins", lambda e: light.ShellCrossingMeasureStep(None, [1.0], mu_bins=e), "signed_square"),
    "grid x": ("axis 'x'", lambda e: light.PositionGridMeasureStep(None, ("x",), [e]), None),
    "grid r": ("axis 'r'", lambda e: light.PositionGridMeasureStep(None, ("r",), [e]), "square"),
}
BAD = {                                                    # bad for every entry point
    "NaN": [0.25, NAN, 0.75], "inf": [0.25, 0.5, INF], "not increasing": [0.25, 0.75, 0.5], "a tie": [0.25, 0.5, 0.5],
    "too many bins": np.linspace(0.0, 1.0, 1026), "wrong rank": [[0.25, 0.5], [0.5, 0.75]], "one edge": [0.5], "no edge": [],
    "a scalar": 0.5, "not numbers": "abc", "not an array": [[0.25], [0.5, 0.75]],
}
BY_TRANSFORM = {                                           # input -> the transforms it is bad under: the transform alone decides
    "the square is inf": ([0.0, 1e200], {"square", "signed_square"}),
    "the signed squares tie at +-0": ([-1e-200, 0, 1e-200], {"signed_square", "square"}),   # (a radius: negative as well)
    "the squares tie at 0": ([1e-200, 2e-200], {"square", "signed_square"}),
    "a negative radius": ([-0.5, 0.5], {"square"}),
}


@pytest.mark.parametrize("entry", sorted(ENTRY))
@pytest.mark.parametrize("kind", sorted(BAD))
def test_bad_edges_are_refused_by_name(entry, kind):
    name, make, _ = ENTRY[entry]
    with pytest.raises(ValueError) as e:
        make(BAD[kind])
    assert name in str(e.value)
    if kind == "too many bins":
        assert "1024" in str(e.value) and "1025" in str(e.value)        # the limit, and what was asked for


@pytest.mark.parametrize("entry", sorted(ENTRY))
@pytest.mark.parametrize("kind", sorted(BY_TRANSFORM))
def test_the_transform_alone_decides(entry, kind):
    name, make, transform = ENTRY[entry]
    edges, bad_under = BY_TRANSFORM[kind]
    if transform in bad_under:
        with pytest.raises(ValueError) as e:
            make(edges)
        assert name in str(e.value)
    else:
        make(edges)                                        # plain edges: finite and increasing is all that is asked


def test_limits_are_the_header_s_and_good_edges_come_back_as_float64():
    assert (_hip.GRID_MAX_BINS, _hip.SHELL_MAX_BINS, light._MAX_E_BINS) == (1024, 1024, 1024)
    for name, make, _ in ENTRY.values():
        make(np.linspace(0.0, 1.0, 1025))                  # 1024 bins: the most
    e = tally.check_edges("edges", range(4), 3, "square")
    assert e.dtype == np.float64 and e.flags.c_contiguous and e.tolist() == [0.0, 1.0, 2.0, 3.0]
    with pytest.raises(ValueError, match="edges.* 3 bins, at most 2"):
        tally.check_edges("edges", range(4), 2)


@pytest.mark.parametrize("make", [lambda c: light.PositionGridMeasureStep(None, ("x",), [[0.0, 1.0]], center=c),
                                  lambda c: light.ShellCrossingMeasureStep(None, [1.0], center=c)], ids=["grid", "shell"])
@pytest.mark.parametrize("center", [(0, NAN, 0), (0, INF, 0), (0, 0), (0, 0, 0, 0), 1.0, "c", None, [[0, 0, 0]]])
def test_a_bad_centre_is_refused_by_name(make, center):
    with pytest.raises(ValueError, match="center"):
        make(center)
    assert make((1, 2.5, -3)).center.tolist() == [1.0, 2.5, -3.0]
