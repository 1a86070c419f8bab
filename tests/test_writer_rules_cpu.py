"""The rules the writer sweeps' numpy restatements are built from (physicl_amd/light.py), each on its own: exact, no tolerance
but the frame's 4 ulp."""
import numpy as np
import pytest

from physicl_amd import light

EDGES = np.array([0.5, 1.0, 2.0, 3.0])
E_EDGES = np.array([1.0, 2.0, 4.0, 8.0])
EPS = np.finfo(np.float64).eps


def plain_bin(v, edges):
    """numpy.histogram's bin, spelt out: [e_b, e_(b+1)), the last one closed, -1 outside and for a NaN."""
    if not (v >= edges[0] and v <= edges[-1]):
        return -1
    if v == edges[-1]:
        return len(edges) - 2
    return max(b for b in range(len(edges) - 1) if edges[b] <= v)


def around(e):
    return [np.nextafter(e, -np.inf), e, np.nextafter(e, np.inf)]


def test_bin_of_at_every_edge():
    values = np.array([x for e in E_EDGES for x in around(e)] + [0.25, 100.0, np.nan, np.inf, -np.inf, 3.0])
    got = light._bin_of(values, E_EDGES)
    assert got.dtype == np.int64
    assert got.tolist() == [plain_bin(v, E_EDGES) for v in values]
    # an energy on a bin edge opens the bin above it; the last edge closes the last bin; just outside is in no bin
    assert got[:9].tolist() == [-1, 0, 0, 0, 1, 1, 1, 2, 2] and got[9:12].tolist() == [2, 2, -1]
    assert got[12:17].tolist() == [-1, -1, -1, -1, -1]
    # the histogram numpy itself makes of the values inside
    inside = values[got >= 0]
    assert np.array_equal(np.bincount(got[got >= 0], minlength=3), np.histogram(inside, bins=E_EDGES)[0])


def test_bin_of_one_bin():
    got = light._bin_of(np.array([0.9, 1.0, 1.5, 2.0, 2.1, np.nan]), np.array([1.0, 2.0]))
    assert got.tolist() == [-1, 0, 0, 0, -1, -1]


def test_layer_of_compares_q_with_squared_edges():
    center = np.array([0.25, -1.0, 2.0])
    xs = [x for e in EDGES for x in around(e)]
    rows = [(x, 0.0, 0.0) for x in xs] + [(0.0, -x, 0.0) for x in xs] + [(0.0, 0.0, x) for x in xs]
    rows += [(np.nan, 0.0, 0.0), (0.0, np.inf, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (9.0, 0.0, 0.0)]
    d = np.array(rows)
    got = light._layer_of(d + center, EDGES, center)
    d = (d + center) - center                                  # what the rule itself subtracts
    q = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert got.tolist() == [plain_bin(v, EDGES * EDGES) for v in q]
    # q both just inside and just outside the innermost and the outermost edge, and exactly on every edge
    e2 = EDGES * EDGES
    on = np.array([[e, 0.0, 0.0] for e in EDGES])
    assert light._layer_of(on, EDGES, np.zeros(3)).tolist() == [0, 1, 2, 2]
    for e, below, above in ((EDGES[0], -1, 0), (EDGES[-1], 2, -1)):       # the layer one ulp below and one ulp above the edge
        lo, hi = np.nextafter(e, 0.0), np.nextafter(e, 9.0)
        assert lo * lo < e * e < hi * hi                       # (one ulp of the radius moves the square)
        assert light._layer_of(np.array([[lo, 0.0, 0.0], [hi, 0.0, 0.0]]), EDGES, np.zeros(3)).tolist() == [below, above]
    assert e2[0] == 0.25
    # no edges: one layer that holds everything, a NaN included
    assert light._layer_of(np.array(rows), None, center).tolist() == [0] * len(rows)


def test_at_rest_and_scattered():
    v = np.array([[0.0, 0.0, 0.0], [-0.0, 0.0, -0.0], [0.0, 1e-300, 0.0], [np.nan, 0.0, 0.0], [0.0, 0.0, np.inf]])
    assert light._at_rest(v).tolist() == [True, True, False, False, False]
    assert light._scattered(v, [True] * 5).tolist() == [False, False, True, True, True]
    assert light._scattered(v, [True, True, False, True, False]).tolist() == [False, False, False, True, False]
    assert light._workable(np.array([0.0, -0.0, 1e-320, 1.0, np.inf, np.nan])).tolist() == [False, False, True, True, False, False]


def test_stored_rounds_once():
    x = np.array([1.0 + 2.0 ** -30, 1e-50, 1e300, np.nan])
    assert np.array_equal(light._stored(x, np.float64), x, equal_nan=True) and light._stored(x, np.float64).dtype == np.float64
    with np.errstate(over="ignore"):
        assert np.array_equal(light._stored(x, np.float32), np.array([1.0, 0.0, np.inf, np.nan]), equal_nan=True)


def test_frame_is_orthonormal_to_4_ulp():
    rs = np.random.RandomState(7)
    w = rs.normal(size=(6, 3))
    w = w / np.sqrt((w * w).sum(axis=1))[:, None]
    w = np.concatenate([np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [-0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, -1.0, -0.0]]), w])
    e1, e2 = light._frame(w)
    dot = lambda x, y: (x[:, 0] * y[:, 0] + x[:, 1] * y[:, 1]) + x[:, 2] * y[:, 2]   # noqa: E731
    for name, val, want in (("e1.e1", dot(e1, e1), 1.0), ("e2.e2", dot(e2, e2), 1.0), ("e1.e2", dot(e1, e2), 0.0),
                            ("e1.w", dot(e1, w), 0.0), ("e2.w", dot(e2, w), 0.0)):
        err = np.abs(val - want) / EPS
        print(name, err.max())
        assert np.all(err <= 4.0), (name, err)
    # the poles are exact
    assert np.array_equal(e1[0], [1.0, 0.0, -0.0]) and np.array_equal(e2[0], [0.0, 1.0, -0.0])
    assert np.array_equal(e1[1], [1.0, -0.0, 0.0]) and np.array_equal(e2[1], [0.0, -1.0, -0.0])


@pytest.mark.parametrize("law, phase, g", [("isotropic", "isotropic", 0.0), (("hg", 0.85), "hg", 0.85), ("rayleigh", "rayleigh", 0.0)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_one_law_without_edges_is_the_phase_function(law, phase, g, dtype):
    rs = np.random.RandomState(11)
    n = 1500
    c = 299792458.0
    v = rs.normal(size=(n, 3)) * c
    dv = np.where(rs.rand(n, 1) < 0.7, rs.normal(size=(n, 3)) * c, 0.0)
    v[:5], dv[:5] = dv[:5], dv[:5]                             # an old velocity of zero: scattered, not re-directed
    dv[5, 0], v[6, 1] = np.nan, np.inf
    photon = rs.rand(n) < 0.9
    ids = rs.permutation(n).astype(np.int64) + (1 << 32)
    one = light._phase_redirect(v, dv, photon, ids, phase, g, c, 99, 3, dtype)
    laws, _, cum, edges, center = light._check_layered_phase([law], None, None, (0, 0, 0))
    two = light._layered_phase_apply(np.zeros((n, 3)), v, dv, photon, ids, laws, cum, edges, center, c, 99, 3, dtype)
    assert one["redirected"].sum() > 500
    for key in ("v", "dv", "mu", "w"):
        assert one[key].dtype == two[key].dtype and one[key].shape == two[key].shape
        assert one[key].tobytes() == two[key].tobytes(), key
    assert np.array_equal(one["redirected"], two["redirected"])
