"""States, tables and the comparison for the tests of PathAbsorptionStep (tests/test_path_absorb_cpu.py and the GPU tests).  Not a test
file: a helper they import.  The restatement of the kernel itself is physicl_amd.light._absorb_path; nothing here has a tolerance.

The layout of a state (``layout``).  Everybody moves at c with a random direction, stands at a random radius between 1.05 and 2.95
about CENTER (inside the two layers of EDGES) and has a random energy between 1.05 and 2.95 (inside the three bands of E_EDGES),
except for the planted slots -- a later line wins over an earlier one:
    v:  i % 3 == 0   at rest (of these, i % 6 == 0 carries a -0.0);       i % 13 == 0   a NaN in v0 (moving)
        i % 29 == 0  v = (0, 0, c): moving, but not by v0
    r:  i % 5 == 0   exactly on the first radius (layer 0);              i % 7 == 0    exactly on the last radius (layer 1: closed)
        i % 11 == 0  a NaN in r (no layer);   i % 17 == 0  beyond the last radius;   i % 19 == 0  inside the first radius (both: none)
        i % 23 == 0  exactly on the inner edge (layer 1)
    E:  i % 4 == 1   exactly on a band edge, 1.5 (band 1);               i % 9 == 2    exactly on the last band edge (band 2: closed)
        i % 10 == 3  NaN (no band);   i % 14 == 5  below the first edge;   i % 15 == 7  above the last edge (both: none)
        i % 16 == 9  exactly on the first edge (band 0)
All planted values are exact in float32 as well, and so are their distances from CENTER and the squares of those.
"""
import numpy as np

from physicl_amd import light
from writer_reference import photons, same_bits, wide

C = 299792458.0
SEED = 0x5EED5A7F
ID_BASE = 7_000_000_001
CENTER = np.array([0.5, -0.25, 0.125])
EDGES = np.array([1.0, 2.0, 3.0])                     # two layers
E_EDGES = np.array([1.0, 1.5, 2.0, 3.0])              # three bands
# a transparent cell and a black one among them; every value is a float64 the device gets as it stands
P_CELLS = np.array([[0.0, 0.25, 1.0], [0.5, 0.75, 0.125]])
P_LAYERS = np.array([0.25, 0.75])
P_BANDS = np.array([0.0, 0.5, 1.0])
P_GREY = 0.5
R_PLANTS = ((5, 1.0, 0), (7, 3.0, 1), (11, np.nan, -1), (17, 3.5, -1), (19, 0.5, -1), (23, 2.0, 1))       # modulus, radius, layer
E_PLANTS = ((4, 1, 1.5, 1), (9, 2, 3.0, 2), (10, 3, np.nan, -1), (14, 5, 0.5, -1), (15, 7, 3.5, -1), (16, 9, 1.0, 0))   # mod, rest, E, band


def configs():
    """name -> (p, edges, E_edges): layers and bands, layers only, bands only, neither."""
    return {"both": (P_CELLS, EDGES, E_EDGES), "layers": (P_LAYERS, EDGES, None), "bands": (P_BANDS, None, E_EDGES),
            "neither": (P_GREY, None, None)}


def unit(x):
    return x / np.sqrt((x * x).sum(axis=1))[:, None]


def layout(n, dtype=np.float64, seed=1):
    """{"r", "v", "dr", "dv": (n, 3), "E": (n,)} of float64 arrays that hold ``dtype`` values, laid out as the module's docstring
    says."""
    rng = np.random.RandomState(seed + n)
    i = np.arange(n)
    r = CENTER + rng.uniform(1.05, 2.95, size=n)[:, None] * unit(rng.normal(size=(n, 3)))
    v = C * unit(rng.normal(size=(n, 3)))
    E = rng.uniform(1.05, 2.95, size=n)
    v[i % 3 == 0] = 0.0
    v[i % 6 == 0, 1] = -0.0
    v[i % 13 == 0, 0] = np.nan
    v[i % 29 == 0] = [0.0, 0.0, C]
    for mod, radius, _ in R_PLANTS:
        r[i % mod == 0] = CENTER + np.array([radius, 0.0, 0.0])
    for mod, rest, value, _ in E_PLANTS:
        E[i % mod == rest] = value
    state = {"r": r, "v": v, "dr": rng.normal(size=(n, 3)), "dv": rng.normal(size=(n, 3)), "E": E}
    return {k: a.astype(dtype).astype(np.float64) for k, a in state.items()}


def planted(n):
    """(moving, layer, band) by the layout's own arithmetic on the slot numbers: who moves, and for the planted slots the layer and
    the band they must be found in (-1: none; -2: not planted, a random value inside)."""
    i = np.arange(n)
    moving = (i % 3 != 0) | (i % 13 == 0) | (i % 29 == 0)
    layer, band = np.full(n, -2), np.full(n, -2)
    for mod, _, b in R_PLANTS:
        layer[i % mod == 0] = b
    for mod, rest, _, e in E_PLANTS:
        band[i % mod == rest] = e
    return moving, layer, band


def check_path_absorb(before, after, answer, p, edges, center, E_edges, seed, n_pass, what):
    """A state downloaded before the sweep, the state downloaded after it and the sweep's answer against the numpy restatement: no
    tolerance anywhere.  ``answer``: (exposed, absorbed, absorbed_by_cell).  Returns the restatement's dict."""
    b, a = wide(before), wide(after)
    T = np.asarray(before["E"]).dtype.type
    ref = light._absorb_path(b["r"], b["v"], b["dv"], np.asarray(before["E"]).astype(np.float64), photons(before), before["id"], p, edges,
                             center, E_edges, seed, n_pass, T)
    for f in set(before) - {"r", "v", "dr", "dv", "count"}:              # E, ids, kinds
        assert same_bits(before[f], after[f]), (what, f)
    assert before.get("count") == after.get("count") and len(before["E"]) == len(after["E"]), what
    for f in ("r", "dr"):
        assert same_bits(a[f], b[f]), (what, f)
    gone = ref["absorbed"]
    for f in ("v", "dv"):
        assert same_bits(a[f], ref[f].astype(T).astype(np.float64)), (what, f)
        assert same_bits(a[f][~gone], b[f][~gone]), (what, f)           # who is not absorbed is not written
        assert same_bits(a[f][gone], np.zeros((int(gone.sum()), 3))), (what, f)             # +0.0, bit for bit
    exposed, absorbed, cells = answer
    print("%s: exposed %d, absorbed %d of %d" % (what, ref["exposed"].sum(), gone.sum(), len(gone)))
    assert (int(exposed), int(absorbed)) == (int(ref["exposed"].sum()), int(gone.sum())), what
    assert np.asarray(cells).shape == ref["absorbed_by_cell"].shape and np.asarray(cells).tolist() == ref["absorbed_by_cell"].tolist(), what
    assert int(np.asarray(cells).sum()) == int(absorbed), what
    return ref


# ------------------------------------------------------------------------------------------------ the ABI, by hand
def abi_args(**kw):
    """The arguments of a good call (behind the context), and what ``kw`` changes of them: L, B, p, edges, center, E_edges, counts,
    cells."""
    a = dict(L=2, B=3, p=P_CELLS, edges=EDGES, center=CENTER, E_edges=E_EDGES, counts=np.full(4, -7, dtype=np.int64),
             cells=np.full(4096 + 2, -7, dtype=np.int64))
    a.update(kw)
    arr = lambda x: None if x is None else np.ascontiguousarray(x, dtype=np.float64)                        # noqa: E731
    keep = [arr(a[k]) for k in ("p", "edges", "center", "E_edges")]
    ptr = lambda x: None if x is None else x.ctypes.data                                                    # noqa: E731
    return keep, (int(a["L"]), int(a["B"]), ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), 1, 1, ptr(a["counts"]),
                  ptr(a["cells"])), (a["counts"], a["cells"])


BAD_CALLS = [dict(p=None), dict(counts=None), dict(cells=None), dict(L=-1), dict(B=-1),
             dict(L=65, p=np.full((65, 3), 0.5), edges=np.arange(66.0)), dict(B=1025, p=np.full((2, 1025), 0.5), E_edges=np.arange(1026.0)),
             dict(L=64, B=65, p=np.full((64, 65), 0.5), edges=np.arange(65.0), E_edges=np.arange(66.0)),                 # 4160 cells
             dict(p=[[0.0, 0.25, 1.5], [0.5, 0.75, 0.125]]), dict(p=[[0.0, 0.25, 1.0], [0.5, np.nan, 0.125]]),
             dict(p=[[-0.1, 0.25, 1.0], [0.5, 0.75, 0.125]]), dict(L=0, B=0, p=[1.5]), dict(edges=None), dict(E_edges=None),
             dict(edges=[1.0, 3.0, 2.0]), dict(edges=[-1.0, 2.0, 3.0]), dict(edges=[1.0, 2.0, np.inf]), dict(edges=[1.0, 2.0, 1e200]),
             dict(edges=[1.0, 1.0, 3.0]), dict(E_edges=[1.0, 2.0, 1.5, 3.0]), dict(E_edges=[1.0, 1.5, np.nan, 3.0]),
             dict(E_edges=[1.0, 1.5, 2.0, np.inf]), dict(center=[0, np.nan, 0]), dict(center=[np.inf, 0, 0])]
