"""GPU: the cosine of the scattering angle that the two phase sweeps (pcl_step_phase_redirect, pcl_step_phase_layered) leave in
the store, against exact arithmetic (tests/direction_exact.py) -- not against the numpy restatement, which shares the kernels'
formula and their operation order (tests/test_gpu_scatter_phase.py and test_layered_phase_gpu.py hold those two together).

A small store -- two full workgroups and a ragged wave, ids above 2^32 in scrambled order, one particle in ten a plain Object, a
few photons with dv = 0 -- is uploaded, swept once and downloaded.  Of every re-directed photon the old direction is recovered
from the download alone, w = (v' - dv') / |v' - dv'|, and mu_got = (v'.w) / c, in mpmath, is compared with ``mu_exact`` of the
photon's own draw (light._philox_block: tests/test_writer_streams_gpu.py holds it to the device); |v'| / c is 1 within the same
direction bound, and every row that is not re-directed is bit for bit what was uploaded.

Bound of |mu_got - mu_exact|: the law's (direction_exact.law_bound: what tests/test_direction_exact_cpu.py asks of the cosine in
double precision) + the contract of a direction built from the project's sincos (tests/writer_reference.py: DIR_ULP = 8 ulp(c)
per component of v', 8.5 ulp of float32 c in an fp32 store: sqrt 3 times that for the vector, relative to c) + one rounding of
dv' = v' - o, a value up to 2c: one more ulp(c) per component of the recovered o.

With the closed Henyey-Greenstein inverse alone (before the form for |g| < 1/2) the cases |g| <= 1e-8 fail in fp64 and
|g| <= 1e-17 in fp32, with an error up to 1: every photon at 90 degrees.  g = 1e-8 is below fp32's resolution and only holds the bound.
"""
import mpmath
import numpy as np
import pytest

from physicl_amd import light
from direction_exact import HG_SWITCH, dot, law_bound, mu_exact, norm, vec
from phase_reference import AXES, C, SEED, unit
from writer_reference import DIR_ULP, KIND_OBJECT, KIND_PHOTON, same_bits

pytestmark = pytest.mark.gpu

N = 2 * 256 + 37                                     # two full workgroups and a ragged wave
ID_BASE = 7_000_000_001                              # above 2^32: the counter's second word is in use
FIELDS = ("r", "v", "dr", "dv")
SQRT3 = 3.0 ** 0.5
DIR_BOUND = {"f64": (DIR_ULP + 1.0) * SQRT3 * 2.0 ** -52, "f32": (DIR_ULP + 0.5 + 1.0) * SQRT3 * 2.0 ** -23}
CENTER = np.array([0.5, -1.0, 2.0])
EDGES = np.array([1.0, 2.0, 3.0])                    # two layers, a hole inside and an outside
TABLE3 = ("table", [-1.0, 0.3, 1.0], [1.0, 5.0])
TABLE17 = ("table", np.linspace(-1.0, 1.0, 17), 1.0 + np.arange(16.0) % 5 + 0.1 * np.arange(16.0))
BELOW = float(np.nextafter(HG_SWITCH, 0.0))
PHASES = [("isotropic", 0.0), ("rayleigh", 0.0)] + [("hg", s * g) for g in (5e-324, 1e-17, 1e-12, 1e-8, 1e-3) for s in (1, -1)] + \
         [("hg", BELOW), ("hg", HG_SWITCH), ("hg", 0.85), ("hg", -0.999999)]
DECKS = {"one law": ([("hg", 1e-12)], None, None),
         "three laws, two layers": ([("hg", -1e-17), TABLE17, "rayleigh"], [[0.5, 0.3, 0.2], [0.0, 0.6, 0.4]], EDGES),
         "a table": ([TABLE3], None, EDGES[[0, -1]])}


@pytest.fixture(scope="module")
def dev():
    from physicl_amd import _hip
    d = _hip.Device(0)
    yield d
    d.close()


def population(dtype):
    """What is uploaded: old directions everywhere on the sphere, the first twelve along the axes (the frame's poles among them);
    rows with index % 50 == 7 were missed (dv = 0), those with index % 10 == 3 are plain Objects; r at 0.5, 1.5, 2.5 and 3.5 from
    CENTER, a fifth off either way: nobody near an edge."""
    T = np.float32 if dtype == "f32" else np.float64
    rng = np.random.RandomState(12)
    old, new = C * unit(rng.normal(size=(N, 3))), C * unit(rng.normal(size=(N, 3)))
    old[:12] = C * AXES[np.arange(12) % 6]
    i = np.arange(N)
    missed = i % 50 == 7
    old = old.astype(T).astype(np.float64)
    v = np.where(missed[:, None], old, new).astype(T).astype(np.float64)
    dv = (v - old).astype(T).astype(np.float64)
    assert not dv[missed].any() and dv[~missed].any(axis=1).all()
    r = CENTER + (0.5 + i % 4 + rng.uniform(-0.2, 0.2, size=N))[:, None] * unit(rng.normal(size=(N, 3)))
    return {"r": r, "v": v, "dr": rng.normal(size=(N, 3)), "dv": dv, "E": 1.0 + rng.uniform(size=N), "id_base": ID_BASE,
            "id": ID_BASE + rng.permutation(N).astype(np.int64), "kind": np.where(i % 10 == 3, KIND_OBJECT, KIND_PHOTON).astype(np.uint8)}


def sweep_and_compare(dev, dtype, call, laws, pick, go, n_pass, what):
    """Upload, ``call`` once, download; ``laws``: (kind, g, nodes, F) each, ``pick``: per particle the law it draws from, ``go``:
    who must be re-directed.  Returns the largest |mu_got - mu_exact| over its bound."""
    state = population(dtype)
    dev.store_alloc(N, dtype)
    dev.upload_state(state)
    before = dev.download_state()
    answer = call()
    after = dev.download_state()
    assert dev.count == N and same_bits(after["E"], before["E"]) and same_bits(after["id"], state["id"]), what
    b, a = ({f: np.stack(s[f], 1) for f in FIELDS} for s in (before, after))
    for f in ("v", "dv"):                                              # the store holds what was uploaded (values of its dtype)
        assert same_bits(b[f], state[f].astype(b[f].dtype)), (what, f)
    for f in FIELDS:                                                   # not re-directed: bit-identical; r and dr: everybody
        assert same_bits(a[f][~go], b[f][~go]), (what, f)
    assert same_bits(a["r"], b["r"]) and same_bits(a["dr"], b["dr"]), what
    assert 200 < go.sum() < N and not go[state["kind"] == KIND_OBJECT].any() and not go[np.arange(N) % 50 == 7].any()
    (u_a, _), (u_c, u_d) = (light._philox_block(state["id"], SEED, n_pass, word) for word in (10, 11))
    c, worst, speed = mpmath.mpf(C), 0.0, 0.0
    for i in np.flatnonzero(go):
        kind, g, nodes, F = laws[pick[i]]
        v_new = vec(a["v"][i])
        o = [x - y for x, y in zip(v_new, vec(a["dv"][i]))]            # the velocity before the scatter, from the download alone
        mu_got = dot(v_new, o) / (norm(o) * c)
        exact = mu_exact(kind, g, nodes, F, u_a[i], u_c[i], u_d[i])
        bound = law_bound(kind, g) + DIR_BOUND[dtype]
        err = float(abs(mu_got - mpmath.mpf(exact.numerator) / exact.denominator))
        worst, speed = max(worst, err / bound), max(speed, float(abs(norm(v_new) / c - 1)))
        assert err <= bound, (what, int(i), kind, g, float(mu_got), float(exact), err, bound)
    print("%s %s: |mu_got - mu_exact| up to %.3g of its bound, ||v'|/c - 1| = %.3g (bound %.3g)" % (what, dtype, worst, speed, DIR_BOUND[dtype]))
    assert speed <= DIR_BOUND[dtype], what
    return answer


def scattered_photons(state):
    return state["dv"].any(axis=1) & (state["kind"] != KIND_OBJECT)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("phase,g", PHASES, ids=["%s %r" % p if p[0] == "hg" else p[0] for p in PHASES])
def test_phase_redirect_leaves_the_exact_cosine(dev, phase, g, dtype):
    go = scattered_photons(population(dtype))
    n_pass = 1 + PHASES.index((phase, g))
    count = sweep_and_compare(dev, dtype, lambda: dev.phase_redirect(phase, g, C, SEED, n_pass), [(phase, g, None, None)],
                              np.zeros(N, dtype=np.int64), go, n_pass, "phase_redirect %s %r" % (phase, g))
    assert count == go.sum()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("deck", list(DECKS))
def test_phase_layered_leaves_the_exact_cosine(dev, deck, dtype):
    laws, weights, edges = DECKS[deck]
    checked, _, cum, edges_c, center = light._check_layered_phase(laws, weights, edges, CENTER)
    state = population(dtype)
    scattered = scattered_photons(state)
    layer = np.zeros(N, dtype=np.int64)
    if edges is not None:                                              # (nobody stands within 0.3 of an edge: no rounding decides)
        rad = np.sqrt(((state["r"] - CENTER) ** 2).sum(axis=1))
        layer = np.where((rad < edges[0]) | (rad > edges[-1]), -1, np.searchsorted(edges, rad) - 1)
    go = scattered & (layer >= 0)
    n_pass = 40 + list(DECKS).index(deck)
    u_s = light._philox_block(state["id"], SEED, n_pass, 13)[0]
    pick = (cum[np.maximum(layer, 0)] <= u_s[:, None]).sum(axis=1)    # the first law with u_s < C[layer][j]
    got = sweep_and_compare(dev, dtype, lambda: dev.phase_layered(checked, cum, edges_c, center, C, SEED, n_pass), checked, pick, go,
                            n_pass, "phase_layered, " + deck)
    assert got[:2] == (scattered.sum(), go.sum())
    assert got[2].tolist() == np.bincount(layer[go], minlength=len(cum)).tolist() and got[3].tolist() == np.bincount(pick[go], minlength=len(laws)).tolist()
    assert edges is None or (0 < go.sum() < scattered.sum() and min(got[2]) > 50)
    assert len(laws) == 1 or min(got[3]) > 30                          # every law of the mixture is used
