"""CPU: the scattering-angle pipeline the direction-turning sweeps share -- light._law_mu, the lambertian ground's cosine and
light._turn_about -- against exact arithmetic (tests/direction_exact.py), not against itself.

The restatement repeats the kernels operation for operation (every other test of these sweeps holds the two together), so what is
measured here is the kernels' formula.  Bounds: tests/direction_exact.py (``law_bound``) for the cosines; for the direction the
figures below.  Every test prints what it measured, in units of eps = 2^-52.

Henyey-Greenstein, measured with the form for |g| < 1/2 in place (maximum over the 406 u of ``U`` and both signs of g, in eps):
5e-324, 1e-300, 1e-160: below 1e-140;  1e-17: 0.063;  1e-15: 1.09;  1e-12: 1.14;  1e-8: 1.32;  1e-5: 1.59;  1e-3: 1.27;  0.01: 1.41;
0.1: 1.47;  0.3: 1.42;  below 0.5: 3.47;  0.5: 2.5;  0.7: 5.37;  0.85: 17.3;  0.95: 30.2;  0.999: 2.26e3;  0.999999: 2.2e6;
1 - 2^-53: 4.38e14.  With the closed inverse alone every g up to 0.1 misses its bound (CHANGELOG.md has that column).
"""
from fractions import Fraction

import mpmath
import numpy as np
import pytest

from physicl_amd import light
from direction_exact import EPS, HG_SWITCH, along, direction_exact, dot, law_bound, mp, mu_exact, norm
from phase_reference import AXES, C, SEED, unit

N_U = 400
IDS = np.arange(N_U, dtype=np.int64) + 7_000_000_001
TOP = 1.0 - 2.0 ** -53                               # the largest uniform, and the cosine next to 1
U = np.concatenate([[0.0, 2.0 ** -53, 0.25, 0.5, 0.75, TOP], light._philox_block(IDS, SEED, 1, 10)[0]])
G = [5e-324, 1e-300, 1e-160, 1e-17, 1e-15, 1e-12, 1e-8, 1e-5, 1e-3, 0.01, 0.1, 0.3, float(np.nextafter(HG_SWITCH, 0.0)), HG_SWITCH,
     0.7, 0.85, 0.95, 0.999, 0.999999, TOP]


def worst(got, exact):
    """max |got - exact| over the pairs, exactly, as a float."""
    return float(max(abs(Fraction(float(a)) - b) for a, b in zip(got, exact)))


# ------------------------------------------------------------------------------------------------ 2a: Henyey-Greenstein
@pytest.mark.parametrize("g", G, ids=repr)
def test_henyey_greenstein_s_cosine_is_the_exact_inverse(g):
    assert len(U) >= 400 and np.all((U >= 0) & (U < 1))
    for signed in (g, -g):
        with np.errstate(all="ignore"):
            got = light._law_mu("hg", signed, None, None, U, None, SEED, 1)
        err = worst(got, [mu_exact("hg", signed, u_a=u) for u in U])
        print("hg g = %r: max |mu - exact| = %.3g eps (bound %.3g eps)" % (signed, err / EPS, law_bound("hg", signed) / EPS))
        assert np.all(np.abs(got) <= 1.0)
        assert err <= law_bound("hg", signed), signed


def test_tiny_g_runs_the_other_way_through_u_than_g_zero():
    """mu(u) -> -(1 - 2u) as g -> 0, while g == 0 is the isotropic line +(1 - 2u): both are uniform, and it stays that way."""
    iso = light._law_mu("hg", 0.0, None, None, U, None, SEED, 1)
    assert np.array_equal(iso, 1.0 - 2.0 * U) and np.array_equal(iso, light._law_mu("isotropic", 0.7, None, None, U, None, SEED, 1))
    assert worst(iso, [mu_exact("isotropic", u_a=u) for u in U]) == 0.0 == law_bound("isotropic") == law_bound("hg", 0.0)
    assert [mu_exact("hg", 0.0, u_a=u) for u in U] == [mu_exact("isotropic", u_a=u) for u in U]
    for g in (5e-324, -5e-324, 1e-300, -1e-160):                       # (mu + (1 - 2u) = g (3 - (1 - 2u)^2)/2 + O(g^2))
        assert np.max(np.abs(light._law_mu("hg", g, None, None, U, None, SEED, 1) + iso)) <= 2 * abs(g)


# ------------------------------------------------------------------------------------------------ 2b: the other cosines
def test_rayleigh_s_cosine_is_the_mixture_the_header_states():
    edge = np.array([0.0, 2.0 ** -53, 0.25, 0.5, 0.75, np.nextafter(0.75, 0), np.nextafter(0.75, 1), 0.875, np.nextafter(0.875, 0), TOP])
    u_a = np.concatenate([edge, U[6:]])
    ids = np.concatenate([IDS[-1] + 1 + np.arange(len(edge)), IDS])
    u_c, u_d = light._philox_block(ids, SEED, 3, 11)
    got = light._law_mu("rayleigh", 0.0, None, None, u_a.copy(), ids, SEED, 3)
    exact = [mu_exact("rayleigh", u_a=a, u_c=c, u_d=d) for a, c, d in zip(u_a, u_c, u_d)]
    err = worst(got, exact)
    part = u_a >= 0.75                                                 # one in four: the largest of three, which is exact
    print("rayleigh: max |mu - exact| = %.3g eps (bound %g eps); %d of %d in the 3/2 mu^2 part" % (err / EPS, law_bound("rayleigh") / EPS, part.sum(), len(u_a)))
    assert err <= law_bound("rayleigh") and 60 < part.sum() < 150
    assert worst(got[part], [e for e, p in zip(exact, part) if p]) == 0.0
    assert got[0] == -1.0 and got[4] == -1.0 and got[7] == max(u_c[7], u_d[7]) and np.all(np.abs(got) <= 1.0)


def tables():
    """(nodes, F) of a 3-node and a 17-node table, F as LayeredPhaseStep makes it."""
    out = []
    for edges, p in (([-1.0, 0.3, 1.0], [1.0, 5.0]), (np.linspace(-1.0, 1.0, 17), 1.0 + np.arange(16.0) % 5 + 0.1 * np.arange(16.0))):
        (law,), _, _, _, _ = light._check_layered_phase([("table", edges, p)], None, None, (0, 0, 0))
        assert law[0] == "table" and len(law[2]) == len(law[3]) == len(edges) and law[3][0] == 0.0 and law[3][-1] == 1.0
        out.append((law[2], law[3]))
    return out


@pytest.mark.parametrize("k", [0, 1], ids=["3 nodes", "17 nodes"])
def test_a_table_s_cosine_is_the_inverse_of_the_piecewise_linear_F(k):
    nodes, F = tables()[k]
    near = np.concatenate([F, np.nextafter(F, 0.0), np.nextafter(F, 1.0)])
    u_a = np.concatenate([near[(near >= 0) & (near < 1)], U])          # every F node and one ulp either side, where that is a uniform
    assert len(u_a) >= 3 * len(F) - 3 + len(U)
    got = light._law_mu("table", 0.0, nodes, F, u_a, None, SEED, 1)
    err = worst(got, [mu_exact("table", nodes=nodes, F=F, u_a=u) for u in u_a])
    print("table of %d nodes: max |mu - exact| = %.3g eps (bound %g eps)" % (len(F), err / EPS, law_bound("table") / EPS))
    assert err <= law_bound("table") and np.all(np.abs(got) <= 1.0)
    assert np.array_equal(got[:len(F) - 1], nodes[:-1])                # u on a node: the node


def test_the_lambertian_ground_s_cosine_is_the_root_of_one_minus_u():
    rng = np.random.RandomState(8)
    p = 1.5 * unit(rng.normal(size=(N_U, 3)))                          # outside the unit sphere, a move that ends inside it
    r = 0.5 * unit(rng.normal(size=(N_U, 3)))
    o = light._surface_bounce(r, r - p, C * unit(r - p), np.ones(N_U, dtype=bool), IDS, 1.0, (0.0, 0.0, 0.0), 1.0, "lambertian", C, SEED, 2)
    assert o["reflected"].all()
    u_a = light._philox_block(IDS, SEED, 2, 8)[0]
    err = max(abs(mp(m) - mu_exact("lambertian", u_a=u)) for m, u in zip(o["mu"], u_a))
    print("lambertian: max |mu - exact| = %.3g eps (bound %g eps)" % (float(err) / EPS, law_bound("lambertian") / EPS))
    assert err <= law_bound("lambertian")


# ------------------------------------------------------------------------------------------------ 2c: the turned direction
# |d.w - mu| and ||d| - 1|: 8 eps each.  d_k = (sc*e1_k + ss*e2_k) + mu*w_k is five rounded operations per component on values <= 1
# behind s (two more and a root), the azimuth and the frame (four each): the project's own contract for such a direction is 8
# ulp per component (tests/writer_reference.py: DIR_ULP), and d.w and |d| are projections of that error.
# Along the device's e1 and e2: 16 eps.  numpy's azimuth is libm's sin / cos of psi = (u*2)*pi -- a rounded product with a rounded
# pi, up to 2 pi * 0.7 eps = 4.4 eps off the angle that is meant -- times s (1 eps) and once more rounded (0.5); the frame's
# |e1|^2 - 1, e1.e2 and e1.w are a few eps each (4, weighted by (sc, ss, mu), a unit vector: 4 sqrt 3 = 7), and the two sums 1.5.
TURN_EPS, AZIMUTH_EPS = 8.0, 16.0
SPECIAL_MU = [-1.0, 1.0, TOP, -TOP, 0.0]


def axes_and_poles():
    w = [(x, y, z) for z in (1.0, -1.0) for x in (0.0, -0.0) for y in (0.0, -0.0)]          # both poles, both signs of zero
    low = -TOP                                                                              # w2 one ulp from -1
    rest = np.sqrt((1.0 - low) * (1.0 + low))
    w += [(rest, 0.0, low), (0.0, -rest, low), (rest * 0.6, rest * 0.8, low), (rest, 0.0, TOP)]
    return np.array(w + [tuple(a) for a in AXES])


def check_turn(w, mu, u_b):
    """One row: (|d.w - mu|, ||d| - 1|, the larger error along the device's e1 and e2), in eps."""
    d = light._turn_about(w[None, :], np.array([mu]), np.array([u_b]))[0]
    e1, e2 = (e[0] for e in light._frame(w[None, :]))
    sc, ss = along(mu, u_b)
    if abs(mu) == 1.0:
        assert np.array_equal(d, mu * w), (w, mu)                      # exactly +-w
    return [float(x) / EPS for x in (abs(dot(d, w) - mp(mu)), abs(norm(d) - 1), max(abs(dot(d, e1) - sc), abs(dot(d, e2) - ss)))]


def test_direction_exact_is_a_unit_vector_at_the_cosine_and_the_azimuth():
    """The reference alone, in a frame that is given: its own three properties to 1e-60."""
    rng = np.random.RandomState(3)
    for w in np.concatenate([axes_and_poles(), unit(rng.normal(size=(20, 3)))]):
        for mu, u_b in zip(SPECIAL_MU + [0.3], rng.uniform(size=6)):
            d = direction_exact(w, mu, u_b)
            assert abs(dot(d, w) / norm(w) - mp(mu)) < 1e-60 and abs(norm(d) - 1) < 1e-60
    e1, e2, w = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]      # here the frame is known: Gram-Schmidt from x, then w x e1
    d = direction_exact(w, 0.6, 0.125)
    sc, ss = along(0.6, 0.125)
    assert abs(dot(d, e1) - sc) < 1e-60 and abs(dot(d, e2) - ss) < 1e-60 and abs(sc - mpmath.sqrt(mp(0.32))) < 1e-15 and abs(sc - ss) < 1e-60


def test_the_turned_direction_has_the_cosine_the_length_and_the_azimuth():
    rng = np.random.RandomState(4)
    o = rng.normal(size=(200, 3))
    ws = np.concatenate([axes_and_poles(), o / np.sqrt(light._dot3(o, o))[:, None]])      # unit vectors as the kernel makes them
    worst3 = np.zeros(3)
    for w in ws:
        mus = SPECIAL_MU + list(rng.uniform(-1.0, 1.0, size=3))
        for mu, u_b in zip(mus, np.concatenate([[0.0, 0.25, 0.5, TOP], rng.uniform(size=len(mus) - 4)])):
            worst3 = np.maximum(worst3, check_turn(w, mu, u_b))
    print("turned direction over %d unit vectors: |d.w - mu| %.3g eps, ||d| - 1| %.3g eps (bound %g); along e1, e2 %.3g eps (bound %g)"
          % (len(ws), worst3[0], worst3[1], TURN_EPS, worst3[2], AZIMUTH_EPS))
    assert worst3[0] <= TURN_EPS and worst3[1] <= TURN_EPS and worst3[2] <= AZIMUTH_EPS


# ------------------------------------------------------------------------------------------------ 2d: the distribution
N_DRAWS = 20000
DRAW_SEED = 20261021                                 # chosen on the reference: mu_exact of these draws holds every line below
SIGMAS = 5.0


def draws():
    return light._philox_block(np.arange(N_DRAWS, dtype=np.int64) + 7_000_000_001, DRAW_SEED, 1, 10)[0]


def moments_hold(mu, g, second):
    """<mu> = g and -- ``second`` -- <mu^2> = (1 + 2 g^2)/3 within SIGMAS standard errors.  Var(mu^2) = 1/5 - 1/9 of the uniform law:
    asked for at |g| <= 1e-8 alone, where the law's own differs from it by the order of g."""
    m1, m2 = float(np.mean(mu)), float(np.mean(mu * mu))
    law2 = (1 + 2 * g * g) / 3
    ok1 = abs(m1 - g) <= SIGMAS * np.sqrt((law2 - g * g) / len(mu))
    ok2 = not second or abs(m2 - law2) <= SIGMAS * np.sqrt((1 / 5 - 1 / 9) / len(mu))
    return ok1, ok2, m1, m2


@pytest.mark.parametrize("g", [1e-17, -1e-17, 1e-12, -1e-12, 1e-8, -1e-8, 0.3], ids=repr)
def test_fixed_draws_have_the_law_s_moments(g):
    """The test a physicist would have written.  (With the closed inverse alone, g = 1e-17 gives mu = 0 for every draw.)"""
    u = draws()
    second = abs(g) <= 1e-8
    exact = np.array([float(mu_exact("hg", g, u_a=x)) for x in u])
    ok1, ok2, m1, m2 = moments_hold(exact, g, second)
    assert ok1 and ok2, ("the seed does not hold on the reference: choose another", m1, m2)
    with np.errstate(all="ignore"):
        got = light._law_mu("hg", g, None, None, u, None, DRAW_SEED, 1)
    ok1, ok2, m1, m2 = moments_hold(got, g, second)
    print("hg g = %r: <mu> = %.6g, <mu^2> = %.6g over %d draws" % (g, m1, m2, len(u)))
    assert ok1, m1
    assert ok2, m2
