"""The scattering cosine and the turned direction from the mathematics, in exact or 60-digit arithmetic (tests/
test_direction_exact_cpu.py and test_writers_direction_exact_gpu.py).  Not a test file: a helper they import.

Every other test of the direction-turning sweeps compares a kernel with physicl_amd.light's numpy restatement, which repeats the
kernel's operations in the kernel's order: a formula that is wrong, or that loses its digits, is wrong on both sides alike.  What
stands here shares nothing with that order:

* ``mu_exact``: the cosine of the scattering angle by one law, per photon, in ``fractions.Fraction`` on the exact values of the
  double inputs (``sqrt(1 - u)`` of the lambertian ground through mpmath);
* ``direction_exact``: the unit vector at the cosine mu and the azimuth 2 pi u_b about w, in mpmath, in a frame of its own.  What
  may be compared with a device's direction does not depend on the frame: d.w, |d| and -- along the DEVICE's e1 and e2 -- the
  two numbers ``along`` returns.

The uniforms are light._philox_block's: tests/test_writer_streams_*.py hold those to the device.
"""
from fractions import Fraction

import mpmath

mpmath.mp.dps = 80                                   # (60 digits or more)
EPS = 2.0 ** -52


# What the double-precision cosine of a law may differ by from mu_exact.  None of these figures comes from the code under test.
# Henyey-Greenstein below the switch point: 8 eps (a form measured at 2.5 eps against exact arithmetic from g = 5e-324 up: a factor
# of three); at and above it 32 eps / (1 - |g|) -- the closed inverse's q = (1 - g^2) / (1 - g + 2 g u) has a denominator as small
# as 1 - |g|, whose rounding q*q carries into mu: measured at 20 eps up to |g| = 0.95 and growing as 1 / (1 - |g|) beyond.
# Rayleigh, a table, the lambertian ground: at most four rounded operations on values <= 4.  Isotropic: 1 - 2u is exact.
HG_SWITCH = 0.5
LAW_EPS = {"isotropic": 0.0, "rayleigh": 4.0, "table": 4.0, "lambertian": 4.0}


def law_bound(kind, g=0.0):
    """The bound of |mu - mu_exact| for a law, in absolute terms."""
    if kind == "hg" and g != 0:
        return (8.0 if abs(g) < HG_SWITCH else 32.0 / (1.0 - abs(g))) * EPS
    return LAW_EPS["isotropic" if kind == "hg" else kind] * EPS


def _fr(x):
    return x if isinstance(x, Fraction) else Fraction(float(x))


def mu_exact(kind, g=0.0, nodes=None, F=None, u_a=0.0, u_c=None, u_d=None):
    """The cosine of the scattering angle one photon draws by the law ``kind`` from the uniform ``u_a`` (and, Rayleigh's 3/2 mu^2
    part, ``u_c`` and ``u_d``), exactly: a Fraction -- for "lambertian" an mpf.

    * "isotropic": 1 - 2u.
    * "hg": the inverse of Henyey-Greenstein's cumulative distribution, P(mu) = (1 - g^2)/(2g) (1/sqrt(1 + g^2 - 2 g mu) - 1/(1 + g)),
      at u:  mu = ((1 + g^2) - q^2) / (2g),  q = (1 - g^2) / (1 - g + 2 g u);  g = 0 is the isotropic law.
      (As g -> 0 this tends to -(1 - 2u), while g = 0 gives +(1 - 2u): both are uniform.)
    * "rayleigh": 3/8 (1 + mu^2) as the mixture the header states -- j = floor(4u), f = 4u - j, x = 2f - 1;  j < 3: mu = x;
      j = 3: mu = the largest of |x|, u_c and u_d, with the sign of x.
    * "table": the inverse of the piecewise linear F through (nodes_k, F_k) at u.
    * "lambertian": sqrt(1 - u), the cosine-weighted hemisphere of the ground."""
    u = _fr(u_a)
    if kind == "lambertian":
        return mpmath.sqrt(mpmath.mpf(1) - mpmath.mpf(u.numerator) / mpmath.mpf(u.denominator))
    if kind == "isotropic" or (kind == "hg" and g == 0):
        return 1 - 2 * u
    if kind == "hg":
        g = _fr(g)
        q = (1 - g * g) / (1 - g + 2 * g * u)
        return ((1 + g * g) - q * q) / (2 * g)
    if kind == "rayleigh":
        s4 = 4 * u
        j = s4.numerator // s4.denominator
        x = 2 * (s4 - j) - 1
        if j < 3:
            return x
        big = max(abs(x), _fr(u_c), _fr(u_d))
        return -big if x < 0 else big
    if kind == "table":
        nodes, F = [_fr(x) for x in nodes], [_fr(x) for x in F]
        k = max(i for i in range(len(F) - 1) if F[i] <= u)       # F_0 = 0 <= u < 1 = F_K
        return nodes[k] + (u - F[k]) * (nodes[k + 1] - nodes[k]) / (F[k + 1] - F[k])
    raise ValueError(kind)


def mp(x):
    """An mpf of a float, a Fraction or an mpf: exactly, to the working precision."""
    if isinstance(x, Fraction):
        return mpmath.mpf(x.numerator) / mpmath.mpf(x.denominator)
    return x if isinstance(x, mpmath.mpf) else mpmath.mpf(float(x))


def vec(x):
    return [mp(t) for t in x]


def dot(a, b):
    return mpmath.fsum(mp(x) * mp(y) for x, y in zip(a, b))


def norm(a):
    return mpmath.sqrt(dot(a, a))


def along(mu, u_b):
    """(s cos psi, s sin psi), s = sqrt(1 - mu^2), psi = 2 pi u_b: the components of the turned direction along the first and the
    second vector of a right-handed orthonormal frame (e1, e2, w)."""
    mu, psi = mp(mu), 2 * mpmath.pi * mp(u_b)
    s = mpmath.sqrt((1 - mu) * (1 + mu))
    return s * mpmath.cos(psi), s * mpmath.sin(psi)


def direction_exact(w, mu, u_b):
    """The unit vector at the cosine ``mu`` and the azimuth 2 pi ``u_b`` about ``w`` (normalised here), as three mpf.  The frame is
    this function's own -- Gram-Schmidt from the axis w is furthest from -- so the azimuth's origin is not the device's: compare
    d.w, |d| and ``along`` only."""
    w = vec(w)
    n = norm(w)
    w = [x / n for x in w]
    k = min(range(3), key=lambda i: abs(w[i]))
    a = [mpmath.mpf(int(i == k)) for i in range(3)]
    aw = dot(a, w)
    e1 = [x - aw * y for x, y in zip(a, w)]
    n1 = norm(e1)
    e1 = [x / n1 for x in e1]
    e2 = [w[1] * e1[2] - w[2] * e1[1], w[2] * e1[0] - w[0] * e1[2], w[0] * e1[1] - w[1] * e1[0]]
    sc, ss = along(mu, u_b)
    return [sc * x + ss * y + mp(mu) * z for x, y, z in zip(e1, e2, w)]
