"""The draws of a PhotonSource restated in numpy (include/physicl_hip.h: pcl_store_apply_source), for tests/test_source_cpu.py
and the GPU tests of the sources.  Not a test file: a helper both import.

Every operation is the IEEE double operation the kernel performs, in the kernel's order; numpy's sqrt is correctly rounded like
the device's, so ``mu``, ``s``, ``rho`` of the disc and the angles are the device's bit for bit.  What is NOT pinned bit for bit
is sin / cos (the project's pcl_sincos_2pi on the device, < 1 ulp; libm here) and the gaussian's log.
"""
import numpy as np

from oracle.physicl_oracle import philox4x32_10, u53

_U32 = np.uint64(0xFFFFFFFF)


def _block(ids, seed, block):
    ids = np.asarray(ids, dtype=np.uint64)
    w = philox4x32_10(ids & _U32, ids >> np.uint64(32), np.uint64(0xFFFFFFFF), np.uint64(block), int(seed) & 0xFFFFFFFF,
                      (int(seed) >> 32) & 0xFFFFFFFF)
    return u53(w[0], w[1]), u53(w[2], w[3])


def source_state(src, ids, seed, c):
    """{"r": (n, 3), "v": (n, 3), "mu": (n,) or None, "rho": (n,) or None} of the photons ``ids`` in float64."""
    ids = np.asarray(ids, dtype=np.uint64)
    n = len(ids)
    c = np.float64(c)
    e1, e2, d, origin = (np.asarray(x, dtype=np.float64) for x in (src.e1, src.e2, src.d, src.origin))
    mu = rho = None
    if src.angular == "beam":
        v = np.broadcast_to(c * d, (n, 3)).copy()
    else:
        u_a, u_b = _block(ids, seed, 4)
        if src.angular == "isotropic":
            mu = 1.0 - 2.0 * u_a
        elif src.angular == "cone":
            mu = 1.0 - u_a * (1.0 - np.float64(src.cos_half_angle))
        else:
            mu = np.sqrt(1.0 - u_a)
        s = np.sqrt((1.0 - mu) * (1.0 + mu))
        psi = (u_b * 2.0) * np.pi
        sc, ss = s * np.cos(psi), s * np.sin(psi)
        v = np.stack([c * ((sc * e1[k] + ss * e2[k]) + mu * d[k]) for k in range(3)], axis=1)
    if src.spatial == "point":
        r = np.broadcast_to(origin, (n, 3)).copy()
    else:
        u_c, u_d = _block(ids, seed, 5)
        radius = np.float64(src.radius)
        rho = radius * np.sqrt(u_c) if src.spatial == "disc" else radius * np.sqrt(-2.0 * np.log(1.0 - u_c))
        phi = (u_d * 2.0) * np.pi
        rc, rs = rho * np.cos(phi), rho * np.sin(phi)
        r = np.stack([origin[k] + (rc * e1[k] + rs * e2[k]) for k in range(3)], axis=1)
    return {"r": r, "v": v, "mu": mu, "rho": rho}


# ---- the statistical conditions (5 sigma of the estimator, from the distribution's own variance) ----------------------------
#   isotropic: each component of v/c is uniform in [-1, 1]: variance 1/3 -> |mean| <= 5/sqrt(3n)
#   cone:      mu uniform in [cos a, 1]: mean (1 + cos a)/2, variance (1 - cos a)^2/12
#   lambert:   mu = sqrt(1 - u): mean 2/3, variance 1/2 - 4/9 = 1/18
#   disc:      rho^2/R^2 uniform in [0, 1]: mean 1/2, variance 1/12
#   gaussian:  rho^2/(2 sigma^2) exponential(1): mean 1, variance 1
def check_isotropic(v_over_c):
    n = len(v_over_c)
    assert np.all(np.abs(np.mean(v_over_c, axis=0)) <= 5.0 / np.sqrt(3.0 * n)), np.mean(v_over_c, axis=0)


def check_cone(mu, half_angle, slack=4e-16):
    n, ca = len(mu), np.cos(half_angle)
    assert np.all(mu >= ca - slack), mu.min()
    assert abs(np.mean(mu) - (1.0 + ca) / 2.0) <= 5.0 * (1.0 - ca) / np.sqrt(12.0 * n), np.mean(mu)


def check_lambertian(mu):
    n = len(mu)
    assert np.all(mu > 0), mu.min()
    assert abs(np.mean(mu) - 2.0 / 3.0) <= 5.0 * np.sqrt(1.0 / (18.0 * n)), np.mean(mu)


def check_disc(rho, R, slack=4e-16):
    n = len(rho)
    assert np.all(rho <= R * (1.0 + slack)), rho.max()
    assert abs(np.mean(rho * rho) / R ** 2 - 0.5) <= 5.0 / np.sqrt(12.0 * n), np.mean(rho * rho) / R ** 2


def check_gaussian(rho, sigma):
    n = len(rho)
    assert abs(np.mean(rho * rho) / (2.0 * sigma ** 2) - 1.0) <= 5.0 / np.sqrt(n), np.mean(rho * rho) / (2.0 * sigma ** 2)
