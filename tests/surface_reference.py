"""Populations for the tests of SurfaceReflectStep (tests/test_surface_cpu.py and the GPU tests).  Not a test file: a helper
they import.  The restatement of the kernel itself is physicl_amd.light._surface_bounce."""
import numpy as np

C = 299792458.0
RADIUS = 10.0
CENTER = np.array([3.0, -2.0, 1.25])
SEED = 0x5EED5A7F


def cloud(n, seed=1, dtype=np.float64, radius=RADIUS, center=CENTER):
    """(r, dr, v) as (n, 3) float64 arrays holding ``dtype`` values: every particle's previous position r - dr lies outside the
    sphere, the current one inside for even indices (about half are hit) and further out for odd ones; |v| = c along dr."""
    rng = np.random.RandomState(seed)
    unit = lambda a: a / np.sqrt((a * a).sum(axis=1))[:, None]                                                   # noqa: E731
    prev = unit(rng.normal(size=(n, 3))) * (radius * (1.001 + rng.uniform(0.0, 0.8, size=n)))[:, None]
    now = unit(rng.normal(size=(n, 3))) * (radius * 0.999 * rng.uniform(0.0, 1.0, size=n) ** (1.0 / 3.0))[:, None]
    odd = np.arange(n) % 2 == 1
    now[odd] = prev[odd] * 1.1
    r, dr = (now + center).astype(dtype).astype(np.float64), (now - prev).astype(dtype).astype(np.float64)
    v = (C * unit(dr)).astype(dtype).astype(np.float64)
    return r, dr, v


def ulp(x, dtype=np.float64):
    return float(np.spacing(dtype(abs(x))))
