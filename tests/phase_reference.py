"""Populations for the tests of PhaseFunctionStep (tests/test_phase_cpu.py and the GPU tests).  Not a test file: a helper they
import.  The restatement of the kernel itself is physicl_amd.light._phase_redirect."""
import numpy as np

C = 299792458.0
SEED = 0x5EED5A7F
AXES = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=np.float64)


def unit(a):
    return a / np.sqrt((a * a).sum(axis=1))[:, None]


def cloud(n, seed=1, dtype=np.float64):
    """(v, dv) as (n, 3) float64 arrays holding ``dtype`` values, as a scatter step leaves them: every third row (index % 3 == 0)
    was scattered -- v is the new velocity, dv = v - v_old, both of length about c in unrelated directions -- the others were
    missed: v is the old velocity and dv is +0.  Old directions cover all octants; of the scattered rows every 8th (index % 24 ==
    0) had an old direction exactly along an axis, +z, -z (the frame's pole), +x, -x, +y, -y in turn."""
    rng = np.random.RandomState(seed)
    old = C * unit(rng.normal(size=(n, 3)))
    on_axis = np.flatnonzero(np.arange(n) % 24 == 0)
    old[on_axis] = C * AXES[(on_axis // 24) % 6]
    new = C * unit(rng.normal(size=(n, 3)))
    hit = np.arange(n) % 3 == 0
    v = np.where(hit[:, None], new, old).astype(dtype).astype(np.float64)
    old = old.astype(dtype).astype(np.float64)
    dv = np.where(hit[:, None], v - old, 0.0).astype(dtype).astype(np.float64)
    return v, dv


def frame(w):
    """(e1, e2) of the branch-free frame (Duff et al. 2017) about the unit vectors ``w``, as the kernel builds it."""
    w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2]
    sg = np.copysign(1.0, w2)
    aa = -1.0 / (sg + w2)
    bb, sw0 = (w0 * w1) * aa, sg * w0
    return np.stack([1.0 + (sw0 * w0) * aa, sg * bb, -sw0], axis=1), np.stack([bb, sg + (w1 * w1) * aa, -w1], axis=1)


def ulp(x, dtype=np.float64):
    return float(np.spacing(dtype(abs(x))))
