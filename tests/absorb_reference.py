"""Populations for the tests of AbsorptionStep (tests/test_absorb_cpu.py and the GPU tests).  Not a test file: a helper they
import.  The restatement of the kernel itself is physicl_amd.light._absorb_scattered."""
import numpy as np

C = 299792458.0
SEED = 0x5EED5A7F
CENTER = np.array([0.5, -0.25, 2.0])              # (dyadic: centre + d - centre gives d back exactly for the d used on the edges)
EDGES = np.array([1.0, 2.0, 3.5, 4.0])            # three layers about CENTER
E_BINS = np.linspace(1.0, 3.0, 9)                 # eight energy bins; the cloud's energies reach from 0.8 to 3.2


def unit(a):
    return a / np.sqrt((a * a).sum(axis=1))[:, None]


def cloud(n, seed=1, dtype=np.float64):
    """A dict of float64 arrays holding ``dtype`` values, as a scatter step leaves a store: ``r`` (n, 3) at distances uniform in
    [0, 5.2) from CENTER -- inside the hole below EDGES[0], in every layer and beyond EDGES[-1] --, ``v``, ``dv`` (n, 3): about
    half of the rows were hit (dv = v - v_old, lengths about c), the others missed (dv = +0); ``E`` in [0.8, 3.2); ``photon``:
    every 7th row (index % 7 == 0) is a plain Object; ``ids``.  Rows with index % 101 == 5 have a NaN in r, rows with index % 103
    == 3 a NaN in dv (they interacted, by the rule) and rows with index % 107 == 9 a NaN energy."""
    rng = np.random.RandomState(seed)
    r = CENTER + rng.uniform(0.0, 5.2, size=n)[:, None] * unit(rng.normal(size=(n, 3)))
    old, new = C * unit(rng.normal(size=(n, 3))), C * unit(rng.normal(size=(n, 3)))
    hit = rng.uniform(size=n) < 0.5
    cast = lambda a: a.astype(dtype).astype(np.float64)                                                        # noqa: E731
    v = cast(np.where(hit[:, None], new, old))
    dv = cast(np.where(hit[:, None], v - cast(old), 0.0))
    E = 0.8 + 2.4 * rng.uniform(size=n)
    k = np.arange(n)
    r[k % 101 == 5, 1] = np.nan
    dv[k % 103 == 3, 0] = np.nan
    E[k % 107 == 9] = np.nan
    return {"r": cast(r), "v": v, "dv": dv, "E": cast(E), "photon": k % 7 != 0, "ids": k + 7_000_000_001}


def same_bits(a, b):
    """Equal bit for bit (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
