"""The numpy restatement of pcl_step_position_grid (include/physicl_hip.h), for the tests of the position grids.

Per axis a particle is in bin b iff e_b <= v < e_(b+1), the last bin closed; a particle whose value on any axis is outside
[e_0, e_n] or NaN is in no cell -- ``numpy.histogramdd(sample, bins=[edges...])`` for Cartesian axes.  A radius axis bins
q = ((x-cx)*(x-cx) + (y-cy)*(y-cy)) + (z-cz)*(z-cz), in float64 and in that order, against the SQUARED edges e*e: no square
root is taken anywhere, so every operation here is the device's operation (one rounding each, nothing fused)."""
import numpy as np

COORDS = {"x": 0, "y": 1, "z": 2, "r": 3}


def axis_values(r, axis, center=(0.0, 0.0, 0.0)):
    """What axis ``axis`` compares with its edges: the coordinate, or q for the radius axis."""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)          # (an fp32 store's rows widen exactly)
    if axis != "r":
        return r[:, COORDS[axis]]
    c = np.asarray(center, dtype=np.float64).reshape(3)
    dx, dy, dz = r[:, 0] - c[0], r[:, 1] - c[1], r[:, 2] - c[2]
    return (dx * dx + dy * dy) + dz * dz


def axis_bins(v, edges):
    """(bin of every value, whether it is inside the axis's range): searchsorted, the last bin closed."""
    e = np.asarray(edges, dtype=np.float64)
    n = len(e) - 1
    b = np.searchsorted(e, v, side="right") - 1                  # e_b <= v < e_(b+1)
    b[v == e[-1]] = n - 1                                        # the last bin is closed
    with np.errstate(invalid="ignore"):
        inside = (v >= e[0]) & (v <= e[-1])                      # False for NaN
    return np.where(inside, b, 0), inside


def position_grid(r, axes, edges, center=(0.0, 0.0, 0.0)):
    """int64 grid of shape (bins of axis 0, ...) of the positions ``r`` ((n, 3))."""
    r = np.asarray(r, dtype=np.float64).reshape(-1, 3)
    shape = [len(e) - 1 for e in edges]
    inside, cell = np.ones(len(r), dtype=bool), np.zeros(len(r), dtype=np.int64)
    for a, e in zip(axes, edges):
        e = np.asarray(e, dtype=np.float64)
        b, ok = axis_bins(axis_values(r, a, center), e * e if a == "r" else e)
        inside &= ok
        cell = cell * (len(e) - 1) + b
    return np.bincount(cell[inside], minlength=int(np.prod(shape))).astype(np.int64).reshape(shape)
