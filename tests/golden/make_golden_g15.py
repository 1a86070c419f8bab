#!/usr/bin/env python3
"""Generate tests/golden/g15_plane_spectrum.npz by RUNNING the reference's own ScatterMeasureStep(measure_E=True).

    python tests/golden/make_golden_g15.py [path of the reference checkout, default /root/reference]

Only CPU code of the reference runs (``Simulation(cl_on=False)``: NewtonianKinematicsStep.run newton.py:10-16,
ScatterIsotropicStep.__run_py light.py:335-350, ScatterMeasureStep.run light.py:374-404), imported from where it lies;
``pyopencl`` is not installed, so two empty modules of that name are registered for ``import physicl`` to find, and the
ragged measure row (``np.array(out)``, light.py:404) becomes the object array it was under the numpy of the reference's day.
300 photons with distinct energies start at the origin along +x (np.random.seed(15)); 8 passes of [Newton, isotropic
scatter with hit probability 0.3, measure at the planes x = 2.5 steps and y = 0.3 steps].  Stored (data only): the
energies, per pass the positions r and last moves dr the measure step saw, and its rows -- t, N, and per plane the count
and the list of crossing energies (lists concatenated, with their lengths).
"""
import os
import sys
import types

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
N, PASSES, DT = 300, 8, 0.0005


def main():
    for name in ("pyopencl", "pyopencl.array"):
        sys.modules[name] = types.ModuleType(name)
    sys.modules["pyopencl"].array = sys.modules["pyopencl.array"]
    sys.path.insert(0, REF)
    import physicl
    import physicl.light as light
    import physicl.newton as newton

    class OldNumpy:                                    # np.array of a ragged row made an object array when the reference was
        def __getattr__(self, name):                   # written (numpy < 1.24); today it raises.  Only light.py's view of np.
            return getattr(np, name)

        @staticmethod
        def array(obj, *a, **kw):
            try:
                return np.array(obj, *a, **kw)
            except ValueError:
                out = np.empty(len(obj), dtype=object)
                for k, x in enumerate(obj):
                    out[k] = x
                return out
    light.np = OldNumpy()

    np.random.seed(15)
    E = 1.0 + 2.0 * np.random.permutation(N) / N                       # distinct
    cval = float(np.asarray(light.c))
    step_len = cval * DT
    planes = [[2.5 * step_len, np.nan, np.nan], [np.nan, 0.3 * step_len, np.nan]]
    sim = physicl.Simulation(cl_on=False)
    sim.ts = []                                        # what Simulation.run sets up before its loop
    sim.add_objs(light.generate_photons_from_E(list(E)))
    upd = physicl.UpdateTimeStep(lambda s: DT)
    move = newton.NewtonianKinematicsStep()
    scat = light.ScatterIsotropicStep(n=0.3 / step_len, A=1.0)
    meas = light.ScatterMeasureStep(None, measure_n=True, measure_locs=planes, measure_E=True)
    r, dr = [], []
    for _ in range(PASSES):
        for st in (upd, move, scat):
            st.run(sim)
        r.append(np.array([np.asarray(o.r, dtype=np.float64) for o in sim.objects]))
        dr.append(np.array([np.asarray(o.dr, dtype=np.float64) for o in sim.objects]))
        meas.run(sim)
    rows = meas.data
    t = np.array([float(np.asarray(row[0])) for row in rows])
    n_obj = np.array([int(row[1]) for row in rows], dtype=np.int64)
    counts = np.array([[int(row[2 + 2 * p]) for p in range(len(planes))] for row in rows], dtype=np.int64)
    lists = [[np.array([float(np.asarray(x)) for x in row[3 + 2 * p]], dtype=np.float64) for p in range(len(planes))] for row in rows]
    assert all(len(lists[k][p]) == counts[k][p] for k in range(PASSES) for p in range(len(planes)))
    assert sum(1 for k in range(PASSES) if counts[k].sum() > 0) >= 3, counts
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "g15_plane_spectrum.npz")
    np.savez_compressed(out, E=E, planes=np.array(planes), dt=DT, r=np.array(r), dr=np.array(dr), t=t, n=n_obj, counts=counts,
                        list_lengths=np.array([[len(x) for x in row] for row in lists], dtype=np.int64),
                        list_values=np.concatenate([x for row in lists for x in row]))
    print(out, os.path.getsize(out), "bytes; counts per pass:", counts.tolist())


if __name__ == "__main__":
    main()
