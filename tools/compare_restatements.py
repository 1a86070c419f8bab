#!/usr/bin/env python3
"""Do the numpy restatements of the writer sweeps (physicl_amd/light.py) in two source trees compute the same bytes?
For a refactor of the restatements, the sibling of compare_unit_asm.py:

    python tools/compare_restatements.py <old tree> <new tree>

One child process per tree imports that tree's physicl_amd.light and runs the six restatements, _source_emit,
_path_probability and the _check_* functions (accepted results and refusal texts) over a fixed seeded corpus of 4096 particles
per case, float64 and float32, and writes every result to a temporary .npz / JSON.  The parent compares every array byte for
byte (tobytes, dtype and shape) and every text.  Exit status 1 on any difference.
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

N = 4096
EDGES = [0.5, 1.0, 2.0, 3.0]
E_EDGES = [1.0, 2.0, 4.0, 8.0]


def corpus():
    """r, dr, v, dv (n, 3), E, photon, ids: plain Objects among the photons, NaN / inf rows, v of 0.0 and -0.0, positions on the
    layer edges with q just inside and just outside, energies on and outside the bin edges, w[2] of both signs and exactly +-1."""
    rs = np.random.RandomState(20240607)
    r = rs.uniform(-2.5, 2.5, (N, 3))
    dr = rs.normal(0, 0.8, (N, 3))
    v = rs.normal(0, 1.0, (N, 3))
    dv = np.where(rs.rand(N, 1) < 0.6, rs.normal(0, 1.0, (N, 3)), 0.0)
    E = rs.uniform(0.5, 9.0, N)
    photon = rs.rand(N) < 0.9
    ids = rs.permutation(N).astype(np.int64) + (1 << 33)
    k = 0
    for field in (r, dr, v, dv):                               # NaN and inf in every vector field
        for bad in (np.nan, np.inf, -np.inf):
            field[k, k % 3] = bad
            k += 1
    E[k], E[k + 1] = np.nan, np.inf
    k += 2
    v[k:k + 40] = 0.0                                          # at rest, with both zeros
    v[k + 20:k + 40, 1] = -0.0
    v[k + 40:k + 50, 0], v[k + 40:k + 50, 1:] = -0.0, 0.0
    k += 50
    for e in EDGES:                                            # exactly on an edge, and one ulp to either side of it
        for x in (e, np.nextafter(e, 0.0), np.nextafter(e, 9.0)):
            r[k] = (x, 0.0, 0.0)
            r[k + 1] = (0.0, 0.0, -x)
            k += 2
    for e in E_EDGES + [0.25, 100.0]:                          # on a bin edge and outside all bins
        E[k], E[k + 1], E[k + 2] = e, np.nextafter(e, 0.0), np.nextafter(e, 1e9)
        k += 3
    for s in (1.0, -1.0):                                      # old directions along +-z exactly, and w[2] of both signs
        for z in (1.0, 1e-300, 0.0):
            dv[k] = (0.3, -0.2, 0.1)
            v[k] = dv[k] + (0.0 if z == 1.0 else 0.5, 0.0, s * z if z else s * 0.0)
            k += 1
    dv[k:k + 8] = 0.0                                          # dv of +-0: not scattered
    dv[k + 4:k + 8] = -0.0
    return r, dr, v, dv, E, photon, ids


def child(out):
    from physicl_amd import light
    from physicl_amd.core import PhotonBatch
    r, dr, v, dv, E, photon, ids = corpus()
    arrays, texts = {}, {}

    def keep(name, res):
        if isinstance(res, dict):
            for key, val in sorted(res.items()):
                keep("%s/%s" % (name, key), val)
        elif isinstance(res, (tuple, list)):
            for i, val in enumerate(res):
                keep("%s/%d" % (name, i), val)
        elif isinstance(res, np.ndarray) or isinstance(res, np.generic):
            arrays[name] = np.asarray(res)
        else:
            texts[name] = repr(res)

    def run(name, fn, *args, **kw):
        try:
            keep(name, fn(*args, **kw))
        except ValueError as exc:
            texts[name] = "ValueError: %s" % exc

    c, seed = 299792458.0, 0x1234567811223344
    table1 = ("table", [-1.0, 1.0], [2.5])
    mu1024 = np.linspace(-1.0, 1.0, 1025)
    table1024 = ("table", mu1024, 1.0 + 0.9 * np.cos(np.arange(1024)))
    sources = [light.PhotonSource(origin=(1, -2, 3), direction=(0.3, -0.5, 0.8), angular=a, spatial=s,
                                  half_angle=0.7 if a == "cone" else None, radius=0.4 if s != "point" else None)
               for a in ("beam", "isotropic", "cone", "lambertian") for s in ("point", "disc", "gaussian")]
    for dtype in (np.float64, np.float32):
        t = np.dtype(dtype).name
        for mode in ("lambertian", "specular"):
            for albedo in (0.0, 0.6, 1.0):
                run("surface/%s/%s/%g" % (t, mode, albedo), light._surface_bounce, r, dr, v, photon, ids, 1.0, (0.1, 0, 0), albedo, mode, c, seed, 3, dtype)
        for phase, g in (("isotropic", 0.0), ("hg", 0.0), ("hg", 0.85), ("hg", -0.3), ("hg", 1e-9), ("rayleigh", 0.0)):
            run("phase/%s/%s/%g" % (t, phase, g), light._phase_redirect, v, dv, photon, ids, phase, g, c, seed, 4, dtype)
        for name, om, ed, eb in (("flat0", 0.0, None, None), ("flat1", 1.0, None, E_EDGES), ("flat", 0.4, None, E_EDGES),
                                 ("layers", [0.0, 1.0, 0.5], EDGES, E_EDGES), ("layers_noE", [0.3, 0.7, 0.5], EDGES, None)):
            run("absorb/%s/%s" % (t, name), light._absorb_scattered, r, v, dv, E, photon, ids, om, ed, (0, 0, 0), eb, seed, 5, dtype)
        laws = ["isotropic", "rayleigh", ("hg", 0.7), ("hg", 0.0), table1, table1024]
        for name, lw, wt, ed in (("one", ["rayleigh"], None, None), ("table1", [table1], None, None), ("table1024", [table1024], None, None),
                                 ("mix", laws, [1, 2, 3, 1, 2, 3], None),
                                 ("layers", laws, [[1, 0, 0, 0, 0, 0], [0, 0, 1, 1, 2, 2], [0, 3, 0, 1, 0, 5]], EDGES)):
            run("layered/%s/%s" % (t, name), light._layered_phase_redirect, r, v, dv, photon, ids, lw, wt, ed, (0, 0, 0), c, seed, 6, dtype)
        for si, src in enumerate(sources):
            run("recycle/%s/%d" % (t, si), light._recycle_spent, r, v, E, photon, ids, src, 2.0 if si % 2 else None, (0, 0, 0), True,
                ([3.5], [1.0]) if si % 3 == 0 else ([1.0, 2.0, 3.0], [0.2, 0.2, 1.0]) if si % 3 == 1 else None, c, seed, 7, dtype)
        run("recycle/%s/top_only" % t, light._recycle_spent, r, v, E, photon, ids, sources[4], 2.0, (0, 0, 0), False, None, c, seed, 7, dtype)
        for name, p, ed, eb in (("p0", [[0.0]], None, None), ("p1", [[1.0]], None, None), ("bands", [[0.0, 1.0, 0.3]], None, E_EDGES),
                                ("cells", [[0.0, 1.0, 0.3], [0.5, 0.5, 0.0], [1.0, 0.2, 0.9]], EDGES, E_EDGES), ("layers", [[0.3], [0.0], [1.0]], EDGES, None)):
            run("path/%s/%s" % (t, name), light._absorb_path, r, v, dv, E, photon, ids, np.array(p), ed, (0, 0, 0), eb, seed, 8, dtype)
    for si, src in enumerate(sources):
        run("emit/%d" % si, light._source_emit, ids, src, c, seed, 9, 14, 15)
    for k, dt in (([0.0, 1e-9, 3.0], 1e-3), ([[1.0, 2.0]], 0.0), (1.0, -1.0), (1.0, np.nan), (1.0, "x"), (1.0, [1, 2])):
        run("pprob/%r/%r" % (k, dt), light._path_probability, k, c, dt)
    nan = float("nan")
    checks = {
        "_check_surface": [(1.0, (0, 0, 0), 0.5, "specular"), ("x", (0, 0, 0), 1, "lambertian"), (-1.0, (0, 0, 0), 1, "lambertian"), (1e200, (0, 0, 0), 1, "lambertian"),
                           (1.0, (0, 0, 0), None, "lambertian"), (1.0, (0, 0, 0), 1.5, "lambertian"), (1.0, (0, 0, 0), nan, "lambertian"), (1.0, (0, 0, 0), 1, "mirror"),
                           ([1.0, 2.0], (0, 0, 0), 1, "lambertian")],
        "_check_phase": [("hg", 0.5), ("rayleigh", 0), ("hg", 1.0), ("hg", nan), ("hg", "g"), ("hg", [0.1, 0.2]), ("mie", 0.0), (3, 0.0)],
        "_check_absorb": [(0.5, None, (0, 0, 0), None), ([0.1, 0.2, 0.3], EDGES, (0, 0, 0), E_EDGES), ([0.1], None, (0, 0, 0), None), ([0.1], EDGES, (0, 0, 0), None),
                          (1.5, None, (0, 0, 0), None), (nan, None, (0, 0, 0), None), ("x", None, (0, 0, 0), None), (0.5, [1.0, 0.5], (0, 0, 0), None)],
        "_check_table_law": [(0, [-1.0, 0.0, 1.0], [1.0, 2.0], 1024), (1, [-1.0, 1.0], [1.0], 1024), (2, [-1.0], [], 4), (3, np.linspace(-1, 1, 6), np.ones(5), 4),
                             (4, [-1.0, 0.5, 0.2, 1.0], [1, 1, 1], 8), (5, [-1.0, 0.0, 1.0], [1.0], 8), (6, [-1.0, 0.0, 1.0], [1.0, 0.0], 8), (7, "ab", [1.0], 8),
                             (8, [-1.0, 0.0, 1.0], [1e-30, 1e30], 8)],
        "_check_layered_phase": [(["isotropic"], None, None, (0, 0, 0)), (["rayleigh", ("hg", 0.5)], [1, 3], None, (0, 0, 0)), ([("hg", 1.0)], None, None, (0, 0, 0)),
                                 ([("hg", "g")], None, None, (0, 0, 0)), ("isotropic", None, None, (0, 0, 0)), ([], None, None, (0, 0, 0)), (["mie"], None, None, (0, 0, 0)),
                                 (["isotropic", "rayleigh"], None, None, (0, 0, 0)), (["isotropic", "rayleigh"], [0, 0], None, (0, 0, 0)),
                                 (["isotropic", "rayleigh"], [[1, 0], [0, 1], [1, 1]], EDGES, (0, 0, 0)), (["isotropic", "rayleigh"], [1, 1], EDGES, (0, 0, 0)),
                                 ([("table", [-1.0, 1.0], [1.0])], None, None, (0, 0, 0))],
        "_check_path_absorb": [(1.0, None, (0, 0, 0), None), ([1.0, 2.0, 3.0], EDGES, (0, 0, 0), None), ([[1.0] * 3] * 3, EDGES, (0, 0, 0), E_EDGES), ([1.0], None, (0, 0, 0), None),
                               (-1.0, None, (0, 0, 0), None), (nan, None, (0, 0, 0), None), ("k", None, (0, 0, 0), None), ([1.0, 2.0], None, (0, 0, 0), E_EDGES)],
    }
    for fn, cases in checks.items():
        for i, args in enumerate(cases):
            run("%s/%d" % (fn, i), getattr(light, fn), *args)
    src = sources[0]
    batch = PhotonBatch(4, 0.0, 1.0, 0, table=(np.array([0.5, 1.0]), np.array([1.0, 2.0])))
    for i, args in enumerate([(src, 2.0, (0, 0, 0), True, None), (src, None, (0, 0, 0), False, None), ("lamp", 2.0, (0, 0, 0), True, None), (src, "t", (0, 0, 0), True, None),
                              (src, -2.0, (0, 0, 0), True, None), (src, 1e200, (0, 0, 0), True, None), (src, None, (0, 0, 0), True, ([1.0, 2.0], [0.5, 1.0])),
                              (src, None, (0, 0, 0), True, ([1.0, 2.0], [0.5, 0.9])), (src, None, (0, 0, 0), True, 5), (src, None, (0, 0, 0), True, batch),
                              (src, None, (0, 0, 0), True, PhotonBatch(4, 0.0, 1.0, 0))]):
        run("_check_recycle/%d" % i, lambda *a: light._check_recycle(*a)[1:], *args)
    np.savez(out + ".npz", **{k.replace("/", "|"): a for k, a in arrays.items()})
    with open(out + ".json", "w") as f:
        json.dump(texts, f)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    got = []
    with tempfile.TemporaryDirectory(prefix="pcl_restate_") as work:
        for side, tree in zip(("old", "new"), sys.argv[1:]):
            out = os.path.join(work, side)
            env = dict(os.environ, PYTHONPATH=os.path.abspath(tree))
            subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", out], env=env, cwd=os.path.abspath(tree))
            with np.load(out + ".npz") as z:
                got.append(({k: z[k] for k in z.files}, json.load(open(out + ".json"))))
    (a_old, t_old), (a_new, t_new) = got
    bad = sorted(set(a_old) ^ set(a_new)) + sorted(set(t_old) ^ set(t_new))
    for k in sorted(set(a_old) & set(a_new)):
        x, y = a_old[k], a_new[k]
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            bad.append(k)
    bad += [k for k in sorted(set(t_old) & set(t_new)) if t_old[k] != t_new[k]]
    for k in bad:
        print("DIFFERS: %s" % k.replace("|", "/"))
    print("%d arrays and %d texts compared, %d differ" % (len(a_old), len(t_old), len(bad)))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
