#!/usr/bin/env python3
"""What one pass of the spectral ground (Device.ground_spectral, SpectralSurfaceStep) costs on the device, beside the grey ground's
sweep (Device.surface_reflect) on the same store in the same process.

    python tools/bench_spectral_surface.py [--n 100000000] [--runs 5] [--dtype f64]

One store of ``--n`` photons with energies from 1 to 3, one process.  A call changes the photons it hits, so the state is made anew
before every timed call, on the device (not timed), as tools/bench_surface.py makes it: the photons are put on one point
(Device.apply_source) and moved one Newton step of 150 km.  What is quoted is the wall time around the synchronising call,
``--runs`` repeats after one warm-up call, the median with the spread (max - min) / median.  One JSON line each:
  nobody_hit         isotropic source, a sphere the cloud is wholly outside of: the grey ground (lambertian, albedo 0.5), then the
                     spectral ground with 1 band and with 1024; 48 B per slot (fp64) are read and nothing is written -- the tables
                     (56 B and 32 KiB of LDS per workgroup) are loaded all the same
  everybody_hit_1    a beam, a sphere just ahead of it that every move enters: the grey ground (lambertian, albedo 0.5), then one band
                     that holds every energy with albedo 0.5 and specular 0 -- the grey ground's own draws, plus kind, E and the lookup
  everybody_hit_1024 the same beam and 1024 bands from 0.5 to 3.5, albedo 0.5 and specular 0.5 in each: the lookup is ten probes of
                     LDS, a reflected lane draws a third block, and every hit lane adds to its band's cell (an LDS atomic)
No ratio is fixed in advance: ``over_ground`` is the case's median over the grey ground's median of the same case.
Hit lanes also load E (1 word) and v (3 words) and write r, v, dr, dv (12 words): bytes_per_slot = 6 words + share_hit * 16 words.
"""
import numpy as np

from bench_surface import Beam, off
from sweep_bench import C_LIT, STEP, DT, Isotropic, emit, main, photons, timed

ALBEDO, SPECULAR = 0.5, 0.5
# case -> (source, centre of the sphere, its radius, bands, specular): the position before the move is outside every sphere
CASES = [("nobody_hit", Isotropic, off(100.0), STEP, (1, 1024), SPECULAR),
         ("everybody_hit_1", Beam, off(1.2, Beam.d), 0.5 * STEP, (1,), 0.0),
         ("everybody_hit_1024", Beam, off(1.2, Beam.d), 0.5 * STEP, (1024,), SPECULAR)]


def bench(n, runs, dtype):
    esz = 8 if dtype == "f64" else 4
    base = {"n": n, "dtype": dtype}
    with photons(n, dtype) as dev:
        def reset(source):
            dev.apply_source(source, C_LIT, 1)
            dev.step_newton(DT)
            dev.sync()

        for case, source, center, radius, bands, specular in CASES:
            sweeps = [("ground_lambertian", 15, lambda k: sum(dev.surface_reflect(radius, center, ALBEDO, "lambertian", C_LIT, 1, 1 + k)))]
            for B in bands:
                edges = np.linspace(0.5, 3.5, B + 1)
                sweeps.append(("spectral_%d" % B, 16, lambda k, B=B, edges=edges: int(dev.ground_spectral(
                    radius, edges, np.full(B, ALBEDO), np.full(B, specular), center, C_LIT, 1, 1 + k)[0][:2].sum())))
            ground = None
            for name, words, call in sweeps:
                s, got, _ = timed(runs, lambda k: reset(source), call)
                ground = ground or s["median_s"]
                share = got / n
                bps = (6 + words * share) * esz
                emit(base, case, sweep=name, share_hit=share, bytes_per_slot=bps, GBps=bps * n / s["median_s"] / 1e9,
                     over_ground=s["median_s"] / ground, **s)


if __name__ == "__main__":
    main(bench, "100000000")
