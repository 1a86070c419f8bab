#!/usr/bin/env python3
"""What a photon source costs on top of the bulk fill.

    python tools/bench_source.py --n 100000000 --runs 5

Wall time around fill_photons + sync (the yardstick: 13 rows, 104 B/photon in fp64) and around fill_photons + apply_source +
sync for a few source forms, medians over ``--runs``; the overwrite's own bytes (0, 24 or 48 B/photon), the rate they imply and
that rate over the plain fill's.  One JSON line per form.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicl_amd import _hip, light  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=100_000_000)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--dtype", default="f64", choices=["f64", "f32"])
a = ap.parse_args()
C = 299792458.0
FORMS = [("beam_off_axis", light.PhotonSource(direction=(1, -2, 0.5)), 24),
         ("isotropic_point", light.PhotonSource(origin=(6371000.0, 0, 0), angular="isotropic"), 48),
         ("cone_disc", light.PhotonSource(origin=(6371000.0, 0, 0), angular="cone", half_angle=0.3, spatial="disc", radius=1000.0), 48),
         ("lambertian_gaussian", light.PhotonSource(origin=(6371000.0, 0, 0), angular="lambertian", spatial="gaussian", radius=1000.0), 48)]
esz = 8 if a.dtype == "f64" else 4

with _hip.Device(0) as dev:
    dev.store_alloc(a.n, a.dtype)

    def timed(src):
        out = []
        for _ in range(a.runs + 1):                          # (the first run warms the code objects up and is dropped)
            dev.sync()
            t0 = time.perf_counter()
            dev.fill_photons(a.n, 0, C, 1.0, 2.0, 7)
            if src is not None:
                dev.apply_source(src, C, 7)
            dev.sync()
            out.append(time.perf_counter() - t0)
        return statistics.median(out[1:])
    t_fill = timed(None)
    fill_rate = 13 * esz * a.n / t_fill / 1e9
    print(json.dumps({"form": "plain_fill", "n": a.n, "dtype": a.dtype, "median_s": t_fill, "bytes_per_photon": 13 * esz, "GB_per_s": fill_rate}))
    for name, src, extra in FORMS:
        t = timed(src)
        extra = extra * esz // 8
        rate = extra * a.n / max(t - t_fill, 1e-9) / 1e9
        print(json.dumps({"form": name, "n": a.n, "dtype": a.dtype, "median_s": t, "source_s": t - t_fill, "bytes_per_photon": extra,
                          "GB_per_s": rate, "rate_over_fill": rate / fill_rate}))
