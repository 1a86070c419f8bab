"""What the cost tools of the writer sweeps (tools/bench_surface.py, bench_phase.py, bench_absorb.py, bench_layered_phase.py,
bench_recycle.py, bench_path_absorb.py, bench_reemit.py) share; not run by itself.

A tool keeps what is its own -- its docstring, ``CASES``, how a state is prepared, which call is timed and what a slot costs in
bytes -- and takes from here the population, the two timed loops, the JSON lines and the command line:

    def bench(n, runs, dtype):
        with photons(n, dtype) as dev:
            y, got = yardstick(runs, reset, call)          # a call that changes nothing: the state is made once
            s, got, prepared = timed(runs, reset, call)    # a call that writes photons: the state is made anew every time
            emit({"n": n, "dtype": dtype}, case, **s)
    main(bench, "100000000")
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from physicl_amd import _hip as hip  # noqa: E402

C_LIT, H_LIT, DT = 299792458.0, 6.62607015e-34, 0.0005
STEP = C_LIT * DT                                               # one Newton step of a photon: 150 km
ORIGIN = (3.0 * STEP, -1.0 * STEP, 0.5 * STEP)


class Isotropic:                                                # the point every tool puts its photons on before the move
    origin, e1, e2, d = ORIGIN, (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
    angular, spatial, cos_half_angle, radius = "isotropic", "point", 0.0, 0.0


@contextlib.contextmanager
def photons(n, dtype):
    """Device 0 with one store of ``n`` photons, energies from 1 to 3; closed on the way out."""
    dev = hip.Device(0)
    try:
        dev.store_alloc(n, dtype)
        dev.fill_photons(n, 0, C_LIT, 1.0, 3.0, 1)
        yield dev
    finally:
        dev.close()


def stats(t):
    med = statistics.median(t)
    return {"s": t, "median_s": med, "spread": (max(t) - min(t)) / med}


def emit(base, case, **kw):
    print(json.dumps(dict(base, case=case, **kw)), flush=True)


def timed(runs, reset, call):
    """``runs`` timed calls after one warm-up call; ``reset(k)`` makes the state anew before call ``k`` (0 is the warm-up) and is
    not timed.  The wall time is taken around ``call(k)``, which synchronises.  Gives the statistics, the last call's answer and
    what the last ``reset`` returned."""
    t, got, prepared = [], None, None
    for k in range(runs + 1):
        prepared = reset(k)
        t0 = time.perf_counter()
        got = call(k)
        if k:
            t.append(time.perf_counter() - t0)
    return stats(t), got, prepared


def yardstick(runs, reset, call):
    """The same for a call that leaves the store as it is: ``reset()`` once, then the warm-up ``call(0)`` -- the first look at the
    store pays the core's materialise pass -- and ``runs`` timed calls.  Gives the statistics and the last call's answer."""
    reset()
    call(0)
    t, got = [], None
    for k in range(runs):
        t0 = time.perf_counter()
        got = call(1 + k)
        t.append(time.perf_counter() - t0)
    return stats(t), got


def main(bench, sizes):
    """The tools' command line; ``bench(n, runs, dtype)`` is run for every size of ``--n`` (default: ``sizes``)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default=sizes, help="store sizes, comma separated")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dtype", default="f64")
    a = ap.parse_args()
    for n in (int(float(x)) for x in a.n.split(",")):
        bench(n, a.runs, a.dtype)
