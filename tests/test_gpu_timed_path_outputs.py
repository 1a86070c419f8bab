"""GPU: a plain bench.py run (no --full) times exactly --steps steps after --warmup and nothing else, and --dump-outputs writes
what the timed path computed in its last step (small N so it runs in seconds)."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_line(stdout):
    """The one stdout line, parsed as the driver does (the last line of the last ~8 000 characters)."""
    lines = [ln for ln in stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    assert len(lines[-1]) < 4000, len(lines[-1])
    line = json.loads(stdout.rstrip()[-8000:].splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config", "roofline",
              "roofline_hbm", "cpu_baseline", "collective", "detail_file"):
        assert k in line, k
    return line


def run_plain(dump, *extra):
    """A plain run (no --full) with --dump-outputs: the parsed line, the detail record and the dumped arrays."""
    with tempfile.TemporaryDirectory() as tmp:
        detail = os.path.join(tmp, "bench_detail.json")
        out = subprocess.check_output([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--photons", "300000",
                                       "--steps", "6", "--warmup", "3", "--dump-outputs", dump, *extra], cwd=ROOT,
                                      env=dict(os.environ, PCL_BENCH_DETAIL=detail), stderr=subprocess.DEVNULL, timeout=600)
        line = check_line(out.decode())
        d = json.load(open(detail))
    arrays = {name: np.load(os.path.join(dump, name + ".npy")) for name in ("counters", "r", "v", "E", "id")}
    return line, d, arrays


def test_plain_run_times_exactly_the_steps_and_dumps_what_they_computed(tmp_path):
    """Without --full the run times ONE block of exactly --steps steps, runs no other leg, and --dump-outputs writes the
    last step's counters and photons: the same arrays from a second run with another --steps-per-launch."""
    line, d, a = run_plain(str(tmp_path / "a"))
    assert line["steps"] == 6 and line["warmup"] == 3 and line["repeats"] == 1 and len(line["repeat_ms_per_step"]) == 1
    assert line["metric"] == "particle-steps/sec" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 / 300000 - 1.0) < 1e-9
    assert line["cpu_baseline"] is None and line["roofline_hbm"] is None and "legs" not in line
    for k in ("single_step", "tame", "delete", "iso_1e7", "mixed", "api", "cpu_baseline"):
        assert k not in d, k
    assert d["config"]["steps_per_timed_launch"] == 6 and d["roofline"]["launches"] == 1
    assert a["counters"].dtype == np.float64 and a["counters"].shape == (5,)
    assert list(a["counters"]) == [float(d["counters_last_step"][k]) for k in ("N", "hits", "xp", "yp", "zp")]
    assert a["r"].shape == a["v"].shape == (300000, 3) and a["E"].shape == (300000,) and a["r"].dtype == np.float64
    assert np.array_equal(a["id"], np.arange(300000, dtype=np.float64))
    assert np.all(np.isfinite(a["r"])) and np.all(a["E"] > 0)
    assert np.allclose(np.linalg.norm(a["v"], axis=1), 299792458.0, rtol=1e-12)      # scattering keeps |v| = c
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")) <= 64 << 20
    # a second run, one launch per step: the same arrays, bit for bit
    _, _, c = run_plain(str(tmp_path / "c"), "--steps-per-launch", "1")
    for name in a:
        assert np.array_equal(a[name], c[name]), name
