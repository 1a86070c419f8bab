"""CPU: the stdout line bench.py prints is a bounded projection of the run's record (no GPU: committed full records
of earlier runs are projected again).  Round 4's line had grown to 31 kB and the driver, which keeps the last ~8 000
characters of stdout, could not parse it."""
import glob
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


RECORDS = sorted(p for p in glob.glob(os.path.join(ROOT, "profiles", "r0[45]_bench_*.json")) if "_bench_line_" not in p)
LINES = sorted(glob.glob(os.path.join(ROOT, "profiles", "r0[56]_bench_line_*.json")))


@pytest.mark.parametrize("path", RECORDS, ids=[os.path.basename(p) for p in RECORDS])
def test_contract_line_of_a_full_record_fits_the_drivers_window(path):
    b = bench_module()
    rec = json.load(open(path))
    if "config" not in rec or "roofline" not in rec:
        pytest.skip("not a full record")
    line = b.contract_line(rec, "bench_detail.json")
    s = json.dumps(line)
    assert len(s) < b.LINE_LIMIT == 4000
    back = json.loads(("x" * 9000 + "\n" + s + "\n").rstrip()[-8000:].splitlines()[-1])     # the driver's view
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "roofline_hbm", "cpu_baseline", "collective", "detail_file"):
        assert k in back, k
    assert back["value"] == rec["value"] and back["roofline"]["frac"] == rec["roofline"]["frac"]
    assert "model" not in back["config"] and "workload" in back["config"]
    for k in ("per_block", "instruction_counts", "k_step_launch_work", "delete", "api", "mixed"):
        assert k not in back and k not in back["roofline"]


@pytest.mark.parametrize("path", LINES, ids=[os.path.basename(p) for p in LINES])
def test_the_committed_lines_are_what_the_driver_can_read(path):
    """The stdout lines of the round's own runs (driver's command, default, 2-rank rehearsal), as printed."""
    text = open(path).read()
    assert text.count("\n") == 1 and len(text) < 4000
    line = json.loads(text[-8000:].splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config", "roofline", "roofline_hbm",
              "cpu_baseline", "collective", "detail_file"):
        assert k in line, k
    r = line["roofline"]
    assert r["bound"] == "valu" and r["unit"] == "SIMD-cycles/s" and 0 < r["frac"] <= 1.0 and 1.5 < r["clock_GHz"] < 2.6
    assert isinstance(r["traffic"], (int, float)) and abs(r["traffic"] / line["config"]["photons_per_gpu"] - 128) < 2
    if line["n_gpus"] == 1:
        assert line["roofline_hbm"]["frac"] >= 0.6 and line["cpu_baseline"]["kind"] == "port" and line["cpu_baseline"]["cores"] >= 1


def test_line_sheds_optional_parts_rather_than_outgrow_the_window():
    b = bench_module()
    rec = json.load(open(RECORDS[0]))
    rec["config"]["workload"] = "w" * 1500
    rec["cpu_baseline"] = dict(rec.get("cpu_baseline") or {}, sample="s" * 900, value=1.0, cores=1, kind="port")
    s = json.dumps(b.contract_line(rec, "bench_detail.json"))
    assert len(s) < 4000 and "roofline" in json.loads(s)


def test_detail_file_is_written_atomically_and_is_the_full_record(tmp_path, monkeypatch):
    b = bench_module()
    rec = json.load(open(RECORDS[0]))
    monkeypatch.setenv("PCL_BENCH_DETAIL", str(tmp_path / "d.json"))
    rel = b.write_detail(rec)
    assert json.load(open(tmp_path / "d.json")) == rec and rel.endswith("d.json")
    assert not [p for p in os.listdir(tmp_path) if ".tmp" in p]


def test_a_plain_run_times_one_block_and_full_keeps_five():
    b = bench_module()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.repeats == 1 and not a.full and a.dump_outputs is None
    assert b.parse_args(["--full"]).repeats == 5 and b.parse_args(["--full", "--repeats", "2"]).repeats == 2
    assert b.parse_args(["--dump-outputs", "out"]).dump_outputs == "out"


class _FakeStore:
    """The four calls dump_outputs makes, on host arrays: field f of slot i holds f * 1e9 + i, ids are id_base + i."""

    def __init__(self, n, id_base=0):
        self.count, self.id_base = n, id_base

    def download(self, field, n, offset):
        assert 0 <= offset and offset + n <= self.count
        return field * 1e9 + np.arange(offset, offset + n, dtype=np.float64)

    def download_ids(self, n, offset):
        assert 0 <= offset and offset + n <= self.count
        return self.id_base + np.arange(offset, offset + n, dtype=np.int64)


class _FakeBench:
    def __init__(self, n, rank=0):
        from types import SimpleNamespace
        self.rank, self.dev, self.totals = rank, _FakeStore(n), np.array([n, 7, 1, 2, 3], dtype=np.int64)
        self.hip = SimpleNamespace(R0=0, R1=1, R2=2, V0=3, V1=4, V2=5, E=12)


def _dumped(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_writes_every_photon_of_a_small_store(tmp_path):
    b = bench_module()
    b.dump_outputs(_FakeBench(1000), str(tmp_path / "d"))
    d = _dumped(tmp_path / "d")
    assert sorted(d) == ["E", "counters", "id", "r", "v"] and all(a.dtype == np.float64 for a in d.values())
    assert list(d["counters"]) == [1000, 7, 1, 2, 3]
    assert np.array_equal(d["id"], np.arange(1000)) and d["r"].shape == d["v"].shape == (1000, 3)
    assert np.array_equal(d["v"][:, 1], 4e9 + np.arange(1000)) and np.array_equal(d["E"], 12e9 + np.arange(1000))


def test_dump_outputs_samples_a_big_store_the_same_way_every_time(tmp_path):
    """1e8 photons: a fixed sample of whole blocks, rows of the same slots in every array, at most 64 MB in all."""
    b = bench_module()
    b.dump_outputs(_FakeBench(100_000_000), str(tmp_path / "a"))
    b.dump_outputs(_FakeBench(100_000_000), str(tmp_path / "b"))
    b.dump_outputs(_FakeBench(100_000_000, rank=1), str(tmp_path / "c"))        # only rank 0 writes
    a, again = _dumped(tmp_path / "a"), _dumped(tmp_path / "b")
    assert not os.path.exists(tmp_path / "c")
    assert all(np.array_equal(a[k], again[k]) for k in a)
    ids = a["id"]
    assert len(ids) == b.DUMP_SAMPLE and len(np.unique(ids)) == len(ids) and np.all(np.diff(ids) > 0)
    assert np.all(ids[::b.DUMP_BLOCK] % b.DUMP_BLOCK == 0) and ids[-1] < 100_000_000
    assert np.array_equal(a["r"][:, 2] - 2e9, ids) and np.array_equal(a["E"] - 12e9, ids)
    assert sum(os.path.getsize(os.path.join(tmp_path, "a", f)) for f in os.listdir(tmp_path / "a")) <= 64 << 20
