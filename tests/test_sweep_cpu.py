"""CPU: the host arithmetic the add-on units share (physicl_amd/csrc/pcl_sweep.h, the layer above its __HIPCC__ section).

tests/native/sweep_host.cpp includes the header as a plain C++ program, is built with g++ under the address and
undefined-behaviour sanitizers and run as a child process (it is not loaded into Python).  Its answers are held against

* the properties a sweep's geometry needs (every workgroup takes ``trips`` or ``trips - 1`` trips, fewer than 2^32 slots);
* literal transcriptions, kept here, of what pcl_spectrum.hip / pcl_shell.hip / pcl_grid.hip did in place before the header,
  and of the offsets into a call's device block that every entry of pcl_surface.hip derived by hand before ``layout_of``;
* numpy slicing, for the zero / copy / add of a call's output spans (an empty span is NULL there, as a caller may pass it).
"""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")
K_BLOCK, MAX_SLOTS = 256, 2 ** 32 - 256
PLAIN, SIGNED_SQUARE, SQUARE = 0, 1, 2


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sweep") / "sweep_host")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g", "-I",
                           os.path.join(ROOT, "physicl_amd", "csrc"), os.path.join(ROOT, "tests", "native", "sweep_host.cpp"), "-o", exe])

    def run(lines):
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.returncode, p.stderr[-3000:])
        out = p.stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


# ------------------------------------------------------------------------------------------------ balanced_grid
def grid_as_the_units_had_it(N, n_cu, per_cu):
    blocks = (N + K_BLOCK - 1) // K_BLOCK
    grid, cap = blocks, (n_cu if n_cu > 0 else 256) * per_cu
    if grid > cap:
        trips = (blocks + cap - 1) // cap
        while trips * K_BLOCK > MAX_SLOTS:
            cap *= 2
            trips = (blocks + cap - 1) // cap
        grid = (blocks + trips - 1) // trips
    return grid


SLOTS = [1, 255, 256, 257, 2048 * 8 * 256 - 1, 2048 * 8 * 256 + 1, 10 ** 7, 10 ** 8, 2 ** 40]
GRID_CASES = [(N, n_cu, per_cu) for N in SLOTS for n_cu in (0, 1, 256) for per_cu in (1, 3, 8)]


def test_balanced_grid(ask):
    got = [int(x) for x in ask(["grid %d %d %d" % c for c in GRID_CASES])]
    forced_seen = 0
    for (N, n_cu, per_cu), grid in zip(GRID_CASES, got):
        blocks = -(-N // K_BLOCK)
        cap = (n_cu if n_cu > 0 else 256) * per_cu
        assert 1 <= grid <= blocks, (N, n_cu, per_cu, grid)
        if blocks > cap:
            forced = -(-blocks // cap) * K_BLOCK > MAX_SLOTS      # a workgroup of ``cap`` would sweep 2^32 slots or more
            forced_seen += forced
            while -(-blocks // cap) * K_BLOCK > MAX_SLOTS:
                cap *= 2
            assert grid <= cap, (N, n_cu, per_cu, grid, forced)
        else:
            assert grid == blocks
        trips = -(-blocks // grid)
        assert (grid - 1) * trips < blocks and trips * K_BLOCK <= MAX_SLOTS, (N, n_cu, per_cu, grid, trips)
        assert grid == grid_as_the_units_had_it(N, n_cu, per_cu), (N, n_cu, per_cu)
    assert forced_seen >= 1                                        # 2^40 slots on one CU


def test_resident_per_cu_and_tile_log(ask):
    lds = [0, 1, 20 * 1024, 40 * 1024, 64 * 1024, 200 * 1024]
    got = [int(x) for x in ask(["lds %d" % b for b in lds])]
    assert got == [8, 8, 8, 4, 2, 1]
    for b, g in zip(lds, got):                                     # as pcl_grid.hip had it (with its guard) and pcl_shell.hip (lds > 0)
        assert g == min(8, max(1, 160 * 1024 // (b if b > 0 else 1)))
    tiles = [2048, 1, 2, 0, 3, -4, 2047, 2 ** 62, 2 ** 62 + 1, 2 ** 63 - 1]
    assert [int(x) for x in ask(["tile %d" % t for t in tiles])] == [11, 0, 1, -1, -1, -1, -1, 62, -1, -1]


# ------------------------------------------------------------------------------------------------ the edge check
def edges_as_the_units_had_them(e, transform):
    """None, or the edges the kernel compares against: the loops of plane_spectra (pcl_spectrum.hip), check_edges
    (pcl_shell.hip) and check_spec (pcl_grid.hip) before pcl_sweep.h, statement by statement."""
    out = []
    if transform == PLAIN:
        for b in range(len(e)):
            if not math.isfinite(e[b]) or (b > 0 and not e[b] > e[b - 1]):
                return None
        return list(e)
    if transform == SIGNED_SQUARE:
        for b in range(len(e)):
            if not math.isfinite(e[b]) or (b > 0 and not e[b] > e[b - 1]):
                return None
            v = e[b] * math.fabs(e[b])
            if not math.isfinite(v) or (b > 0 and not v > out[-1]):
                return None
            out.append(v)
        return out
    for b in range(len(e)):
        v = e[b]
        if not math.isfinite(v):
            return None
        if v < 0:
            return None
        v = v * v
        if not math.isfinite(v):
            return None
        if b > 0 and not v > out[-1]:
            return None
        out.append(v)
    return out


# edges -> accepted under (plain, e*|e|, e*e), by hand
EDGE_CASES = [
    ([0.5, 1.0, 2.0, 4.0], (True, True, True)),                    # increasing
    ([-1.0, -0.25, 0.0, 0.5, 1.0], (True, True, False)),           # ... with a negative edge: no radius
    ([0.0, 0.1, 0.7], (True, True, True)),
    ([1.0, 1.0, 2.0], (False, False, False)),                      # equal neighbours
    ([0.0, 1.0, 2.0, 2.0], (False, False, False)),
    ([2.0, 1.0], (False, False, False)),                           # decreasing
    ([0.0, 2.0, 1.0, 3.0], (False, False, False)),
    ([NAN, 1.0], (False, False, False)),
    ([0.0, NAN, 1.0], (False, False, False)),
    ([0.0, 1.0, NAN], (False, False, False)),
    ([0.0, INF], (False, False, False)),
    ([-INF, 0.0], (False, False, False)),
    ([1e200, 1e201], (True, False, False)),                        # squares overflow
    ([-1e200, 0.0, 1.0], (True, False, False)),
    ([1.0, 1.5e154], (True, False, False)),
    ([-1e-200, 1e-200], (True, False, False)),                     # distinct, equal (-0, +0) after e*|e|
    ([1e-200, 2e-200], (True, False, False)),                      # ... and after e*e
    ([0.0, 1e-200], (True, False, False)),
    ([0.0, 1.0], (True, True, True)),                              # a single bin
    ([-1.0, 1.0], (True, True, False)),
    ([3.0, 3.0], (False, False, False)),
]


def test_edge_check(ask):
    asked = [(e, t) for e, _ in EDGE_CASES for t in (PLAIN, SIGNED_SQUARE, SQUARE)]
    got = ask(["edges %d %d %s" % (t, len(e) - 1, " ".join(float(x).hex() for x in e)) for e, t in asked])
    by_hand = [ok[t] for _, ok in EDGE_CASES for t in (PLAIN, SIGNED_SQUARE, SQUARE)]
    for (e, t), line, want_ok in zip(asked, got, by_hand):
        want = edges_as_the_units_had_them(e, t)
        assert (want is not None) == want_ok, (e, t)
        tok = line.split()
        assert tok[0] == ("1" if want_ok else "0"), (e, t, line)
        if want_ok:                                                # bit for bit (a signed zero included)
            assert [float.fromhex(x).hex() for x in tok[1:]] == [float(x).hex() for x in want], (e, t, line)


# ------------------------------------------------------------------------------------------------ the staged block
def block_as_the_units_had_it(out_bytes, tab_bytes, n_ids, n_kind):
    """Where a call's tables, ids and kind bytes start, and the size of its device block: ``base + out_bytes (+ tab_bytes (+
    id_bytes))`` as every entry of pcl_surface.hip derived its pointers, and the sum stage() allocated, before layout_of."""
    id_bytes = n_ids * 8
    tables = out_bytes
    ids = out_bytes + tab_bytes
    kind = out_bytes + tab_bytes + id_bytes
    return tables, ids, kind, out_bytes + tab_bytes + id_bytes + n_kind


LAYOUT_CASES = [
    (16, 0, 0, 0),                                                 # no tables, no ids, no kinds
    (16, 40, 0, 0), (8 * 26, 8 * 13, 0, 0),                        # tables only
    (16, 0, 1000, 0), (16, 24, 1000, 0),                           # ids without kinds
    (16, 0, 0, 1000), (16, 24, 0, 1001),                           # kinds without ids
    (8 * 30, 8 * 21, 4097, 4097), (16, 8 * 2048, 10 ** 8, 10 ** 8),   # everything present
    (8, 0, 0, 0), (8, 0, 3, 3), (8, 8, 3, 0), (8, 8, 0, 3), (8, 16, 5, 5),   # an out_bytes of one cell
]


def test_block_layout(ask):
    got = ask(["layout %d %d %d %d" % c for c in LAYOUT_CASES])
    for c, line in zip(LAYOUT_CASES, got):
        assert tuple(int(x) for x in line.split()) == block_as_the_units_had_it(*c), c


# ------------------------------------------------------------------------------------------------ the output spans
SPAN_CASES = [
    ("absorption, L=0, n_E=0: E_hist NULL", [2 + 1, 0]),
    ("absorption, L=3, n_E=8", [2 + 3, 3 * 8]),
    ("path absorption, 1 x 1 cells", [2, 1]),
    ("path absorption, 2 x 3 cells", [2, 6]),
    ("shell, 2 shells, no energy bins (NULL), 5 mu bins", [4, 0, 20]),
]


def test_output_spans(ask):
    rs = np.random.RandomState(11)
    asked, want = [], []
    for _, lens in SPAN_CASES:
        cells = sum(lens)
        before = np.concatenate([1000 * (i + 1) + np.arange(n, dtype=np.int64) for i, n in enumerate(lens)])
        flat = rs.randint(-2 ** 40, 2 ** 40, cells).astype(np.int64)
        head = "%d %s" % (len(lens), " ".join(str(n) for n in lens))
        vals = " ".join(str(int(x)) for x in flat)
        for op in ("zero", "copy", "add"):
            asked.append("spans %s %s%s" % (op, head, "" if op == "zero" else " " + vals))
            after, at = [], 0
            for n in lens:                                         # span by span, with numpy slicing
                was, new = before[at:at + n], flat[at:at + n]
                after.append(np.zeros(n, dtype=np.int64) if op == "zero" else new.copy() if op == "copy" else was + new)
                at += n
            want.append([cells] + np.concatenate(after).tolist())
    got = ask(asked)                                               # (exit status 0 under the sanitizers: the NULL spans were not touched)
    for line, line_want, q in zip(got, want, asked):
        assert [int(x) for x in line.split()] == line_want, q


# ------------------------------------------------------------------------------------------------ the core
def test_the_core_does_not_know_the_header():
    csrc = os.path.join(ROOT, "physicl_amd", "csrc")
    for name in ("physicl_hip.hip", "pcl_device.h", "pcl_sincos.h"):
        assert "pcl_sweep" not in open(os.path.join(csrc, name)).read(), name
    text = open(os.path.join(csrc, "pcl_sweep.h")).read()
    assert "pcl_device.h" not in text.split("#pragma once")[1] and "pcl_sincos.h" not in text.split("#pragma once")[1]
