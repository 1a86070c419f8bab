"""CPU: the sweeps of the build's third table (physicl_amd/build.py: ``MORE``) -- what tests/test_build_later_cpu.py checks per row
of ``LATER``, with every expectation read from the row itself (entries, kernel, count, src, vgprs): the built library exports both
entry points, the header declares them and ``_hip.EXPORTS`` lists them; the unit's device assembly, compiled once with the library's
own options, holds the row's instantiations in its forms with no scratch and no VGPR spills within the row's budget.  The next sweep
is one more row; this file asserts only that ``k_absorb_grid`` is among them.

And for pcl_step_absorb_grid: the header's words and LDS formula and their mirror in ``_hip``, the binding's marshalling, the refusals
that need no device, the older kernels against the commit in front of the one that brought the sweep (tools/compare_unit_asm.py), and
the table of past-one-trip cases of tests/test_grid_absorb_trips_gpu.py."""
import ast
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from physicl_amd import _hip, build
from grid_absorb_reference import BAD_CALLS, CENTER, GOOD_OM, GOOD_P, abi_args
from test_build_cpu import FORMS
from test_grid_absorb_trips_gpu import TRIP_CASES

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
ENTRIES = ("pcl_step_absorb_grid", "pcl_group_step_absorb_grid")
by_row = pytest.mark.parametrize("row", build.MORE, ids=[s["kernel"] for s in build.MORE])


def test_the_table_describes_sweeps_of_the_units_there_are():
    assert "k_absorb_grid" in [s["kernel"] for s in build.MORE]
    older = [s for u in build.ADDONS for s in u["sweeps"]] + build.LATER
    for s in build.MORE:
        assert set(s) == {"entries", "kernel", "count", "src", "vgprs"} and s["src"] in [u["src"] for u in build.ADDONS], s
        assert len(s["entries"]) == 2 and s["entries"][1].startswith("pcl_group_") and s["kernel"].startswith("k_"), s
        assert s["count"] in FORMS and isinstance(s["vgprs"], int) and 0 < s["vgprs"] <= 512, s
    every = older + build.MORE
    entries = [e for s in every for e in s["entries"]]
    assert len(set(entries)) == len(entries) == 2 * len(every)            # no entry point belongs to two sweeps
    # (a sweep's instantiations are found by the kernel's name inside the mangled one: no name holds another)
    assert not any(a is not b and a["kernel"] in b["kernel"] for a in every for b in every)
    (row,) = [s for s in build.MORE if s["kernel"] == "k_absorb_grid"]
    assert row["entries"] == ENTRIES and row["count"] == 4 and os.path.basename(row["src"]) == "pcl_surface.hip"
    assert build.csrc_sha() == "b54e0443ee3f400f"                       # the tuned core has not moved


@by_row
def test_library_exports_both_entry_points_and_the_header_declares_them(row):
    build.build_lib()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert lib.pcl_abi_version() == 1
    text = re.sub(r"/\*.*?\*/", "", open(build.ABI_HEADER).read(), flags=re.S)
    for entry in row["entries"]:
        assert hasattr(lib, entry) and entry in _hip.EXPORTS and re.search(r"\b%s\s*\(" % entry, text), entry


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """source -> its device assembly, compiled with the library's own options; each unit is compiled once for the module."""
    texts = {}

    def get(src):
        if src not in texts:
            out = str(tmp_path_factory.mktemp("asm") / "unit.s")
            subprocess.check_call([build.HIPCC] + [f for f in build.FLAGS if f not in ("-shared", "-fPIC")] +
                                  ["--cuda-device-only", "-S", "-o", out, src], stderr=subprocess.DEVNULL)
            texts[src] = open(out).read()
        return texts[src]
    return get


@by_row
def test_kernels_use_no_scratch(row, assembly):
    """From the unit's assembly: every instantiation of the row's kernel in its forms, nothing in scratch, no spills, the row's budget."""
    text = assembly(row["src"])
    kernels = re.findall(r"\.name:\s+(_Z\w*%s\w*)\n(.*?)\.wavefront_size" % row["kernel"], text, re.S)
    assert len(kernels) == row["count"], [k for k, _ in kernels]
    form, forms = FORMS[row["count"]]
    assert sorted(re.search(row["kernel"] + form, k).groups() for k, _ in kernels) == forms
    for kernel, blk in kernels:
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))                                  # noqa: E731
        print(kernel, "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "sgpr spills", get("sgpr_spill_count"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, kernel
        assert get("vgpr_count") <= row["vgprs"], kernel


# ------------------------------------------------------------------------------------------------ the header and its mirror
def test_the_header_states_the_rule_the_words_and_the_lds_formula():
    text = open(build.ABI_HEADER).read()
    flat = " ".join(text.split()).replace("* ", "")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "#define PCL_ABI_VERSION 1\n" in text
    for line in ("(id_lo, id_hi, pass, 27)", "(id_lo, id_hi, pass, 28)", "words 27 and 28 are used by nothing else",
                 "with this call's 27 and 28 the taken words are 0-5 and 8-28", "absorbed iff u < p_host[c]", "absorbed iff not (u < omega0_host[c])",
                 "exposed and (dv0 != 0 or dv1 != 0 or dv2 != 0)", "v_k = 0 and dv_k = 0", "the particle is not written at all",
                 "8 E + 8 t C + 4 (4 + C) <= PCL_ABSORB_GRID_LDS_BYTES", "C <= PCL_ABSORB_GRID_LDS_CELLS", "p = -expm1(-k (c*dt))",
                 "the ids go along only if some p > 0 or some omega0 < 1", "an empty store answers zeros without a launch"):
        assert line in flat, line
    for older in ("0-5 and 8-26 are taken", "words 25 and 26 are used by nothing else"):       # the older sentences stand
        assert older in flat
    for name, value in (("MAX_BANDS", "1024"), ("MAX_CELLS", r"\(1 << 20\)"), ("LDS_CELLS", "4096"), ("LDS_BYTES", "65536")):
        assert re.search(r"#define PCL_ABSORB_GRID_%s %s" % (name, value), code), name
    assert (_hip.ABSORB_GRID_MAX_BANDS, _hip.ABSORB_GRID_MAX_CELLS, _hip.ABSORB_GRID_LDS_CELLS, _hip.ABSORB_GRID_LDS_BYTES) == (1024, 1 << 20, 4096, 65536)
    for entry in ENTRIES:
        assert len(_hip._PROTOTYPES[entry]) == 14
    from physicl_amd.multidev import MultiDevice
    assert all(hasattr(c, "absorb_grid") for c in (_hip.Device, _hip.DeviceGroup, MultiDevice))


def test_the_lds_formula_is_mirrored_and_puts_16_cubed_in_lds_with_one_table_only():
    assert _hip.absorb_grid_lds_bytes(1, 51, 4096) == 8 * 51 + 8 * 4096 + 4 * 4100 == 49576
    assert _hip.absorb_grid_lds_form(1, 51, 4096) and not _hip.absorb_grid_lds_form(2, 51, 4096)
    assert not _hip.absorb_grid_lds_form(1, 52, 17 * 16 * 16) and _hip.absorb_grid_lds_form(2, 15 + 4, 64 * 3)
    assert _hip.absorb_grid_lds_form(2, 4 * 1025, 2048) == (8 * 4100 + 16 * 2048 + 4 * 2052 <= 65536)
    src = open(os.path.join(build.CSRC, "pcl_surface.hip")).read()
    assert "kGridAbsorbLdsCells = PCL_ABSORB_GRID_LDS_CELLS" in src and "kGridAbsorbLdsBytes = PCL_ABSORB_GRID_LDS_BYTES" in src


def test_the_counter_words_are_named_constants_used_once():
    src = open(os.path.join(build.CSRC, "pcl_surface.hip")).read()
    assert "constexpr uint32_t kGridAbsorbPath = 27, kGridAbsorbHit = 28;" in src
    for name in ("kGridAbsorbPath", "kGridAbsorbHit"):
        assert len(re.findall(r"pcl_philox4x32_10\([^;]*?, %s, " % name, src)) == 1 and len(re.findall(r"\b%s\b" % name, src)) == 2
    body = src[src.index("void __launch_bounds__(kBlock) k_absorb_grid"):src.index("struct gabsorb_spec")]
    assert body.index("if (!gone) continue;") > body.rindex("__ballot(") and "asm" not in body
    assert src.index("k_absorb_grid(gabsorb_args<T> a)") > src.index("k_phase_grid(gphase_args<T> a)")       # at the end of the unit
    for f in sorted(os.listdir(build.CSRC)):                            # nobody else draws from 27 or 28, by literal or by constant
        if f.endswith((".hip", ".h", ".inc")):
            text = open(os.path.join(build.CSRC, f)).read()
            words = [int(w) for w in re.findall(r"pcl_philox4x32_10\([^;]*?, (\d+)u, ", text)]
            words += [int(w) for k, w in re.findall(r"\b(k[A-Z]\w+) = (\d+)", text) if not k.startswith("kGridAbsorb")]
            assert 27 not in words and 28 not in words, f


# ------------------------------------------------------------------------------------------------ the binding and the refusals
def test_binding_marshals_the_call():
    def entry(handle, n_axes, coords, n_bins, ed, ce, B, Ee, p, om, seed, n_pass, counts, cells):
        dbl = lambda q, k: None if q is None else np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_double)), (k,)).tolist()   # noqa: E731
        i32 = lambda q, k: np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_int32)), (k,)).tolist()                          # noqa: E731
        bins = i32(n_bins, n_axes)
        n_p = int(np.prod(bins)) * max(B, 1)
        seen.append((handle, n_axes, i32(coords, n_axes), bins, dbl(ed, sum(bins) + n_axes), dbl(ce, 3), B, dbl(Ee, B + 1), dbl(p, n_p), dbl(om, n_p),
                     seed, n_pass))
        np.ctypeslib.as_array(ctypes.cast(counts, ctypes.POINTER(ctypes.c_int64)), (4,))[:] = [100, 50, 20, 10]
        np.ctypeslib.as_array(ctypes.cast(cells, ctypes.POINTER(ctypes.c_int64)), (n_p,))[:] = np.arange(n_p)
        return 0
    seen = []
    counts, cells = _hip._absorb_grid(entry, "h", [0.5, 0.25], None, ("z", "r"), [[0.0, 1.0], [1.0, 2.0]], CENTER, [1.0, 1.5, 3.0], -1, 2 ** 32 + 3)
    assert counts.tolist() == [100, 50, 20, 10] and cells.tolist() == [[[0, 1]]] and cells.dtype == counts.dtype == np.int64
    counts, cells = _hip._absorb_grid(entry, "h", None, np.arange(6) / 8.0, ("x", "y"), [[0.0, 1.0, 2.0], [0.0, 1.0, 2.0, 3.0]], None, None, 1, 1)
    assert cells.tolist() == [[0, 1, 2], [3, 4, 5]]
    assert seen[0] == ("h", 2, [2, 3], [1, 1], [0.0, 1.0, 1.0, 2.0], CENTER.tolist(), 2, [1.0, 1.5, 3.0], [0.5, 0.25], None, 2 ** 64 - 1, 3)
    assert seen[1][1:10] == (2, [0, 1], [2, 3], [0.0, 1.0, 2.0, 0.0, 1.0, 2.0, 3.0], None, 0, None, None, (np.arange(6) / 8.0).tolist())
    with pytest.raises(ValueError, match="omega0 holds 3 values"):
        _hip._absorb_grid(entry, "h", None, [0.5, 0.5, 0.5], ("x",), [[0.0, 1.0, 2.0]], None, None, 1, 1)
    with pytest.raises(ValueError, match="both None"):
        _hip._absorb_grid(entry, "h", None, None, ("x",), [[0.0, 1.0, 2.0]], None, None, 1, 1)
    with pytest.raises(ValueError, match="one sequence of edges per axis"):
        _hip._absorb_grid(entry, "h", [0.5], None, ("x", "y"), [[0.0, 1.0]], None, None, 1, 1)


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context and a NULL group, refused as well); the outputs stay as
    they were."""
    build.build_lib()
    lib = _hip.load()
    assert (GOOD_P == 0.0).any() and (GOOD_P == 1.0).any() and (GOOD_OM == 0.0).any() and (GOOD_OM == 1.0).any()
    for kw in BAD_CALLS:
        keep, args, (counts, cells) = abi_args(**kw)
        assert lib.pcl_step_absorb_grid(None, *args) == -2, kw
        assert lib.pcl_group_step_absorb_grid(None, *args) == -2, kw
        assert (counts is None or (counts == -7).all()) and (cells is None or (cells == -7).all()), kw
    for kw in ({}, dict(p=None), dict(omega0=None)):                    # a good call without a context is refused, too
        keep, args, (counts, cells) = abi_args(**kw)
        assert lib.pcl_step_absorb_grid(None, *args) == -2 and lib.pcl_group_step_absorb_grid(None, *args) != 0
        assert (counts == -7).all() and (cells == -7).all()


# ------------------------------------------------------------------------------------------------ untouched code
def git(*args):
    return subprocess.run(["git", "-c", "safe.directory=*", "-C", ROOT] + list(args), capture_output=True)


def test_every_older_kernel_is_the_code_it_was(tmp_path):
    """tools/compare_unit_asm.py between the newest commit whose pcl_surface.hip does not hold the sweep and this tree."""
    path = "physicl_amd/csrc/pcl_surface.hip"
    revs = git("rev-list", "HEAD", "--", path)
    if revs.returncode != 0 or not revs.stdout.split():
        pytest.skip("no git history to compare with")
    base = next((rev for rev in revs.stdout.decode().split() if b"k_absorb_grid" not in git("show", "%s:%s" % (rev, path)).stdout), None)
    assert base is not None, "no commit in front of the sweep"
    old = tmp_path / "old"
    old.mkdir()
    tar = subprocess.run(["git", "-c", "safe.directory=*", "-C", ROOT, "archive", base, "physicl_amd/csrc", "include"], capture_output=True, check=True)
    subprocess.run(["tar", "-x", "-C", str(old)], input=tar.stdout, check=True)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "compare_unit_asm.py"), str(old), ROOT], capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "DIFFERS" not in out.stdout and "k_absorb_grid<double, true>" in out.stdout and "k_scatter_grid<double, true>" in out.stdout


# ------------------------------------------------------------------------------------------------ the trip cases
def test_every_described_sweep_has_a_trip_case_that_exists():
    assert sorted(TRIP_CASES) == sorted(s["kernel"] for s in build.MORE)
    for kernel, (name, test) in TRIP_CASES.items():
        path = os.path.join(TESTS, name)
        assert name.startswith("test_") and os.path.isfile(path), (kernel, name)
        with open(path) as f:
            defined = {node.name for node in ast.parse(f.read()).body if isinstance(node, ast.FunctionDef)}
        assert test.startswith("test_") and test in defined, (kernel, name, test)
