"""CPU: the sweeps of the build's fourth table (physicl_amd/build.py: ``ROWS``) -- what tests/test_grid_absorb_build_cpu.py checks per
row of ``MORE``, with every expectation read from the row itself (entries, kernel, count, src, vgprs, trip): the built library exports
both entry points, the header declares them and ``_hip.EXPORTS`` lists them; the unit's device assembly, compiled once with the
library's own options, holds the row's instantiations in its forms with no scratch and no VGPR spills within the row's budget; the
row's own past-one-trip test exists.  The next sweep is one more row; this file asserts only that ``k_plane_flux`` is among them.

And for pcl_step_plane_flux: the header's sentences and limits and their mirror in ``_hip``, the LDS formula on both sides of its
boundary, the binding's marshalling and the refusals that need no device."""
import ast
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from physicl_amd import _hip, build
from test_build_cpu import FORMS

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
ENTRIES = ("pcl_step_plane_flux", "pcl_group_step_plane_flux")
NAN, INF = float("nan"), float("inf")
by_row = pytest.mark.parametrize("row", build.ROWS, ids=[s["kernel"] for s in build.ROWS])


def test_the_table_describes_sweeps_of_the_units_there_are():
    assert "k_plane_flux" in [s["kernel"] for s in build.ROWS]
    older = [s for u in build.ADDONS for s in u["sweeps"]] + build.LATER + build.MORE
    for s in build.ROWS:
        assert set(s) == {"entries", "kernel", "count", "src", "vgprs", "trip"} and s["src"] in [u["src"] for u in build.ADDONS], s
        assert len(s["entries"]) == 2 and s["entries"][1].startswith("pcl_group_") and s["kernel"].startswith("k_"), s
        assert s["count"] in FORMS and isinstance(s["vgprs"], int) and 0 < s["vgprs"] <= 512, s
    every = older + build.ROWS
    entries = [e for s in every for e in s["entries"]]
    assert len(set(entries)) == len(entries) == 2 * len(every)            # no entry point belongs to two sweeps
    assert not any(a is not b and a["kernel"] in b["kernel"] for a in every for b in every)
    (row,) = [s for s in build.ROWS if s["kernel"] == "k_plane_flux"]
    assert row["entries"] == ENTRIES and row["count"] == 4 and os.path.basename(row["src"]) == "pcl_shell.hip" and row["vgprs"] == 64
    assert build.csrc_sha() == "b54e0443ee3f400f"                       # the tuned core has not moved
    assert len(build.UNITS) == 6                                          # no new translation unit


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


@by_row
def test_the_row_s_trip_case_exists(row):
    name, test = row["trip"]
    path = os.path.join(TESTS, name)
    assert name.startswith("test_") and name.endswith("_gpu.py") and os.path.isfile(path), row
    with open(path) as f:
        text = f.read()
    defined = {node.name for node in ast.parse(text).body if isinstance(node, ast.FunctionDef)}
    assert test.startswith("test_") and test in defined, row
    assert "pytestmark = pytest.mark.gpu" in text and "has_work(" in text and "slots(cap, size)" in text, row


# ------------------------------------------------------------------------------------------------ the header and its mirror
def test_the_header_states_the_rule_and_the_limits():
    text = open(build.ABI_HEADER).read()
    flat = " ".join(text.split()).replace("* ", "")
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "#define PCL_ABI_VERSION 1\n" in text
    for line in ("0 gives (y, z), 1 gives (x, z), 2 gives (x, y)", "now = r_a; m = dr_a; prev = now - m;",
                 "up iff prev < X and now >= X; down iff prev >= X and now < X", "on the plane is above; a NaN crosses nothing",
                 "Every change of side is counted exactly once", "cumsum(up - down) per level is the change of the population at or above it",
                 "every particle that crossed, photon or not", "G = |X - prev|; D = |m|;", "p_t = r_t - dr_t; H_t = p_t*D + dr_t*G",
                 "bin b of t iff e_b*D <= H_t < e_(b+1)*D, the last bin closed", "Rounded products are monotone in b",
                 "in no cell iff D or an H_t is not finite, or H_t lies outside [e_0*D, e_n*D] on either axis",
                 "No division and no square root is taken anywhere", "it is tallied at each of them, with that level's G",
                 "maps_out_host[dir][s][band][iu][iv] += 1", "is counted and lands in no cell",
                 "C <= PCL_PLANE_FLUX_LDS_CELLS and 8 * (S + n_u + 1 + n_v + 1 + (B ? B + 1 : 0)) + 4 * (2 S + C) <= PCL_PLANE_FLUX_LDS_BYTES",
                 "it was not tuned for this sweep", "an empty store answers zeros without a launch", "with the outputs untouched"):
        assert line.replace("* ", "") in flat, line
    for name, value in (("MAX_LEVELS", "16"), ("MAX_BINS", "1024"), ("MAX_BANDS", "1024"), ("MAX_CELLS", r"\(1 << 20\)"), ("LDS_CELLS", "4096"),
                        ("LDS_BYTES", "65536")):
        assert re.search(r"#define PCL_PLANE_FLUX_%s %s" % (name, value), code), name
    assert (_hip.PLANE_FLUX_MAX_LEVELS, _hip.PLANE_FLUX_MAX_BINS, _hip.PLANE_FLUX_MAX_BANDS, _hip.PLANE_FLUX_MAX_CELLS, _hip.PLANE_FLUX_LDS_CELLS,
            _hip.PLANE_FLUX_LDS_BYTES) == (16, 1024, 1024, 1 << 20, 4096, 65536)
    assert _hip.PLANE_FLUX_AXES == {"x": 0, "y": 1, "z": 2}
    for entry in ENTRIES:
        assert len(_hip._PROTOTYPES[entry]) == 12
    from physicl_amd.multidev import MultiDevice
    assert all(hasattr(c, "plane_flux") for c in (_hip.Device, _hip.DeviceGroup, MultiDevice))


def test_the_lds_formula_is_mirrored_on_both_sides_of_its_boundary():
    assert _hip.plane_flux_lds_bytes(16, 8, 16, 0, 4096) == 8 * (16 + 9 + 17) + 4 * (32 + 4096) == 16848
    assert _hip.plane_flux_lds_bytes(3, 7, 5, 3, 630) == 8 * (3 + 8 + 6 + 4) + 4 * (6 + 630)
    assert _hip.plane_flux_lds_form(16, 8, 16, 0) and not _hip.plane_flux_lds_form(16, 8, 17, 0)            # 4096 cells, 4352 cells
    assert _hip.plane_flux_lds_form(2, 1024, 1, 0) and not _hip.plane_flux_lds_form(2, 1024, 1, 2)          # 4096 cells, 8192 with two bands
    assert _hip.plane_flux_lds_form(1, 2, 2, 512) and not _hip.plane_flux_lds_form(1, 2, 2, 513)            # the bands count
    # The byte bound: within the argument limits the cell bound is the tighter one -- the largest LDS form asks for 16 levels, three
    # tables of 1025 edges and fewer than 4096 + 32 tallies, 41 KiB -- so no call the entry point accepts fails the bytes alone.  The
    # formula stands for a later change of either limit, and its own boundary is checked on the numbers:
    assert max(_hip.plane_flux_lds_bytes(16, 1024, 1024, 1024, 4096), 8 * (16 + 3 * 1025) + 4 * (32 + 4096)) == 41240 < _hip.PLANE_FLUX_LDS_BYTES
    assert _hip.plane_flux_lds_bytes(0, 0, 0, 0, 16380) == 65536 and _hip.plane_flux_lds_bytes(0, 0, 0, 0, 16381) > _hip.PLANE_FLUX_LDS_BYTES
    src = open(os.path.join(build.CSRC, "pcl_shell.hip")).read()
    assert "kPlaneFluxLdsCells = PCL_PLANE_FLUX_LDS_CELLS" in src and "kPlaneFluxLdsBytes = PCL_PLANE_FLUX_LDS_BYTES" in src
    assert "n_map() <= (size_t)kPlaneFluxLdsCells && lds_whole() <= kPlaneFluxLdsBytes" in src


def test_the_kernel_stands_at_the_end_of_the_unit_with_its_ballots_at_the_head():
    src = open(os.path.join(build.CSRC, "pcl_shell.hip")).read()
    assert src.index("k_plane_flux(pflux_args<T> a)") > src.index("k_detector_image(detector_args<T> a)") > src.index("k_shell_crossings(shell_args<T> a)")
    body = src[src.index("void __launch_bounds__(kBlock) k_plane_flux"):src.index("struct pflux_spec")]
    assert body.index("if (!crossed) continue;") > body.rindex("__ballot(") and "asm" not in body
    assert body.index("a.rt[0][ti]") > body.index("if (!crossed) continue;") > body.index("a.dra[ti]")      # the transverse loads are deferred
    assert " / " not in re.sub(r"//.*", "", body).replace("/ 64 * 64", "") and "sqrt" not in body           # no division, no square root
    assert "flush_cells(s_cnt, a.out, n_cnt)" in body and "bin_of(s_u, nu, Hu, D)" in body


# ------------------------------------------------------------------------------------------------ the binding and the refusals
def test_binding_marshals_the_call():
    def entry(handle, axis, S, lv, ue, nu, ve, nv, Ee, nE, counts, maps):
        dbl = lambda q, k: None if q is None else np.ctypeslib.as_array(ctypes.cast(q, ctypes.POINTER(ctypes.c_double)), (k,)).tolist()   # noqa: E731
        seen.append((handle, axis, S, dbl(lv, S), dbl(ue, nu + 1), nu, dbl(ve, nv + 1), nv, dbl(Ee, nE + 1), nE))
        n = 2 * S * max(nE, 1) * nu * nv
        np.ctypeslib.as_array(ctypes.cast(counts, ctypes.POINTER(ctypes.c_int64)), (2 * S,))[:] = 100 + np.arange(2 * S)
        np.ctypeslib.as_array(ctypes.cast(maps, ctypes.POINTER(ctypes.c_int64)), (n,))[:] = np.arange(n)
        return 0
    seen = []
    counts, maps = _hip._plane_flux(entry, "h", "y", [0, 1], [[0, 1, 2], (0.0, 1.0, 2.0, 4.0)], [1, 2, 4])
    assert seen[0] == ("h", 1, 2, [0.0, 1.0], [0.0, 1.0, 2.0], 2, [0.0, 1.0, 2.0, 4.0], 3, [1.0, 2.0, 4.0], 2)
    assert counts.dtype == maps.dtype == np.int64 and counts.tolist() == [[100, 101], [102, 103]]
    assert maps.shape == (2, 2, 2, 2, 3) and maps.reshape(-1).tolist() == list(range(48))                   # C order: dir, level, band, u, v
    counts, maps = _hip._plane_flux(entry, "h", 2, [0.5], [[0, 1], [0, 1]])
    assert seen[1] == ("h", 2, 1, [0.5], [0.0, 1.0], 1, [0.0, 1.0], 1, None, 0) and maps.shape == (2, 1, 1, 1, 1)   # no bands: NULL and 0
    with pytest.raises(ValueError, match="two sequences of edges"):
        _hip._plane_flux(entry, "h", "z", [0.5], [[0, 1]])

    class Lib:
        pcl_step_plane_flux = staticmethod(lambda *a: entry(*a))
        pcl_group_step_plane_flux = staticmethod(lambda *a: entry(*a))
    for cls, handle in ((_hip.Device, "ctx"), (_hip.DeviceGroup, "g")):
        d = cls.__new__(cls)
        d.lib = Lib
        setattr(d, handle, handle)
        d.plane_flux("x", [1.0], [[0, 1], [0, 2]], E_edges=[1, 2])
        assert seen[-1] == (handle, 0, 1, [1.0], [0.0, 1.0], 1, [0.0, 2.0], 1, [1.0, 2.0], 1)


def abi_args(**kw):
    """(what must stay alive, the arguments behind the handle, (counts, maps)) of a call; ``kw`` replaces arguments, None: NULL."""
    a = dict(axis=2, S=2, levels=np.array([0.0, 1.0]), u_edges=np.array([-1.0, 0.0, 1.0]), nu=2, v_edges=np.array([-1.0, 1.0]), nv=1,
             E_edges=np.array([1.0, 2.0, 3.0]), nE=2, counts=np.full(4, -7, np.int64), maps=np.full(16, -7, np.int64))
    a.update(kw)
    p = lambda x: None if x is None else x.ctypes.data      # noqa: E731
    args = (a["axis"], a["S"], p(a["levels"]), p(a["u_edges"]), a["nu"], p(a["v_edges"]), a["nv"], p(a["E_edges"]), a["nE"], p(a["counts"]), p(a["maps"]))
    return a, args, (a["counts"], a["maps"])


BAD_CALLS = [
    dict(levels=None), dict(u_edges=None), dict(v_edges=None), dict(E_edges=None), dict(counts=None), dict(maps=None),
    dict(axis=-1), dict(axis=3), dict(S=0), dict(S=-1), dict(S=17, levels=np.arange(17.0)),
    dict(levels=np.array([0.0, NAN])), dict(levels=np.array([0.0, INF])), dict(levels=np.array([1.0, 1.0])), dict(levels=np.array([1.0, 0.0])),
    dict(u_edges=np.array([0.0, 0.0, 1.0])), dict(u_edges=np.array([0.0, NAN, 1.0])), dict(u_edges=np.array([0.0, 1.0, INF])), dict(u_edges=np.array([0.0, 1.0, 0.5])),
    dict(v_edges=np.array([1.0, 1.0])), dict(v_edges=np.array([NAN, 1.0])), dict(v_edges=np.array([1.0, -1.0])),
    dict(E_edges=np.array([1.0, 1.0, 2.0])), dict(E_edges=np.array([1.0, NAN, 2.0])), dict(E_edges=np.array([1.0, 2.0, INF])),
    dict(nu=0), dict(nu=-1), dict(nu=1025, u_edges=np.linspace(-1, 1, 1026)), dict(nv=0), dict(nv=1025, v_edges=np.linspace(-1, 1, 1026)),
    dict(nE=-1), dict(nE=1025, E_edges=np.linspace(1, 2, 1026)),
    dict(nu=1024, u_edges=np.linspace(-1, 1, 1025), nv=1024, v_edges=np.linspace(-1, 1, 1025), nE=0),       # 2 x 2 x 1024 x 1024 cells
    dict(S=1, nu=1024, u_edges=np.linspace(-1, 1, 1025), nv=512, v_edges=np.linspace(-1, 1, 513), nE=2),    # 2 x 1 x 2 x 1024 x 512: one band too many
]


def test_refused_calls_need_no_device():
    """PCL_ERR_ARG comes before the store is looked at (here: a NULL context and a NULL group, refused as well); the outputs stay as
    they were."""
    build.build_lib()
    lib = _hip.load()
    assert all(hasattr(lib, e) for e in ENTRIES) and lib.pcl_abi_version() == 1
    for kw in BAD_CALLS:
        keep, args, (counts, maps) = abi_args(**kw)
        assert lib.pcl_step_plane_flux(None, *args) == -2, kw
        assert lib.pcl_group_step_plane_flux(None, *args) == -2, kw
        assert (counts is None or (counts == -7).all()) and (maps is None or (maps == -7).all()), kw
    for kw in ({}, dict(E_edges=None, nE=0)):                           # a good call without a context is refused, too
        keep, args, (counts, maps) = abi_args(**kw)
        assert lib.pcl_step_plane_flux(None, *args) == -2 and lib.pcl_group_step_plane_flux(None, *args) != 0
        assert (counts == -7).all() and (maps == -7).all()
