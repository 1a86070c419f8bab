"""CPU: the sweeps the build describes behind its table of units (physicl_amd/build.py: ``LATER``) -- every check tests/test_build_cpu.py
applies per sweep of ``ADDONS``, applied to that table: the built library exports both entry points, the header declares them and
``_hip.EXPORTS`` lists them; the unit's device assembly, compiled once with the library's own options, holds a double and a float
instantiation with no scratch and no VGPR spills within the sweep's register budget; and no kernel's name holds another's.  And
tests/test_writer_trips_cpu.py's two checks on the table of past-one-trip cases of tests/test_writers_grid_phase_trips_gpu.py."""
import ast
import ctypes
import os
import re
import subprocess

import pytest

from physicl_amd import _hip, build
from test_build_cpu import FORMS
from test_writers_grid_phase_trips_gpu import TRIP_CASES

TESTS = os.path.dirname(os.path.abspath(__file__))
by_sweep = pytest.mark.parametrize("sweep", build.LATER, ids=[s["kernel"] for s in build.LATER])
# k_phase_layered's row of tests/test_build_cpu.py: six waves per SIMD or more
ASM = {"k_phase_grid": dict(vgprs=80)}


def test_the_table_describes_sweeps_of_the_units_there_are():
    older = [s for u in build.ADDONS for s in u["sweeps"]]
    assert [s["kernel"] for s in build.LATER] == list(ASM)
    for s in build.LATER:
        assert set(s) == {"entries", "kernel", "count", "src"} and s["src"] in [u["src"] for u in build.ADDONS], s
        assert len(s["entries"]) == 2 and s["entries"][1].startswith("pcl_group_") and s["kernel"].startswith("k_"), s
    every = older + build.LATER
    entries = [e for s in every for e in s["entries"]]
    assert len(set(entries)) == len(entries) == 2 * len(every)            # no entry point belongs to two sweeps
    # (a sweep's instantiations are found by the kernel's name inside the mangled one: no name holds another)
    assert not any(a is not b and a["kernel"] in b["kernel"] for a in every for b in every)


@by_sweep
def test_library_exports_both_entry_points_and_the_header_declares_them(sweep):
    build.build_lib()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert lib.pcl_abi_version() == 1
    text = re.sub(r"/\*.*?\*/", "", open(build.ABI_HEADER).read(), flags=re.S)
    for entry in sweep["entries"]:
        assert hasattr(lib, entry) and entry in _hip.EXPORTS and re.search(r"\b%s\s*\(" % entry, text), entry


def test_the_header_lists_the_new_kernel_among_the_users_of_its_counter_words():
    text = open(build.ABI_HEADER).read()
    assert re.search(r"pcl_step_phase_grid \(this call\) 10, 11 and 13", text) and "#define PCL_ABI_VERSION 1\n" in text


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


@by_sweep
def test_kernels_use_no_scratch(sweep, assembly):
    """From the unit's assembly: every instantiation of the sweep's kernel in its forms, nothing in scratch, no spills, its budget."""
    text, want = assembly(sweep["src"]), ASM[sweep["kernel"]]
    kernels = re.findall(r"\.name:\s+(_Z\w*%s\w*)\n(.*?)\.wavefront_size" % sweep["kernel"], text, re.S)
    assert len(kernels) == sweep["count"] == 2, [k for k, _ in kernels]
    form, forms = FORMS[sweep["count"]]
    assert sorted(re.search(sweep["kernel"] + form, k).groups() for k, _ in kernels) == forms == [("d",), ("f",)]
    for kernel, blk in kernels:
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))                                  # noqa: E731
        print(kernel, "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "sgpr spills", get("sgpr_spill_count"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, kernel
        assert get("vgpr_count") <= want["vgprs"], kernel


# ------------------------------------------------------------------------------------------------ the trip cases
def test_every_described_sweep_has_a_trip_case_and_no_other_kernel_is_named():
    assert sorted(TRIP_CASES) == sorted(s["kernel"] for s in build.LATER)


def test_every_named_test_exists_in_the_named_file():
    for kernel, (name, test) in TRIP_CASES.items():
        path = os.path.join(TESTS, name)
        assert name.startswith("test_") and os.path.isfile(path), (kernel, name)
        with open(path) as f:
            defined = {node.name for node in ast.parse(f.read()).body if isinstance(node, ast.FunctionDef)}
        assert test.startswith("test_") and test in defined, (kernel, name, test)
