"""CPU: the build (physicl_amd/build.py) -- its table of units, what is rebuilt when, and what every add-on unit's compile gives.

* the table: which units exist, their link order, what csrc_sha() covers (none of the add-on units), every path exists and
  every ``#include "..."`` of a unit is one of its declared dependencies;
* ``needs_build()`` and ``build_lib()`` against modification times, with no compiler run: a library newer than everything
  is left alone, one newer file recompiles the units that depend on it and no other, and the library is linked once;
* per sweep of every add-on unit: the built library exports both entry points, ``_hip`` and the header know them, and the
  unit's device assembly, compiled once with the library's own options, holds the sweep's instantiations with no scratch and
  no spills, within the sweep's register budget.
"""
import ctypes
import os
import re
import subprocess

import pytest

from physicl_amd import _hip, build

CORE_FILES = ["physicl_hip.hip", "pcl_device.h", "pcl_sincos.h"]
ORDER = ["physicl_hip.hip", "pcl_spectrum.hip", "pcl_source.hip", "pcl_shell.hip", "pcl_grid.hip", "pcl_surface.hip"]
PER_UNIT = {"pcl_spectrum.hip": 1, "pcl_source.hip": 1, "pcl_shell.hip": 2, "pcl_grid.hip": 1, "pcl_surface.hip": 12}     # sweeps
SWEEP_H = os.path.join(build.CSRC, "pcl_sweep.h")
name = os.path.basename
names = lambda paths: [name(p) for p in paths]                                                              # noqa: E731
by_name = lambda rows: pytest.mark.parametrize("unit", rows, ids=[name(u["src"]) for u in rows])            # noqa: E731
SWEEPS = [(u, s) for u in build.ADDONS for s in u["sweeps"]]
by_sweep = pytest.mark.parametrize("unit,sweep", SWEEPS, ids=["%s-%s" % (name(u["src"]), s["kernel"]) for u, s in SWEEPS])
# What a sweep's kernels must show beyond the instantiations without scratch or VGPR spills: no SGPR spills, a VGPR count
# (64: eight waves per SIMD -- the shell unit's, where occupancy is left to LDS, and the surface unit's later sweeps; 80: six waves
# per SIMD or more), and instructions in the unit's assembly.  One row per sweep of the table, in the table's order.
ASM = {
    "k_plane_spectra": {},
    "k_apply_source": dict(no_sgpr_spills=True, has=["v_fma_f64"]),          # (the sincos' explicit FMAs; everything else is unfused)
    "k_shell_crossings": dict(no_sgpr_spills=True, vgprs=64),
    "k_detector_image": dict(no_sgpr_spills=True, vgprs=64),
    # 64-bit adds on the device grid, 32-bit ones in LDS; q is unfused, and no square root anywhere
    "k_position_grid": dict(no_sgpr_spills=True, has=["global_atomic_add_x2", "ds_add_u32"], lacks=["v_fma_f64", "v_sqrt"]),
    "k_surface_reflect": dict(vgprs=80),
    "k_phase_redirect": dict(vgprs=80),
    "k_absorb_scattered": dict(vgprs=80),
    "k_phase_layered": dict(vgprs=80),
    "k_recycle_spent": dict(vgprs=80),
    "k_absorb_path": dict(vgprs=80),
    "k_reemit_parked": dict(vgprs=80),
    "k_refract_surface": dict(vgprs=80),
    "k_ground_spectral": dict(vgprs=80),
    "k_scatter_layered": dict(vgprs=64),
    "k_scatter_grid": dict(vgprs=64),
    "k_box_walls": dict(vgprs=64),
}
# The forms a kernel template is instantiated in, by their number: what follows the kernel's name in the mangled one, and the sorted
# matches -- a float and a double form; an LDS and a global form of each, as the position grid's and the grid scatter's.
FORMS = {2: (r"I([df])E", [("d",), ("f",)]), 4: (r"I([df])Lb([01])E", [("d", "0"), ("d", "1"), ("f", "0"), ("f", "1")])}


# ------------------------------------------------------------------------------------------------ the table
def test_source_hash_of_the_priced_kernels_has_not_moved():
    assert build.csrc_sha() == "b54e0443ee3f400f"
    assert names(build.HASHED) == CORE_FILES
    assert not set(build.HASHED) & ({u["src"] for u in build.ADDONS} | {SWEEP_H})
    assert set(build.HASHED) <= {build.CORE["src"]} | set(build.CORE["deps"])


def test_units_and_their_link_order():
    assert names(u["src"] for u in build.UNITS) == ORDER               # each unit once, the core first
    assert build.UNITS[0] is build.CORE and build.UNITS[1:] == build.ADDONS
    assert names(build.CORE["deps"]) == ["pcl_device.h", "pcl_sincos.h", "physicl_hip.h", "pcl_rtc_source.inc"]
    assert SWEEP_H not in build.CORE["deps"] and SWEEP_H not in [u["src"] for u in build.UNITS]
    for u in build.ADDONS:
        assert SWEEP_H in u["deps"] and build.ABI_HEADER in u["deps"], u["src"]
        assert set(u) == {"src", "deps", "sweeps"} and len(u["sweeps"]) == PER_UNIT[name(u["src"])]
        for s in u["sweeps"]:
            assert len(s["entries"]) == 2 and s["entries"][1].startswith("pcl_group_") and s["kernel"].startswith("k_"), s
    entries = [e for _, s in SWEEPS for e in s["entries"]]
    assert len(SWEEPS) == 17 and len(set(entries)) == len(entries) == 34          # no entry point belongs to two sweeps
    # (a sweep's instantiations are found by the kernel's name inside the mangled one: no name holds another)
    assert not any(a is not b and a["kernel"] in b["kernel"] for _, a in SWEEPS for _, b in SWEEPS)
    assert [s["kernel"] for _, s in SWEEPS] == list(ASM) and all(os.path.isfile(p) for p in table_files())


@by_name(build.UNITS)
def test_every_include_is_a_declared_dependency(unit):
    """Of the unit and of the headers it declares: the modification times of the declared files are all a rebuild looks at."""
    for path in [unit["src"]] + [d for d in unit["deps"] if not d.endswith(".inc")]:      # (the generated text includes nothing)
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(path).read(), re.M):
            assert os.path.normpath(os.path.join(os.path.dirname(path), inc)) in unit["deps"], (path, inc)


# ------------------------------------------------------------------------------------------------ what is rebuilt when
def table_files():
    build._generate_rtc_source()
    return sorted({p for u in build.UNITS for p in [u["src"]] + u["deps"]})


def touch(monkeypatch, path):
    monkeypatch.setattr(os.path, "getmtime", lambda p, real=os.path.getmtime: real(p) + (1e6 if p == path else 0))


@pytest.fixture
def built(tmp_path, monkeypatch):
    """A library and objects in tmp_path, newer than every file of the table (``touch`` makes one file newer than
    both).  Gives the list the command lines are collected in: no compiler runs."""
    newest = max(os.path.getmtime(p) for p in table_files() + [build.__file__])
    monkeypatch.setattr(build, "LIB", str(tmp_path / "lib.so"))
    monkeypatch.setattr(build, "OBJDIR", str(tmp_path / "obj"))
    os.makedirs(build.OBJDIR)
    for path, age in [(build._obj(u), 10) for u in build.UNITS] + [(build.LIB, 20)]:
        open(path, "w").write("before")
        os.utime(path, (newest + age, newest + age))
    lines = []

    def check_call(cmd, **kw):
        lines.append(cmd)
        open(cmd[cmd.index("-o") + 1], "w").write("after")
    monkeypatch.setattr(subprocess, "check_call", check_call)
    return lines


def compiled(lines):
    """The units the collected lines compile, after a look at the lines: compiles with FLAGS less -shared, then one link."""
    *compiles, link = lines
    objs = [build._obj(u) for u in build.UNITS]
    assert link == [build.HIPCC] + build.FLAGS + objs + ["-o", build.LIB + ".tmp", "-ldl"] and "-shared" in link
    for cmd in compiles:
        assert cmd[:-4] == [build.HIPCC] + [f for f in build.FLAGS if f != "-shared"] and cmd[-4] == "-c" and cmd[-2] == "-o"
        assert cmd[-1] == objs[names(u["src"] for u in build.UNITS).index(name(cmd[-3]))]
    assert open(build.LIB).read() == "after" and not os.path.exists(build.LIB + ".tmp")
    return sorted(name(cmd[-3]) for cmd in compiles)


NEWER = [(u, [u]) for u in ORDER] + [("pcl_sweep.h", ORDER[1:]), ("physicl_hip.h", ORDER), ("pcl_rtc_source.inc", ORDER[:1]),
                                     ("pcl_device.h", ["pcl_source.hip", "pcl_surface.hip", "physicl_hip.hip"])]


@pytest.mark.parametrize("newer,users", NEWER, ids=[n for n, _ in NEWER])
def test_a_newer_file_recompiles_the_units_that_depend_on_it_and_no_other(built, monkeypatch, newer, users):
    (path,) = [p for p in table_files() if name(p) == newer]
    assert not build.needs_build()
    assert build.build_lib() == build.LIB and built == []             # nothing touched: no hipcc at all
    touch(monkeypatch, path)
    assert build.needs_build()                                         # that file alone newer than the library
    build.build_lib()
    assert compiled(built) == sorted(users)


def test_a_missing_library_a_newer_build_py_and_force(built, monkeypatch):
    os.remove(build.LIB)
    assert build.needs_build()
    build.build_lib()
    assert compiled(built) == []                                       # the objects are fresh: linked only
    del built[:]
    build.build_lib(force=True)
    assert compiled(built) == sorted(ORDER)
    del built[:]
    touch(monkeypatch, build.__file__)
    assert build.needs_build()
    build.build_lib()
    assert compiled(built) == sorted(ORDER)


def test_a_failing_compile_leaves_the_library_that_was_there(built, monkeypatch):
    def check_call(cmd, **kw):
        raise subprocess.CalledProcessError(1, cmd)
    monkeypatch.setattr(subprocess, "check_call", check_call)
    touch(monkeypatch, build.ADDONS[-1]["src"])
    with pytest.raises(subprocess.CalledProcessError):
        build.build_lib()
    assert open(build.LIB).read() == "before" and not os.path.exists(build.LIB + ".tmp")


# ------------------------------------------------------------------------------------------------ per sweep of an add-on unit
@by_sweep
def test_library_exports_both_entry_points_and_the_header_declares_them(unit, sweep):
    build.build_lib()
    lib = ctypes.CDLL(_hip.LIB_PATH)
    assert lib.pcl_abi_version() == 1
    text = re.sub(r"/\*.*?\*/", "", open(build.ABI_HEADER).read(), flags=re.S)
    for entry in sweep["entries"]:
        assert hasattr(lib, entry) and entry in _hip.EXPORTS and re.search(r"\b%s\s*\(" % entry, text), entry


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    """unit -> its device assembly, compiled with the library's own options; each unit is compiled once for the module."""
    texts = {}

    def get(unit):
        src = unit["src"]
        if src not in texts:
            out = str(tmp_path_factory.mktemp("asm") / "unit.s")
            subprocess.check_call([build.HIPCC] + [f for f in build.FLAGS if f not in ("-shared", "-fPIC")] +
                                  ["--cuda-device-only", "-S", "-o", out, src], stderr=subprocess.DEVNULL)
            print("compiled", name(src))
            texts[src] = open(out).read()
        return texts[src]
    return get


@by_sweep
def test_kernels_use_no_scratch(unit, sweep, assembly):
    """From the unit's assembly: every instantiation of the sweep's kernel in its forms, nothing in scratch, no spills, its budget."""
    text, want = assembly(unit), ASM[sweep["kernel"]]
    kernels = re.findall(r"\.name:\s+(_Z\w*%s\w*)\n(.*?)\.wavefront_size" % sweep["kernel"], text, re.S)
    assert len(kernels) == sweep["count"], [k for k, _ in kernels]
    form, forms = FORMS[sweep["count"]]
    assert sorted(re.search(sweep["kernel"] + form, k).groups() for k, _ in kernels) == forms
    for kernel, blk in kernels:
        get = lambda k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1))                                  # noqa: E731
        print(kernel, "vgprs", get("vgpr_count"), "sgprs", get("sgpr_count"), "sgpr spills", get("sgpr_spill_count"))
        assert get("private_segment_fixed_size") == 0 and get("vgpr_spill_count") == 0, kernel
        assert get("sgpr_spill_count") == 0 or not want.get("no_sgpr_spills"), kernel
        assert "vgprs" not in want or get("vgpr_count") <= want["vgprs"], kernel
    assert all(word in text for word in want.get("has", [])) and not any(word in text for word in want.get("lacks", []))
