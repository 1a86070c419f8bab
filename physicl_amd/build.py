"""Build libphysicl_hip.so (gfx950) in-tree with hipcc.  Used by __graft_entry__.build().

    python -m physicl_amd.build            # recompile the units that are older than their sources, link if anything is newer
    python -m physicl_amd.build --force    # recompile every unit
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "_lib")
LIB = os.path.join(LIBDIR, "libphysicl_hip.so")
OBJDIR = os.path.join(LIBDIR, "obj")


def _c(name):
    return os.path.join(CSRC, name)


ABI_HEADER = os.path.join(os.path.dirname(HERE), "include", "physicl_hip.h")
# what csrc_sha() covers: the device sources of the kernels bench.py prices
HASHED = [_c("physicl_hip.hip"), _c("pcl_device.h"), _c("pcl_sincos.h")]
# The library, one row per translation unit, in link order.  ``deps``: every file the unit includes, directly or not (a unit is
# recompiled when one of them is newer than its object; tests/test_build_cpu.py holds the list against the #include lines).
CORE = dict(src=_c("physicl_hip.hip"), deps=[_c("pcl_device.h"), _c("pcl_sincos.h"), ABI_HEADER, _c("pcl_rtc_source.inc")])
# The units on the public ABI beside it, one row per translation unit.  ``sweeps``: one element per sweep the unit holds, in
# the file's order -- ``entries``: the context's and the group's entry point; ``kernel``, ``count``: the kernel template and how
# many instantiations of it the unit's assembly holds.  A new unit is one more row, a new sweep in a unit one more element
# (tests/test_build_cpu.py checks every element alike).  Why a unit's sweeps stand together:
#   pcl_shell.hip    the crossing tallies: the aperture's image stands behind the shells'.
#   pcl_grid.hip     four instantiations, an LDS and a global form per dtype (as k_scatter_grid's).
#   pcl_surface.hip  the sweeps that write photons: they share their rules (pcl_rules.h), hit-point arithmetic and tables.
SWEEP = [_c("pcl_sweep.h"), ABI_HEADER]
DEVICE = SWEEP + [_c("pcl_device.h"), _c("pcl_sincos.h")]
RULES = DEVICE + [_c("pcl_rules.h")]          # the units that write photons share their rules


def _sweep(ctx_entry, group_entry, kernel, count=2):
    return dict(entries=(ctx_entry, group_entry), kernel=kernel, count=count)


ADDONS = [
    dict(src=_c("pcl_spectrum.hip"), deps=SWEEP, sweeps=(_sweep("pcl_step_plane_spectra", "pcl_group_step_plane_spectra", "k_plane_spectra"),)),
    dict(src=_c("pcl_source.hip"), deps=RULES, sweeps=(_sweep("pcl_store_apply_source", "pcl_group_apply_source", "k_apply_source"),)),
    dict(src=_c("pcl_shell.hip"), deps=SWEEP, sweeps=(
        _sweep("pcl_step_shell_crossings", "pcl_group_step_shell_crossings", "k_shell_crossings"),
        _sweep("pcl_step_detector_image", "pcl_group_step_detector_image", "k_detector_image"))),
    dict(src=_c("pcl_grid.hip"), deps=SWEEP, sweeps=(_sweep("pcl_step_position_grid", "pcl_group_step_position_grid", "k_position_grid", count=4),)),
    dict(src=_c("pcl_surface.hip"), deps=RULES, sweeps=(
        _sweep("pcl_step_surface_reflect", "pcl_group_step_surface_reflect", "k_surface_reflect"),
        _sweep("pcl_step_phase_redirect", "pcl_group_step_phase_redirect", "k_phase_redirect"),
        _sweep("pcl_step_absorb_scattered", "pcl_group_step_absorb_scattered", "k_absorb_scattered"),
        _sweep("pcl_step_phase_layered", "pcl_group_step_phase_layered", "k_phase_layered"),
        _sweep("pcl_step_recycle_spent", "pcl_group_step_recycle_spent", "k_recycle_spent"),
        _sweep("pcl_step_absorb_path", "pcl_group_step_absorb_path", "k_absorb_path"),
        _sweep("pcl_step_reemit_parked", "pcl_group_step_reemit_parked", "k_reemit_parked"),
        _sweep("pcl_step_refract_surface", "pcl_group_step_refract_surface", "k_refract_surface"),
        _sweep("pcl_step_ground_spectral", "pcl_group_step_ground_spectral", "k_ground_spectral"),
        _sweep("pcl_step_scatter_layered", "pcl_group_step_scatter_layered", "k_scatter_layered"),
        _sweep("pcl_step_scatter_grid", "pcl_group_step_scatter_grid", "k_scatter_grid", count=4),
        _sweep("pcl_step_box_walls", "pcl_group_step_box_walls", "k_box_walls"))),
]
UNITS = [CORE] + ADDONS
# Sweeps added to a unit since: a row has a sweep's shape plus ``src``, the unit that holds it (no new translation unit: the unit's row
# above compiles and links it).  tests/test_build_later_cpu.py checks every row as tests/test_build_cpu.py checks a sweep of ADDONS.
LATER = [
    dict(_sweep("pcl_step_phase_grid", "pcl_group_step_phase_grid", "k_phase_grid"), src=_c("pcl_surface.hip")),
]
# Sweeps added since, a row each, shaped as LATER's plus ``vgprs``, the row's own register budget: tests/test_grid_absorb_build_cpu.py
# reads every expectation from the row, so the next sweep is one more row here and no further table.
MORE = [
    # k_scatter_grid's budget (eight waves per SIMD): this kernel does less arithmetic than that one
    dict(_sweep("pcl_step_absorb_grid", "pcl_group_step_absorb_grid", "k_absorb_grid", count=4), src=_c("pcl_surface.hip"), vgprs=64),
]
# Sweeps added since, a row each, shaped as MORE's plus ``trip``: (test file, test name) of the case that takes the sweep past one trip
# of its grid and compares every tally, so the row names its own.  tests/test_plane_flux_build_cpu.py reads every expectation, the trip
# case included, from the row: the next sweep is one more row here, no further table and no further file to hold against.
ROWS = [
    # the shell unit's budget (eight waves per SIMD)
    dict(_sweep("pcl_step_plane_flux", "pcl_group_step_plane_flux", "k_plane_flux", count=4), src=_c("pcl_shell.hip"), vgprs=64,
         trip=("test_plane_flux_trips_gpu.py", "test_the_sweep_past_one_trip")),
]

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -ffp-contract=off: the reference's kernels must be evaluated unfused (bit-exact parity)
# -disable-machine-licm: the pre-RA pass hoists every scalar constant out of the kernels' long loops, the scalar register file
# overflows and the overflow comes back as v_readlane inside the loops -- VALU work in kernels bound by VALU issue.  Without
# it: 8500 -> 5676 spilled SGPRs over the library, k_mixed<double> +10 %, nothing slower (profiles/r05_ab_machine_licm.md).
# The hipRTC specialisations are compiled with the same options (physicl_hip.hip: get_rtc).
EXTRA_OPTS = ["-mllvm", "-disable-machine-licm"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared",
         "-Wall", "-Wno-unused-variable", "-Wno-unused-function"] + EXTRA_OPTS


def _generate_rtc_source():
    """Embed pcl_device.h as a string so hipRTC can specialise it for a variable_n_fn expression."""
    text = open(os.path.join(CSRC, "pcl_device.h")).read()
    inc = [ln for ln in text.splitlines() if ln.startswith('#include "pcl_sincos.h"')]
    assert len(inc) == 1
    text = text.replace(inc[0], open(os.path.join(CSRC, "pcl_sincos.h")).read())   # hipRTC sees one self-contained text
    delim = "PCLRTC"
    assert (")" + delim + '"') not in text
    out = os.path.join(CSRC, "pcl_rtc_source.inc")
    body = "// GENERATED by physicl_amd/build.py from pcl_device.h -- do not edit\n" \
           "static const char pcl_rtc_source[] = R\"%s(%s)%s\";\n" % (delim, text, delim)
    if not os.path.exists(out) or open(out).read() != body:
        with open(out, "w") as f:
            f.write(body)
    return out


def csrc_sha():
    """sha256 (16 hex digits) over the device sources every kernel of the library -- ahead-of-time and hipRTC -- is compiled
    from, and the code-generation options.  Counter records measured under rocprofv3 (profiles/pmc_traffic.json) carry the value they were measured at:
    bench.py only quotes a record whose value is still this one (tests/test_profiles_fresh_cpu.py).  The hash covers the kernels
    bench.py prices (HASHED), not ADDONS: those units are built on the public ABI beside them and change none of their code."""
    import hashlib
    h = hashlib.sha256()
    for path in HASHED:
        h.update(open(path, "rb").read())
    h.update(" ".join(EXTRA_OPTS).encode())          # code-generation options change the instruction counts too
    return h.hexdigest()[:16]


def _older(out, unit):
    """Is ``out`` missing, or older than the unit's source, one of its declared dependencies or this file?"""
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(not os.path.exists(p) or os.path.getmtime(p) > t for p in [unit["src"]] + unit["deps"] + [__file__])


def _obj(unit):
    return os.path.join(OBJDIR, os.path.splitext(os.path.basename(unit["src"]))[0] + ".o")


def needs_build():
    return any(_older(LIB, u) for u in UNITS)


def build_lib(force=False, verbose=False):
    if not force and not needs_build():
        return LIB
    os.makedirs(OBJDIR, exist_ok=True)
    _generate_rtc_source()

    def run(cmd):
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    stale = [u for u in UNITS if force or _older(_obj(u), u)]
    if stale:
        with ThreadPoolExecutor(min(len(stale), int(os.environ.get("MAX_JOBS", "8")))) as pool:
            list(pool.map(lambda u: run([HIPCC] + [f for f in FLAGS if f != "-shared"] + ["-c", u["src"], "-o", _obj(u)]), stale))
    tmp = LIB + ".tmp"                               # a failing link leaves the library that was there
    run([HIPCC] + FLAGS + [_obj(u) for u in UNITS] + ["-o", tmp, "-ldl"])        # libhiprtc is dlopen'ed at run time, not linked
    os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv, verbose=True))
