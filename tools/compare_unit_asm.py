#!/usr/bin/env python3
"""Is the device code of the add-on units (physicl_amd/build.py: ADDONS) in two source trees the same code?
For a refactor of their host side, of pcl_sweep.h or of the build, in place of a speed measurement:

    python tools/compare_unit_asm.py <old tree> <new tree> [--md]

Each tree's units are its own: every ``*.hip`` of its physicl_amd/csrc but the core, so two trees whose build tables differ
can be compared.  Each is compiled to gfx950 assembly with this tree's options (physicl_amd/build.py: FLAGS without
-shared / -fPIC, plus --cuda-device-only -S, as tests/test_build_cpu.py does).  The kernels of a tree are pooled by mangled
name, so one that moved between units is compared with itself.  Per kernel the register and segment metadata must be equal and
the instruction lines must be the same multiset (the scheduler may swap neighbours when a helper moves into a header, so not
the same sequence).  A kernel that only the new tree has is listed as new with its metadata (a unit that gained a sweep: the
kernels it had must still be the code they were) and must be a sweep this tree's build describes (``build.ADDONS``, ``build.LATER``,
``build.MORE``, ``build.ROWS``); one
that only the old tree has counts as a difference.  Exit status 1 if any kernel differs or a new one is not described.
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from physicl_amd import build  # noqa: E402

CORE = os.path.basename(build.CORE["src"])
DESCRIBED = [s["kernel"] for u in build.ADDONS for s in u["sweeps"]] + [s["kernel"] for s in build.LATER + build.MORE + build.ROWS]  # every sweep this tree's build describes
META = ["vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"]


def units(tree):
    return sorted(f for f in os.listdir(os.path.join(tree, "physicl_amd", "csrc")) if f.endswith(".hip") and f != CORE)


def compile_unit(tree, unit, out):
    src = os.path.join(tree, "physicl_amd", "csrc", unit)
    subprocess.check_call([build.HIPCC] + [f for f in build.FLAGS if f not in ("-shared", "-fPIC")] +
                          ["--cuda-device-only", "-S", "-o", out, src], stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(asm):
    """{kernel: (metadata, Counter of instruction lines)} of one unit's assembly"""
    out = {}
    lines = asm.splitlines()
    # a kernel's metadata keys are sorted: .group_segment_fixed_size stands before its .name, the others behind it
    for m in re.finditer(r"\.(group_segment_fixed_size:\s+\d+)\n(?:(?!\.group_segment_fixed_size).)*?\.name:\s+(_Z\w+)\n(.*?)\.wavefront_size", asm, re.S):
        name, blk = m.group(2), "." + m.group(1) + "\n" + m.group(3)
        meta = {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in META}
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        ins = [t.split(";")[0].strip() for t in (ln.strip() for ln in lines[start + 1:end]) if t and t[0] not in ";."]
        out[name] = (meta, collections.Counter(ins))
    return out


def pooled(by_unit):
    """{kernel: (unit, metadata, Counter)} over a tree's units; a kernel's mangled name stands in one unit only."""
    out = {}
    for unit, found in sorted(by_unit.items()):
        for name, (meta, ins) in found.items():
            assert name not in out, "%s is in %s and in %s" % (name, out[name][0], unit)
            out[name] = (unit, meta, ins)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--md", action="store_true", help="print a markdown table")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(prefix="pcl_cmp_") as work, ThreadPoolExecutor(max_workers=8) as pool:
        jobs = {side: {u: pool.submit(compile_unit, tree, u, os.path.join(work, "%s_%s.s" % (side, u))) for u in units(tree)}
                for side, tree in (("old", a.old), ("new", a.new))}
        old, new = (pooled({u: kernels(j.result()) for u, j in jobs[side].items()}) for side in ("old", "new"))
    dem = lambda n: subprocess.run(["c++filt", n], capture_output=True, text=True).stdout.strip()  # noqa: E731
    dem_short = lambda n: re.sub(r"\(.*$", "", dem(n).replace("(anonymous namespace)::", "").replace("void ", ""))  # noqa: E731
    bad = 0
    if a.md:
        print("| unit | kernel | vgpr | sgpr | LDS | scratch | spills v/s | instructions | same metadata | same multiset |")
        print("|---|---|---|---|---|---|---|---|---|---|")
    if set(old) - set(new):
        bad += 1
        print("kernels of the old tree are missing: %s" % sorted(set(old) - set(new)))
    for name in sorted(set(new) - set(old), key=lambda k: (new[k][0], k)):
        u, m1, i1 = new[name]
        if a.md:
            print("| %s | `%s` | %d | %d | %d | %d | %d/%d | new: %d | new | new |" % (
                u, dem_short(name), m1["vgpr_count"], m1["sgpr_count"], m1["group_segment_fixed_size"], m1["private_segment_fixed_size"],
                m1["vgpr_spill_count"], m1["sgpr_spill_count"], sum(i1.values())))
        else:
            print("%-18s %-44s %5d instructions  new: %s" % (u, dem_short(name), sum(i1.values()), m1))
        if not any(re.match(r"%s\b" % k, dem_short(name)) for k in DESCRIBED):
            bad += 1
            print("    not described in physicl_amd/build.py (ADDONS, LATER, MORE, ROWS)")
    for name in sorted(set(old) & set(new), key=lambda k: (new[k][0], k)):
        (u0, m0, i0), (u, m1, i1) = old[name], new[name]
        same_m, same_i = m0 == m1, i0 == i1
        bad += not (same_m and same_i)
        if a.md:
            print("| %s | `%s` | %d | %d | %d | %d | %d/%d | %d -> %d | %s | %s |" % (
                u, dem_short(name), m1["vgpr_count"], m1["sgpr_count"], m1["group_segment_fixed_size"], m1["private_segment_fixed_size"],
                m1["vgpr_spill_count"], m1["sgpr_spill_count"], sum(i0.values()), sum(i1.values()), "yes" if same_m else "NO",
                "yes" if same_i else "NO"))
        else:
            print("%-18s %-44s %5d instructions  metadata %s  multiset %s" % (u, dem_short(name), sum(i1.values()),
                                                                            "same" if same_m else "DIFFERS", "same" if same_i else "DIFFERS"))
        if u0 != u:
            print("    moved here from %s" % u0)
        if not same_m:
            print("    metadata: %s" % {k: (m0[k], m1[k]) for k in META if m0[k] != m1[k]})
        if not same_i:
            for line, n in sorted(((i0 - i1) + (i1 - i0)).items()):
                print("    %+d  %s" % (i1[line] - i0[line], line))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
