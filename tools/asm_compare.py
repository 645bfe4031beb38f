"""Before / after comparison of the kernel units' instruction streams (profiles/*/existing_units_asm.txt).

  python tools/asm_compare.py [--parent REV | --parent-tree DIR] [--jobs 8] [--keep DIR] > existing_units_asm.txt

Every kernel unit the parent tree has (wbc_kernel.hip as `main`, and each wbc_kernel_<unit>.hip of the parent
Makefile's KTU) is compiled in both trees with the flags of that tree's Makefile (-O3 -std=c++17 --offload-arch,
the include paths, -DWBC_WAVES_PER_SIMD, KFLAGS, the unit's own <UNIT>_KFLAGS) and -S --offload-device-only.
--parent REV (default HEAD) takes the parent tree from `git archive REV` into a temporary directory; the other
tree is this checkout's working tree.

What is compared: the instruction lines of the device assembly, i.e. the lines that start with a tab and are
neither a directive (.xxx) nor a comment, with the trailing comment cut, white space squeezed and branch-target
labels normalised (.LBB<function>_<block> -> .LBB: they are numbered per function, and a unit that gains a
function renumbers them).  Per unit the report gives the number of instruction lines before and after, the
multiset difference (`<` lines only the parent has, `>` lines only this tree has, each with its count), and whether
the two streams are in the same order once those differing lines are left out.  `s_nop 0` is left out of the
order check as well: the assembler's hazard padding moves when a scalar register pair changes, which is how the
8-byte shift of the kernel-argument segment shows in the resident kernel.  Units only this tree has are listed as
new and not compared."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("quadrupedwholebodycontroller_amd", "csrc")


def makefile(tree):
    mk = open(os.path.join(tree, CSRC, "Makefile")).read()
    var = lambda v, default=None: (re.search(rf"^{v} [:?]?= (.*)$", mk, re.M) or [None, default])[1]
    units = var("KTU").split()
    flags = {"main": []}
    for u in units:
        ref = re.search(rf"^KFLAGS_{u} = \$\((\w+)\)$", mk, re.M)
        flags[u] = var(ref.group(1)).split() if ref else []
    return dict(hipcc=var("HIPCC", "/opt/rocm/bin/hipcc"), arch=var("ARCH", "gfx950"), waves=var("WAVES", "2"),
                kflags=var("KFLAGS").split(), units=["main"] + units, flags=flags)


def compile_unit(tree, mk, unit, out):
    src = "wbc_kernel.hip" if unit == "main" else f"wbc_kernel_{unit}.hip"
    cmd = [mk["hipcc"], "-O3", "-std=c++17", f"--offload-arch={mk['arch']}", "-I", os.path.join(tree, "include"), "-I",
           os.path.join(tree, CSRC), f"-DWBC_WAVES_PER_SIMD={mk['waves']}", *mk["kflags"], *mk["flags"][unit], "-S",
           "--offload-device-only", os.path.join(tree, CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"{unit}: {r.stderr[-2000:]}")
    return out


def instructions(path):
    out = []
    for l in open(path):
        if not l.startswith("\t"):
            continue
        t = l.strip()
        if not t or t.startswith(".") or t.startswith(";"):
            continue
        t = re.sub(r"\.LBB\d+_\d+", ".LBB", t.split(";")[0].strip())
        out.append(re.sub(r"\s+", " ", t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", default=None, help="keep the .s files under this directory")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        parent = args.parent_tree
        if not parent:
            parent = os.path.join(tmp, "parent")
            os.makedirs(parent)
            ar = subprocess.run(["git", "-C", ROOT, "archive", args.parent, CSRC, "include"], capture_output=True, check=True)
            subprocess.run(["tar", "-x", "-C", parent], input=ar.stdout, check=True)
        work = args.keep or tmp
        mko, mkn = makefile(parent), makefile(ROOT)
        jobs = []
        for tag, tree, mk in (("old", parent, mko), ("new", ROOT, mkn)):
            os.makedirs(os.path.join(work, tag), exist_ok=True)
            jobs += [(tree, mk, u, os.path.join(work, tag, u + ".s")) for u in mk["units"]]
        with ThreadPoolExecutor(args.jobs) as ex:
            list(ex.map(lambda j: compile_unit(*j), jobs))
        print(f"# tools/asm_compare.py --parent {args.parent if not args.parent_tree else '<tree>'}: each unit of the parent compiled "
              "with its Makefile flags and -S --offload-device-only,")
        print("# parent against this tree: instruction lines that differ (branch-target labels normalised: they are numbered per "
              "function);")
        print("# `<` only the parent has, `>` only this tree has, with counts")
        for u in mko["units"]:
            a, b = instructions(os.path.join(work, "old", u + ".s")), instructions(os.path.join(work, "new", u + ".s"))
            da, db = collections.Counter(a) - collections.Counter(b), collections.Counter(b) - collections.Counter(a)
            same = [x for x in a if x not in da and x != "s_nop 0"] == [x for x in b if x not in db and x != "s_nop 0"]
            print(f"== {u} instr lines {len(a)} -> {len(b)}, same order apart from the lines below (every s_nop 0 left out of the "
                  f"order check): {same}; differing:")
            for k in sorted(da):
                print(f"  {da[k]:5d} < {k}")
            for k in sorted(db):
                print(f"  {db[k]:5d} > {k}")
        new = [u for u in mkn["units"] if u not in mko["units"]]
        if new:
            print("== new units, not compared: " + ", ".join(f"{u} ({len(instructions(os.path.join(work, 'new', u + '.s')))} instr lines)"
                                                              for u in new))
    return 0


if __name__ == "__main__":
    sys.exit(main())
