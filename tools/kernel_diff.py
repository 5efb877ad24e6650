#!/usr/bin/env python3
"""Device code of the throughput kernels in two source trees, kernel for kernel: every build the Makefile makes of
cpecan_kernel_systolic.hip and cpecan_kernel_wave.hip is compiled to gfx950 assembly in both trees (the Makefile's flags
plus -S --cuda-device-only) and, per kernel name, the instructions between the label and s_endpgm and the resource
lines of the metadata block are compared.  A refactor of the host side must leave all of them as they were.
usage: tools/kernel_diff.py PARENT_TREE BRANCH_TREE [WORKDIR]     (needs hipcc, no GPU; about 17 s per wave build)"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall",
         "-Wno-unused-function"]
BUILDS = [("systolic", ["-DSY_R=%d" % r]) for r in (1, 2, 3)] + [("systolic", [])] + \
         [("wave", ["-DWV_L=%d" % l] + m) for m in ([], ["-DWV_HDP"]) for l in (2, 3, 4)] + \
         [("wave", ["-DWV_L=%d" % l, "-DWV_VANILLA"]) for l in (2, 3, 4)]
META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "kernarg_segment_size")


def kernels(tree, unit, defs, work):
    """{kernel name: (instruction text, metadata figures)} of one build of one tree"""
    src = os.path.join(tree, "cpecan-signal_amd", "csrc", "cpecan_kernel_%s.hip" % unit)
    out = os.path.join(work, "%s%s.s" % (unit, "".join(defs).replace("-D", "_").replace("=", "")))
    subprocess.check_call([HIPCC] + FLAGS + defs + ["-I" + os.path.join(tree, "include"), "-I" + os.path.dirname(src),
                                                    "-S", "--cuda-device-only", "-o", out, src],
                          stderr=subprocess.DEVNULL)
    text = open(out).read()
    found = {}
    for block in text[text.index("amdhsa.kernels:"):].split("\n  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        body = text[text.index("\n%s:" % name):]
        body = "\n".join(l for l in body[:body.index("s_endpgm")].splitlines() if not l.lstrip().startswith(";"))
        found[name] = (body, tuple(re.search(r"\.%s:\s+(\d+)" % k, block).group(1) for k in META))
    return found


def main():
    parent, branch = sys.argv[1], sys.argv[2]
    work = sys.argv[3] if len(sys.argv) > 3 else "kernel_diff_out"
    for t in ("P", "B"):
        os.makedirs(os.path.join(work, t), exist_ok=True)
    jobs = [(t, sub, u, d) for u, d in BUILDS for t, sub in ((parent, "P"), (branch, "B"))]
    with ThreadPoolExecutor(max_workers=int(os.environ.get("JOBS", "8"))) as pool:
        # (the four-cell vanilla build is no longer made: its sweeps are expected among "only in the parent")
        res = list(pool.map(lambda j: {} if j[1] == "B" and j[3] == ["-DWV_L=4", "-DWV_VANILLA"] else
                            kernels(j[0], j[2], j[3], os.path.join(work, j[1])), jobs))
    # a kernel is compared with the same build of the parent, or (it moved) with the parent build that has it
    everywhere = {}
    for p in res[0::2]:
        for name, v in p.items():
            everywhere.setdefault(name, v)
    same, differ, new, kept = 0, [], [], set()
    for (u, d), p, b in zip(BUILDS, res[0::2], res[1::2]):
        for name, v in b.items():
            ref = p.get(name, everywhere.get(name))
            kept.add(name)
            if ref is None:
                new.append(name)
            elif ref == v:
                same += 1
            else:
                differ.append("%s (%s %s)" % (name, u, " ".join(d)))
    gone = sorted(set(everywhere) - kept)
    print("kernels identical: %d; differing: %d %s; only in the parent: %d %s; only in the branch: %d %s" %
          (same, len(differ), differ, len(gone), gone, len(new), new))
    return 1 if differ or new else 0


if __name__ == "__main__":
    sys.exit(main())
