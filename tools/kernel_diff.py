#!/usr/bin/env python3
"""Device code of the throughput kernels in two source trees, kernel for kernel: every build the branch tree's Makefile
makes of cpecan_kernel_systolic.hip and cpecan_kernel_wave.hip (make print-builds), and the files around them that are
compiled once (ONCE below: a unit is a file of csrc,
and one that a tree lacks or that defines no kernel there counts for nothing, and so does a build that a tree's source
refuses with #error: a build from before it existed), is compiled to gfx950 assembly in both trees (the branch Makefile's flags, make print-hipflags, plus -S --cuda-device-only) and, per
kernel name, the instructions between the label and the function's end and the resource lines of the metadata block are
compared.  A kernel that moved to another file is compared with whichever parent build had it: the number of its
function in the file, which the compiler puts into its local labels (.LBB<n>_), is taken out first.  A refactor of the
host side, or one that moves kernels between files, must leave all of them as they were.
usage: tools/kernel_diff.py PARENT_TREE BRANCH_TREE [WORKDIR]     (needs hipcc, no GPU; about 17 s per wave build)"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ONCE = ("cpecan_kernel_prep.hip", "cpecan_kernel_general.hip", "cpecan_kernel_generalh.hip", "cpecan_hip.hip",
        "cpecan_run.hip", "cpecan_readback.hip")
META = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "group_segment_fixed_size", "private_segment_fixed_size",
        "kernarg_segment_size")


def make_print(tree, target):
    return subprocess.check_output(["make", "-s", "-C", os.path.join(tree, "cpecan-signal_amd"), target], text=True)


def kernels(tree, unit, defs, flags, work):
    """{kernel name: (instruction text, metadata figures)} of one build of one tree; none where the tree lacks the file"""
    amd = os.path.join(tree, "cpecan-signal_amd")
    if not os.path.exists(os.path.join(amd, "csrc", unit)):
        return {}
    out = os.path.abspath(os.path.join(work, "%s%s.s" % (unit[:-4], "".join(defs).replace("-D", "_").replace("=", ""))))
    r = subprocess.run([HIPCC] + flags + defs + ["-S", "--cuda-device-only", "-o", out, os.path.join("csrc", unit)],
                       cwd=amd, stderr=subprocess.PIPE, text=True)  # (from where make runs: the flags' -I are relative)
    if r.returncode != 0 and "#error" in r.stderr:
        return {}
    if r.returncode != 0:
        raise subprocess.CalledProcessError(r.returncode, r.args, stderr=r.stderr)
    text = open(out).read()
    found = {}
    if "amdhsa.kernels:" not in text:
        return found
    for block in text[text.index("amdhsa.kernels:"):].split("\n  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        body = text[text.index("\n%s:" % name):]
        body = "\n".join(l.split(";")[0].rstrip() for l in body[:body.index("\n.Lfunc_end")].splitlines())
        body = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\n+", "\n", body))  # (comments gone: they name blocks by function too)
        found[name] = (body, tuple(re.search(r"\.%s:\s+(\d+)" % k, block).group(1) for k in META))
    return found


def main():
    parent, branch = sys.argv[1], sys.argv[2]
    work = sys.argv[3] if len(sys.argv) > 3 else "kernel_diff_out"
    for t in ("P", "B"):
        os.makedirs(os.path.join(work, t), exist_ok=True)
    flags = make_print(branch, "print-hipflags").split()
    builds = [(os.path.basename(src), defs.split()) for _, _, src, defs in
              (line.split("\t") for line in make_print(branch, "print-builds").splitlines())] + [(u, []) for u in ONCE]
    jobs = [(t, sub, u, d) for u, d in builds for t, sub in ((parent, "P"), (branch, "B"))]
    with ThreadPoolExecutor(max_workers=int(os.environ.get("JOBS", "8"))) as pool:
        res = list(pool.map(lambda j: kernels(j[0], j[2], j[3], flags, os.path.join(work, j[1])), jobs))
    # a kernel is compared with the same build of the parent, or (it moved) with the parent build that has it
    everywhere = {}
    for p in res[0::2]:
        for name, v in p.items():
            everywhere.setdefault(name, v)
    same, differ, new, kept = 0, [], [], set()
    for (u, d), p, b in zip(builds, res[0::2], res[1::2]):
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
    print("units compiled: %d; kernels identical: %d; differing: %d %s; only in the parent: %d %s; only in the branch: %d %s" %
          (len(builds), same, len(differ), differ, len(gone), gone, len(new), new))
    return 1 if differ or new else 0


if __name__ == "__main__":
    sys.exit(main())
