#!/usr/bin/env python3
"""The kernel choice of two built trees, question for question: cpecan_hip_plan_dispatch, cpecan_hip_plan_assembly_sweeps
and (where a tree has it) cpecan_hip_plan_expectation_pass of each tree's libcpecan_hip.so, asked over one grid of
machines, modes, kernel requests, flags, band widths and environment settings; the rows that differ are printed.  A
refusal is an answer too: its code and its text.  The grid comes from the branch tree (the flags of its
include/cpecan_hip.h, the variables its read_batch_env reads); every environment setting is asked in a child process of
its own per tree, which loads that tree's library through CPECAN_HIP_LIB (CPECAN_DNA_GENERAL is read once per process).
An answer only one tree can give (plan_expectation_pass before it existed) is not compared.  A refactor of the host
side must report 0 differing rows.
usage: tools/dispatch_diff.py PARENT_TREE BRANCH_TREE     (needs both trees built, no GPU; JOBS environment settings at a time)"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

WIDTHS = (0, 1, 56, 57, 120, 121, 158, 159, 184, 185, 192, 193, 248, 249, 376, 377, 504, 505)
BASES = ("WORKGROUP_KERNELS", "GENERAL_KERNEL", "UNBANDED", "DEBUG_DUMP", "WIDE_BANDS")
WITH = ("WIDE_BANDS", "WIDE_BANDS_HDP", "WIDE_BANDS_HDP_ESTEP", "WIDE_BANDS_VANILLA_ESTEP", "WORKGROUP_FUSED_ESTEP",
        "WIDE_BANDS_FUSED_ESTEP", "ASM_NARROW_BANDS", "VANILLA_FUSED_ESTEP", "WIDE_BANDS_VANILLA_FUSED_ESTEP",
        "HDP_FUSED_ESTEP", "WIDE_BANDS_HDP_FUSED_ESTEP", "HDP_FOUR_CELLS_FUSED_ESTEP")  # the wide, fused and asm flags


def grid_of(branch):
    """(flags, environment settings) of the grid, from the branch tree's header and source"""
    header = open(os.path.join(branch, "include", "cpecan_hip.h")).read()
    flag = dict((n, int(v)) for n, v in re.findall(r"#define CPECAN_FLAG_(\w+) (\d+)", header))
    flags = [0] + list(flag.values()) + [flag[b] | flag[w] for b in BASES for w in WITH]
    source = open(os.path.join(branch, "cpecan-signal_amd", "csrc", "cpecan_hip.hip")).read()
    at = source.index("static BatchEnv read_batch_env()")
    names = re.findall(r'getenv\("(CPECAN_[A-Z0-9_]+)"\)', source[at:source.index("\n}\n", at)])
    envs = [{}] + [{n: v} for n in names for v in ("0", "1")] + [{"CPECAN_KERNELS": "systolic"}]
    envs += [{"CPECAN_SYSTOLIC_ROWS": str(r)} for r in range(6)] + [{"CPECAN_ASM": str(a)} for a in range(3)]
    seen, out = set(), []
    for e in envs:
        if json.dumps(e) not in seen:
            seen.add(json.dumps(e))
            out.append(e)
    return sorted(set(flags)), out


def child(flags):
    """every row of the grid under this process's environment, one line each: the question, then the three answers"""
    L = C.CDLL(os.environ["CPECAN_HIP_LIB"])
    L.cpecan_hip_last_error.restype = C.c_char_p
    has_pass = hasattr(L, "cpecan_hip_plan_expectation_pass")
    o = [C.c_int32() for _ in range(4)]
    refs = [C.byref(x) for x in o]
    one = C.c_int32()
    out = []
    for machine in range(6):
        for mode in (0, 1):
            for kernel in (0, 1, 2):
                for f in flags:
                    for w in WIDTHS:
                        for edges in (1, 0):
                            q = (machine, mode, kernel, f, w, edges)
                            rc = L.cpecan_hip_plan_dispatch(*q, *refs)
                            d = [rc, L.cpecan_hip_last_error().decode()] if rc else [x.value for x in o]
                            a = [L.cpecan_hip_plan_assembly_sweeps(*q, C.byref(one)), one.value]
                            if rc:
                                a.append(L.cpecan_hip_last_error().decode())
                            p = None
                            if has_pass:
                                p = [L.cpecan_hip_plan_expectation_pass(*q, C.byref(one)), one.value]
                                if rc:
                                    p.append(L.cpecan_hip_last_error().decode())
                            out.append(json.dumps([q, d, a, p]))
    sys.stdout.write("\n".join(out) + "\n")


def ask(tree, env, flags):
    e = dict((k, v) for k, v in os.environ.items() if not k.startswith("CPECAN_"))
    e.update(env, CPECAN_HIP_LIB=os.path.join(os.path.abspath(tree), "cpecan-signal_amd", "libcpecan_hip.so"))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(flags)], env=e,
                       stdout=subprocess.PIPE, text=True, check=True)
    return [json.loads(line) for line in r.stdout.splitlines()]


def compare(parent, branch, env, flags):
    """(rows, rows whose expectation pass both trees answer, the differing rows as text) of one environment setting"""
    p, b = ask(parent, env, flags), ask(branch, env, flags)
    assert len(p) == len(b) and len(p) > 0
    passes, diffs = 0, []
    for (q, pd, pa, pp), (q2, bd, ba, bp) in zip(p, b):
        assert q == q2
        both = pp is not None and bp is not None
        passes += both
        if pd != bd or pa != ba or (both and pp != bp):
            diffs.append("differs: env %s, (machine, mode, kernel, flags, width, edges) %s\n  parent: dispatch %s, assembly "
                         "sweeps %s, expectation pass %s\n  branch: dispatch %s, assembly sweeps %s, expectation pass %s" %
                         (env, q, pd, pa, pp, bd, ba, bp))
    return len(p), passes, diffs


def main():
    if sys.argv[1] == "--child":
        return child(json.loads(sys.argv[2]))
    parent, branch = sys.argv[1], sys.argv[2]
    flags, envs = grid_of(branch)
    with ThreadPoolExecutor(max_workers=int(os.environ.get("JOBS", "4"))) as pool:
        res = list(pool.map(lambda e: compare(parent, branch, e, flags), envs))
    for _, _, diffs in res:
        for d in diffs:
            print(d)
    rows, passes, differing = sum(r[0] for r in res), sum(r[1] for r in res), sum(len(r[2]) for r in res)
    print("environment settings: %d; flags: %d; rows per tree: %d (plan_dispatch and plan_assembly_sweeps each; "
          "plan_expectation_pass compared on %d); differing: %d" % (len(envs), len(flags), rows, passes, differing))
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
