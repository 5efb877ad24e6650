"""The builds of the two multiply-compiled sweep files (cpecan_kernel_systolic.hip, cpecan_kernel_wave.hip) as the
Makefile lists them (make print-builds), each one's gfx950 assembly under the Makefile's own flags, and what the
compiler's metadata says of a kernel in it.  The Makefile is the one place that knows which builds exist."""
import atexit
import collections
import functools
import os
import re
import shutil
import subprocess
import tempfile

from cpecan_load import ROOT

AMD = os.path.join(ROOT, "cpecan-signal_amd")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

# name: tag and number ("" for the unsuffixed four-wave build); suffix: what its symbols end in; rows: waves per
# workgroup or cells per lane; obj, src: absolute paths; defines: as on the Makefile's command line
Build = collections.namedtuple("Build", "name tag rows suffix family obj src defines")


def make_print(target):
    return subprocess.check_output(["make", "-s", "-C", AMD, target], text=True)


@functools.lru_cache(maxsize=None)
def builds():
    found = []
    for line in make_print("print-builds").splitlines():
        name, obj, src, defines = line.split("\t")
        family = re.fullmatch(r"csrc/cpecan_kernel_(systolic|wave)\.hip", src).group(1)
        tag, rows = (name[:-1], int(name[-1])) if name else ("r", 4)
        found.append(Build(name, tag, rows, "_" + name if name else "", family, os.path.join(AMD, obj),
                           os.path.join(AMD, src), tuple(defines.split())))
    return tuple(found)


@functools.lru_cache(maxsize=None)
def asm_dir():
    path = tempfile.mkdtemp(prefix="cpecan_sweep_asm_")
    atexit.register(shutil.rmtree, path, ignore_errors=True)
    return path


@functools.lru_cache(maxsize=None)
def device_asm(build):
    """the build's gfx950 assembly: compiled once per process, as the Makefile compiles the object"""
    out = os.path.join(asm_dir(), "%s_%s.s" % (build.family, build.name or "r4"))
    subprocess.check_call([HIPCC] + make_print("print-hipflags").split() + list(build.defines) +
                          ["-S", "--cuda-device-only", "-o", out, build.src], cwd=AMD, stderr=subprocess.DEVNULL)
    return open(out).read()


def kernel_meta(text, name):
    """registers, spills, static LDS, scratch and workgroup size of one kernel of an assembly text, and its body"""
    kernels = text[text.index("amdhsa.kernels:"):].split("\n  - .agpr_count")
    meta = [m for m in kernels if ".name:           %s\n" % name in m]
    assert len(meta) == 1, "%s is not in the build" % name
    get = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, meta[0]).group(1))  # noqa: E731
    body = text[text.index("\n" + name + ":"):]
    body = body[:body.index("s_endpgm")]
    return dict(vgpr=get("vgpr_count"), sgpr=get("sgpr_count"), spill=get("vgpr_spill_count"),
                lds=get("group_segment_fixed_size"), scratch=get("private_segment_fixed_size"),
                threads=get("max_flat_workgroup_size"), body=body)


def kernel_names(text):
    """the kernels of an assembly text"""
    return set(re.findall(r"^    \.name:\s+(\S+)$", text[text.index("amdhsa.kernels:"):], re.M))


def defined(path, *flags):
    out = subprocess.check_output(["nm", "--defined-only"] + list(flags) + [path], text=True)
    return set(l.split()[-1] for l in out.splitlines() if l.strip())
