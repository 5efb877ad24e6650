"""The two kernels that pack a run's candidates for the host are compiled in cpecan_readback.hip, with the readback
that launches them; cpecan_hip.hip and cpecan_run.hip, the rest of the C-ABI layer (contexts, the kernel choice and batch
creation; how a run is queued), are host code and define no kernel.  Symbol tables of the built objects only: CPU-only."""
import os
import shutil
import subprocess

import pytest

from cpecan_load import ROOT

AMD = os.path.join(ROOT, "cpecan-signal_amd")
PACK = ("cpecan_k_pack_pairs", "cpecan_k_pack_base")


def defined(path):
    out = subprocess.check_output(["nm", "--defined-only", path], text=True)
    return set(l.split()[-1] for l in out.splitlines() if l.strip())


@pytest.fixture(scope="module")
def objects():
    """{object path: names it defines} of the objects the library is linked from"""
    if not os.path.exists(os.path.join(AMD, "libcpecan_hip.so")):
        pytest.skip("library not built")
    if shutil.which("nm") is None:
        pytest.skip("nm not available: the symbols cannot be listed")
    paths = [os.path.join(AMD, o) for o in subprocess.check_output(["make", "-s", "-C", AMD, "print-objects"],
                                                                   text=True).split()]
    if not all(os.path.exists(p) for p in paths):
        pytest.skip("the library's objects are not here")
    return dict((p, defined(p)) for p in paths)


def test_pack_kernels_are_in_the_readback_object_alone(objects):
    for name in PACK:
        where = [os.path.basename(p) for p, names in objects.items() if name in names]
        assert where == ["cpecan_readback.o"], "%s is defined in %s" % (name, where)


def test_the_batch_layer_defines_no_kernel(objects):
    for obj in ("cpecan_hip.o", "cpecan_run.o"):
        names = objects[os.path.join(AMD, "csrc", obj)]
        assert names, "%s defines nothing?" % obj
        assert sorted(n for n in names if n.startswith("cpecan_k_")) == [], obj
