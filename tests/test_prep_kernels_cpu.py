"""What the throughput kernels need once per batch or once per library -- the k-mer, track and counts kernels, the
division self-test, the six SweepMachine records -- is compiled once, in cpecan_kernel_prep.hip; an object of the two
multiply-compiled sweep files (cpecan_kernel_systolic.hip, cpecan_kernel_wave.hip) defines nothing but its own build's
sweeps.  Symbol tables of the built objects only: CPU-only."""
import os
import re
import shutil
import subprocess

import pytest

from cpecan_load import ROOT
from sweep_builds import builds, defined
from test_sweep_build_resources import WAVE

AMD = os.path.join(ROOT, "cpecan-signal_amd")
ONCE = ("cpecan_k_kmer_index", "cpecan_k_hdp_kmer_id", "cpecan_k_track", "cpecan_k_sy_track_hdp", "cpecan_k_wv_track",
        "cpecan_k_wv_track_vanilla", "cpecan_k_wv_track_hdp", "cpecan_k_sy_counts", "cpecan_k_wv_counts",
        "cpecan_k_divtest")
MACHINES = ("cpecan_systolic_machine", "cpecan_systolic_machine_vanilla", "cpecan_systolic_machine_hdp",
            "cpecan_wave_machine", "cpecan_wave_machine_hdp", "cpecan_wave_machine_vanilla")
# tags of the workgroup builds without an expectation kernel: posterior decode only, or the E-step fused into the sweep
NO_EXPECT = ("v", "h", "f", "vf", "hf")


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


def test_once_kernels_are_in_the_prep_object_alone(objects):
    for name in ONCE:
        where = [os.path.basename(p) for p, names in objects.items() if name in names]
        assert where == ["cpecan_kernel_prep.o"], "%s is defined in %s" % (name, where)


def test_sweep_objects_define_their_own_build_only(objects):
    listed = dict((b.obj, b) for b in builds() if b.name)
    assert len(listed) >= 31 and set(listed) <= set(objects)
    seen = 0
    for p, names in objects.items():
        m = re.fullmatch(r"cpecan_kernel_(systolic|wave)(_[a-z]+\d)\.o", os.path.basename(p))
        if m is None:
            continue
        seen += 1
        assert listed[p].suffix == m.group(2)
        kernels = set(n for n in names if n.startswith("cpecan_k_"))
        assert kernels, os.path.basename(p)
        stray = sorted(n for n in kernels if not n.endswith(m.group(2)))
        assert not stray, "%s defines %s" % (os.path.basename(p), stray)
        assert not set(ONCE) & names
        assert "cpecan_%s_build%s" % m.groups() in names
        if m.group(1) == "systolic":  # forward and backward, and an expectation kernel where the E-step is not elsewhere
            stems = ("forward", "backward") + (() if listed[p].tag in NO_EXPECT else ("expect",))
            assert kernels == set("cpecan_k_sy_%s%s" % (s, m.group(2)) for s in stems), os.path.basename(p)
        else:  # the kernels of the tag's row
            assert kernels == set("cpecan_k_wv_%s%s" % (s, m.group(2)) for s in WAVE[listed[p].tag][0]), os.path.basename(p)
    assert seen == len(listed)  # every suffixed build of the Makefile's list, and no other object of that name


def test_unsuffixed_workgroup_object_has_three_kernels(objects):
    names = objects[os.path.join(AMD, "csrc", "cpecan_kernel_systolic.o")]
    assert set(n for n in names if n.startswith("cpecan_k_")) == {"cpecan_k_sy_forward", "cpecan_k_sy_backward",
                                                                 "cpecan_k_sy_expect"}


def test_library_exports_the_machine_records(objects):
    assert set(MACHINES) <= defined(os.path.join(AMD, "libcpecan_hip.so"), "-D")
