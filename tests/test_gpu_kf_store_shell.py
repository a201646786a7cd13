"""GPU test of the host shell of the resident keyframes (csrc/host/KeyFrameStore.h / .cc behind ygz::FuseBatch, ORBmatcher::Fuse and
ygz::SearchAndFuseBatch): tests/cpp/kf_store_shell.cc, built with g++ over the stand-alone classes as fuse_shell.cc is, on seeds 1-3."""
import os
import subprocess

import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


def _build_shell(tmp):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
    exe = os.path.join(tmp, "kf_store_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "kf_store_shell.cc")] + [os.path.join(host, f) for f in
            ("ORBextractor.cc", "ORBmatcher.cc", "ORBmatcherFuse.cc", "ORBmatcherLoop.cc", "KeyFrameStore.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_kf_store_shell_end_to_end(tmp_path):
    """With the store on, FuseBatch and SearchAndFuseBatch leave the graphs of the sequential restatements and of the store-off runs; each distinct
    keyframe is put once, an overlap hits, another mnId at an address and an Erase put again."""
    from orb_ygz_slam_amd import load_library
    load_library()
    exe = _build_shell(str(tmp_path))
    script = " && ".join("%s %d" % (exe, seed) for seed in (1, 2, 3))
    out = subprocess.run(["sh", "-c", script], capture_output=True, text=True, timeout=300)      # one subprocess, one time limit
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("kf store shell ok") == 3, out.stdout
