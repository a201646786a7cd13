"""CPU test of the exact sequential application of batched Fuse candidates (orb_ygz_slam_amd/csrc/host/FuseApply.h): on deep copies of seeded
synthetic maps, the reference's sequential ORBmatcher::Fuse loop and fuse_apply over the restated candidate search must leave the same final
graph (tests/cpp/fuse_apply_cpu.cc); a variant without the survivor re-query must diverge somewhere, so the test can see the hazard."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    out = str(tmp_path_factory.mktemp("fuse") / "fuse_apply_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I", host, "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "fuse_apply_cpu.cc"), "-o", out])
    return out


def run(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fuse apply ok" in r.stdout
    line = r.stdout.splitlines()[-2].split()
    return {line[k]: int(line[k + 1]) for k in range(2, len(line) - 1, 2)}


def test_fuse_apply_equals_sequential(exe):
    stats = [run(exe, s) for s in range(1, 9)]
    for s in stats:
        assert s["fused"] > 0 and s["bad0"] > 0 and s["stereo"] > 0 and s["mono"] > 0 and s["added"] > 0
        assert s["into_kf"] > 0 and s["into_mp"] > 0 and s["equal_obs"] > 0   # both Replace branches, and ties of the observation counts
        assert s["requeried"] > 0                       # survivors were searched again
    assert sum(s["bad_in_kf"] for s in stats) > 0      # a bad pMPinKF
    assert any(s["diverged"] for s in stats)            # and without that, the result is wrong
