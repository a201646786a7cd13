"""CPU test of the exact sequential application of batched loop-closing candidates (orb_ygz_slam_amd/csrc/host/LoopApply.h): on deep copies of
seeded synthetic maps, LoopClosing::SearchAndFuse restated sequentially and search_and_fuse_apply over the restated candidate search must leave
the same final graph, and SearchByProjection(pKF, Scw, ..) restated sequentially and search_by_projection_apply the same vpMatched
(tests/cpp/loop_apply_cpu.cc).  Without the survivor re-query the graph must differ somewhere, so the test can see the hazard."""
import os
import subprocess

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    out = str(tmp_path_factory.mktemp("loop") / "loop_apply_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I", host, "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "loop_apply_cpu.cc"), "-o", out])
    return out


def run(exe, seed):
    r = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "loop apply ok" in r.stdout
    line = r.stdout.splitlines()[-2].split()
    return {line[k]: int(line[k + 1]) for k in range(2, len(line) - 1, 2)}


def test_loop_apply_equals_sequential(exe):
    stats = [run(exe, s) for s in range(1, 9)]
    for s in stats:
        # SearchAndFuse: duplicate list entries, bad points, points already in the keyframe, both outcomes of :991-998, Replace survivors
        assert s["fused"] > 0 and s["dups"] > 0 and s["bad0"] > 0 and s["in_kf0"] > 0 and s["added"] > 0 and s["replaced"] > 0
        assert s["requeried"] > 0                       # survivors were searched again
        # SearchByProjection: matches, a non-empty vpMatched at entry, points that lose their best key to an earlier point
        assert s["matched"] > 0 and s["preset"] > 0 and s["conflicts"] > 0
        assert s["requeries1"] > 0                      # n_best = 1 exhausts its lists and still matches
    assert any(s["listed_in_slot"] for s in stats)      # a later point found an earlier listed point in its key's slot
    assert any(s["diverged"] for s in stats)            # and without the re-query, the result is wrong
