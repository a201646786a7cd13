"""host/Sim3Replay.h and csrc/sim3_math.h as a plain host program (tests/cpp/sim3_host.cc), built with -fsanitize=address,undefined, against
tests/sim3_cases.py on every case: the hypotheses the kernel's own arithmetic text gives on one host thread are mode "device" bit for bit, and
the replay -- state carried across iterate calls, bNoMore, the mapping through mvnIndices1, find -- is `sim3_iterate`; mRansacMaxIts for a
table of (N, minInliers, p, maxIterations); the draws of a solver's triples on a scripted RandomInt."""
import os
import subprocess

import numpy as np
import pytest

from tests import sim3_cases as SC
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3_host") / "sim3_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-I", os.path.join(CSRC, "host"), os.path.join(ROOT, "tests", "cpp", "sim3_host.cc"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", SC.NAMES + SC.SCENE_NAMES)
def test_case_on_the_host(prog, tmp_path, name):
    c = SC.case_by_name(name)
    want = SC.expected(c, "device")
    SC.write_case(c.problem, str(tmp_path / "in.bin"))
    r = subprocess.run([prog, "case", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = SC.read_result(c.problem, str(tmp_path / "out.bin"))
    nan = np.isnan(want.hyps.hyp)
    assert np.array_equal(np.isnan(got.hyps.hyp), nan)
    assert np.array_equal(got.hyps.hyp.view(np.uint32)[~nan], want.hyps.hyp.view(np.uint32)[~nan]), "hyp differs from mode device in some bit"
    assert np.array_equal(got.hyps.count, want.hyps.count) and np.array_equal(got.hyps.bits, want.hyps.bits)
    assert SC.same_calls(got.calls, want.calls)


def test_max_its_table(prog):
    text = "".join("%d %d %r %d\n" % (N, m, p, mx) for N, m, p, mx, _ in SC.MAX_ITS_TABLE)
    r = subprocess.run([prog, "table"], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert [int(v) for v in r.stdout.split()] == [w for *_, w in SC.MAX_ITS_TABLE]


@pytest.mark.parametrize("n,count,seed", [(3, 10, 1), (4, 50, 2), (20, 300, 3), (500, 300, 4)])
def test_draws(prog, n, count, seed):
    r = subprocess.run([prog, "draws", str(n), str(count), str(seed)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([int(v) for v in r.stdout.split()], np.int32).reshape(-1, 3)
    assert np.array_equal(got, SC.draw_triples(n, count, SC.Lcg(seed).random_int))
