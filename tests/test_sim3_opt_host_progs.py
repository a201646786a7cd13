"""csrc/sim3_opt_math.h as a plain host program (tests/cpp/sim3_opt_host.cc: one thread, the reference's order of sums), built with
-fsanitize=address,undefined and -ffp-contract=off, against tests/sim3_opt_cases.py on every case: the Sim3, the removed flags, the return
value, nBad and per round the iterations, trials, stop reason, lambda and chi2 equal mode "reference" bit for bit."""
import os
import subprocess

import pytest

from tests import sim3_opt_cases as SC
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sim3_opt_host") / "sim3_opt_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-I", os.path.join(CSRC, "host"), os.path.join(ROOT, "tests", "cpp", "sim3_opt_host.cc"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", SC.NAMES)
def test_case_on_the_host(prog, tmp_path, name):
    c = SC.case_by_name(name)
    want = SC.expected(c, "reference")
    SC.write_case(c.problem, str(tmp_path / "in.bin"))
    r = subprocess.run([prog, "case", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = SC.read_result(c.problem, str(tmp_path / "out.bin"))
    assert (got.ret, got.n_bad, list(got.iters), list(got.trials), list(got.stop)) == (want.ret, want.n_bad, list(want.iters), list(want.trials), list(want.stop))
    assert SC.same(got, want), "the host program differs from mode reference in some bit"
