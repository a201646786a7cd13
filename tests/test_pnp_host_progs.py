"""host/PnPReplay.h, host/PnPHost.h and csrc/pnp_math.h as a plain host program (tests/cpp/pnp_host.cc), built with
-fsanitize=address,undefined, against tests/pnp_cases.py on every case: the poses, counts, masks, record flags and Refine results that the
kernels' own arithmetic text gives on one host thread are the restatement's bit for bit, and the replay -- state carried across iterate calls,
the `||` overrun evaluated when reached, bNoMore, the mapping through mvKeyPointIndices, find -- is `pnp_iterate`; SetRansacParameters for a
table of arguments; the draws of a solver's sample sets on a scripted RandomInt."""
import os
import subprocess

import numpy as np
import pytest

from tests import pnp_cases as PC
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pnp_host") / "pnp_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, "-I", os.path.join(CSRC, "host"), os.path.join(ROOT, "tests", "cpp", "pnp_host.cc"), "-o", exe])
    return exe


@pytest.mark.parametrize("name", PC.NAMES + PC.SCENE_NAMES)
def test_case_on_the_host(prog, tmp_path, name):
    c = PC.case_by_name(name)
    want = PC.expected(c)
    PC.write_case(c.problem, str(tmp_path / "in.bin"))
    r = subprocess.run([prog, "case", str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = PC.read_result(c.problem, str(tmp_path / "out.bin"))
    assert len(got.hyps.count) == len(want.hyps.count)
    assert PC.same_hyps(got.hyps, want.hyps), "poses, counts, masks or Refine results differ from the restatement in some bit"
    assert PC.same_calls(got.calls, want.calls)


def test_parameter_table(prog):
    text = "".join("%d %r %d %d %d %r\n" % row for row in PC.PARAMETER_TABLE)
    r = subprocess.run([prog, "table"], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([int(v) for v in r.stdout.split()]).reshape(-1, 2).tolist()
    assert got == [list(PC.ransac_parameters(*row)) for row in PC.PARAMETER_TABLE]


@pytest.mark.parametrize("n,min_set,count,seed", [(4, 4, 10, 1), (5, 5, 50, 2), (20, 4, 300, 3), (500, 4, 300, 4), (9, 8, 20, 5), (3, 4, 5, 6)])
def test_draws(prog, n, min_set, count, seed):
    r = subprocess.run([prog, "draws", str(n), str(min_set), str(count), str(seed)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([int(v) for v in r.stdout.split()], np.int32).reshape(-1, min_set)
    assert np.array_equal(got, PC.draw_quads(n, min_set, count, PC.Lcg(seed).random_int))
