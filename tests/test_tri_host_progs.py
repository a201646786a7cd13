"""csrc/tri_math.h as a plain host program (tests/cpp/tri_host.cc), built with -fsanitize=address,undefined and -ffp-contract=off, against
tests/triangulate_cases.py: the x3D, the status byte and the sweep count the kernel's own arithmetic text gives on one host thread are the
restatement's bit for bit on every constructed case, every svd case and every seeded scene.  The program is stand-alone: no sanitizer runtime
is preloaded anywhere."""
import os
import subprocess

import numpy as np
import pytest

from tests import triangulate_cases as TC
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tri_host") / "tri_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "tri_host.cc"), "-o", exe])
    return exe


def run(prog, mode, tmp_path):
    r = subprocess.run([prog, mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("name", TC.NAMES)
def test_case_on_the_host(prog, tmp_path, name):
    c = TC.case_by_name(name)
    want = TC.as_arrays([TC.expected(c)])
    TC.write_pairs(str(tmp_path / "in.bin"), c.kf1, c.kf2, [c.idx1], [c.idx2], c.ratio)
    run(prog, "pairs", tmp_path)
    x3d, status, sweeps = TC.read_pairs(str(tmp_path / "out.bin"), 1)
    assert status[0] == want[1][0] and sweeps[0] == want[2][0]
    assert same_bits(x3d, want[0]), "x3D differs from the restatement in some bit"


@pytest.mark.parametrize("name", TC.SCENE_NAMES)
def test_scene_on_the_host(prog, tmp_path, name):
    k1, k2, i1, i2, ratio = TC.scene(name)
    want = TC.as_arrays(TC.scene_expected(name))
    TC.write_pairs(str(tmp_path / "in.bin"), k1, k2, i1, i2, ratio)
    run(prog, "pairs", tmp_path)
    x3d, status, sweeps = TC.read_pairs(str(tmp_path / "out.bin"), len(i1))
    assert np.array_equal(status, want[1]) and np.array_equal(sweeps, want[2])
    assert same_bits(x3d, want[0])


@pytest.mark.parametrize("name", TC.SVD_NAMES)
def test_svd_on_the_host(prog, tmp_path, name):
    A = TC.svd_case(name).make()
    want = TC.jacobi_svd4(A)
    np.ascontiguousarray(A, np.float32).tofile(str(tmp_path / "in.bin"))
    run(prog, "svd", tmp_path)
    with open(str(tmp_path / "out.bin"), "rb") as f:
        V, sv, sweeps = np.fromfile(f, np.float32, 16).reshape(4, 4), np.fromfile(f, np.float32, 4), int(np.fromfile(f, np.int32, 1)[0])
    assert sweeps == want.sweeps and same_bits(V, want.V) and same_bits(sv, want.sv)


# ---- host/TriangulateApply.h over mock keyframes and points (tests/cpp/tri_apply_cpu.cc) --------------------------------------------------------------
@pytest.fixture(scope="module")
def apply_prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tri_apply") / "tri_apply_cpu")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(CSRC, "host"), os.path.join(ROOT, "tests", "cpp", "tri_apply_cpu.cc"), "-o", exe])
    return exe


def run_apply(exe, seed, shared, dup, stop):
    r = subprocess.run([exe, str(seed), str(shared), str(int(dup)), str(stop)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "triangulate apply ok" in r.stdout
    line = r.stdout.splitlines()[-2].split()
    return {line[k]: int(line[k + 1]) for k in range(0, len(line) - 1, 2)}


@pytest.mark.parametrize("shared", [2, 3])
def test_apply_equals_the_sequential_loop_where_neighbours_share_a_feature(apply_prog, shared):
    """two / three neighbours match the same KF1 features: the snapshot batch drops what the reference never sees and equals it; with the drop
    rule off it does not"""
    for seed in range(1, 7):
        s = run_apply(apply_prog, seed, shared, False, -1)
        assert s["created"] > 20 and s["dropped"] > 0 and s["stopped_at"] == -1
        assert s["diverged"] > 0, "the drop rule is what makes these scenes come out right"


def test_apply_without_shared_features_needs_no_drop(apply_prog):
    """exactly the scenes built for the drop rule differ without it: where no feature is shared, nothing is dropped and nothing diverges"""
    for seed in range(1, 7):
        s = run_apply(apply_prog, seed, 1, False, -1)
        assert s["created"] >= 10 and s["dropped"] == 0 and s["diverged"] == 0


def test_apply_with_one_idx2_matched_twice(apply_prog):
    """one neighbour matches one of its features to two KF1 features: both points are created and the second takes the slot, in both forms"""
    for seed in range(1, 7):
        s = run_apply(apply_prog, seed, 2, True, -1)
        assert s["overwritten"] > 0 and s["dropped"] > 0


@pytest.mark.parametrize("stop", [1, 2, 4, 5])
def test_apply_stops_where_the_poll_says(apply_prog, stop):
    """CheckNewKeyFrames() turning true before neighbour 1, 2, the last one, and only after the last one (never seen)"""
    never = run_apply(apply_prog, 3, 3, True, -1)
    s = run_apply(apply_prog, 3, 3, True, stop)
    assert s["stopped_at"] == (stop if stop < 5 else -1)
    assert s["created"] < never["created"] if stop < 5 else s["created"] == never["created"]


# ---- the sweep cap's own exit (status 9), through the C text built with a lower cap ---------------------------------------------------------------
def test_sweep_cap_status_through_the_c_text(tmp_path_factory, tmp_path, monkeypatch):
    """csrc/tri_math.h built with the cap at 3: the suite's matrix of the most sweeps (4) meets it, as does the pair it comes from, which ends
    with status 9 and x3D = 0, and so does a pair that needs exactly 3 (a clean fourth sweep is what shows convergence); the restatement under the same cap says the
    same, and a pair that needs 2 sweeps is untouched"""
    exe = str(tmp_path_factory.mktemp("tri_host_cap") / "tri_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-DYGZF_TRI_MAX_SWEEPS=3", "-I", CSRC, os.path.join(ROOT, "tests", "cpp", "tri_host.cc"), "-o", exe])
    A = TC.most_sweeps_matrix()
    assert TC.jacobi_svd4(A).sweeps == 4
    np.ascontiguousarray(A, np.float32).tofile(str(tmp_path / "in.bin"))
    run(exe, "svd", tmp_path)
    with open(str(tmp_path / "out.bin"), "rb") as f:
        f.seek(80)
        assert int(np.fromfile(f, np.int32, 1)[0]) == 3 == TC.jacobi_svd4(A, max_sweeps=3).sweeps
    monkeypatch.setattr(TC, "MAX_SWEEPS", 3)
    for name, status in (("z2_behind", TC.SWEEP_CAP), ("mono_accept", TC.SWEEP_CAP), ("mono_cos_below_9998", TC.ACCEPTED)):
        c = TC.case_by_name(name)
        want = TC.tri_pair(c.kf1, c.kf2, c.idx1, c.idx2, c.ratio)   # (not the cached result: that is the full cap's)
        assert want.status == status and want.source == TC.FROM_SVD
        TC.write_pairs(str(tmp_path / "in.bin"), c.kf1, c.kf2, [c.idx1], [c.idx2], c.ratio)
        run(exe, "pairs", tmp_path)
        x3d, st, sweeps = TC.read_pairs(str(tmp_path / "out.bin"), 1)
        assert st[0] == TC.status_byte(want) and st[0] & 15 == status and same_bits(x3d, [want.x3d])
        if status == TC.SWEEP_CAP:
            assert sweeps[0] == 3 and not x3d.any()
