"""Which quad of a cell a lane of FAST pass 1 tests in which round (orb_ygz_slam_amd/csrc/fast_lane_quads.h, included by the kernel and by the host
program tests/cpp/fast_lane_quads_cpu.hip).  The definition: a cell of dw x dh tested pixels has nq = (dw + 3) >> 2 quads per row, and in round k
lane l holds quad i = 64 k + l of the raster order -- row i // nq, column i % nq -- as long as i < nq * dh; the polarity mask drops the pixels past
the cell's width in column nq - 1.  The kernel walks that sequence in two ways, a generic one (reciprocal multiply, then steps with a wrap) and, where
nq divides 64, one in which the lane keeps its column.  The program (built with AddressSanitizer and UBSan, a fresh process) steps both as the kernel
does for every dw 1 .. 41 and dh 1 .. 34 (and the wide cells up to dw = 64 of k_fast_quads) and compares every (round, lane) with the definition;
for a few cells it prints both walks and this file compares them with its own restatement, so that the two forms are seen to give the same lanes,
the same (y, q) and the same mask -- hence the same quad list in the same order."""
import json
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

ALL_FOUR = 0x03030303


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = next((p for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if p and os.path.exists(p)), None)
    assert hipcc, "hipcc not found"
    out = str(tmp_path_factory.mktemp("fast_lane_quads") / "fast_lane_quads_cpu")
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-g", "-std=c++17",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "orb_ygz_slam_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "fast_lane_quads_cpu.hip"),
                           "-L", rocm_lib, "-lamdhip64", "-o", out])
    return out


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    return json.loads(r.stdout)


def test_both_walks_follow_the_raster_order_for_every_cell_size(exe):
    got = run(exe)
    print(got)
    assert got["mismatches"] == 0
    assert got["cells"] == 41 * 34
    # nq divides 64 for dw 1 .. 4 (1), 5 .. 8 (2), 13 .. 16 (4) and 29 .. 32 (8)
    assert got["fixed_cells"] == 16 * 34
    assert got["wide_cells"] == 23 * 34


# full-width cells (nq = 8), the clipped widths of the GPU test, the smallest and the widest cell, one and several rounds, a last round with one lane
@pytest.mark.parametrize("dw,dh", [(29, 30), (30, 34), (31, 1), (32, 33), (1, 34), (1, 1), (5, 30), (13, 17), (16, 34), (17, 30), (23, 31), (41, 34),
                                   (36, 29), (64, 34), (61, 5)])
def test_the_two_walks_give_the_same_lanes_quads_and_masks(exe, dw, dh):
    got = run(exe, dw, dh)
    nq = (dw + 3) >> 2
    last_mask = ALL_FOUR >> (8 * (4 * nq - dw))
    assert got["nq"] == nq and got["rounds"] == (nq * dh + 63) // 64 and got["last_mask"] == last_mask
    want = []
    for k in range(got["rounds"]):
        rnd = []
        for lane in range(64):
            i = 64 * k + lane
            rnd.append((i // nq, i % nq, last_mask if i % nq == nq - 1 else ALL_FOUR) if i < nq * dh else None)
        want.append(rnd)
    assert (got["fixed"] is not None) == (64 % nq == 0)
    for name in ("generic", "fixed"):
        walk = got[name]
        if walk is None:
            continue
        assert len(walk) == got["rounds"]
        for k, rnd in enumerate(walk):
            assert [bool(a) for a, _, _, _ in rnd] == [w is not None for w in want[k]], (name, k)
            assert [(y, q, m) for a, y, q, m in rnd if a] == [w for w in want[k] if w is not None], (name, k)
    if got["fixed"] is not None:      # lane for lane the same: within a round the lanes ascend in (y, q) in both, so the quad list's order is the same
        for rg, rf in zip(got["generic"], got["fixed"]):
            assert [(a, y, q, m) for a, y, q, m in rg if a] == [(a, y, q, m) for a, y, q, m in rf if a]
            assert [a for a, _, _, _ in rg] == [a for a, _, _, _ in rf]
