"""LDS bank conflicts of describe_window's raw window, counted on the CPU from the committed layout and lane mappings.

The rule (gfx950, ds_read_b32 and ds_write_b32): a wave's access is served in two groups of 32 lanes, {0..31} and {32..63}; the bank of byte
address a is (a / 4) mod 32; lanes of a group that read the same dword share one access, and a group costs as many cycles as the most distinct
dwords it has on one bank ("N-way").  The layout (row offsets, LDS-DMA slots, overlay sizes) and the item-to-lane mappings are not restated here:
tests/cpp/describe_lds_cpu.hip prints them from orb_ygz_slam_amd/csrc/describe_lds.h, the header the kernel computes its addresses with.  What
is restated is the kernel's address arithmetic on top of them (describe_window in csrc/extract_kernels.hip):

    column 0 of window row r     raw + row_byte(r) + ((rowOff0 + r * rowOffStep) & 15)       rowOff0 0..15, rowOffStep = pitch & 15 in {0, 4, 8, 12}
    row blur, item (r, sg)       five dwords from the aligned dword of  column 0 + 10 sg
    centroid, item (r, j)        two dwords from the aligned dword of   column 0 + 6 + 4 j
    hb store, item (r, sg)       five dwords at  hb + 2 * (r * hb_pitch + 10 sg)

The bounds are for row pitches that are a multiple of 16 (every pyramid level, and level 0 of the usual image widths): blur reads at most 1.5-way
on average and 2-way at worst, the same for the centroid.  For the other three pitch classes the layout must be no worse than the one it replaces
(rows 64 bytes apart, centroid rows 8 consecutive per step), which is written out here and pinned at its 4-way / 2-way."""
import json
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

OFF0 = range(16)
STEPS = (0, 4, 8, 12)


@pytest.fixture(scope="module")
def lay(tmp_path_factory):
    hipcc = next((p for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if p and os.path.exists(p)), None)
    assert hipcc, "hipcc not found"
    tmp = tmp_path_factory.mktemp("describe_lds")
    out = str(tmp / "describe_lds_cpu")
    rocm_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "lib")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "--cuda-host-only", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "orb_ygz_slam_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "describe_lds_cpu.hip"), "-L", rocm_lib, "-lamdhip64", "-o", out])
    r = subprocess.run([out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return json.loads(r.stdout)


def group_costs(addr_of_lane):
    """addr_of_lane: {lane: byte address of the dword it accesses} of one wave instruction (inactive lanes absent) -> cost of every group that has a lane"""
    costs = []
    for group in (range(0, 32), range(32, 64)):
        banks = {}
        for lane in group:
            if lane in addr_of_lane:
                dword = addr_of_lane[lane] // 4
                banks.setdefault(dword % 32, set()).add(dword)
        if banks:
            costs.append(max(len(d) for d in banks.values()))
    return costs


def sweep(items, steps, first_byte, ndwords, row_offsets):
    """items[64 * step + lane] = (row, k, row's byte offset); first_byte(k) = the item's first byte past the row's column 0.
    -> {rowOffStep: (mean, worst)} over every rowOff0, step and dword"""
    out = {}
    for rstep in row_offsets:
        costs = []
        for off0 in OFF0:
            for s in range(steps):
                lanes = {}
                for lane in range(64):
                    if 64 * s + lane < len(items):
                        row, k, row_byte = items[64 * s + lane]
                        lanes[lane] = (row_byte + ((off0 + row * rstep) & 15) + first_byte(k)) & ~3
                for d in range(ndwords):
                    costs += group_costs({lane: a + 4 * d for lane, a in lanes.items()})
        out[rstep] = (sum(costs) / len(costs), max(costs))
    return out


def blur_ways(items, steps):
    return sweep(items, steps, lambda sg: 10 * sg, 5, STEPS)


def centroid_ways(items, steps):
    return sweep(items, steps, lambda j: 6 + 4 * j, 2, STEPS)


# the layout this one replaces: rows 64 bytes apart, blur item t -> row t >> 2, segment t & 3, centroid step s -> rows 6 + 8 s + (lane >> 3)
OLD_BLUR = [(t >> 2, t & 3, 64 * (t >> 2)) for t in range(172)]
OLD_CENTROID = [(6 + 8 * (i >> 6) + ((i & 63) >> 3), i & 7, 64 * (6 + 8 * (i >> 6) + ((i & 63) >> 3))) for i in range(256)]


@pytest.fixture(scope="module")
def ways(lay):
    w = {"blur": blur_ways([tuple(x) for x in lay["blur"]], lay["blur_steps"]), "centroid": centroid_ways([tuple(x) for x in lay["centroid"]], lay["centroid_steps"]),
         "old_blur": blur_ways(OLD_BLUR, 3), "old_centroid": centroid_ways(OLD_CENTROID, 4)}
    for name, v in w.items():
        print(name, {k: "%.3f-way mean, %d-way worst" % x for k, x in v.items()})
    return w


def test_the_model_gives_the_old_layout_its_four_way(ways):
    for rstep in STEPS:
        mean, worst = ways["old_blur"][rstep]
        assert worst == 4 and abs(mean - 11 / 3) < 1e-9      # five full groups 4-way, the sixth (rows 40..42) 2-way
        assert ways["old_centroid"][rstep] == (2.0, 2)


def test_reads_at_pitches_that_are_a_multiple_of_16(ways):
    mean, worst = ways["blur"][0]
    assert mean <= 1.5 and worst <= 2
    mean, worst = ways["centroid"][0]
    assert mean <= 1.5 and worst <= 2


@pytest.mark.parametrize("rstep", [4, 8, 12])
def test_reads_at_the_other_pitch_classes_are_no_worse_than_before(ways, rstep):
    for new, old in (("blur", "old_blur"), ("centroid", "old_centroid")):
        assert ways[new][rstep][0] <= ways[old][rstep][0] and ways[new][rstep][1] <= ways[old][rstep][1]


def test_items_cover_the_window_once_and_use_the_row_offsets(lay):
    rb = lay["row_byte"]
    blur = [tuple(x) for x in lay["blur"]]
    assert sorted((r, sg) for r, sg, _ in blur) == [(r, sg) for r in range(lay["win"]) for sg in range(4)]
    assert all(b == rb[r] for r, _, b in blur)
    cen = [tuple(x) for x in lay["centroid"]]
    assert sorted((r, j) for r, j, _ in cen) == [(r, j) for r in range(6, 38) for j in range(8)]      # rows 21 - 15 .. 21 + 15, and the empty row 37
    assert all(b == rb[r] for r, _, b in cen)


def test_rows_do_not_overlap_and_slots_match_them(lay):
    rb, span = lay["row_byte"], lay["span"]
    assert len(rb) == lay["win"] == 43 and rb[0] == 0
    assert all(b % 16 == 0 for b in rb)
    assert all(rb[r] + span <= rb[r + 1] for r in range(len(rb) - 1))
    assert rb[-1] + span + lay["raw_slack"] == lay["raw_bytes"]
    slots = lay["slot_item"]
    assert len(slots) == 3 * 64 and 16 * len(slots) + lay["raw_slack"] == lay["raw_bytes"]      # three LDS-DMA instructions
    data = [(s, it) for s, it in enumerate(slots) if it >= 0]
    assert [it for _, it in data] == list(range(4 * 43))
    assert all(16 * s == rb[it >> 2] + 16 * (it & 3) for s, it in data)


def test_per_wave_lds_and_the_overlay(lay):
    rb, front = lay["row_byte"], lay["hb_front"]
    assert lay["lds_bytes"] == front + lay["raw_bytes"] and lay["lds_bytes"] <= 5120      # 160 KB / 32 wave slots
    hb_row = 2 * lay["hb_pitch"]
    assert 43 * hb_row <= lay["lds_bytes"]
    # hb rows written in blur step s lie only over raw rows that earlier steps consumed; step 0's over none
    n = lay["blur_step_rows"]
    for s in range(lay["blur_steps"]):
        rows = [r for r, _, _ in lay["blur"][64 * s:64 * (s + 1)]]
        assert min(rows) == n * s and max(rows) == min(n * s + n, 43) - 1
        hb_end = hb_row * (max(rows) + 1)
        first_live = front + (rb[n * s] if s else 0)
        assert hb_end <= first_live


def test_hb_stores_stay_conflict_free(lay):
    costs = []
    for s in range(lay["blur_steps"]):
        lanes = {lane: 2 * (r * lay["hb_pitch"] + 10 * sg) for lane, (r, sg, _) in enumerate(lay["blur"][64 * s:64 * (s + 1)])}
        assert all(a % 4 == 0 for a in lanes.values())
        for d in range(5):
            costs += group_costs({lane: a + 4 * d for lane, a in lanes.items()})
    assert max(costs) == 1
