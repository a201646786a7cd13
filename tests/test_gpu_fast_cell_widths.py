"""FAST pass 1 on cells of every kind of width.  A lane of pass 1 finds its quad (row y, column q of the cell's nq = (dw + 3) >> 2 quads per row) by
one of two walks (orb_ygz_slam_amd/csrc/fast_lane_quads.h): with a fixed column where nq divides 64 -- every full cell 29 .. 32 px wide has
nq = 8 --, with a stepped (y, q) otherwise; tests/test_fast_lane_quads_cpu.py compares the walks on the CPU.  Here the kernels run them: the image
widths are chosen by level 0's cell geometry (the reference's: 30-px cells over width - 32, the last column clipped at the border) so that
  full cells are 30, 31 and 32 px wide (fixed column, last-quad masks of 2, 3 and 4 pixels) and, in two sizes, 35 and 40 px (nq = 9, 10: stepped);
  the clipped last column is 1, 5, 13 and 29 px wide (nq = 1, 2, 4, 8: fixed column; 29 is the last-quad mask of one pixel) and 17, 23, 24 and 32 px
  (nq = 5, 6, 6, 8).
Wide and low images reach the narrow last columns with few pixels (dw = 1 needs 25 columns); the upper pyramid levels bring further widths.  One
context, 1 and 3 frames, 8 levels at 1.2, frames from synth_frame.  Candidates (x, y, score, order) of every level are compared with the oracle
under both threshold plans, through k_fast_tab (every cell here is at most 41 px wide), through k_fast_tab with the persistent loop forced, and
with every size forced through k_fast_quads."""
import math

import numpy as np
import pytest

from orb_ygz_slam_amd.synth import synth_frame

pytestmark = pytest.mark.gpu

# (width, height) -> level 0's (full cell width, last column's width)
SIZES = {(152, 100): (30, 24), (185, 100): (31, 23), (303, 100): (31, 17), (423, 100): (31, 13), (663, 100): (31, 5), (783, 100): (31, 1),
         (160, 160): (32, 26), (172, 100): (35, 29), (150, 100): (40, 32)}
NFRAMES = 3


def level0_cells(w):
    """dw of level 0's cells from left to right, as the reference cuts them (ComputeKeyPointsOctTree)"""
    width = w - 32
    ncols = int(width / 30.0)
    wcell = math.ceil(width / ncols)
    out = []
    for j in range(ncols):
        ini = 16 + j * wcell
        if ini >= w - 16 - 6:
            continue
        out.append(min(ini + wcell + 6, w - 16) - ini - 6)
    return out


def test_the_sizes_give_the_cell_widths_they_are_chosen_for():
    full, last = set(), set()
    for (w, _), (wc, wl) in SIZES.items():
        cells = level0_cells(w)
        assert set(cells[:-1]) == {wc} and cells[-1] == wl and max(cells) <= 41
        full.add(wc)
        last.add(wl)
    assert {30, 31, 32} <= full and {1, 5, 13, 17, 23, 29} <= last
    nq = {(d + 3) >> 2 for d in full | last}
    assert {1, 2, 4, 8} <= nq and {5, 6, 9, 10} <= nq      # both walks


_expected = {}


def expected(oracle, w, h):
    """frames and, per frame, the oracle's candidates of every level: computed once per size and shared"""
    if (w, h) not in _expected:
        frames = np.stack([synth_frame(1700 + w + i, w, h) for i in range(NFRAMES)])
        frames.setflags(write=False)
        oex = oracle.Extractor(500, 1.2, 8, 20, 7)
        cands = []
        for f in range(NFRAMES):
            oex.extract(frames[f])
            cands.append([oex.cell_candidates(l) for l in range(8)])
        _expected[(w, h)] = (frames, cands)
    return _expected[(w, h)]


def check(ex, frames, cands, what):
    for plan in (1, 2):
        ex.set_fast_plan(plan)
        for n in (1, NFRAMES):
            ex.extract_batch_host(frames[:n])
            for f in range(n):
                for l in range(8):
                    xs, ys, sc = cands[f][l]
                    gx, gy, gs = ex.batch_fetch_candidates(f, l)
                    assert len(gx) == len(xs), (what, plan, n, f, l, len(gx), len(xs))
                    assert np.array_equal(gx, xs) and np.array_equal(gy, ys) and np.array_equal(gs, sc), (what, plan, n, f, l)


@pytest.mark.parametrize("w,h", sorted(SIZES))
@pytest.mark.parametrize("path", ["tab", "tab_persist", "quads"])
def test_candidates_equal_the_oracle(oracle, monkeypatch, w, h, path):
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import force_env
    frames, cands = expected(oracle, w, h)
    assert sum(len(c[0][0]) for c in cands) > 50                       # level 0 has corners to list
    if path == "tab_persist":
        monkeypatch.setenv("YGZF_FORCE", force_env(fast_persist=1))     # (read when the context is created)
    ex = Extractor(500, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=NFRAMES)
    ex.set_fast_kernel(1 if path == "quads" else 2)
    check(ex, frames, cands, (w, h, path))
    ex.close()
