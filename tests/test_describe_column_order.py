"""describe_window's column pass on the CPU: the committed point table (csrc/orb_pattern_table.h) against the pattern it is made from, the
addresses its sample steps read, and what those reads cost in LDS cycles under the bank rule of csrc/describe_lds.h.  The functions are the
ones of tools/describe_column_banks.py; the cost of the parent's lane order (lane l of step it takes pair 64 it + l) is computed here from
kBriefPattern alone."""
import importlib.util
import os

import pytest

from tests.conftest import ROOT


@pytest.fixture(scope="module")
def B():
    spec = importlib.util.spec_from_file_location("describe_column_banks", os.path.join(ROOT, "tools", "describe_column_banks.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def T(B):
    return B.load_tables()


def test_every_pair_finds_its_own_coordinates(T):
    pat, pts, pairs = T["pattern"], T["points"], T["pairs"]
    assert len(pat) == 1024 and len(pairs) == 256
    for p, (i0, i1) in enumerate(pairs):
        assert i0 < T["count"] and i1 < T["count"]
        assert pts[i0] + pts[i1] == tuple(pat[4 * p:4 * p + 4]), p


def test_the_points_are_the_375_distinct_ones_padded_with_the_last(T):
    pat, pts = T["pattern"], T["points"]
    assert T["count"] == 375 and T["slots"] == 384 == len(pts)
    assert len(set(pts[:375])) == 375 and set(pts[:375]) == {(pat[i], pat[i + 1]) for i in range(0, 1024, 2)}
    assert all(p == pts[374] for p in pts[375:])


def test_val_starts_behind_hb(T):
    """(that it ends inside the wave's LDS is a static_assert of the header, which knows kDescLdsBytes)"""
    assert T["val_byte"] >= T["hb_bytes"] and T["val_byte"] % 4 == 0


def test_every_sample_address_lies_inside_hb(B, T):
    """all seven taps of every slot (the padding included), at every whole angle"""
    hbp, win = T["hbp"], T["win"]
    for angle in range(360):
        r, q = B.rotate(T["points"], float(angle))
        assert (18 + r).min() >= 0 and (18 + r + 6).max() < win, angle
        assert (18 + q).min() >= 0 and (18 + q).max() < 37, angle      # kHb columns hold blurred values
        first = B.sample_addresses(T["points"], float(angle), hbp)
        assert first.min() >= 0 and (first + 2 * hbp * 6 + 2).max() <= T["hb_bytes"], angle


def test_sample_reads_cost_at_most_0_55_of_the_pair_order(B, T):
    ang = B.angles(200, seed=20)[:200]
    assert len(ang) == 200
    old_pts = B.pair_order_points(T["pattern"])
    assert len(old_pts) == 512
    old = sum(B.sample_cost(old_pts, a, T["hbp"]) for a in ang) / len(ang)
    new = sum(B.sample_cost(T["points"], a, T["hbp"]) for a in ang) / len(ang)
    print("mean LDS cycles per keypoint of the sample reads: pair order %.1f, committed point order %.1f, ratio %.3f" % (old, new, new / old))
    assert old >= 2 * 7 * 8 and new >= 2 * 7 * 6      # the floors: groups x taps x steps
    assert new <= 0.55 * old
