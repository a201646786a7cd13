#!/usr/bin/env python3
"""LDS cycles of describe_window's column pass, counted on the CPU (no GPU needed).

The column pass reads hb, the row-blurred 43 x kHbP window of u16 (csrc/describe_lds.h), at the rotated positions of the rBRIEF pattern: seven
reads per sampled point, rows r .. r + 6 of one column.  The bank rule is the header's: a read is served in two groups of 32 lanes, the bank of
byte address a is (a / 4) mod 32, lanes of a group that read the same dword share one access, and a group costs as many cycles as the most
distinct dwords it has on one bank.  So what a step costs depends on WHICH points its 64 lanes hold:

  pair order    lane l of step it samples both end points of test pair 64 it + l (the order of kBriefPattern): 512 samples in 8 half steps,
                each group's 32 points scattered over the whole patch.
  point order   lane l of step s samples point 64 s + l of kBriefPoint (csrc/orb_pattern_table.h, written by tools/gen_pattern.py): the 375
                distinct points once, in tile order, so that a group's 32 points are a compact cluster at any angle -- neighbouring columns
                share a dword, neighbouring rows lie kHbP / 2 = 20 banks apart.  The lanes store the blurred bytes at val[slot] and the
                pairs read their two bytes back (compare reads).

Everything is read from the committed headers: the pattern, the point table and the pair slots from orb_pattern_table.h, kHbP, kWin and the
place of val from describe_lds.h.  The rotation is the kernel's: float32 products and sums without contraction, round half to even.

    python tools/describe_column_banks.py            the table: mean / p95 / max cycles per keypoint over 200 seeded angles and the axis angles
    python tools/describe_column_banks.py --search   the same for other tile shapes and Morton order (how gen_pattern.TILE was chosen)
"""
import math
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc")
TAPS = 7
HB_CENTRE = 18                                   # hb row / column of the keypoint's first tap row and its own column (describe_window)


def _ints(text, name):
    body = text[re.search(r"\b%s\[\d+\] = \{" % name, text).end():]
    return [int(v) for v in re.findall(r"-?\d+", body[:body.index("}")])]


def load_tables():
    """-> dict: pattern (1024), points [(x, y)] * slots, count, pairs [(i0, i1)] * 256, hbp, win, val_byte, lds_bytes, hb_bytes"""
    pat = open(os.path.join(CSRC, "orb_pattern_table.h")).read()
    lds = open(os.path.join(CSRC, "describe_lds.h")).read()

    def const(name):
        return int(re.search(r"\b%s\s*=\s*(\d+)" % name, lds).group(1))
    pts = _ints(pat, "kBriefPoint")
    pr = _ints(pat, "kBriefPairPoint")
    t = {"pattern": _ints(pat, "kBriefPattern"), "points": list(zip(pts[0::2], pts[1::2])), "pairs": list(zip(pr[0::2], pr[1::2])),
         "count": int(re.search(r"kBriefPointCount\s*=\s*(\d+)", pat).group(1)), "slots": int(re.search(r"kBriefPointSlots\s*=\s*(\d+)", pat).group(1)),
         "hbp": const("kHbP"), "win": const("kWin"), "val_byte": const("kDescValByte")}
    t["hb_bytes"] = t["win"] * t["hbp"] * 2
    return t


def angles(n=200, seed=20):
    """the fixed set: n seeded angles in [0, 360) and the four axis angles"""
    rng = np.random.default_rng(seed)
    return [float(np.float32(a)) for a in rng.uniform(0.0, 360.0, n)] + [0.0, 90.0, 180.0, 270.0]


def rotate(points, angle_deg):
    """the kernel's rotation and rounding of pattern points (x, y) -> (row offsets r, column offsets q), int arrays"""
    rad = float(np.float32(angle_deg) * np.float32(math.pi / 180.0))
    a, b = np.float32(math.cos(rad)), np.float32(math.sin(rad))
    p = np.asarray(points, np.float32)
    x, y = p[:, 0], p[:, 1]
    r = np.rint(x * b + y * a).astype(np.int64)
    q = np.rint(x * a - y * b).astype(np.int64)
    return r, q


def group_cost(byte_addrs):
    """cycles of one group of up to 32 lanes"""
    banks = {}
    for a in byte_addrs:
        dword = int(a) // 4
        banks.setdefault(dword % 32, set()).add(dword)
    return max(len(d) for d in banks.values()) if banks else 0


def sample_addresses(points, angle_deg, hbp):
    """byte address in hb of the first tap of every point: u16 at row 18 + r, column 18 + q; tap k is k rows further down"""
    r, q = rotate(points, angle_deg)
    return 2 * ((HB_CENTRE + r) * hbp + HB_CENTRE + q)


def sample_cost(points, angle_deg, hbp):
    """LDS cycles per keypoint of the seven tap reads when lane l of step s holds points[64 s + l]"""
    first = sample_addresses(points, angle_deg, hbp)
    cost = 0
    for g in range(0, len(points), 32):
        for k in range(TAPS):
            cost += group_cost(first[g:g + 32] + 2 * hbp * k)
    return cost


def pair_order_points(pattern):
    """the parent's lane order as a point list: half step (it, end) holds end point `end` of pairs 64 it .. 64 it + 63"""
    out = []
    for it in range(4):
        for end in range(2):
            out += [(pattern[4 * p + 2 * end], pattern[4 * p + 2 * end + 1]) for p in range(64 * it, 64 * it + 64)]
    return out


def compare_cost(pairs, val_byte):
    """LDS cycles per keypoint of the byte reads val[i0], val[i1] of pair 64 it + lane"""
    cost = 0
    for g in range(0, len(pairs), 32):
        for end in range(2):
            cost += group_cost([val_byte + p[end] for p in pairs[g:g + 32]])
    return cost


def store_cost(slots, val_byte):
    """LDS-array cycles per keypoint of the byte stores val[64 s + lane]"""
    return sum(group_cost(range(val_byte + g, val_byte + g + 32)) for g in range(0, slots, 32))


def stats(costs):
    c = np.asarray(costs, float)
    return float(c.mean()), float(np.percentile(c, 95)), float(c.max())


def morton_order(pts):
    def key(p):
        x, y, k = p[0] + 13, p[1] + 13, 0
        for b in range(5):
            k |= ((x >> b) & 1) << (2 * b) | ((y >> b) & 1) << (2 * b + 1)
        return k
    return sorted(pts, key=key)


def main():
    t = load_tables()
    ang = angles()
    rows = [("pair order: 512 samples, 8 steps (floor %d)" % (2 * TAPS * 8), pair_order_points(t["pattern"])),
            ("point order: %d points, %d steps (floor %d)" % (t["count"], t["slots"] // 64, 2 * TAPS * t["slots"] // 64), t["points"])]
    if "--search" in sys.argv:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import gen_pattern
        pad = lambda o: o + [o[-1]] * (t["slots"] - len(o))
        for tile in ((3, 8), (4, 8), (6, 6), (8, 3), (8, 4), (7, 4), (9, 3), (10, 3), (14, 2), (3, 27), (27, 3)):
            rows.append(("tiles of %d rows x %d columns" % tile, pad(gen_pattern.point_order(t["pattern"], tile))))
        rows.append(("Morton order", pad(morton_order(sorted(set(t["points"]))))))
    print("LDS cycles per keypoint, %d angles (kHbP = %d)" % (len(ang), t["hbp"]))
    print("%-52s %8s %8s %8s" % ("sample reads", "mean", "p95", "max"))
    for name, pts in rows:
        print("%-52s %8.1f %8.1f %8.0f" % ((name,) + stats([sample_cost(pts, a, t["hbp"]) for a in ang])))
    print("point order, compare reads (2 bytes per pair, floor 16)  %d" % compare_cost(t["pairs"], t["val_byte"]))
    print("point order, byte stores                                  %d" % store_cost(t["slots"], t["val_byte"]))


if __name__ == "__main__":
    main()
