"""What share of the keypoints that k_match_last's speculative scan visits passes the filters in front of the descriptor distance?  CPU only:
the oracle's extractor on the first frames of bench.py's make_frames clip, then the matcher's window arithmetic restated in numpy
(cell_window of match_rules.h, Frame::AssignFeaturesToGrid's rounding) for SearchByProjection(Cur, Last) as ygzf_match_batch_prev calls it:
identity pose, unit-depth world points (a Last keypoint projects onto itself), th = 15, mono, check_level, nobody owned at the start.

  visited: every keypoint of the query's cell window (columns minCx..maxCx, rows minCy..maxCy)
  passing: of those, the ones on octaves oct-1 .. oct+1 inside the box |dx| < r and |dy| < r, r = th * scale[oct]

    python tools/match_pass_ratio.py [--frames 16] [--json out.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRID_COLS, GRID_ROWS = 64, 48


def count_pair(cur, last, scale, w, h, th=15.0, check_level=True):
    """-> per Last keypoint: (octave, visited, after level, after level + radius)"""
    f = np.float32
    inv_w, inv_h = f(GRID_COLS) / f(w), f(GRID_ROWS) / f(h)
    x, y, o = cur["x"].astype(f), cur["y"].astype(f), cur["octave"].astype(np.int64)
    px = np.floor(x * inv_w + f(0.5)).astype(np.int64)          # roundf of a non-negative value
    py = np.floor(y * inv_h + f(0.5)).astype(np.int64)
    ingrid = (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)
    out = np.zeros((len(last), 4), np.int64)
    for i, k in enumerate(last):
        u, v, oct_ = f(k["x"]), f(k["y"]), int(k["octave"])
        r = f(th) * scale[oct_]
        x0, x1 = max(0, int(np.floor((u - r) * inv_w))), min(GRID_COLS - 1, int(np.ceil((u + r) * inv_w)))
        y0, y1 = max(0, int(np.floor((v - r) * inv_h))), min(GRID_ROWS - 1, int(np.ceil((v + r) * inv_h)))
        vis = ingrid & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        lvl = vis & (o >= oct_ - 1) & (o <= oct_ + 1) if check_level else vis
        box = lvl & (np.abs(x - u) < r) & (np.abs(y - v) < r)
        out[i] = (oct_, vis.sum(), lvl.sum(), box.sum())
    return out


def wave_steps(cur, last, scale, w, h, th=15.0, queues=(1, 2, 4, 8, 16)):
    """Steps a wave of k_match_last's scan takes over one pair under the kernel's lane plan for one workgroup per pair (sixteen waves, runs of
    queries of equal weight scale^2, 64 / g lanes per query, lane qr takes every (64 / g)-th entry of each grid column of the window).
    A step = all lanes of the wave move one keypoint.  -> per form, summed over the pair's waves:
      nested     the loops `for column: for entry`: per column ordinal as many steps as the fullest lane
      flat       the walk as per-lane state (column, entry): as many steps as the busiest lane visits
      stop_next  every lane stops at its next passing keypoint until all have one, then they are scored: (walk steps, score steps)
      queue d    flat walk; the wave scores when one lane holds d passing keypoints or the walk is over: score steps (the walk is `flat`)"""
    f = np.float32
    inv_w, inv_h = f(GRID_COLS) / f(w), f(GRID_ROWS) / f(h)
    x, y, o = cur["x"].astype(f), cur["y"].astype(f), cur["octave"].astype(np.int64)
    px = np.floor(x * inv_w + f(0.5)).astype(np.int64)
    py = np.floor(y * inv_h + f(0.5)).astype(np.int64)
    wgt = np.array([max(1, int(scale[int(k["octave"])] * scale[int(k["octave"])] * f(16))) for k in last])
    ws, n_use = np.cumsum(wgt), 16
    bounds = [int(np.searchsorted(ws, int(ws[-1]) * k // n_use, side="right")) for k in range(n_use)] + [len(last)]
    out = {"waves": 0, "nested": 0, "flat": 0, "stop_next": [0, 0], "queue": {d: 0 for d in queues}}
    for wv in range(n_use):
        jb, je = bounds[wv], bounds[wv + 1]
        g = 1
        while g < je - jb and g < 64:
            g <<= 1
        lpq = 64 // g
        cols = []                                   # per lane: per grid column of its query's window, the pass flags of its entries
        for lane in range(64):
            j, qr = jb + lane // lpq, lane % lpq
            if j >= je:
                continue
            k = last[j]
            u, v, oc = f(k["x"]), f(k["y"]), int(k["octave"])
            r = f(th) * scale[oc]
            x0, x1 = max(0, int(np.floor((u - r) * inv_w))), min(GRID_COLS - 1, int(np.ceil((u + r) * inv_w)))
            y0, y1 = max(0, int(np.floor((v - r) * inv_h))), min(GRID_ROWS - 1, int(np.ceil((v + r) * inv_h)))
            lane_cols = []
            for cx in range(x0, x1 + 1):
                idx = np.nonzero((px == cx) & (py >= y0) & (py <= y1))[0]
                idx = idx[np.lexsort((idx, py[idx]))][qr::lpq]
                lane_cols.append(list((np.abs(o[idx] - oc) <= 1) & (np.abs(x[idx] - u) < r) & (np.abs(y[idx] - v) < r)))
            cols.append(lane_cols)
        flat = [[b for c in lc for b in c] for lc in cols]
        if not any(flat):
            continue
        out["waves"] += 1
        out["nested"] += sum(max((len(lc[c]) for lc in cols if len(lc) > c), default=0) for c in range(max(len(lc) for lc in cols)))
        out["flat"] += max(len(t) for t in flat)
        pos = [0] * len(flat)                       # stop_next
        while any(p < len(t) for p, t in zip(pos, flat)):
            gap, found = 0, False
            for i, t in enumerate(flat):
                p = pos[i]
                while p < len(t) and not t[p]:
                    p += 1
                if p < len(t):
                    p, found = p + 1, True
                gap, pos[i] = max(gap, p - pos[i]), p
            out["stop_next"][0] += gap
            out["stop_next"][1] += int(found)
        for d in queues:
            held, steps = [0] * len(flat), 0
            for s in range(max(len(t) for t in flat)):
                for i, t in enumerate(flat):
                    if s < len(t) and t[s]:
                        held[i] += 1
                if max(held) >= d:
                    steps, held = steps + max(held), [0] * len(flat)
            out["queue"][d] += steps + max(held)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--json", default=None)
    ap.add_argument("--waves", type=int, default=0, metavar="PAIRS", help="also model the steps per wave of the scan's forms on the first PAIRS pairs")
    a = ap.parse_args()
    import bench
    from oracle import oracle_py as O
    w, h, nl, sf, nf, ini, mn = bench.WORKLOADS["euroc752x480_8lvl_1000feat"]
    frames = bench.make_frames(a.frames, w, h)
    ex = O.Extractor(nf, sf, nl, ini, mn)
    scale = np.asarray(ex.tables()["scale"], np.float32)
    keys = [ex.extract(fr)[0] for fr in frames]
    rows = np.concatenate([count_pair(keys[i], keys[i - 1], scale, w, h) for i in range(1, len(keys))])
    res = {"workload": "euroc752x480_8lvl_1000feat", "frames": a.frames, "pairs": a.frames - 1, "th": 15, "check_level": True, "mono": True,
           "queries": int(len(rows)), "visited": int(rows[:, 1].sum()), "pass_level": int(rows[:, 2].sum()), "pass_all": int(rows[:, 3].sum()),
           "pass_ratio": round(float(rows[:, 3].sum()) / float(rows[:, 1].sum()), 4),
           "visited_per_query": round(float(rows[:, 1].mean()), 2), "passing_per_query": round(float(rows[:, 3].mean()), 2), "per_octave": {}}
    for o in range(nl):
        m = rows[rows[:, 0] == o]
        if len(m):
            res["per_octave"][str(o)] = {"queries": int(len(m)), "visited": int(m[:, 1].sum()), "pass_level": int(m[:, 2].sum()),
                                         "pass_all": int(m[:, 3].sum()), "pass_ratio": round(float(m[:, 3].sum()) / max(1.0, float(m[:, 1].sum())), 4),
                                         "visited_per_query": round(float(m[:, 1].mean()), 2)}
    if a.waves:
        tot = None
        for i in range(1, min(a.waves, len(keys) - 1) + 1):
            s = wave_steps(keys[i], keys[i - 1], scale, w, h)
            if tot is None:
                tot = s
            else:
                tot = {"waves": tot["waves"] + s["waves"], "nested": tot["nested"] + s["nested"], "flat": tot["flat"] + s["flat"],
                       "stop_next": [p + q for p, q in zip(tot["stop_next"], s["stop_next"])], "queue": {d: tot["queue"][d] + s["queue"][d] for d in s["queue"]}}
        n = float(tot["waves"])
        res["steps_per_wave"] = {"pairs": min(a.waves, len(keys) - 1), "waves": tot["waves"], "nested": round(tot["nested"] / n, 1), "flat": round(tot["flat"] / n, 1),
                                 "stop_next_walk": round(tot["stop_next"][0] / n, 1), "stop_next_score": round(tot["stop_next"][1] / n, 1),
                                 "queue_score": {str(d): round(v / n, 1) for d, v in tot["queue"].items()}}
    print(json.dumps(res, indent=1))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
