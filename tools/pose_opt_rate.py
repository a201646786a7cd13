"""tools/pose_opt_rate.py -- what Optimizer::PoseOptimization(Frame *) on the device costs (ygzf_pose_optimization: upload, one launch of
k_pose_opt, download, one synchronisation).  Writes a small text table (default profiles/pose_opt_rate.txt) and prints it.  Report only: no
threshold -- nobody has measured this step before, the file records what is found.

  (a) one call of 1 problem at 200, 1000 and 2000 correspondences;
  (b) one call of 8, 64 and 256 problems at 1000 correspondences each (per call and per problem).
  (c) beside them, on the same host: the numpy restatement of the same algorithm (tests/pose_opt_cases.py, one thread) on the same problems.
      That is NOT g2o -- the reference's g2o cannot be built here for want of Eigen -- and numpy's per-call overhead dominates it: it bounds
      nothing about the reference, it only says what this machine does with a plain evaluation of the same arithmetic.
Every device figure: median [fastest .. slowest] of the timed windows, one untimed window first; the host clock around calls that synchronise.
Runs on the GPU machine:  timeout -k 10 600 python tools/pose_opt_rate.py
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def windows(fn, n_windows, per_window):
    """us per call of fn (every call synchronises): n_windows timed windows of per_window calls; one untimed window first"""
    out = []
    for k in range(-1, n_windows):
        t0 = time.perf_counter()
        for _ in range(per_window):
            fn()
        if k >= 0:
            out.append((time.perf_counter() - t0) * 1e6 / per_window)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_opt_rate.txt"))
    args = ap.parse_args()
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import KP_DTYPE, Camera
    from tests import pose_opt_cases as PC

    def as_dict(P):
        n = len(P.octave)
        keys = np.zeros(n, KP_DTYPE)
        keys["x"], keys["y"], keys["octave"] = P.xy[:, 0], P.xy[:, 1], P.octave
        return dict(keys=keys, u_right=P.u_right, mp_valid=P.mp_valid, world=P.world, Tcw=P.Tcw, outlier=P.outlier_in)
    fx, fy, cx, cy, bf = PC.EUROC
    cam = Camera(fx, fy, cx, cy, 0.0, bf, 0.0, 0.0, 752.0, 480.0)
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=1)
    f3 = lambda t: "%9.1f [%9.1f .. %9.1f]" % t
    lines = ["Optimizer::PoseOptimization(Frame *) on the device (tools/pose_opt_rate.py): us, median [fastest .. slowest] of %d windows of %d calls" % (
        args.windows, args.calls), "seeded scenes of tests/pose_opt_cases.py: 20 % outliers, half the correspondences stereo", ""]
    lines.append("(a) one call, one problem                      us per call          iterations / trials of the four rounds")
    for n in (200, 1000, 2000):
        P = PC.scene(4000 + n, n, frac_out=0.2)
        d = as_dict(P)
        r = ex.pose_optimization(cam, [d], PC.INV_SIGMA2)[0]
        t = windows(lambda: ex.pose_optimization(cam, [d], PC.INV_SIGMA2), args.windows, args.calls)
        t0 = time.perf_counter()
        ref = PC.pose_opt(P, "device")
        host = (time.perf_counter() - t0) * 1e6
        assert r["ret"] == ref.ret, (r["ret"], ref.ret)
        lines.append("    n = %4d   device %s   %s / %s   | numpy restatement on this host, one thread (not g2o): %.0f us" % (
            n, f3(t), r["iterations"], r["trials"], host))
    lines += ["", "(b) one call, B problems of 1000                us per call                          us per problem"]
    for B in (8, 64, 256):
        ds = [as_dict(PC.scene(7000 + k, 1000, frac_out=0.2)) for k in range(B)]
        ex.pose_optimization(cam, ds, PC.INV_SIGMA2)
        t = windows(lambda: ex.pose_optimization(cam, ds, PC.INV_SIGMA2), args.windows, max(2, args.calls // 4))
        lines.append("    B = %4d   device %s   %9.1f" % (B, f3(t), t[0] / B))
    lines += ["", "(the per-call figures include the Python binding's packing of the arrays, a few microseconds per problem)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
