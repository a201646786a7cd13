"""tools/fuse_rate.py -- what ORBmatcher::Fuse costs on the CPU and what ygzf_fuse_candidates takes, on the two shapes of
LocalMapping::SearchInNeighbors.  Prints one JSON line.

  forward: 20 distinct targets x 1 500 points, ~1.7 k keys per keyframe (src/LocalMapping.cc:1259-1269).  The device call gets the 20 distinct
           rows FuseBatch sends; the CPU loop runs the 30 targets the reference visits (10 duplicates).
  reverse: 1 keyframe x 30 000 points (:1273-1304).

device_us:    median wall time of one ygzf_fuse_candidates call (copies in and out included) over --calls calls, ctypes arguments prepared once.
cpu_ms:       single-thread median of the sequential Fuse loop of tests/cpp/fuse_restate.h (the reference's order, map updates included) on a
              synthetic map of the same shape (tests/cpp/fuse_shell.cc, built here with g++ -O2 against libygzf).
fusebatch_ms: median of ygz::FuseBatch on copies of that same map, end to end: packing, every device call (the re-search of Replace
              survivors included), the host application.  same_graph: its final map equals the CPU loop's.
Runs on the GPU machine:  timeout -k 10 600 python tools/fuse_rate.py
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_ygz_slam_amd.capi import KP_DTYPE, Extractor, FuseKf, FusePoints, FrameView, _p  # noqa: E402
from orb_ygz_slam_amd.fuse_scene import _rot, make_kf, make_points  # noqa: E402


def device_call(ex, kfs, pts):
    """ctypes arguments of one ygzf_fuse_candidates call, prepared once; returns a zero-argument callable."""
    keep = []
    arr = (FuseKf * len(kfs))()
    for k, kf in enumerate(kfs):
        ck, cd = np.ascontiguousarray(kf["keys"], KP_DTYPE), np.ascontiguousarray(kf["desc"], np.uint8)
        u = None if kf["u_right"] is None else np.ascontiguousarray(kf["u_right"], np.float32)
        sf, ig = kf["scale_factors"], kf["inv_level_sigma2"]
        keep.extend([ck, cd, u, sf, ig])
        f = arr[k]
        f.view = FrameView(len(ck), ck.ctypes.data, cd.ctypes.data, None if u is None else u.ctypes.data, sf.ctypes.data, len(sf))
        f.cam = kf["cam"]
        f.inv_level_sigma2 = ig.ctypes.data
        f.Rcw[:] = [float(x) for x in kf["Rcw"].reshape(9)]
        f.tcw[:] = [float(x) for x in kf["tcw"]]
        f.Ow[:] = [float(x) for x in kf["Ow"]]
        f.log_scale_factor = float(kf["log_scale_factor"])
    w, nr, mx, mn, mf, d = (np.ascontiguousarray(a) for a in pts)
    keep.extend([w, nr, mx, mn, mf, d])
    fp = FusePoints(w.ctypes.data, nr.ctypes.data, mx.ctypes.data, mn.ctypes.data, mf.ctypes.data, d.ctypes.data)
    K, P = len(kfs), len(w)
    bi = np.zeros((K, P), np.int32)
    bd = np.zeros((K, P), np.int32)
    keep.extend([bi, bd])
    fn, h, pbi, pbd = ex.L.ygzf_fuse_candidates, ex.h, _p(bi), _p(bd)
    ref = C.byref(fp)

    def call():
        rc = fn(h, K, arr, P, ref, None, 3.0, pbi, pbd)
        assert rc == 0, ex.L.ygzf_last_error(h)
        return keep
    return call, bi


def median_us(call, n):
    for _ in range(10):
        call()
    t = []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "fuse_shell")
        host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
        lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
        srcs = [os.path.join(ROOT, "tests", "cpp", "fuse_shell.cc")] + [os.path.join(host, f) for f in
                                                                      ("ORBextractor.cc", "ORBmatcher.cc", "ORBmatcherFuse.cc", "ygzf_pool.cc")]
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                               "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
        cpu_fwd = json.loads(subprocess.check_output([exe, "time", "20", "4000", "1500", "10", "5"], text=True))
        cpu_rev = json.loads(subprocess.check_output([exe, "time", "20", "35000", "30000", "-1", "5"], text=True))
    ex = Extractor(1000, 1.2, 8, 20, 7, 752, 480)
    rng = np.random.default_rng(3)
    kfs = [make_kf(rng, 752, 480, 1700, 8, 1.2, _rot(*rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.3, 0.3, 3), mbf=40.0 if k % 2 == 0 else 0.0,
                   stereo_frac=0.5) for k in range(20)]
    pts = make_points(rng, kfs, 1500)
    call, bi = device_call(ex, kfs, pts)
    fwd_us = median_us(call, args.calls)
    out["forward"] = dict(kfs=20, points=1500, keys_per_kf=1700, device_us=round(fwd_us, 1), found=int((bi >= 0).sum()),
                          cpu_ms=cpu_fwd["cpu_ms"], fusebatch_ms=cpu_fwd["fusebatch_ms"], same_graph=cpu_fwd["same_graph"],
                          cpu_targets=cpu_fwd["targets"], cpu_points=cpu_fwd["points"],
                          cpu_keys_per_kf=cpu_fwd["keys_per_kf"])
    kf = make_kf(rng, 752, 480, 2000, 8, 1.2, np.eye(3), [0, 0, 0], mbf=40.0, stereo_frac=0.5)
    pts = make_points(rng, [kf], 30000)
    call, bi = device_call(ex, [kf], pts)
    rev_us = median_us(call, args.calls)
    out["reverse"] = dict(kfs=1, points=30000, keys_per_kf=2000, device_us=round(rev_us, 1), found=int((bi >= 0).sum()),
                          cpu_ms=cpu_rev["cpu_ms"], fusebatch_ms=cpu_rev["fusebatch_ms"], same_graph=cpu_rev["same_graph"],
                          cpu_targets=cpu_rev["targets"], cpu_points=cpu_rev["points"],
                          cpu_keys_per_kf=cpu_rev["keys_per_kf"])
    ex.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
