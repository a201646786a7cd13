"""tools/triangulate_rate.py -- what the per-pair body of LocalMapping::CreateNewMapPoints costs on the device (ygzf_triangulate_pairs: one packed
upload, one launch of k_triangulate, one download, one synchronisation) beside the same text (csrc/tri_math.h) on one host thread.  Writes a small
text table (default profiles/triangulate_rate.txt) and prints it.  Nobody has measured this step before: the file records what is found, and
the crossover it shows is where a shell's host threshold belongs.

  neighbours x pairs: 1 x 100, 1 x 300, 10 x 300, 20 x 300, 20 x 1000 -- seeded stereo scenes of tests/triangulate_cases.py, every neighbour a
  keyframe of its own over KF1's cloud
  device, one call      the C call on records packed once (what a C++ shell pays per call), host clock around the synchronising call
  device, binding       the same through the Python binding, which packs the records on every call
  device, per neighbour one C call per neighbour
  host                  tests/cpp/tri_host.cc, g++ -O2 -ffp-contract=off, one thread, every pair of every neighbour
  whole loop            the neighbour loop of CreateNewMapPoints end to end, searches and map updates included, over the stand-alone classes
                        (tests/cpp/tri_shell.cc: every neighbour matches KF1's features through ORBmatcher::SearchForTriangulation, one device call
                        per neighbour): ygz::CreateNewMapPointsBatch; the same loop neighbour by neighbour with one triangulation call each; and
                        CreateNewMapPointsBatch with the triangulation forced onto the host thread
Every figure: us, median [fastest .. slowest] of 9 timed windows, one untimed window first.
Runs on the GPU machine:  timeout -k 10 600 python tools/triangulate_rate.py
"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "orb_ygz_slam_amd")
SIZES = ((1, 100), (1, 300), (10, 300), (20, 300), (20, 1000))


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
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate_rate.txt"))
    args = ap.parse_args()
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import Camera, TriProblem
    from tests import triangulate_cases as TC

    def api_kf(kf):
        d = {k: kf.get(k) for k in ("keys", "u_right", "depth", "cos_stereo", "scale_factors", "level_sigma2", "Rcw", "tcw", "Ow", "Twc_q", "Twc_t", "invfx", "invfy")}
        d["cam"] = Camera(*[float(kf[k]) for k in ("fx", "fy", "cx", "cy", "mb", "mbf")], 0, 0, 0, 0)
        return d
    tmp = tempfile.mkdtemp(prefix="tri_rate")
    host = os.path.join(tmp, "tri_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "cpp", "tri_host.cc"), "-o", host])
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=1)
    f3 = lambda t: "%8.1f [%8.1f .. %8.1f]" % t
    lines = ["LocalMapping::CreateNewMapPoints, the per-pair body, on the device (tools/triangulate_rate.py): us per call, median [fastest .. slowest] of %d windows of %d calls"
             % (args.windows, args.calls), "copies and the synchronisation included; seeded stereo scenes of tests/triangulate_cases.py (6 in 10 features stereo, 1 pair in 10 a mismatch)",
             "host: the same text (csrc/tri_math.h) as a plain one-thread program, g++ -O2 -- NOT the reference's Eigen code", "",
             "neigh. x pairs   accepted   device, one call             device, binding              device, one call per neigh.  host, one thread             host / device"]
    rows = {}
    for B, n in SIZES:
        k1, problems, ratio = TC.make_scene(5000 + 37 * B + n, n, True, B)
        k1d = api_kf(k1)
        pd = [dict(kf2=api_kf(k2), idx1=i1, idx2=i2) for k2, i1, i2 in problems]
        got = ex.triangulate_pairs(k1d, ratio, pd)
        accepted = sum(int((s & 15 == 0).sum()) for _, s in got)
        # the records packed once
        keep, cache = [], {}
        K1 = ex._tri_kf(k1d, keep, cache)
        recs = (TriProblem * B)()
        outs = []
        for j, q in enumerate(pd):
            i1, i2 = np.ascontiguousarray(q["idx1"], np.int32), np.ascontiguousarray(q["idx2"], np.int32)
            keep += [i1, i2]
            recs[j].kf2 = ex._tri_kf(q["kf2"], keep, cache)
            recs[j].n_pairs, recs[j].idx1, recs[j].idx2 = len(i1), i1.ctypes.data, i2.ctypes.data
            outs.append((np.zeros((len(i1), 3), np.float32), np.zeros(len(i1), np.uint8)))
        xp = (C.c_void_p * B)(*[o[0].ctypes.data for o in outs])
        sp = (C.c_void_p * B)(*[o[1].ctypes.data for o in outs])
        L, h, r = ex.L, ex.h, float(ratio)

        def one_call():
            assert L.ygzf_triangulate_pairs(h, C.byref(K1), r, B, recs, xp, sp) == 0
        singles = [((TriProblem * 1)(recs[j]), (C.c_void_p * 1)(outs[j][0].ctypes.data), (C.c_void_p * 1)(outs[j][1].ctypes.data)) for j in range(B)]

        def per_neighbour():
            for rec, x, s in singles:
                assert L.ygzf_triangulate_pairs(h, C.byref(K1), r, 1, rec, x, s) == 0
        one_call()
        for (x, s), (gx, gs) in zip(outs, got):   # the raw call is the binding's result
            assert np.array_equal(x.view(np.uint32), gx.view(np.uint32)) and np.array_equal(s, gs)
        calls = max(10, args.calls // B)
        t_one = windows(one_call, args.windows, calls)
        t_bind = windows(lambda: ex.triangulate_pairs(k1d, ratio, pd), args.windows, calls)
        t_per = windows(per_neighbour, args.windows, max(5, calls // 2))
        files = []
        for j, (k2, i1, i2) in enumerate(problems):
            files.append(os.path.join(tmp, "p%d.bin" % j))
            TC.write_pairs(files[-1], k1, k2, i1, i2, ratio)
        o = subprocess.run([host, "time", str(max(20, 20000 // (B * n)))] + files, capture_output=True, text=True, check=True).stdout.split()
        t_host = tuple(float(v) for v in o[:3])
        rows[(B, n)] = (t_one[0], t_host[0])
        lines.append("  %3d x %4d     %6d     %s   %s   %s   %s     %5.2f" % (B, n, accepted, f3(t_one), f3(t_bind), f3(t_per), f3(t_host), t_host[0] / t_one[0]))
    lines += ["", "(device, binding: the Python binding packs every record on every call -- that is the binding's cost, not the library's)", ""]
    fixed, per_pair = rows[SIZES[0]][0], rows[SIZES[-1]][1] / (SIZES[-1][0] * SIZES[-1][1])
    cross = fixed / per_pair
    lines += ["crossover: the smallest device call costs %.1f us, the host thread %.2f us per pair on the measuring host: they meet near %.0f pairs." % (fixed, per_pair, cross),
              "A shell that may run the same text on the calling thread should do so below %d pairs per call (YGZF_TRI_DEVICE_MIN), the next power of two." % (1 << int(np.ceil(np.log2(cross)))), ""]
    # ---- the whole loop, searches included --------------------------------------------------------------------------------------------------
    hostdir, lib = os.path.join(PKG, "csrc", "host"), os.path.join(PKG, "lib")
    shell = os.path.join(tmp, "tri_shell")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", hostdir, "-I", os.path.join(hostdir, "standalone"), "-I", os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "tri_shell.cc")] + [os.path.join(hostdir, f) for f in ("LocalMappingTriangulate.cc", "ORBmatcher.cc", "ORBextractor.cc", "ygzf_pool.cc")] +
                          ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", shell])
    lines += ["the whole neighbour loop of CreateNewMapPoints, searches (one ygzf_search_for_triangulation call per neighbour) and map updates included, stand-alone classes,",
              "every neighbour matching the features of KF1 (the drop rule takes most pairs of the later neighbours): us per call",
              "neigh. x feat.   created    CreateNewMapPointsBatch      neighbour by neighbour       batch, triangulation on host"]
    for B, n in ((10, 300), (20, 300), (20, 1000)):
        k1, problems, ratio = TC.make_scene(6000 + 37 * B + n, n, True, B)
        files = []
        for j, (k2, i1, i2) in enumerate(problems):
            files.append(os.path.join(tmp, "w%d.bin" % j))
            TC.write_pairs(files[-1], k1, k2, i1, i2, ratio)
        o = subprocess.run([shell, "time", str(max(3, 6000 // (B * n) * 3)), repr(float(k1["mb"]))] + files, capture_output=True, text=True, check=True).stdout.split("\n")
        t = [tuple(float(v) for v in o[k].split()) for k in range(3)]
        lines.append("  %3d x %4d     %6s     %s   %s   %s" % (B, n, o[3].split()[1], f3(t[0]), f3(t[1]), f3(t[2])))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
