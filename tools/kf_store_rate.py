"""tools/kf_store_rate.py -- what keeping keyframes resident on the device changes for the two Fuse members.  Writes a small text table (default
profiles/r11_kf_store_rate.txt) and prints it.

Shapes: those of tools/fuse_rate.py -- forward, 20 distinct targets x 1 500 points at ~1.7 k keys per keyframe (FuseBatch end to end: 30 targets,
10 of them duplicates), and reverse, 1 keyframe x 30 000 points -- and the SearchAndFuse shapes of tools/loop_rate.py, 20 and 60 keyframes x 2 000
and 8 000 loop points.
Device calls (this process, ctypes arguments prepared once):
  non-resident: one ygzf_fuse_candidates / ygzf_fuse_sim3_candidates call, every keyframe's keys, descriptors and mvuRight uploaded and its grid
                rebuilt by every workgroup -- unchanged code, the baseline
  resident:     one ygzf_fuse_*_candidates_resident call against keyframes put beforehand
  put:          one ygzf_kf_put per keyframe of the shape (upload + k_kf_grid_build), with the erase that makes room for it
  upload KB:    what crosses the link per call: keyframe arrays + point arrays + row table (non-resident), point arrays + row table (resident)
End to end (tests/cpp/kf_store_shell.cc `time`, built here with g++ -O2 against libygzf): ygz::FuseBatch and ygz::SearchAndFuseBatch with
KeyFrameDeviceStore::sResident off and on, on one map whose keyframes keep their addresses across repeats (after the first, untimed, store-on call
every keyframe is resident); the device queries and hits per call and the bytes the first call's puts uploaded.
Each figure is the median [fastest .. slowest] of at least --repeats timed repeats lasting at least --seconds in total, after one untimed repeat.
`same`: equal candidates (device calls) / an equal final graph (end to end).  The condition this tool checks: in no shape is the resident form's
median above the non-resident one's by more than the non-resident form's own spread.
Runs on the GPU machine:  timeout -k 10 900 python tools/kf_store_rate.py
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

from orb_ygz_slam_amd.capi import KP_DTYPE, Extractor, FrameView, FuseKf, FusePoints, KfRef, KfStatic, _p  # noqa: E402
from orb_ygz_slam_amd.fuse_scene import _rot, make_kf, make_points  # noqa: E402


def timed(call, repeats, seconds):
    call()
    t = []
    while len(t) < repeats or sum(t) < seconds:
        t0 = time.perf_counter()
        call()
        t.append(time.perf_counter() - t0)
    return [1e3 * float(np.median(t)), 1e3 * min(t), 1e3 * max(t)]


def prepare(ex, kfs, pts, sim3):
    """-> (non-resident call, resident call, put-all call, outputs of the two, upload bytes of the two)"""
    keep = []
    K = len(kfs)
    arr, recs, refs = (FuseKf * K)(), (KfStatic * K)(), (KfRef * K)()
    kf_bytes = 0
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
        recs[k] = KfStatic(f.view, f.cam, f.inv_level_sigma2, f.log_scale_factor)
        refs[k].key = 1000 + k
        refs[k].Rcw[:], refs[k].tcw[:], refs[k].Ow[:] = f.Rcw[:], f.tcw[:], f.Ow[:]
        kf_bytes += len(ck) * (28 + 32 + (4 if u is not None else 0))
    w, nr, mx, mn, mf, d = (np.ascontiguousarray(a) for a in pts)
    keep.extend([w, nr, mx, mn, mf, d])
    fp = FusePoints(w.ctypes.data, nr.ctypes.data, mx.ctypes.data, mn.ctypes.data, mf.ctypes.data, d.ctypes.data)
    P = len(w)
    out = [np.zeros((K, P), np.int32) for _ in range(4)]
    L, h, ref = ex.L, ex.h, C.byref(fp)
    th = 4.0 if sim3 else 3.0
    f_non = L.ygzf_fuse_sim3_candidates if sim3 else L.ygzf_fuse_candidates
    f_res = L.ygzf_fuse_sim3_candidates_resident if sim3 else L.ygzf_fuse_candidates_resident
    p = [_p(a) for a in out]

    def non():
        assert f_non(h, K, arr, P, ref, None, th, p[0], p[1]) == 0, L.ygzf_last_error(h)
        return keep

    def res():
        assert f_res(h, K, refs, P, ref, None, th, p[2], p[3]) == 0, L.ygzf_last_error(h)

    def put():
        for k in range(K):
            L.ygzf_kf_erase(h, refs[k].key)
            assert L.ygzf_kf_put(h, refs[k].key, C.byref(recs[k]), None) == 0, L.ygzf_last_error(h)
    pt_bytes = P * (12 + 12 + 4 + 4 + 4 + 32)
    row_bytes = K * 376     # sizeof(ProjRow)
    return non, res, put, out, (kf_bytes + pt_bytes + row_bytes, pt_bytes + row_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_kf_store_rate.txt"))
    args = ap.parse_args()
    ex = Extractor(1000, 1.2, 8, 20, 7, 752, 480)
    rng = np.random.default_rng(3)

    def kf_set(n, keys):
        return [make_kf(rng, 752, 480, keys, 8, 1.2, _rot(*rng.uniform(-0.05, 0.05, 3)), rng.uniform(-0.3, 0.3, 3), mbf=40.0 if k % 2 == 0 else 0.0,
                        stereo_frac=0.5) for k in range(n)]
    shapes = [("Fuse forward", False, kf_set(20, 1700), 1500),
              ("Fuse reverse", False, [make_kf(rng, 752, 480, 2000, 8, 1.2, np.eye(3), [0, 0, 0], mbf=40.0, stereo_frac=0.5)], 30000)]
    for n in (20, 60):
        kfs = kf_set(n, 2000)
        for P in (2000, 8000):
            shapes.append(("SearchAndFuse", True, kfs, P))
    f = lambda t: "%8.3f [%8.3f .. %8.3f]" % tuple(t)
    lines = ["Resident keyframes, ms: median [fastest .. slowest] of >= %d repeats, >= %.1f s in total, after one untimed repeat (tools/kf_store_rate.py)"
             % (args.repeats, args.seconds),
             "device calls",
             "%-14s %-4s %-7s %-30s %-30s %-30s %-18s %s" % ("shape", "kfs", "points", "non-resident call", "resident call", "put, all keyframes",
                                                             "upload KB non / res", "same")]
    ok = True
    for name, sim3, kfs, P in shapes:
        pts = make_points(rng, kfs[:4], P)
        ex.kf_clear()
        non, res, put, out, up = prepare(ex, kfs, pts, sim3)
        t_put = timed(put, args.repeats, args.seconds)
        t_non = timed(non, args.repeats, args.seconds)
        t_res = timed(res, args.repeats, args.seconds)
        same = bool(np.array_equal(out[0], out[2]) and np.array_equal(out[1], out[3]) and (out[0] >= 0).any())
        lines.append("%-14s %-4d %-7d %-30s %-30s %-30s %-18s %s" % (name, len(kfs), P, f(t_non), f(t_res), f(t_put), "%.0f / %.0f" % (up[0] / 1024, up[1] / 1024),
                                                                    same))
        print(lines[-1], flush=True)
        ok = ok and same and t_res[0] <= t_non[0] + (t_non[2] - t_non[1])
    ex.close()
    lines += ["end to end (store off / on; the store-on figures are calls that find every keyframe resident)",
              "%-20s %-4s %-7s %-30s %-30s %-9s %-6s %-10s %-14s %s" % ("call", "kfs", "points", "store off", "store on", "queries", "hits", "first puts",
                                                                        "first put KB", "same")]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "kf_store_shell")
        host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
        lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
        srcs = [os.path.join(ROOT, "tests", "cpp", "kf_store_shell.cc")] + [os.path.join(host, s) for s in
                ("ORBextractor.cc", "ORBmatcher.cc", "ORBmatcherFuse.cc", "ORBmatcherLoop.cc", "KeyFrameStore.cc", "ygzf_pool.cc")]
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                               "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
        runs = [("fuse", 20, 4000, 1500, 10), ("fuse", 20, 35000, 30000, -1)] + [("loop", k, 5000, p, 0) for k in (20, 60) for p in (2000, 8000)]
        for what, k, land, p, dup in runs:
            r = subprocess.run([exe, "time", what, str(k), str(land), str(p), str(dup), str(args.repeats), str(args.seconds)], capture_output=True, text=True)
            if not r.stdout.strip().startswith("{") and not r.stdout.strip().splitlines()[-1:]:
                print(r.stdout + r.stderr)
                ok = False
                continue
            j = json.loads(r.stdout.strip().splitlines()[-1])
            lines.append("%-20s %-4d %-7d %-30s %-30s %-9d %-6d %-10d %-14.0f %s" % (j["what"], j["keyframes"], j["points"], f(j["off_ms"]), f(j["on_ms"]),
                                                                                   j["queries_per_call"], j["hits_per_call"], j["puts_first_call"],
                                                                                   j["bytes_first_call"] / 1024, j["same"]))
            print(lines[-1], flush=True)
            ok = ok and j["same"] and r.returncode == 0 and j["on_ms"][0] <= j["off_ms"][0] + (j["off_ms"][2] - j["off_ms"][1])
    lines.append("resident not slower than non-resident beyond the latter's spread, in every shape: %s" % ok)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
