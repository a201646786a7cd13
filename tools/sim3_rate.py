"""tools/sim3_rate.py -- what Sim3Solver's RANSAC hypotheses cost on the device (ygzf_sim3_ransac: one packed upload, one launch of
k_sim3_ransac, one packed download, one synchronisation).  Writes a small text table (default profiles/sim3_rate.txt) and prints it.  Report
only: no threshold -- nobody has measured this step before, the file records what is found.

  One call for 1 / 3 / 10 loop candidates x 100 / 500 correspondences x 300 hypotheses each (seeded scenes of tests/sim3_cases.py, 30 % outliers).
  Beside each, on the same host: the SAME arithmetic (csrc/sim3_math.h) as a plain one-thread host program (tests/cpp/sim3_host.cc, g++ -O2),
  candidate after candidate.  That is NOT OpenCV and not the reference's Sim3Solver -- cv::Mat allocates per operation and would be slower --: it
  says what this machine's CPU does with a plain evaluation of the same operations.
  The kernel's VGPR count, LDS size and scratch size as the compiler reports them for the code object.
Every device figure: median [fastest .. slowest] of the timed windows, one untimed window first; the host clock around calls that synchronise.
  python tools/sim3_rate.py --prepare     builds the host program and reads the resource figures (no GPU needed)
  timeout -k 10 600 python tools/sim3_rate.py     on the GPU machine
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "orb_ygz_slam_amd")
BIN = os.path.join(ROOT, "tests", "cpp", "bin")   # (kept out of git)
HOST_EXE = os.path.join(BIN, "sim3_host")
PREP = os.path.join(BIN, "sim3_rate_prep.json")


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


def prepare():
    """the one-thread host program, and what the compiler says the kernel takes"""
    from orb_ygz_slam_amd import build as B
    os.makedirs(os.path.dirname(HOST_EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(PKG, "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "sim3_host.cc"), "-o", HOST_EXE])
    src = "csrc/sim3_kernels.hip"
    cmd = [B.hipcc()] + [f for f in B.FLAGS if not f.startswith("-W")] + B.FILE_FLAGS.get(src, []) + [
        "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    err = subprocess.run(cmd, cwd=PKG, check=True, capture_output=True, text=True).stderr
    res = {}
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                     ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
        res[key] = int(re.search(pat, err).group(1))
    assert "k_sim3_ransac" in err and res["scratch"] == 0, res
    with open(PREP, "w") as f:
        json.dump(res, f)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_rate.txt"))
    args = ap.parse_args()
    if args.prepare or not (os.path.exists(HOST_EXE) and os.path.exists(PREP)):
        res = prepare()
        if args.prepare:
            print(res)
            return
    res = json.load(open(PREP))
    import numpy as np
    from orb_ygz_slam_amd import Extractor
    from tests import sim3_cases as SC

    def as_dict(P):
        return dict(X1=P.X1, X2=P.X2, max_err1=SC.gates(P.sigma2_1), max_err2=SC.gates(P.sigma2_2), K1=P.K1, K2=P.K2, fix_scale=P.fix_scale, samples=P.samples)
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=1)
    f3 = lambda t: "%8.1f [%8.1f .. %8.1f]" % t
    lines = ["Sim3Solver's RANSAC hypotheses on the device (tools/sim3_rate.py): us per call, median [fastest .. slowest] of %d windows of %d calls" % (args.windows, args.calls),
             "seeded scenes of tests/sim3_cases.py: 30 % outliers, 300 random triples per candidate; one call evaluates every hypothesis of every candidate",
             "host: the same arithmetic (csrc/sim3_math.h) as a plain one-thread program, g++ -O2, candidate after candidate -- NOT OpenCV, not the reference's solver", "",
             "candidates  correspondences   device, one call                  one-thread host program          host / device"]
    with tempfile.TemporaryDirectory() as tmp:
        for cands in (1, 3, 10):
            for n in (100, 500):
                Ps = [SC._seeded("rate_c%d_n%d_%d" % (cands, n, k), n, 0.3, 9100 + 17 * k + n) for k in range(cands)]
                ds = [as_dict(P) for P in Ps]
                got = ex.sim3_ransac(ds)
                for P, g in zip(Ps, got):
                    assert np.array_equal(g["n_inliers"], SC.sim3_hypotheses(P, "device").count)
                t = windows(lambda: ex.sim3_ransac(ds), args.windows, args.calls)
                host = [0.0, 0.0, 0.0]
                for k, P in enumerate(Ps):
                    path = os.path.join(tmp, "case.bin")
                    SC.write_case(P, path)
                    v = subprocess.run([HOST_EXE, "time", path, str(args.windows)], check=True, capture_output=True, text=True).stdout.split()
                    for j in range(3):
                        host[j] += float(v[j])
                lines.append("    %2d          %4d           %s   %s   %6.2f" % (cands, n, f3(t), f3(tuple(host)), host[0] / t[0]))
    lines += ["", "k_sim3_ransac as compiled for gfx950: %d VGPRs, %d SGPRs, LDS %d bytes, scratch %d bytes per lane, %d waves per SIMD" % (
        res["vgprs"], res["sgprs"], res["lds"], res["scratch"], res["occupancy"]),
        "(the device figures include the Python binding's packing of the arrays, a few microseconds per candidate)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
