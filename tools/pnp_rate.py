"""tools/pnp_rate.py -- what PnPsolver's RANSAC costs on the device (ygzf_pnp_ransac: one packed upload, the launches of k_pnp_hyp and
k_pnp_refine, one packed download, one synchronisation).  Writes a small text table (default profiles/pnp_rate.txt) and prints it.

  One call for 1 / 3 / 10 relocalisation candidates x 50 / 150 / 500 correspondences (40 % outliers), each with the budget that
  SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) gives: mRansacMinInliers = N / 2 and 35 iterations.  Packing and copies included.
  Beside each, on the same host, the SAME arithmetic (csrc/pnp_math.h through host/PnPHost.h) as a plain one-thread host program
  (tests/cpp/pnp_host.cc, g++ -O2), candidate after candidate, in two schedules:
    whole budget   every hypothesis of the budget and the Refine of every record: exactly what the device call computes
    incremental    the reference's schedule: iterate(5) until the first successful Refine (or bNoMore), evaluating as it goes
  That is NOT OpenCV and not the reference's PnPsolver -- cvCreateMat allocates per call and would be slower --: it says what this machine's
  CPU does with a plain evaluation of the same operations.
Every device figure: median [fastest .. slowest] of the timed windows of at least one second each, one untimed window first; the host clock
around calls that synchronise.
  python tools/pnp_rate.py --prepare     builds the host program and reads the resource figures (no GPU needed)
  timeout -k 10 900 python tools/pnp_rate.py     on the GPU machine
"""
import argparse
import json
import math
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
HOST_EXE = os.path.join(BIN, "pnp_host")
PREP = os.path.join(BIN, "pnp_rate_prep.json")


def windows(fn, n_windows, seconds):
    """us per call of fn (every call synchronises): n_windows timed windows of at least `seconds` each; one untimed window first"""
    t0 = time.perf_counter()
    fn()
    fn()
    per_window = max(3, int(math.ceil(seconds / max((time.perf_counter() - t0) / 2, 1e-6))))
    out = []
    for k in range(-1, n_windows):
        t0 = time.perf_counter()
        for _ in range(per_window):
            fn()
        if k >= 0:
            out.append((time.perf_counter() - t0) * 1e6 / per_window)
    out.sort()
    return (out[len(out) // 2], out[0], out[-1]), per_window


def prepare():
    """the one-thread host program, and what the compiler says the kernels take"""
    from orb_ygz_slam_amd import build as B
    os.makedirs(os.path.dirname(HOST_EXE), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(PKG, "csrc", "host"),
                           os.path.join(ROOT, "tests", "cpp", "pnp_host.cc"), "-o", HOST_EXE])
    src = "csrc/pnp_kernels.hip"
    cmd = [B.hipcc()] + [f for f in B.FLAGS if not f.startswith("-W")] + B.FILE_FLAGS.get(src, []) + [
        "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    err = subprocess.run(cmd, cwd=PKG, check=True, capture_output=True, text=True).stderr
    res = {}
    for kernel in ("k_pnp_hyp", "k_pnp_refine"):
        part = err[err.index(kernel):]
        r = {}
        for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"\bAGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
            r[key] = int(re.search(pat, part).group(1))
        assert r["scratch"] == 0, (kernel, r)
        res[kernel] = r
    with open(PREP, "w") as f:
        json.dump(res, f)
    return res


def candidate(n, seed):
    """one relocalisation candidate: n correspondences, 40 % outliers, the tracker's parameters, sets drawn as the solver draws them"""
    import numpy as np
    from tests import pnp_cases as PC
    rng = np.random.default_rng(seed)
    X, uv, _ = PC._scene(rng, n, int(0.4 * n), noise=0.5)
    perm = rng.permutation(n)
    min_inliers, max_its = PC.ransac_parameters(n, 0.99, 10, 300, 4, 0.5)
    sets = PC.draw_quads(n, 4, 2 * max_its + 5, PC.Lcg(seed).random_int)   # (the budget, and what an overrun of the incremental schedule may reach)
    return PC._problem("rate_n%d_%d" % (n, seed), X[perm], uv[perm], PC._gates(rng, n), sets, min_inliers, max_its, (5,), gaps=7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_rate.txt"))
    args = ap.parse_args()
    if args.prepare or not (os.path.exists(HOST_EXE) and os.path.exists(PREP)):
        res = prepare()
        if args.prepare:
            print(res)
            return
    res = json.load(open(PREP))
    import numpy as np
    from orb_ygz_slam_amd import Extractor
    from tests import pnp_cases as PC

    def as_dict(P):
        return dict(P3Dw=P.P3D, P2D=P.P2D, max_err=P.max_err, K=P.K, min_set=P.min_set, min_inliers=P.min_inliers, samples=P.samples[:P.max_its])
    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=1)
    f3 = lambda t: "%8.1f [%8.1f .. %8.1f]" % tuple(t)
    lines = ["PnPsolver's RANSAC on the device (tools/pnp_rate.py): us per call, median [fastest .. slowest] of %d windows of at least %.1f s, packing and copies included" % (args.windows, args.seconds),
             "candidates: 40 % outliers, SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991): mRansacMinInliers = N / 2, a budget of 35 sample sets each",
             "device: one ygzf_pnp_ransac call evaluates every hypothesis of every candidate and the Refine of every record",
             "host:   the same arithmetic (csrc/pnp_math.h) as a plain one-thread program, g++ -O2, candidate after candidate -- NOT OpenCV, not the reference's solver",
             "        whole budget = what the device call computes; incremental = the reference's schedule, iterate(5) until the first successful Refine", "",
             "cand.   N    device, one call                   host, whole budget                 host, incremental                budget / device   incremental / device"]
    with tempfile.TemporaryDirectory() as tmp:
        for cands in (1, 3, 10):
            for n in (50, 150, 500):
                Ps = [candidate(n, 9100 + 17 * k + n) for k in range(cands)]
                ds = [as_dict(P) for P in Ps]
                got = ex.pnp_ransac(ds)
                want = PC.pnp_hypotheses(Ps[0], Ps[0].max_its)
                assert np.array_equal(got[0]["n_inliers"], want.count) and np.array_equal(got[0]["refined_n"], want.refined_n)
                t, per = windows(lambda: ex.pnp_ransac(ds), args.windows, args.seconds)
                host, inc = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
                for P in Ps:
                    path = os.path.join(tmp, "case.bin")
                    PC.write_case(P, path)
                    v = subprocess.run([HOST_EXE, "time", path, "9"], check=True, capture_output=True, text=True).stdout.split()
                    w = subprocess.run([HOST_EXE, "time", path, "9", "incremental"], check=True, capture_output=True, text=True).stdout.split()
                    for j in range(3):
                        host[j] += float(v[j])
                        inc[j] += float(w[j])
                lines.append("  %2d   %4d   %s   %s   %s   %8.2f          %8.2f" % (cands, n, f3(t), f3(host), f3(inc), host[0] / t[0], inc[0] / t[0]))
                print(lines[-1], "(%d calls per window)" % per, flush=True)
    for kernel in ("k_pnp_hyp", "k_pnp_refine"):
        r = res[kernel]
        lines += ["", "%s as compiled for gfx950: %d VGPRs, %d AGPRs, %d SGPRs, LDS %d bytes per workgroup, scratch %d bytes per lane, %d waves per SIMD" % (
            kernel, r["vgprs"], r["agprs"], r["sgprs"], r["lds"], r["scratch"], r["occupancy"])]
    lines += ["(the device figures include the Python binding's packing of the arrays, a few microseconds per candidate)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
