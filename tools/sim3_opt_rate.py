"""tools/sim3_opt_rate.py -- what Optimizer::OptimizeSim3 costs on the device (ygzf_optimize_sim3: one packed upload, one launch of
k_sim3_opt, one packed download, one synchronisation).  Writes a small text table (default profiles/sim3_opt_rate.txt) and prints it.  Report
only: no threshold -- nobody has measured this step before, the file records what is found.

  One call for 1 / 3 / 10 loop candidates x 30 / 100 / 300 correspondences each (seeded scenes of tests/sim3_opt_cases.py, 20 % gross outliers).
  Beside each, on the same host: the SAME arithmetic (csrc/sim3_opt_math.h) as a plain one-thread host program (tests/cpp/sim3_opt_host.cc,
  g++ -O2, no sanitizer), candidate after candidate.  That is NOT g2o -- the reference's optimiser allocates a graph per call and goes through
  virtual edges and would be slower --: it says what this machine's CPU does with a plain evaluation of the same operations.
  The kernel's VGPR count, LDS size and scratch size as the compiler reports them for the code object.
Every device figure: median [fastest .. slowest] of the timed windows, one untimed window first; the host clock around calls that synchronise,
packing and copies included.
  python tools/sim3_opt_rate.py --prepare     builds the host program and reads the resource figures (no GPU needed)
  timeout -k 10 600 python tools/sim3_opt_rate.py     on the GPU machine
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
HOST_EXE = os.path.join(BIN, "sim3_opt_host")
PREP = os.path.join(BIN, "sim3_opt_rate_prep.json")


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
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(PKG, "csrc"), "-I", os.path.join(PKG, "csrc", "host"), os.path.join(ROOT, "tests", "cpp", "sim3_opt_host.cc"),
                           "-o", HOST_EXE])
    src = "csrc/sim3_opt_kernels.hip"
    cmd = [B.hipcc()] + [f for f in B.FLAGS if not f.startswith("-W")] + B.FILE_FLAGS.get(src, []) + [
        "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    err = subprocess.run(cmd, cwd=PKG, check=True, capture_output=True, text=True).stderr
    res = {}
    for key, pat in (("vgprs", r"\bVGPRs: (\d+)"), ("agprs", r"\bAGPRs: (\d+)"), ("sgprs", r"TotalSGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                     ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)")):
        res[key] = int(re.search(pat, err).group(1))
    assert "k_sim3_opt" in err and res["scratch"] == 0, res
    with open(PREP, "w") as f:
        json.dump(res, f)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--prepare", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_opt_rate.txt"))
    args = ap.parse_args()
    if args.prepare or not (os.path.exists(HOST_EXE) and os.path.exists(PREP)):
        res = prepare()
        if args.prepare:
            print(res)
            return
    res = json.load(open(PREP))
    from orb_ygz_slam_amd import Extractor
    from tests import sim3_opt_cases as SC

    ex = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=1)
    f3 = lambda t: "%8.1f [%8.1f .. %8.1f]" % t
    lines = ["Optimizer::OptimizeSim3 on the device (tools/sim3_opt_rate.py): us per call, median [fastest .. slowest] of %d windows of %d calls" % (args.windows, args.calls),
             "seeded scenes of tests/sim3_opt_cases.py: 20 % gross outliers, fixed scale, th2 = 10; one call optimises every candidate (packing and copies included)",
             "host: the same arithmetic (csrc/sim3_opt_math.h) as a plain one-thread program, g++ -O2, candidate after candidate -- NOT g2o", "",
             "candidates  correspondences   device, one call                  one-thread host program          host / device"]
    with tempfile.TemporaryDirectory() as tmp:
        for cands in (1, 3, 10):
            for n in (30, 100, 300):
                Ps = [SC.scene(9100 + 17 * k + n, n, out1=n // 10, out2=n // 10) for k in range(cands)]
                ds = [SC.as_api(P) for P in Ps]
                got = ex.optimize_sim3(ds)
                for P, g in zip(Ps, got):
                    assert SC.same(SC.from_api(g), SC.optimize_sim3(P, "device")), "the device result differs from the restatement"
                t = windows(lambda: ex.optimize_sim3(ds), args.windows, args.calls)
                host = [0.0, 0.0, 0.0]
                for k, P in enumerate(Ps):
                    path = os.path.join(tmp, "case.bin")
                    SC.write_case(P, path)
                    v = subprocess.run([HOST_EXE, "time", path, str(args.windows)], check=True, capture_output=True, text=True).stdout.split()
                    for j in range(3):
                        host[j] += float(v[j])
                lines.append("    %2d          %4d           %s   %s   %6.2f" % (cands, n, f3(t), f3(tuple(host)), host[0] / t[0]))
    lines += ["", "k_sim3_opt as compiled for gfx950: %d VGPRs + %d AGPRs, %d SGPRs, LDS %d bytes, scratch %d bytes per lane, %d waves per SIMD" % (
        res["vgprs"], res["agprs"], res["sgprs"], res["lds"], res["scratch"], res["occupancy"]),
        "(the device figures include the Python binding's packing of the arrays, a few microseconds per candidate)"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
