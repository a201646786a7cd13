"""tools/loop_rate.py -- what the candidate search of LoopClosing::SearchAndFuse takes on the device, batched and not.  Writes a small text
table (default profiles/r08_loop_rate.txt) and prints it.

Shapes: 20 and 60 corrected keyframes x 2 000 and 8 000 loop points, about 2 k keys per keyframe (synthetic maps of tests/cpp/fuse_restate.h).
  batch:   ygz::SearchAndFuseCandidates for all keyframes, i.e. ONE ygzf_fuse_sim3_candidates call with its packing and copies
  singles: the same pairs as one such call per keyframe
  host:    the C++ restatement of the search (tests/cpp/loop_restate.h) on one CPU thread -- for context only, it is test code
Each figure is the median of at least --repeats timed repeats lasting at least --seconds in total, with the fastest and slowest repeat beside it.
The three must give the same candidates (same_result).  The condition this tool checks: the batch's median is not above the singles' median by
more than the singles' own spread.
Runs on the GPU machine:  timeout -k 10 900 python tools/loop_rate.py
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_loop_rate.txt"))
    args = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "loop_shell")
        host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
        lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
        srcs = [os.path.join(ROOT, "tests", "cpp", "loop_shell.cc")] + [os.path.join(host, f) for f in
                                                                      ("ORBextractor.cc", "ORBmatcher.cc", "ORBmatcherFuse.cc", "ORBmatcherLoop.cc", "ygzf_pool.cc")]
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                               "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
        for kfs in (20, 60):
            for points in (2000, 8000):
                out = subprocess.check_output([exe, "time", str(kfs), "5000", str(points), str(args.repeats), str(args.seconds)], text=True)
                rows.append(json.loads(out.strip().splitlines()[-1]))
                print(rows[-1], flush=True)
    lines = ["SearchAndFuse candidate search, ms: median [fastest .. slowest] of >= %d repeats, >= %.1f s in total (tools/loop_rate.py)" % (args.repeats, args.seconds),
             "%-10s %-7s %-8s %-28s %-28s %-30s %s" % ("keyframes", "points", "keys/kf", "batch (one call)", "singles (call per keyframe)", "host restatement (context)", "same")]
    ok = True
    for r in rows:
        f = lambda t: "%8.3f [%8.3f .. %8.3f]" % tuple(t)
        lines.append("%-10d %-7d %-8d %-28s %-28s %-30s %s" % (r["keyframes"], r["points"], r["keys_per_kf"], f(r["batch_ms"]), f(r["singles_ms"]),
                                                               f(r["host_restatement_ms"]), r["same_result"]))
        spread = r["singles_ms"][2] - r["singles_ms"][1]
        ok = ok and r["same_result"] and r["batch_ms"][0] <= r["singles_ms"][0] + spread
    lines.append("batch not slower than the singles beyond their spread: %s" % ok)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
