"""tools/remap_rate.py -- what the undistortion (cv::remap's fixed-point bilinear path on the device, src/Frame.cc:775-805) costs.
Writes a small text table (default profiles/remap_rate.txt) and prints it.  Report only: no threshold.

The map is the EuRoC calibration's (752 x 480, k1 -0.283, k2 0.074: tests/remap_cases.py), the frames are synthetic scenes.
  (a) ygzf_remap_batch_device of 256 frames alone, per path setting (AUTO = the library's choice, LDS = staged tiles, GATHER = bounds-checked global
      loads) and, for the staged path, per run length (frames that share one read of the map).  us per launch and the rate over the bytes the
      algorithm needs: 256 x (361 KB read + 361 KB written) + the map's records once per run.
  (b) resident frames/s of ygzf_remap_batch_device + ygzf_extract_batch_device against ygzf_extract_batch_device alone on already undistorted
      frames (the extraction is the parent commit's code, unchanged), 256 frames per launch, interleaved windows on one context.
  (c) one frame through the shell: ORBextractor::ComputePyramidUndistorted of the raw image against ORBextractor::ComputePyramid of the
      undistorted one (tests/cpp/remap_shell.cc time), alternating blocks.
Every figure: median [fastest .. slowest] window.  Windows are timed with the host clock around launches that end in ygzf_sync.
Runs on the GPU machine:  timeout -k 10 600 python tools/remap_rate.py
"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H, N = 752, 480, 256


def windows(fn, sync, n_windows, per_window):
    """us per call of fn: n_windows timed windows of per_window calls, each ending in a synchronise; one untimed window first"""
    out = []
    for k in range(-1, n_windows):
        t0 = time.perf_counter()
        for _ in range(per_window):
            fn()
        sync()
        if k >= 0:
            out.append((time.perf_counter() - t0) * 1e6 / per_window)
    out.sort()
    return out[len(out) // 2], out[0], out[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remap_rate.txt"))
    args = ap.parse_args()
    import torch
    torch.cuda.init()
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import force_env
    from orb_ygz_slam_amd.synth import synth_frame
    from tests import remap_cases as R
    case = R.case_by_name("euroc_752x480")
    scenes = np.stack([synth_frame(300 + k, W, H) for k in range(8)])
    raw = torch.from_numpy(np.ascontiguousarray(scenes[np.arange(N) % 8])).to("cuda:0")
    und = torch.empty_like(raw)
    lines = ["Undistortion of 752 x 480 frames through the EuRoC map (tools/remap_rate.py): median [fastest .. slowest] of %d windows of %d launches" % (
        args.windows, args.calls), ""]
    f3 = lambda t: "%8.1f [%8.1f .. %8.1f]" % t

    def context(run=None, max_batch=1):
        old = os.environ.get("YGZF_FORCE")
        if run:
            os.environ["YGZF_FORCE"] = force_env(remap_frames_per_run=run)
        try:
            ex = Extractor(1000, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=max_batch)
        finally:
            if old is None:
                os.environ.pop("YGZF_FORCE", None)
            else:
                os.environ["YGZF_FORCE"] = old
        ex.remap_set(0, W, H, case.map_xy, case.map_tab)
        return ex

    # (a)
    lines += ["(a) ygzf_remap_batch_device, %d frames per launch" % N,
              "%-8s %-6s %-34s %-10s %s" % ("path", "run", "us per launch", "GB/s", "tiles staged / zeroed / gathered")]
    want0 = R.remap_ref(scenes[0], case.map_xy, case.map_tab)
    for pname, path, runs in (("AUTO", 0, (None,)), ("LDS", 1, (2, 4, 8, 16, 32)), ("GATHER", 2, (8, 32))):
        for run in runs:
            ex = context(run)
            ex.remap_set_path(path)
            G = ex.remap_info(0)["frames_per_run"]
            call = lambda: ex.remap_batch_device(0, raw.data_ptr(), N, W, W * H, und.data_ptr(), W, W * H)
            t = windows(call, ex.sync, args.windows, args.calls)
            assert np.array_equal(und[0].cpu().numpy(), want0), "the timed launch does not compute the restated image"
            st = ex.remap_stats()
            need = N * 2 * W * H + -(-N // G) * W * H * (4 if path != 2 else 8)
            lines.append("%-8s %-6d %-34s %-10.0f %d / %d / %d" % (pname, G, f3(t), need / t[0] / 1e3, st["staged"], st["zeroed"], st["gathered"]))
            print(lines[-1], flush=True)
            ex.close()
    lines += ["(the floor: %.0f MB per launch = %.0f us at 4 TB/s; k_pyr_resize takes 173 us per 256 frames over 631 MB, DESIGN.md section 0)" % (
        N * 2 * W * H / 1e6, N * 2 * W * H / 4e6), ""]

    # (b)
    ex = context(max_batch=N)
    und_np = np.stack([R.remap_ref(s, case.map_xy, case.map_tab) for s in scenes])
    ready = torch.from_numpy(np.ascontiguousarray(und_np[np.arange(N) % 8])).to("cuda:0")
    alone = lambda: ex.extract_batch_device(ready.data_ptr(), N, W, H, W, W * H)

    def chained():
        ex.remap_batch_device(0, raw.data_ptr(), N, W, W * H, und.data_ptr(), W, W * H)
        ex.extract_batch_device(und.data_ptr(), N, W, H, W, W * H)
    ta, tc = [], []
    for k in range(args.windows):                   # interleaved: a window of one, a window of the other
        ta.append(windows(alone, ex.sync, 1, 8)[0])
        tc.append(windows(chained, ex.sync, 1, 8)[0])
    counts_chained = ex.batch_counts().copy()
    alone()
    same = np.array_equal(ex.batch_counts(), counts_chained)
    ta.sort()
    tc.sort()
    fps = lambda ts: "%8.0f [%8.0f .. %8.0f]" % (N * 1e6 / ts[len(ts) // 2], N * 1e6 / ts[-1], N * 1e6 / ts[0])
    lines += ["(b) resident frames/s, %d frames per launch, %d interleaved windows of 8 launches" % (N, args.windows),
              "extract_batch_device alone (undistorted frames)      %s" % fps(ta),
              "remap_batch_device + extract_batch_device (raw)      %s" % fps(tc),
              "keypoint counts of the two equal: %s" % same, ""]
    print("\n".join(lines[-5:]), flush=True)
    ex.close()
    del raw, und, ready

    # (c)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "remap_shell")
        host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
        lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
        srcs = [os.path.join(ROOT, "tests", "cpp", "remap_shell.cc")] + [os.path.join(host, f) for f in ("ORBextractor.cc", "ygzf_pool.cc")]
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                               "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
        with open(os.path.join(tmp, "meta.txt"), "w") as f:
            f.write("%d %d %d %d 1\n" % (W, H, W, H))
        case.map_xy.tofile(os.path.join(tmp, "map_xy.bin"))
        case.map_tab.tofile(os.path.join(tmp, "map_tab.bin"))
        scenes[0].tofile(os.path.join(tmp, "raw_0.bin"))
        und_np[0].tofile(os.path.join(tmp, "want_0.bin"))
        out = subprocess.run([exe, "time", tmp, str(args.windows), "200"], capture_output=True, text=True, timeout=240)
        if out.returncode != 0:
            sys.stderr.write(out.stdout + out.stderr)
            return 2
        lines += ["(c) one frame through the shell (host clock around the calls, levels back in host memory)"] + out.stdout.strip().splitlines()
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
