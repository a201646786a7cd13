#!/usr/bin/env python3
"""bench.py -- frames/s of the ORB extract + match hot path on MI355X (BASELINE.json metric).

One "step" = one pass of the hot path (ORBextractor::operator() on every frame of a batch + ORBmatcher::SearchByProjection
of every frame against its predecessor) over one batch of synthetic frames that is already resident in HBM when the
timed region starts.  The resident clip (default 10752 frames of 752x480 = 3.9 GB) is walked `--passes` times per step (default 6:
64512 frames) in sub-batches of 256 frames that rotate over 3 independent extractor contexts (own HIP stream and buffers each), so a
step is 252 sub-batch launches and the driver's 20 steps give a timed region of five to six seconds.  One process per GPU; frames are independent, so each rank owns its own
clip (weak scaling) and there is no collective in the data path -- torch.distributed is used only for the barrier and
the max-over-ranks time.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 --master-port 29500 \
        bench.py --gpus 8 --steps 20 --warmup 3
    python bench.py --devices-in-process 8        # the same sharding inside ONE process: one host thread + contexts per device
    python bench.py --gpus 1 --steps 20 --warmup 3 --full                # + everything beyond the headline (fields below)
    python bench.py --gpus 1 --steps 20 --warmup 3 --dump-outputs DIR    # + the last timed step's results as DIR/*.npy

A plain run sets up, warms up, times the steps and prints the line: `value`, `ms_per_step` and the fields of the timed region.  `--full` adds
the per-kernel profile and rooflines, the CPU baselines, the end-to-end and multi-GPU entry points and the other workloads (the `--no-*` options
switch single parts of it off again); without it those fields are null.

Rank 0 prints ONE JSON line (see DESIGN.md "Measurement" for the definition of every field):
  value              resident-frames rate of the timed region (the contract's number: inputs already in HBM, results left in HBM;
                     value_definition says so in the line itself)
  value_end_to_end   SURVEY 8(d)'s transfers-included rate: host frames in (pinned, H2D) -> kernels -> every keypoint + descriptor out
                     (D2H), two contexts software-pipelined, >= 1 s
  roofline           HBM roofline of the dominant kernel (algorithmic bytes / measured launch time / 8 TB/s)
  roofline_valu      the ceiling that actually binds it: vector-ALU issue cycles (instruction counts from the PMC profile x the
                     issue costs calibrated by tools/micro/valu_peak.hip) / SIMD cycles available
  cpu_baseline       the oracle ("port") on this host's cores; cpu_baseline_reference: the reference's own ORBextractor.cc +
                     ORBmatcher.cc (oracle/_ref, over the OpenCV stand-in), one thread
  other_workloads    short runs of BASELINE configs 4 / 5 (1920x1080/4000, 3840x2160 stereo/12 levels/8000), of config 3 (+ SparseImgAlign)
                     and of a clip cut from the one real image the reference ships (Thirdparty/fast/test/data/test1.png), each with
                     its own roofline
  libfast_sse2_anchor  the reference's own Thirdparty/fast SSE2 detector (detect only, one thread) on the same frames: SURVEY 8(d)'s sanity
                     anchor
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

WORKLOADS = {
    # name: (w, h, nlevels, scale_factor, nfeatures, iniTh, minTh)
    "euroc752x480_8lvl_1000feat": (752, 480, 8, 1.2, 1000, 20, 7),      # BASELINE.json metric / configs[2] shape
    "vga640x480_8lvl_1000feat": (640, 480, 8, 1.2, 1000, 20, 7),        # configs[1]
    "fhd1920x1080_8lvl_4000feat": (1920, 1080, 8, 1.2, 4000, 20, 7),    # configs[3]
    "uhd3840x2160_12lvl_8000feat": (3840, 2160, 12, 1.2, 8000, 20, 7),  # configs[4] (one eye)
}
# (frames per sub-batch launch, sub-batch rounds per step) chosen so that 20 steps take about a second
# (one octree workgroup per (level, frame): the 4K / 1080p sub-batches are sized so that they still fill the chip -- 8 -> 64 frames per
# launch took the 4K rate from 6.4 k to 8.2 k frames/s, 32 -> 128 the 1080p rate from 31.9 k to 35.4 k)
SHAPES = {"euroc752x480_8lvl_1000feat": (256, 14), "vga640x480_8lvl_1000feat": (256, 14), "fhd1920x1080_8lvl_4000feat": (128, 4),
          "uhd3840x2160_12lvl_8000feat": (64, 2)}
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E peak (MI355X_MICROARCH.md)
PCIE_PEAK_GBS = 63.0           # PCIe 5.0 x16, one direction (what the end-to-end rate is bound by: every frame crosses the link)
SIMDS, CLOCK_GHZ = 1024, 2.4   # 256 CUs x 4 SIMDs, peak shader clock


def level_sizes(w, h, nlevels, sf):
    """Pyramid level sizes with the reference's float arithmetic (src/ORBextractor.cc:419-428, 1131-1132)."""
    scale = np.float32(1.0)
    out = []
    for l in range(nlevels):
        if l > 0:
            scale = np.float32(scale * np.float32(sf))
        inv = np.float32(1.0) / scale
        out.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return out


def algorithmic_bytes(w, h, nlevels, sf, nfeat):
    """algorithmic bytes per frame, total and per kernel (see DESIGN.md for the attribution)."""
    sz = level_sizes(w, h, nlevels, sf)
    P = sum(a * b for a, b in sz)
    P0, Pl = sz[0][0] * sz[0][1], sz[-1][0] * sz[-1][1]
    K = nfeat
    per = {
        "k_pyr_resize": (P - Pl) + (P - P0),              # read levels 0..L-2, write levels 1..L-1
        "k_fast_tab": P,                                   # FAST read of every level (k_fast_quads: the register-staging form of the same loop)
        "k_fast_quads": P,
        "k_fast_tab_persist": P,                           # the persistent form of the same loop (frames of >= 1000 cell groups)
        "k_describe": 2 * P + K * (749 + 512 + 32 + 28),   # blur read+write, orientation disc, samples, descriptor, KeyPoint
        "k_match_last": (K + K) * 32 + K * 8,              # B_match
        "k_octree": 0,                                     # candidate lists only (not part of SURVEY's formula)
    }
    total = per["k_pyr_resize"] + per["k_fast_tab"] + per["k_describe"] + per["k_match_last"]
    return total, per


def make_frames(n, w, h, seed0=1000):
    """Synthetic clip: groups of 8 consecutive frames are shifted crops of one scene so that frame-to-frame matching
    has something to find; every 8th frame is a scene cut."""
    from concurrent.futures import ThreadPoolExecutor
    from orb_ygz_slam_amd.synth import synth_frame
    frames = np.empty((n, h, w), np.uint8)
    m = 24
    nscenes = (n + 7) // 8
    # (a 3840x2160 scene takes seconds of numpy; the scenes of a clip are independent and numpy releases the GIL on arrays of this size)
    with ThreadPoolExecutor(max_workers=max(1, min(nscenes, effective_cores()))) as pool:
        scenes = list(pool.map(lambda k: synth_frame(seed0 + k, w + m, h + m), range(nscenes)))
    for i in range(n):
        dx, dy = (3 * (i % 8)) % m, (2 * (i % 8)) % m
        frames[i] = scenes[i // 8][dy:dy + h, dx:dx + w]
    return frames


def make_frames_test1png(n, w, h):
    """Clip cut from the only real image the reference ships, Thirdparty/fast/test/data/test1.png (752x480 gray; pixels carried by the
    committed fixture tests/golden/fast10_test1.npz, written by tools/make_golden_fast10.py): the image is mirror-padded (REFLECT_101) by 24 px,
    groups of 8 consecutive frames are shifted crops of one zoom level (1.00, 1.02, ... bilinear, so that consecutive groups differ in scale
    as a slowly approaching camera would make them); every 8th frame starts a new zoom."""
    img = np.load(os.path.join(ROOT, "tests", "golden", "fast10_test1.npz"))["image"]
    ih, iw = img.shape
    if (iw, ih) != (w, h):
        raise SystemExit("the test1.png clip is %dx%d" % (iw, ih))
    m = 24
    pad = np.pad(img, m, mode="reflect").astype(np.float32)
    frames = np.empty((n, h, w), np.uint8)
    scene = None
    for i in range(n):
        if i % 8 == 0:
            z = 1.0 + 0.02 * ((i // 8) % 12)
            ys = (np.arange(h + m, dtype=np.float32) + 0.5) / np.float32(z) - 0.5 + m / 2 * (1 - 1 / z)
            xs = (np.arange(w + m, dtype=np.float32) + 0.5) / np.float32(z) - 0.5 + m / 2 * (1 - 1 / z)
            y0 = np.clip(np.floor(ys).astype(np.int32), 0, pad.shape[0] - 2)
            x0 = np.clip(np.floor(xs).astype(np.int32), 0, pad.shape[1] - 2)
            fy = (ys - y0).astype(np.float32)[:, None]
            fx = (xs - x0).astype(np.float32)[None, :]
            a = pad[y0][:, x0] * (1 - fx) + pad[y0][:, x0 + 1] * fx
            b = pad[y0 + 1][:, x0] * (1 - fx) + pad[y0 + 1][:, x0 + 1] * fx
            scene = np.clip(np.rint(a * (1 - fy) + b * fy), 0, 255).astype(np.uint8)
        dx, dy = (3 * (i % 8)) % m, (2 * (i % 8)) % m
        frames[i] = scene[dy:dy + h, dx:dx + w]
    return frames


def libfast_anchor(frames, seconds_budget=1.5):
    """SURVEY 8(d)'s sanity anchor: the reference's own Thirdparty/fast (oracle/_ref/libfast_ref.so, fast_corner_detect_10_sse2, threshold 20),
    detect only, one thread, over frames of the clip for a bounded time.  None when oracle/_ref was never built."""
    from oracle import oracle_py as O
    R = O.ref_fast()
    if R is None:
        return None
    n, h, w = frames.shape
    xy = np.zeros((w * h, 2), np.int16)
    t0 = time.perf_counter()
    done = corners = 0
    while time.perf_counter() - t0 < seconds_budget:
        f = np.ascontiguousarray(frames[done % n])
        corners += R.ref_fast10_detect(1, O._p(f), w, h, w, 20, O._p(xy), len(xy))
        done += 1
    sec = time.perf_counter() - t0
    return {"ms_per_frame": round(1e3 * sec / done, 4), "frames": done, "corners_per_frame": round(corners / done, 1), "threads": 1,
            "what": "Thirdparty/fast fast_corner_detect_10_sse2 (FAST-10, threshold 20, level 0 only, detect only) compiled from the reference checkout"}


def effective_cores():
    """Cores this process may actually use: affinity mask, further limited by a cgroup CPU quota when there is one."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        q, p = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = max(1, min(n, int(float(q) / float(p) + 0.5)))
    except Exception:
        pass
    return n


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                return line.split(":", 1)[1].strip()
    except Exception:
        pass
    return "unknown"


def cpu_baseline(frames, cfg, seconds_budget=12.0, match=True, align=False, stereo=False, one_thread=True):
    """The CPU oracle ('port' of the reference path) on this host's cores: every worker thread runs the workload's own steps -- extract, + projection
    match of consecutive frames, + SparseImgAlign of the same pair (`align`), + ComputeStereoMatches on (left, right) pairs (`stereo`) -- over its own
    run of consecutive frames of the same clip for a bounded time (about `seconds_budget` s; a frame that was started is finished, so that even a
    3840x2160 clip at ~2 frames/s/thread yields at least one frame / pair per thread)."""
    from oracle import oracle_py as O
    w, h, nl, sf, nf, ini, mn = cfg
    cores = effective_cores()
    kw = dict(match=match, align=align, stereo=stereo)
    fps1 = None
    if one_thread:
        sec1, _, _, n1 = O.bench_extract_match(frames, nf, sf, nl, ini, mn, threads=1, frames_per_thread=1000, max_seconds=2.0, **kw)
        fps1 = n1 / max(sec1, 1e-6)
    sec, nk, nm, n = O.bench_extract_match(frames, nf, sf, nl, ini, mn, threads=cores, frames_per_thread=100000,
                                           max_seconds=seconds_budget, **kw)
    n = max(n, 1)
    steps = "extract" + (" + SearchByProjection(cur, last)" if match else "") + (" + SparseImgAlign(L-1..1, 10 iterations)" if align else "") + \
            (" + ComputeStereoMatches per (left, right) pair" if stereo else "")
    return {"value": round(n / sec, 2), "unit": "frames/s", "cores": cores, "kind": "port", "cpu_model": cpu_model(), "steps": steps,
            "sample": "%d threads, each on its own run of consecutive frames of the workload's clip, time-bounded: %d frames in %.1f s%s" %
                      (cores, n, sec, ("; 1 thread: %.2f frames/s" % fps1) if fps1 is not None else ""),
            "keypoints_per_frame": round(nk / n, 1), "matches_per_frame": round(nm / n, 1)}


def cpu_baseline_reference(frames, cfg, seconds_budget=6.0):
    """The reference's OWN src/ORBextractor.cc and src/ORBmatcher.cc (compiled where they lie into oracle/_ref over the OpenCV stand-in of
    oracle/ref_shim: cv::resize / cv::FAST / cv::GaussianBlur underneath are the oracle's plain restatements, not an optimised OpenCV),
    one thread, on consecutive frames of the same clip for a bounded time.  None when oracle/_ref was never built."""
    from oracle import oracle_py as O
    if O.ref_extractor_lib() is None or O.ref_matcher_lib() is None:
        return None
    w, h, nl, sf, nf, ini, mn = cfg
    from orb_ygz_slam_amd.capi import EUROC
    scale = O.Extractor(nf, sf, nl, ini, mn).tables()["scale"]
    I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    t0 = time.perf_counter()
    prev, n, nk, nm = None, 0, 0, 0
    while time.perf_counter() - t0 < seconds_budget and n < len(frames):
        k, d = O.ref_extract(frames[n], nf, sf, nl, ini, mn)
        if prev is not None and len(k) and len(prev[0]):
            pk, pd = prev
            world = np.stack([(pk["x"] - np.float32(EUROC["cx"])) / np.float32(EUROC["fx"]), (pk["y"] - np.float32(EUROC["cy"])) / np.float32(EUROC["fy"]),
                              np.ones(len(pk), np.float32)], -1).astype(np.float32)
            with O.reference_matcher():
                m, _, _ = O.search_by_projection_last(k, d, scale, w, h, EUROC, pk, world, pd, I, z, I, z, 15.0)
            nm += m
        prev = (k, d)
        nk += len(k)
        n += 1
    sec = time.perf_counter() - t0
    return {"value": round(n / sec, 2), "unit": "frames/s", "cores": 1, "kind": "reference-over-shim",
            "sample": "the reference's own ORBextractor.cc + ORBmatcher.cc (oracle/_ref) on %d consecutive frames of the bench clip in %.1f s, one thread; "
                      "OpenCV primitives = the oracle's restatements" % (n, sec),
            "keypoints_per_frame": round(nk / max(n, 1), 1), "matches_per_frame": round(nm / max(n - 1, 1), 1)}


class Pipeline:
    """One device's share of the work: `streams` extractor contexts, a resident clip of rounds x streams x sub frames."""

    def __init__(self, device, workload, sub, rounds, streams, seed0, align=False, stereo=False, distinct=None, frames=None, passes=1, match=True):
        import torch
        from orb_ygz_slam_amd import Extractor, make_camera
        self.cfg = WORKLOADS[workload]
        w, h, nl, sf, nf, ini, mn = self.cfg
        self.device, self.sub, self.rounds, self.S, self.align, self.stereo, self.match = device, sub, rounds, streams, align, stereo, match
        D = streams * sub if distinct is None else distinct          # distinct synthetic frames; the resident batch tiles them
        self.frames = make_frames(D, w, h, seed0=seed0) if frames is None else frames
        D = len(self.frames)
        self.passes = passes
        base = torch.from_numpy(self.frames).to("cuda:%d" % device)
        total = rounds * streams * sub
        reps = (total + D - 1) // D
        self.d_frames = base.repeat(reps, 1, 1)[:total].contiguous() if reps > 1 else base
        self.batch = total
        self.exs = [Extractor(nf, sf, nl, ini, mn, max_width=w, max_height=h, max_batch=sub, device=device) for _ in range(streams)]
        self.cam = make_camera(w, h)
        if not (match or align):           # nothing reads the carried "previous frame" (include/ygzf.h: ygzf_set_carry_previous)
            for e in self.exs:
                e.set_carry_previous(False)
        self.w, self.h, self.nl = w, h, nl
        p0 = self.d_frames.data_ptr()
        self.ptrs = [[p0 + ((r * streams + s) * sub) * w * h for s in range(streams)] for r in range(rounds)]

    def launch(self, e, ptr):
        e.extract_batch_device(ptr, self.sub, self.w, self.h)
        if self.match:
            e.match_batch_prev(self.cam, 15.0, True, True, True)
        if self.align:
            e.align_batch_prev(self.cam, self.nl - 1, 1, 10)
        if self.stereo:
            e.stereo_batch(0.11, 47.9)

    def step(self):
        for _ in range(self.passes):                 # the resident clip again: same frames, same work, still no host traffic
            for r in range(self.rounds):
                for s, e in enumerate(self.exs):
                    self.launch(e, self.ptrs[r][s])

    def sync(self):
        for e in self.exs:
            e.sync()

    def profile(self, on):
        for e in self.exs:
            e.profile_enable(on)
            if on:
                e.profile_reset()

    def profile_read(self):
        prof = {}
        for e in self.exs:
            for name, (ms, n) in e.profile_read().items():
                a = prof.get(name, (0.0, 0))
                prof[name] = (a[0] + ms, a[1] + n)
        return prof


def run_timed(pipes, steps, warmup, barrier, sync_all):
    """W untimed steps, then exactly `steps` steps between barrier + synchronise brackets on every device of this process (one host thread
    per device when there are several).  Returns this process's elapsed seconds."""
    def loop(p, n):
        for _ in range(n):
            p.step()
        p.sync()
    if len(pipes) == 1:
        loop(pipes[0], warmup)
        sync_all(); barrier(); sync_all()
        t0 = time.perf_counter()
        loop(pipes[0], steps)
        sync_all(); barrier(); sync_all()
        return time.perf_counter() - t0
    gate = threading.Barrier(len(pipes) + 1)
    def worker(p):
        loop(p, warmup)
        gate.wait()            # warm-up done everywhere
        gate.wait()            # go
        loop(p, steps)
        gate.wait()            # done
    th = [threading.Thread(target=worker, args=(p,)) for p in pipes]
    for t in th:
        t.start()
    gate.wait()
    sync_all(); barrier(); sync_all()
    t0 = time.perf_counter()
    gate.wait()
    gate.wait()
    sync_all(); barrier(); sync_all()
    el = time.perf_counter() - t0
    for t in th:
        t.join()
    return el


DUMP_BYTES_PER_KEYPOINT = 7 * 8 + 32 * 4 + 8 + 2 * 4     # keypoint row (float64) + descriptor (float32) + match (float64) + stereo (2 x float32)


def dump_outputs(pipe, out_dir, budget=56 << 20, max_sample=128, seed=20240611):
    """What the timed path left for its caller after the last step: every context holds the results of its last sub-batch (round rounds-1, last
    pass).  Writes out_dir/*.npy (float32 / float64 only): per-frame keypoint and match counts of all those frames, and for a fixed, seeded sample
    of them (the sample size depends on the configuration only, so that it stays below `budget` bytes) the keypoints, descriptors, matches and --
    when the step runs them -- the stereo and SparseImgAlign results.  Frames are numbered by their index in the resident clip."""
    w, h = pipe.w, pipe.h
    S, sub, last = len(pipe.exs), pipe.sub, pipe.rounds - 1
    unit = 2 if pipe.stereo else 1                       # a stereo pair is sampled as a whole
    stride = max(pipe.exs[0].max_keypoints(w, h), 1)
    units = S * sub // unit
    k_units = max(1, min(units, max_sample // unit, budget // (unit * stride * DUMP_BYTES_PER_KEYPOINT)))
    pick = np.sort(np.random.default_rng(seed).choice(units, k_units, replace=False))
    sample = [u * unit + j for u in pick for j in range(unit)]                         # positions in the (context, frame) order
    clip_index = lambda i: (last * S + i // sub) * sub + i % sub
    res = [e.batch_fetch_all(sub) for e in pipe.exs]
    n_kp = np.concatenate([r[2] for r in res]).astype(np.float64)
    out = {"frames": np.array([clip_index(i) for i in range(S * sub)], np.float64), "keypoint_counts": n_kp}
    if pipe.match:
        out["match_counts"] = np.concatenate([e.match_counts() for e in pipe.exs]).astype(np.float64)
    ncol = len(res[0][0].dtype.names)                   # x, y, size, angle, response, octave, class_id
    kps, desc, match, off, ur, dp, sia_T, sia_info, sia_ret = [], [], [], [0], [], [], [], [], []
    for i in sample:
        s, f = divmod(i, sub)
        n = int(res[s][2][f])
        k = res[s][0][f, :n]
        kps.append(np.stack([k[c].astype(np.float64) for c in k.dtype.names], -1))
        desc.append(res[s][1][f, :n].astype(np.float32))
        off.append(off[-1] + n)
        if pipe.match:
            match.append(pipe.exs[s].match_fetch(f)[0][:n].astype(np.float64))
        if pipe.stereo and f % 2 == 0:
            u, d = pipe.exs[s].stereo_fetch(f // 2)
            ur.append(u[:n].astype(np.float32))
            dp.append(d[:n].astype(np.float32))
        if pipe.align:
            ret, T, info = pipe.exs[s].align_fetch(f)
            sia_ret.append(ret)
            sia_T.append(T.astype(np.float64))
            sia_info.append(info.astype(np.float64))
    out["sample_frames"] = np.array([clip_index(i) for i in sample], np.float64)
    out["sample_keypoint_offsets"] = np.array(off, np.float64)
    out["sample_keypoints"] = np.concatenate(kps).reshape(-1, ncol)
    out["sample_descriptors"] = np.concatenate(desc).reshape(-1, 32)
    if pipe.match:
        out["sample_matches"] = np.concatenate(match)
    if pipe.stereo:                                      # left frames of the sampled pairs, in sample order
        out["sample_stereo_u_right"] = np.concatenate(ur)
        out["sample_stereo_depth"] = np.concatenate(dp)
    if pipe.align:
        out["sample_align_ret"] = np.array(sia_ret, np.float64)
        out["sample_align_Tcr"] = np.array(sia_T, np.float64).reshape(-1, 7)
        out["sample_align_info"] = np.array(sia_info, np.float64).reshape(-1, 2)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        assert a.dtype in (np.float32, np.float64), name
        np.save(os.path.join(out_dir, name + ".npy"), a)


def end_to_end(pipe, min_seconds=1.2, depth=2, host_pitch=None):
    """SURVEY 8(d) 'end-to-end': page-locked host frames in (H2D), kernels, every keypoint + descriptor + count out (D2H) -- `depth` contexts
    software-pipelined: while one sub-batch is in its kernels the next ones' frames go up and the previous one's results come down (the
    upload alone is 1.7 ms per 256 frames, the kernels 1.3 ms; measured: depth 2 134 k, depth 3 133 k, depth 4 113 k frames/s -- the link
    is the limit at ~48 GB/s up + 9 GB/s down)."""
    import torch
    from orb_ygz_slam_amd.capi import KP_DTYPE
    from orb_ygz_slam_amd import Extractor
    w, h, nl, sf, nf, ini, mn = pipe.cfg
    B = pipe.sub
    exs = list(pipe.exs[:depth])
    while len(exs) < depth:
        exs.append(Extractor(nf, sf, nl, ini, mn, max_width=w, max_height=h, max_batch=B, device=pipe.device))
        if not (pipe.match or pipe.align):
            exs[-1].set_carry_previous(False)
    stride = exs[0].max_keypoints(w, h)
    from orb_ygz_slam_amd.capi import host_row_pitch
    hp = host_row_pitch(w) if host_pitch is None else host_pitch      # frames laid out at the device's row pitch go up as whole frames, not row by row
    pins, outs, keep = [], [], []
    for i in range(depth):
        src = np.take(pipe.frames, (np.arange(B) + i * B) % len(pipe.frames), axis=0)      # (the clip may hold fewer distinct frames than a sub-batch)
        pf = torch.zeros((B, h, hp), dtype=torch.uint8).pin_memory()
        pf.numpy()[:, :, :w] = src
        ok = torch.empty((B, stride, KP_DTYPE.itemsize), dtype=torch.uint8).pin_memory()
        od = torch.empty((B, stride, 32), dtype=torch.uint8).pin_memory()
        on = torch.empty(B, dtype=torch.int32).pin_memory()
        keep += [pf, ok, od, on]
        pins.append(pf.numpy()[:, :, :w])
        outs.append((ok.numpy().view(KP_DTYPE).reshape(B, stride), od.numpy(), on.numpy()))

    def submit(i):
        exs[i].extract_batch_host(pins[i])
        if pipe.match:
            exs[i].match_batch_prev(pipe.cam, 15.0, True, True, True)
        if pipe.stereo:
            exs[i].stereo_batch(0.11, 47.9)                                # (its mvuRight / mvDepth rows stay on the device: 8 more bytes per keypoint)
    for i in range(depth):                                                 # warm-up
        submit(i)
    for i in range(depth):
        exs[i].batch_fetch_all(B, outs[i])
    t0 = time.perf_counter()
    it = 0
    while it < 2 * depth or time.perf_counter() - t0 < min_seconds:        # at least min_seconds of steady state (hundreds of sub-batches)
        if it >= depth:                                                    # the context is reused: its previous sub-batch comes down first
            exs[it % depth].batch_fetch_all(B, outs[it % depth])
        submit(it % depth)
        it += 1
    batches = it
    for it in range(batches, batches + depth):                             # drain
        exs[it % depth].batch_fetch_all(B, outs[it % depth])
    sec = time.perf_counter() - t0
    for e in exs[len(pipe.exs[:depth]):]:
        e.close()
    # what crosses the link per frame: the level-0 pixels up; keypoint + descriptor rows of `stride` entries and the count down
    # (a frame goes up as ONE run of (h - 1) x pitch + w bytes: the padding between the rows travels with them)
    return B * batches, sec, {"up": (h - 1) * hp + w, "down": stride * (KP_DTYPE.itemsize + 32) + 4, "host_row_pitch": hp}


def pcie_roofline(link, fps_per_gpu):
    """The bound of the end-to-end rate: bytes that cross the PCIe link per frame (both directions run concurrently; the upstream direction
    carries the pixels and is the one that saturates) x frames/s against one direction's peak."""
    link = dict(link)
    hp = link.pop("host_row_pitch", None)
    up, down = link["up"] * fps_per_gpu / 1e9, link["down"] * fps_per_gpu / 1e9
    return {"bound": "pcie", "achieved": round(max(up, down), 2), "peak": PCIE_PEAK_GBS, "unit": "GB/s", "frac": round(max(up, down) / PCIE_PEAK_GBS, 4),
            "up_GBs": round(up, 2), "down_GBs": round(down, 2), "bytes_per_frame": link, "host_row_pitch": hp}


def mgpu_end_to_end(devices, cfg, frames, min_seconds=0.8):
    """The product's own multi-GPU entry point (ygzf_mgpu_extract_match, include/ygzf.h): host frames in, every keypoint / descriptor / match
    out in input order, frame pairs dealt round-robin over the device slots (one host thread + two alternating contexts per slot).  With one
    device the two slots both sit on it.  Twice: frames in pageable memory (gathered into the slot's page-locked staging first) and in page-locked
    memory (copied to the device from where they lie)."""
    import torch
    from orb_ygz_slam_amd import MultiGpu, make_camera
    w, h, nl, sf, nf, ini, mn = cfg
    slots = list(devices) if len(devices) > 1 else [devices[0], devices[0]]
    # frames per slot and call: sixteen chunks of 128.  The call is synchronous -- its first upload and its last kernels / read-back / scatter overlap
    # nothing -- so its rate depends on its length: 512 frames per slot (round 4's setting) spend a fifth of the call filling and draining the
    # pipeline (100-127 k frames/s box to box); a recorded sequence handed over whole (EuRoC MH01 has 3682 frames) is the case the entry point is for
    per = 2048
    n = per * len(slots)
    clip = np.ascontiguousarray(np.concatenate([frames] * ((n + len(frames) - 1) // len(frames)))[:n])
    mg = MultiGpu(slots, nf, sf, nl, ini, mn, max_width=w, max_height=h, max_frames_per_device=per)
    cam = make_camera(w, h)
    res = {}
    from orb_ygz_slam_amd.capi import host_row_pitch
    keep = torch.zeros((n, h, host_row_pitch(w)), dtype=torch.uint8).pin_memory()      # page-locked frames at the device's row pitch: whole-frame uploads
    keep.numpy()[:, :, :w] = clip
    for name, src in (("pageable", clip), ("page_locked", keep.numpy()[:, :, :w])):
        out = mg.extract_match(src, unit=2, cam=cam)
        t0 = time.perf_counter()
        calls = 0
        while calls < 2 or time.perf_counter() - t0 < min_seconds:
            mg.extract_match(src, unit=2, cam=cam, out=out)
            calls += 1
        sec = time.perf_counter() - t0
        res[name] = {"value": round(calls * n / sec, 1), "calls": calls, "ms_per_call": round(1e3 * sec / calls, 3)}
    chunk = mg.chunk_frames()
    mg.close()
    return {"value": res["page_locked"]["value"], "value_pageable": res["pageable"]["value"], "unit": "frames/s", "frames_per_call": n, "frames_per_slot": per, "runs": res,
            "device_slots": slots, "unit_frames": 2, "chunk_frames": chunk,
            "what": "ygzf_mgpu_extract_match: host frames -> H2D -> extract + match of every pair -> D2H -> host arrays in input order (synchronous calls; "
                    "inside a call every slot sends its frames through in chunks that alternate between two contexts: the upload of one chunk runs beside "
                    "the kernels of the other; page-locked frames are copied from where they lie, pageable ones are gathered into page-locked staging by four "
                    "host threads per slot)"}


def one_unit_kernels(device, wl, unit, stereo):
    """Kernel breakdown (HIP events, us per launch) of one resident step over ONE frame / ONE stereo pair of the workload."""
    p = Pipeline(device, wl, unit, 1, 1, 7100, False, stereo, distinct=unit, match=False)   # (these configurations extract; the pair form adds ComputeStereoMatches)
    for _ in range(3):
        p.step()
    p.sync()
    p.profile(True)
    for _ in range(10):
        p.step()
    p.sync()
    k = {name: v["avg_us"] for name, v in kernel_table(p.profile_read()).items()}
    p.profile(False)
    for e in p.exs:
        e.close()
    return k


def mgpu_literal_configs(devices):
    """BASELINE.json configs[3] and configs[4] as literally stated, through the product's multi-GPU API: 1920x1080 / 8 levels / 4000 features with a batch of
    8 frames, one per device slot; 3840x2160 stereo / 12 levels / 8000 features with a batch of 16 frames = 8 (left, right) pairs, a pair per slot
    (extraction of both eyes + ComputeStereoMatches).  Eight slots: the eight GPUs of the node, or -- on the one-GPU box -- eight slots on its GPU.
    Latency of one call and the rate it amounts to; host frames page-locked."""
    import torch
    from orb_ygz_slam_amd import MultiGpu
    nd = 8
    slots = [devices[i % len(devices)] for i in range(nd)]
    out = {}
    for key, wl, nfr, stereo in (("fhd1920x1080_8lvl_4000feat_batch8", "fhd1920x1080_8lvl_4000feat", 8, False),
                                 ("uhd3840x2160_12lvl_8000feat_stereo_batch16", "uhd3840x2160_12lvl_8000feat", 16, True)):
        w, h, nl, sf, nf, ini, mn = WORKLOADS[wl]
        base = make_frames(8, w, h, seed0=7000)
        clip = np.ascontiguousarray(np.concatenate([base] * ((nfr + 7) // 8))[:nfr])
        if stereo:
            clip[1::2, :, :w - 24] = clip[0::2, :, 24:]           # right eye = the left image shifted by a disparity
        keep = torch.from_numpy(clip).pin_memory()
        src = keep.numpy()
        mg = MultiGpu(slots, nf, sf, nl, ini, mn, max_width=w, max_height=h, max_frames_per_device=2)
        run = (lambda o=None: mg.extract_stereo(src, 0.11, 47.9, out=o)) if stereo else (lambda o=None: mg.extract_match(src, unit=1, out=o))
        o = run()
        lat = []
        t0 = time.perf_counter()
        while len(lat) < 5 or time.perf_counter() - t0 < 0.5:
            t1 = time.perf_counter()
            run(o)
            lat.append(time.perf_counter() - t1)
        lat.sort()
        med = lat[len(lat) // 2]
        kp = int(np.asarray(o[2]).mean())
        matched = int((np.asarray(o[3]) >= 0).sum(axis=1).mean()) if stereo else None
        mg.close()
        # what ONE GPU of the node does in such a call: one FHD frame / one UHD stereo pair, alone on its device (one slot)
        unit = 2 if stereo else 1
        mg1 = MultiGpu([devices[0]], nf, sf, nl, ini, mn, max_width=w, max_height=h, max_frames_per_device=2)
        src1 = src[:unit]
        run1 = (lambda o=None: mg1.extract_stereo(src1, 0.11, 47.9, out=o)) if stereo else (lambda o=None: mg1.extract_match(src1, unit=1, out=o))
        o1 = run1()
        lat1 = []
        t0 = time.perf_counter()
        while len(lat1) < 9 or time.perf_counter() - t0 < 0.4:
            t1 = time.perf_counter()
            run1(o1)
            lat1.append(time.perf_counter() - t1)
        lat1.sort()
        med1 = lat1[len(lat1) // 2]
        mg1.close()
        one = {"frames_per_call": unit, "ms_per_call": round(1e3 * med1, 3), "min_ms": round(1e3 * lat1[0], 3), "calls": len(lat1),
               "extrapolated_8gpu_frames_per_s": round(8 * unit / med1, 1),
               "kernels_us": one_unit_kernels(devices[0], wl, unit, stereo),
               "what": "ONE %s per call on ONE device slot, page-locked host frames in, results out: the per-GPU work of this configuration; "
                       "extrapolated_8gpu = 8 x frames / this latency (an EXTRAPOLATION from one GPU -- eight GPUs, eight links, one unit each -- not a measurement)" % ("(left, right) pair" if stereo else "frame")}
        out[key] = {"frames_per_call": nfr, "device_slots": slots, "unit_frames": 2 if stereo else 1, "ms_per_call": round(1e3 * med, 3), "one_unit": one,
                    "value": round(nfr / med, 1), "unit": "frames/s", "calls": len(lat), "keypoints_per_frame": kp,
                    "stereo_matches_per_pair": matched,
                    "what": ("ygzf_mgpu_extract_stereo" if stereo else "ygzf_mgpu_extract_match (extraction only)") +
                            ": page-locked host frames in, keypoints / descriptors" + (" / uRight / depth" if stereo else "") + " out, one synchronous call"}
    return out


def isolated_pass(pipe, reps=2):
    """Untimed extra launches, one context at a time, so that per-kernel durations are not stretched by the other streams."""
    acc = {}
    for s, e in enumerate(pipe.exs):
        e.profile_enable(True)
        e.profile_reset()
        for _ in range(reps):
            pipe.launch(e, pipe.ptrs[0][s])
            e.sync()
        for name, (ms, n) in e.profile_read().items():
            a = acc.get(name, (0.0, 0))
            acc[name] = (a[0] + ms, a[1] + n)
        e.profile_enable(False)
    return {k: round(1e3 * v[0] / v[1], 2) for k, v in acc.items() if v[1]}


def kernel_table(prof):
    return {name: {"launches": n, "avg_us": round(1e3 * ms / n, 2), "total_ms": round(ms, 3)} for name, (ms, n) in prof.items() if n}


def hbm_roofline(workload, kernels, iso, per_kernel, frames_per_launch, total_bytes, fps_per_gpu, only=None, with_traffic=True, traffic_key=None):
    cand = [k for k in kernels if per_kernel.get(k, 0) > 0 and (only is None or k == only)]
    if not cand:
        return None
    # dominant = the kernel that takes the most device time per sub-batch when it runs ALONE (isolated mean x its launches per sub-batch); the
    # in-pipeline totals rank by how much a kernel is stretched by the other contexts, not by what it costs
    nl1 = WORKLOADS[workload][2] - 1
    dom = max(cand, key=lambda k: (iso.get(k) or kernels[k]["avg_us"]) * (nl1 if k == "k_pyr_resize" else 1))
    div = nl1 if dom == "k_pyr_resize" else 1      # the L-1 resize launches share the pyramid's bytes
    bytes_per_launch = per_kernel[dom] * frames_per_launch / div
    avg_s = kernels[dom]["avg_us"] * 1e-6
    achieved = bytes_per_launch / avg_s / 1e9
    traffic = None
    tfile = os.path.join(ROOT, "profiles", "traffic.json")
    if with_traffic and os.path.exists(tfile):
        try:
            traffic = json.load(open(tfile)).get(traffic_key or workload, {}).get(dom)
        except Exception:
            traffic = None
    iso_us = iso.get(dom)
    return {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBS, 5), "traffic": traffic, "algorithmic_bytes_per_launch": int(bytes_per_launch),
            "isolated_avg_us": iso_us,
            "isolated_frac": round(bytes_per_launch / (iso_us * 1e-6) / 1e9 / HBM_PEAK_GBS, 5) if iso_us else None,
            "pipeline_achieved": round(total_bytes * fps_per_gpu / 1e9, 2),
            "pipeline_frac": round(total_bytes * fps_per_gpu / 1e9 / HBM_PEAK_GBS, 5)}


def valu_roofline(workload, kernels, iso, frames_per_launch):
    """Vector-ALU issue roofline of the dominant kernel.  profiles/valu_mix.json (tools/valu_mix.py) holds, per kernel, the VALU
    instructions per frame (SQ_INSTS_VALU of the PMC profile) and the mean issue cost of one instruction in SIMD cycles (instruction mix of
    the kernel's ISA weighted with the per-opcode costs calibrated by tools/micro/valu_peak.hip: 2 cycles for the full-rate 32-bit ops, 4 for
    the byte / packed / three-operand ones).  achieved = issue cycles per launch / launch time; peak = 1024 SIMDs x 2.4 GHz."""
    f = os.path.join(ROOT, "profiles", "valu_mix.json")
    if not os.path.exists(f):
        return None
    try:
        mix = json.load(open(f)).get(workload, {})
    except Exception:
        return None
    cand = [k for k in kernels if k in mix]
    if not cand:
        return None
    dom = max(cand, key=lambda k: kernels[k]["total_ms"])
    m = mix[dom]
    cycles = m["valu_insts_per_frame"] * frames_per_launch * m["cycles_per_inst"]
    peak = SIMDS * CLOCK_GHZ                                      # G SIMD-cycles / s
    ach = cycles / (kernels[dom]["avg_us"] * 1e-6) / 1e9
    iso_us = iso.get(dom)
    return {"bound": "valu", "kernel": dom, "achieved": round(ach, 1), "peak": round(peak, 1), "unit": "G SIMD-issue-cycles/s",
            "frac": round(ach / peak, 4), "valu_insts_per_frame": m["valu_insts_per_frame"], "cycles_per_inst": m["cycles_per_inst"],
            "isolated_frac": round(cycles / (iso_us * 1e-6) / 1e9 / peak, 4) if iso_us else None,
            "source": "profiles/valu_mix.json"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="frames per GPU per step (default: sub-batch x streams x rounds of the workload, "
                                                          "9216 for the 752x480 metric)")
    ap.add_argument("--sub-batch", type=int, default=0, help="frames per extractor launch (default per workload: 256 / 32 / 8)")
    ap.add_argument("--streams", type=int, default=3,
                    help="independent extractor contexts (own HIP stream + buffers) the sub-batches rotate over, so that the "
                         "latency-bound kernels of one sub-batch overlap the throughput-bound kernels of another")
    ap.add_argument("--workload", default="euroc752x480_8lvl_1000feat", choices=sorted(WORKLOADS))
    ap.add_argument("--align", action="store_true",
                    help="BASELINE config 3: also run SparseImgAlign (levels L-1..1, 10 iterations) of every frame against its "
                         "predecessor; `metric` stays extract+match, the step simply carries the extra work (see config.align)")
    ap.add_argument("--stereo", action="store_true",
                    help="BASELINE config 5 shape: the batch holds (left, right) pairs; Frame::ComputeStereoMatches runs on every pair "
                         "after extraction (extra work inside the step, see config.stereo)")
    ap.add_argument("--devices-in-process", type=int, default=1,
                    help="shard over this many devices inside ONE process (one host thread + contexts per device, SURVEY 8e) instead of / "
                         "in addition to one process per GPU")
    ap.add_argument("--reuse-devices", action="store_true",
                    help="testing aid for --devices-in-process on a box with fewer GPUs: logical device i runs on physical device i %% count "
                         "(exercises the threaded path; the line is then NOT a scaling measurement and says so)")
    ap.add_argument("--passes", type=int, default=0,
                    help="times the resident clip is walked per step (default 6 for the 752x480 / 640x480 workloads: the driver's 20 steps then time "
                         "about five seconds; 1 otherwise)")
    ap.add_argument("--distinct", type=int, default=0, help="distinct synthetic frames of the resident clip (default streams x sub-batch; the clip "
                                                            "tiles them) -- profiling runs of the 4K shape use 8 so that the host-side synthesis stays short")
    ap.add_argument("--share-gpu", action="store_true",
                    help="TEST ONLY: every rank of a multi-process run uses device 0 and the ranks rendezvous over gloo -- the N > 1 control flow (barriers, "
                         "max-over-ranks, per-rank extras) on a box with one GPU; never a valid measurement (the line says so)")
    ap.add_argument("--backend", default="auto", choices=("auto", "nccl", "gloo"),
                    help="what carries the timing barrier and the max-over-ranks reduction of an N > 1 run (there is no collective on the data path): "
                         "nccl = RCCL, gloo = TCP on the host, auto (default) = RCCL when its communicator comes up on every rank, gloo otherwise")
    ap.add_argument("--no-numa-bind", action="store_true", help="do not bind the rank's host thread to the NUMA node of its GPU")
    ap.add_argument("--share-gpu-try-rccl", action="store_true",
                    help="TEST ONLY, with --share-gpu: still try to bring up the RCCL communicator (two ranks on one device: it is expected to refuse) so that "
                         "the all-ranks-together fallback to gloo is exercised on a one-GPU box")
    ap.add_argument("--other-steps", type=int, default=0, help="timed steps of every other_workloads entry (default: max(20, --steps), i.e. >= 1 s each; tests shorten it)")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beyond the headline as well: per-kernel profile and rooflines, CPU baselines, value_end_to_end, host_stream, "
                         "the multi-GPU entry point and other_workloads (a plain run only sets up, warms up, times the steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step computed (counts of every frame of the contexts' last sub-batches; "
                         "keypoints, descriptors, matches of a fixed, seeded sample of them) as DIR/<name>.npy, float32 / float64")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baselines")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-profile", action="store_true", help="with --full: do not bracket kernels with HIP events in the timed region")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip value_end_to_end and other_workloads")
    ap.add_argument("--plumbing-selftest", action="store_true",
                    help="CPU-only check of the multi-process plumbing (gloo): no GPU work, output is NOT a measurement")
    args = ap.parse_args()
    cpu_baselines = args.full and not args.no_cpu_baseline
    profile = args.full and not args.no_profile
    extras = args.full and not args.no_extras

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        raise SystemExit("WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))
    cfg = WORKLOADS[args.workload]
    w, h, nl, sf, nf, ini, mn = cfg
    S = max(1, args.streams)
    sub, rounds = SHAPES[args.workload]
    if args.sub_batch:
        sub = args.sub_batch
    if args.batch:
        if args.batch % (S * sub):
            raise SystemExit("--batch must be a multiple of --streams x --sub-batch (%d)" % (S * sub))
        rounds = args.batch // (S * sub)
    if args.stereo and sub % 2:
        raise SystemExit("--stereo needs an even --sub-batch")
    passes = args.passes if args.passes > 0 else (6 if args.workload in ("euroc752x480_8lvl_1000feat", "vga640x480_8lvl_1000feat") and not args.batch else 1)
    B = S * sub * rounds * passes                  # frames per GPU per step
    ndev = max(1, args.devices_in_process)

    import torch
    dist = None
    use_gpu = not args.plumbing_selftest
    share = bool(args.share_gpu)
    if share:
        local_rank = 0
    nccl = use_gpu and (not share or args.share_gpu_try_rccl) and args.backend != "gloo"
    if use_gpu and torch.cuda.is_available():
        torch.cuda.set_device(local_rank * ndev)   # before the process group: RCCL binds its communicator to the current device
    group = None
    backend_note = None
    if world > 1:
        import datetime
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # The control plane (rendezvous, agreement on what carries the barrier) is gloo: it needs nothing from the GPUs.  The timing barrier and the
        # max-over-ranks reduction go over RCCL when its communicator comes up on EVERY rank; a rank where it does not reports that over gloo and all
        # ranks fall back together (--backend auto), so a hiccup of RCCL costs the run its transport, not its result.
        dist.init_process_group(backend="gloo", timeout=datetime.timedelta(seconds=600))
        if nccl:
            ok = 1
            try:
                group = dist.new_group(backend="nccl", timeout=datetime.timedelta(seconds=120))
                t = torch.ones(1, device="cuda:%d" % (local_rank * ndev))
                dist.all_reduce(t, group=group)
                torch.cuda.synchronize(local_rank * ndev)
                ok = int(float(t[0]) == world)
            except Exception as e:                   # noqa: BLE001 -- whatever RCCL raised, the answer is the same
                ok = 0
                backend_note = "RCCL unavailable on rank %d: %s" % (rank, str(e).splitlines()[0][:200])
            flag = torch.tensor([ok], dtype=torch.int32)
            dist.all_reduce(flag, op=dist.ReduceOp.MIN)
            if int(flag[0]) == 0:
                if args.backend == "nccl":
                    raise SystemExit("--backend nccl: the RCCL communicator did not come up on every rank (%s)" % backend_note)
                nccl, group = False, None
                backend_note = backend_note or "RCCL unavailable on another rank"

    def barrier():
        if dist is not None:
            if nccl:
                dist.barrier(group=group, device_ids=[local_rank * ndev])
            else:
                dist.barrier()

    def max_over_ranks(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=("cuda:%d" % (local_rank * ndev)) if nccl else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
        return float(t[0])

    if args.plumbing_selftest:
        # exercises the N > 1 path without a GPU, with REAL data through every step it has: the clip is dealt round-robin over the ranks (the
        # sharding of DESIGN.md section 5), every rank runs the CPU oracle on its shard, the per-frame keypoint counts are all-gathered,
        # the elapsed time is max-reduced.  Never a valid measurement.
        from oracle import oracle_py as O
        from orb_ygz_slam_amd.synth import synth_frame
        pw, ph, pn = 320, 240, 8
        clip = np.stack([synth_frame(4000 + i, pw, ph) for i in range(pn)])
        mine = list(range(rank, pn, world))
        barrier()
        t0 = time.perf_counter()
        oex = O.Extractor(500, 1.2, 4, 20, 7)
        counts = torch.full((pn,), -1, dtype=torch.int64)
        for f in mine:
            counts[f] = len(oex.extract(clip[f])[0])
        time.sleep(0.01 * (rank + 1))
        el = max_over_ranks(time.perf_counter() - t0)
        if dist is not None:
            gathered = [torch.empty_like(counts) for _ in range(world)]
            dist.all_gather(gathered, counts)
            counts = torch.stack(gathered).max(dim=0).values      # every frame was counted by exactly one rank
        if rank == 0:
            print(json.dumps({"plumbing_selftest": True, "n_gpus": world, "frames_per_rank": B, "max_elapsed_s": el,
                              "shard_keypoint_counts": [int(x) for x in counts], "sharding": "frame f -> rank f % world", "valid_measurement": False}))
        if dist is not None:
            dist.destroy_process_group()
        return

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device: the hot path has no CPU fallback")
    have = torch.cuda.device_count()
    devices = [local_rank * ndev + i for i in range(ndev)]
    if args.reuse_devices:
        devices = [d % have for d in devices]
    if devices[-1] >= have:
        raise SystemExit("device %d requested but only %d visible (no extrapolation: SURVEY 8e)" % (devices[-1], have))

    def sync_all():
        for d in devices:
            torch.cuda.synchronize(d)

    # ---- CPU baselines FIRST (rank 0 of a 1-GPU run): the GPU's timed region then lies in the second half of the command, where an external
    # utilisation sampler sees it, instead of being followed by ~18 s of host-only work
    frames0 = make_frames(min(S * sub, args.distinct) if args.distinct > 0 else S * sub, w, h, seed0=1000 + 97 * (rank * ndev))
    cpu_base = cpu_ref = anchor = None
    if rank == 0 and world * ndev == 1 and cpu_baselines:
        cpu_base = cpu_baseline(frames0, cfg, args.cpu_seconds)
        cpu_ref = cpu_baseline_reference(frames0, cfg, min(6.0, args.cpu_seconds))
        anchor = libfast_anchor(frames0)

    # the rank's host thread onto the CPUs of its GPU's NUMA node BEFORE anything is page-locked: the frames of value_end_to_end are then first
    # touched on the socket the GPU's link ends on (a two-socket 8-GPU node would otherwise stage half of its ranks across the socket link).
    # After the CPU baselines, which use every core the launcher allowed.
    numa_cpus = 0
    if not args.no_numa_bind and ndev == 1:
        from orb_ygz_slam_amd.capi import bind_host_thread_to_device
        numa_cpus = max(0, bind_host_thread_to_device(devices[0]))

    pipes = [Pipeline(d, args.workload, sub, rounds, S, 1000 + 97 * (rank * ndev + i), args.align, args.stereo, frames=frames0 if i == 0 else None, passes=passes,
                      distinct=args.distinct if args.distinct > 0 else None)
             for i, d in enumerate(devices)]
    if profile:
        pipes[0].passes = 1
        pipes[0].step(); pipes[0].sync()           # first-touch allocations out of the way before events are recorded
        pipes[0].passes = passes
        pipes[0].profile(True)
    my_elapsed = run_timed(pipes, args.steps, args.warmup, barrier, sync_all)
    elapsed = max_over_ranks(my_elapsed)
    per_rank = None
    if dist is not None:          # a straggler must be visible in ONE scaling run, not hidden by the max-reduce
        allel = [torch.zeros(1, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(allel, torch.tensor([my_elapsed], dtype=torch.float64))
        allel = [float(t[0]) for t in allel]
        per_rank = {"elapsed_s": [round(x, 4) for x in allel], "min_s": round(min(allel), 4), "max_s": round(max(allel), 4),
                    "slowest_rank": int(np.argmax(allel)), "spread": round(max(allel) / max(min(allel), 1e-9) - 1.0, 4)}
    n_gpus = world * ndev
    total_frames = n_gpus * B * args.steps
    fps = total_frames / elapsed

    pipe = pipes[0]
    fast_plan_id = pipe.exs[0].fast_plan()   # before the contexts are released further down
    if args.dump_outputs and rank == 0:      # before anything else launches on these contexts
        dump_outputs(pipe, args.dump_outputs)
    kernels, iso = {}, {}
    if profile:
        prof = pipe.profile_read()
        pipe.profile(False)
        # the profile covers warm-up + timed steps of device 0 (same launches; events are only read here, after the region)
        kernels = kernel_table(prof)
        # untimed extra pass: one context at a time, so that per-kernel durations are not stretched by the other streams
        iso = isolated_pass(pipe)
    match_fallbacks = sum(e.match_fallbacks() for e in pipe.exs)
    kp_counts = np.concatenate([e.batch_counts() for e in pipe.exs])
    m_counts = np.concatenate([e.match_counts() for e in pipe.exs])

    # ---- end-to-end (PCIe inclusive) on every rank at once ----
    e2e = None
    if extras:
        barrier()
        nfr, sec, link = end_to_end(pipe)
        sec = max_over_ranks(sec)
        e2e = {"value": round(world * nfr / sec, 1), "unit": "frames/s", "frames": world * nfr, "roofline_pcie": pcie_roofline(link, nfr / sec),
               "what": "pinned host frames -> H2D -> extract + match -> D2H of all keypoints, descriptors and counts; two contexts "
                       "software-pipelined per GPU (device 0 of each process)"}

    # ---- what the host's memory can feed (no GPU work): the 8-GPU transfers-included rate needs eight links' worth of DRAM reads at once ----
    host_stream = None
    if extras and rank == 0:
        from orb_ygz_slam_amd.capi import host_stream_probe
        nthr = min(effective_cores(), 16)
        gbs = host_stream_probe(devices[0], nthr, 256 << 20, 1.0)
        up_one = (e2e["roofline_pcie"]["up_GBs"] if e2e else None)
        host_stream = {"host_stream_GBs": round(gbs, 1), "threads": nthr, "bytes_per_thread": 256 << 20, "seconds": 1.0,
                       "one_gpu_upload_GBs": up_one, "eight_gpus_would_read_GBs": round(8 * up_one / max(world, 1), 1) if up_one else None,
                       "what": "threads bound to the GPU's NUMA node stream-read page-locked frame buffers, no GPU involved (ygzf_host_stream_probe); "
                               "eight_gpus_would_read = 8 x this GPU's measured upload rate: an 8-GPU transfers-included run is host-memory-bound "
                               "when that exceeds what ALL the node's cores can stream (this probe used only the cores this process may use)"}

    mgpu = mgpu_lit = None
    if extras and world == 1:
        mgpu = mgpu_end_to_end(devices, cfg, frames0)

    # ---- short runs of the other BASELINE configurations (their own contexts; each rank its own clip) ----
    others = {}
    if extras and args.workload == "euroc752x480_8lvl_1000feat" and not args.align and not args.stereo:
        for p in pipes:
            for e in p.exs:
                e.close()
        del pipes
        torch.cuda.empty_cache()
        # (name, workload, SparseImgAlign, stereo pairs, real-image clip, matcher, passes over the resident clip per step): every one is timed over
        # max(20, --steps) steps of >= 50 ms, i.e. >= 1 s, after 2 warm-up steps -- >= 200 frames after >= 20 warm-up frames many times
        # over -- and gets its own cpu_baseline on a bounded sample of its own clip
        o_steps = args.other_steps if args.other_steps > 0 else max(20, args.steps)
        for name, wl, o_align, o_stereo, o_real, o_match, o_passes in (
                ("fhd1920x1080_8lvl_4000feat", "fhd1920x1080_8lvl_4000feat", False, False, False, True, 7),
                ("uhd3840x2160_12lvl_8000feat_stereo", "uhd3840x2160_12lvl_8000feat", False, True, False, True, 4),
                ("euroc752x480_8lvl_1000feat_align", "euroc752x480_8lvl_1000feat", True, False, False, True, 4),
                ("vga640x480_8lvl_1000feat_extract_only", "vga640x480_8lvl_1000feat", False, False, False, False, 7),
                ("euroc752x480_test1png", "euroc752x480_8lvl_1000feat", False, False, True, True, 6)):
            osub, orounds = SHAPES[wl]
            orounds = 1 if wl not in ("euroc752x480_8lvl_1000feat", "vga640x480_8lvl_1000feat") else max(1, orounds // 4)
            oframes = make_frames_test1png(96, WORKLOADS[wl][0], WORKLOADS[wl][1]) if o_real else None
            odistinct = min(S * osub, 64 if ("uhd" in wl or "fhd" in wl) else 96)
            ps = [Pipeline(d, wl, osub, orounds, S, 5000 + 31 * (rank * ndev + i), o_align, o_stereo, distinct=odistinct, frames=oframes, passes=o_passes,
                           match=o_match)
                  for i, d in enumerate(devices)]
            ps[0].passes = 1
            ps[0].step(); ps[0].sync()
            ps[0].passes = o_passes
            ps[0].profile(True)
            el = max_over_ranks(run_timed(ps, o_steps, 2, barrier, sync_all))
            oprof = kernel_table(ps[0].profile_read())
            ps[0].profile(False)
            oiso = isolated_pass(ps[0], reps=1)
            oframes_step = ps[0].batch * o_passes
            ofps = n_gpus * oframes_step * o_steps / el
            ow, oh, onl, osf, onf = WORKLOADS[wl][:5]
            tb, per = algorithmic_bytes(ow, oh, onl, osf, onf)
            okp = np.concatenate([e.batch_counts() for e in ps[0].exs])
            if o_align and "k_sia_run" in oprof:
                # what k_sia_run moves per pair (the bytes SURVEY 8(d)'s on-chip form counts plus the image rows it reads): per level and feature
                # 7 x 8 reference bytes once, then per iteration 5 x 8 bytes of the current image and the 25 B of cached patch / Jacobian terms
                per = dict(per)
                per["k_sia_run"] = int((onl - 1) * float(okp.mean()) * (56 + 10 * (40 + 25)))
                tb += per["k_sia_run"]
            entry = {"value": round(ofps, 1), "unit": "frames/s" if not o_stereo else "frames/s (2 frames = 1 stereo pair)", "ms_per_step": round(1e3 * el / o_steps, 3),
                     "frames_per_gpu_per_step": oframes_step, "steps": o_steps, "warmup": 2, "timed_region_s": round(el, 3), "distinct_frames": len(ps[0].frames),
                     "what": "extract" + (" + match" if o_match else " only (BASELINE.json configs[1])") + (" + SparseImgAlign" if o_align else "") + (" + ComputeStereoMatches" if o_stereo else ""),
                     "roofline": hbm_roofline(wl, oprof, oiso, per, osub, tb, ofps / n_gpus, traffic_key=name),
                     "kernels": {k: v["avg_us"] for k, v in oprof.items()},
                     "kernels_isolated_avg_us": oiso,
                     "keypoints_per_frame": round(float(okp.mean()), 1),
                     "matches_per_frame": round(float(np.concatenate([e.match_counts() for e in ps[0].exs]).mean()), 1) if o_match else None}
            if rank == 0 and world * ndev == 1 and cpu_baselines:
                # the CPU beside it, on this workload's own clip (north_star: "timed on the node's own host cores in the same run")
                entry["cpu_baseline"] = cpu_baseline(ps[0].frames, WORKLOADS[wl], seconds_budget=min(args.cpu_seconds, 6.0 if "uhd" in wl else 4.0),
                                                     match=o_match, align=o_align, stereo=o_stereo, one_thread=False)
            if o_real:
                entry["data"] = ("96 frames cut from the reference's Thirdparty/fast/test/data/test1.png (the one real image it ships; pixels from "
                                 "tests/golden/fast10_test1.npz): mirror-padded, 12 zoom levels 1.00 .. 1.22, shifted crops")
                entry["fast_plan"] = {1: "one pass at minTh", 2: "iniTh first"}.get(ps[0].exs[0].fast_plan(), "?")
            if not o_real and not o_align:
                # SURVEY 8(d)'s rate for this shape too: H2D of every frame and D2H of every keypoint / descriptor inside
                onfr, osec, olink = end_to_end(ps[0], min_seconds=1.0)
                osec = max_over_ranks(osec)
                entry["value_end_to_end"] = round(world * onfr / osec, 1)
                entry["roofline_pcie"] = pcie_roofline(olink, onfr / osec)
            others[name] = entry
            for p in ps:
                for e in p.exs:
                    e.close()
            del ps
            torch.cuda.empty_cache()

    if extras and world == 1 and args.workload == "euroc752x480_8lvl_1000feat" and not args.align and not args.stereo:
        mgpu_lit = mgpu_literal_configs(devices)

    if rank == 0:
        total_bytes, per_kernel = algorithmic_bytes(w, h, nl, sf, nf)
        fast_plan = {1: "one pass at minTh", 2: "iniTh first"}.get(fast_plan_id, "?") + " (chosen by the library from the clip's statistics)"
        roofline = hbm_roofline(args.workload, kernels, iso, per_kernel, sub, total_bytes, fps / n_gpus) if kernels else None
        out = {
            "metric": "frames/s ORB extract+match, 752x480 8-lvl 1000-feat; 1->8 GPU scaling",
            "value": round(fps, 1), "unit": "frames/s",
            "value_definition": "kernel-only: frames resident in HBM when the timed region starts, results left in HBM (the bench contract); "
                                "value_end_to_end is SURVEY 8(d)'s rate with H2D of every frame and D2H of every keypoint / descriptor inside",
            "n_gpus": n_gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": args.workload, "width": w, "height": h, "levels": nl, "scale_factor": sf, "features": nf,
                       "frames_per_gpu_per_step": B, "sub_batch": sub, "rounds_per_step": rounds, "passes_per_step": passes,
                       "resident_clip_frames": S * sub * rounds, "streams": S, "distinct_frames": min(B, S * sub),
                       "align": bool(args.align), "stereo": bool(args.stereo),
                       "match": "SearchByProjection(cur,last) th=15, identity pose", "fast_plan": fast_plan, "processes": world, "devices_per_process": ndev, "devices_reused": bool(args.reuse_devices and len(set(devices)) < len(devices)),
                       "sharding": "one clip per GPU, no collective", "valid_measurement": not share,
                       "barrier_backend": ("rccl" if nccl else "gloo") if world > 1 else None, "barrier_backend_note": backend_note,
                       "numa_bound_cpus": numa_cpus},
            "timed_region_s": round(elapsed, 4), "per_rank": per_rank, "host_stream": host_stream,
            "value_end_to_end": e2e["value"] if e2e else None, "end_to_end": e2e, "roofline_pcie": e2e["roofline_pcie"] if e2e else None,
            "mgpu_end_to_end": mgpu, "mgpu_literal_configs": mgpu_lit,
            "keypoints_per_frame": round(float(kp_counts.mean()), 1), "matches_per_frame": round(float(m_counts.mean()), 1),
            "match_serial_fallback_pairs": match_fallbacks,   # pairs of device 0 (whole run) that lost the matcher's fixpoint to the one-wave pass
            "roofline": roofline,
            "roofline_valu": valu_roofline(args.workload, kernels, iso, sub) if kernels else None,
            "kernels": kernels,
            "kernels_isolated_avg_us": iso,   # one stream at a time (untimed pass)
            "other_workloads": others or None,
        }
        if roofline is not None and e2e:
            # the two blocks the driver's record keeps verbatim carry SURVEY 8(d)'s own number too: `value` is the resident (kernel-only) rate
            roofline["value_end_to_end"] = e2e["value"]
            roofline["value_end_to_end_pcie_frac"] = e2e["roofline_pcie"]["frac"]
            out["config"]["value_end_to_end"] = e2e["value"]
            out["config"]["value_end_to_end_pcie_frac"] = e2e["roofline_pcie"]["frac"]
        out["cpu_baseline"] = cpu_base
        if cpu_ref is not None:
            out["cpu_baseline_reference"] = cpu_ref
        if anchor is not None:
            out["libfast_sse2_anchor"] = anchor
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
