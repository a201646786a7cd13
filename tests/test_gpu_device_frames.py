"""ygzf_extract_batch_device on real data: caller-owned device frames at every pitch class (tests/device_frame_cases.py).

This is the entry point bench.py's `value` is measured through -- pointers into a torch tensor, row_pitch = w, frame_stride = w * h, sub-batches
at p0 + k * sub * w * h -- and the only one whose level 0 is not the context's own buffer (pitch a multiple of 64, 256-byte aligned base).  The
branches that exist only for it: describe_window's rowOffStep = pitch & 15 and rowOff0, pyr_tile's tail chunk, fast_cell's / fast_tab_cell's /
k_pyr_strips' rows at the caller's pitch, and every later reader of the held frames (ygzf_describe_keys, ygzf_stereo_batch,
ygzf_batch_fetch_level(.., 0, ..)).  All expectations are exact.

Device memory comes from torch, as in bench.py, so the work runs in ONE child process for the module (torch initialises the device before the
library does); the child writes one record per case -- the list of what differed, empty when nothing did -- and the parametrised tests read them.
Every layout runs on two long-lived contexts per geometry: the library's own plans for a launch of a few frames (k_pyr_strips, k_fast_tab) and the
plans of bench-sized launches pinned (k_pyr_resize_tiled = pyr_tile; k_fast_quads = fast_cell)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import device_frame_cases as D
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

LAYOUT_IDS = [lay.name for c, lay in D.all_layouts() if c.name not in ("pitch_sequence", "bench_clip")]
DESCRIBE_IDS = ["describe_" + n for n in D.DESCRIBE_LAYOUTS]
STEREO_IDS = [lay.name for lay in D.STEREO_LAYOUTS]
OTHER_IDS = ["pitch_sequence", "bench_clip", "switch_device_then_host", "switch_host_then_device", "argument_errors"]
VARIANTS = ("own_plans", "bench_plans")
CV_MODES = (0, 2)                                   # YGZF_CV_LEGACY_SSE2, YGZF_CV_4


# ---- the child ------------------------------------------------------------------------------------------------------------------------------------
class _Child:
    def __init__(self):
        import torch
        from oracle import oracle_py
        oracle_py.build()
        self.torch, self.O = torch, oracle_py
        self.records = {}
        self.ctx = {}
        self.keep = []              # every uploaded tensor: a context reads its held frames until its next extraction (include/ygzf.h)
        self.expected = {}

    def record(self, name, lay=None, **info):
        r = self.records.setdefault(name, {"failures": [], "info": {}})
        if lay is not None:
            r["info"].update(pitch_mod16=lay.row_pitch % 16, classes={k: v for k, v in D.layout_classes(lay).items()})
        r["info"].update(info)
        return r["failures"]

    def extractor(self, w, h, nlevels, nfeatures, max_batch, variant="own_plans", cv_mode=0, fast_register_staging=True):
        """one long-lived context per (geometry, configuration, variant)"""
        key = (w, h, nlevels, nfeatures, max_batch, variant, cv_mode, fast_register_staging)
        if key not in self.ctx:
            from orb_ygz_slam_amd import Extractor
            from orb_ygz_slam_amd.capi import force_env
            old = os.environ.get("YGZF_FORCE")
            if variant == "bench_plans":            # (read when the context is created)
                os.environ["YGZF_FORCE"] = force_env(pyr_strip_frames=0)
            try:
                ex = Extractor(nfeatures, D.SCALE_FACTOR, nlevels, D.INI_TH, D.MIN_TH, max_width=w, max_height=h, max_batch=max_batch, cv_mode=cv_mode)
            finally:
                if old is None:
                    os.environ.pop("YGZF_FORCE", None)
                else:
                    os.environ["YGZF_FORCE"] = old
            if variant == "bench_plans" and fast_register_staging:
                ex.set_fast_kernel(1)               # YGZF_FAST_KERNEL_REGISTER_STAGING: k_fast_quads
            self.ctx[key] = ex
        return self.ctx[key]

    def upload(self, lay, frames):
        buf, off0 = D.layout_buffer(lay, frames)
        t = self.torch.from_numpy(buf).to("cuda:0")
        assert t.data_ptr() % D.BUFFER_ALIGN == 0, "the allocator's alignment: the layouts' base classes rest on it"
        self.keep.append(t)
        return t.data_ptr() + off0

    def extract_device(self, ex, lay, ptr, first=0, n=None):
        n = lay.n if n is None else n
        ex.extract_batch_device(ptr + first * lay.frame_stride, n, lay.w, lay.h, lay.row_pitch, lay.frame_stride)

    def oracle_frames(self, case):
        """(keypoints, descriptors) of every frame of the case from the CPU oracle, once"""
        if case.name not in self.expected:
            oex = self.O.Extractor(case.nfeatures, D.SCALE_FACTOR, case.nlevels, D.INI_TH, D.MIN_TH)
            self.expected[case.name] = [oex.extract(f) for f in D.case_frames(case)]
        return self.expected[case.name]

    # -- comparisons: they append to `fails` and never raise
    @staticmethod
    def same_keys(fails, tag, k, d, ek, ed):
        if len(k) != len(ek):
            fails.append("%s: %d keypoints, expected %d" % (tag, len(k), len(ek)))
            return
        for fld in k.dtype.names:
            a, b = k[fld], ek[fld]
            bad = (a.view(np.uint32) != b.view(np.uint32)) if a.dtype.kind == "f" else (a != b)
            if bad.any():
                fails.append("%s: keypoint field %s differs in %d of %d" % (tag, fld, int(bad.sum()), len(k)))
        if not np.array_equal(d, ed):
            fails.append("%s: descriptors differ in %d of %d rows" % (tag, int((d != ed).any(axis=1).sum()), len(d)))

    @staticmethod
    def same_bits(fails, tag, a, b):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if a.shape != b.shape or not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            fails.append("%s differs" % tag)

    def host_results(self, ex, frames, nlevels):
        ex.extract_batch_host(frames)
        kd = [ex.batch_fetch(f) for f in range(len(frames))]
        lv = [[ex.batch_fetch_level(f, l) for l in range(nlevels)] for f in range(len(frames))]
        return kd, lv

    def check_device_batch(self, fails, tag, ex, case, lay, ptr, host):
        frames = D.case_frames(case)
        exp = self.oracle_frames(case)
        self.extract_device(ex, lay, ptr)
        hkd, hlv = host
        for f in range(lay.n):
            k, d = ex.batch_fetch(f)
            self.same_keys(fails, "%s frame %d vs the host path" % (tag, f), k, d, *hkd[f])
            self.same_keys(fails, "%s frame %d vs the oracle" % (tag, f), k, d, *exp[f])
            for l in range(case.nlevels):
                got = ex.batch_fetch_level(f, l)
                self.same_bits(fails, "%s frame %d level %d vs the host path" % (tag, f, l), got, hlv[f][l])
                if l == 0:
                    self.same_bits(fails, "%s frame %d level 0 vs the tight frame" % (tag, f), got, frames[f])

    # -- the cases
    def layouts(self):
        for case in D.CASES:
            if case.name in ("pitch_sequence", "bench_clip"):
                continue
            frames = D.case_frames(case)
            for variant in VARIANTS:
                ex = self.extractor(case.w, case.h, case.nlevels, case.nfeatures, 3, variant)
                host = self.host_results(ex, frames, case.nlevels)
                for f in range(len(frames)):
                    self.same_keys(self.record(case.layouts[0].name, case.layouts[0]), "%s: host path frame %d vs the oracle" % (variant, f),
                                   *host[0][f], *self.oracle_frames(case)[f])
                for lay in case.layouts:
                    fails = self.record(lay.name, lay, keypoints=[len(k) for k, _ in self.oracle_frames(case)])
                    self.check_device_batch(fails, variant, ex, case, lay, self.upload(lay, frames), host)

    def pitch_sequence(self):
        """the same w x h at three pitches in a row on one context, then a host batch, then a device batch again: a plan record remembers no pitch"""
        case = D.case_by_name("pitch_sequence")
        frames = D.case_frames(case)
        fails = self.record("pitch_sequence", pitches=[lay.row_pitch for lay in case.layouts])
        for variant in VARIANTS:
            ex = self.extractor(case.w, case.h, case.nlevels, case.nfeatures, 3, variant)
            host = self.host_results(ex, frames, case.nlevels)
            ptrs = [self.upload(lay, frames) for lay in case.layouts]
            for lay, ptr in zip(case.layouts, ptrs):
                self.check_device_batch(fails, "%s pitch %d" % (variant, lay.row_pitch), ex, case, lay, ptr, host)
            again = self.host_results(ex, frames, case.nlevels)
            for f in range(len(frames)):
                self.same_keys(fails, "%s host batch after the pitches, frame %d" % (variant, f), *again[0][f], *host[0][f])
            lay, ptr = case.layouts[-1], ptrs[-1]
            self.check_device_batch(fails, "%s pitch %d after the host batch" % (variant, lay.row_pitch), ex, case, lay, ptr, again)

    def describe_window(self):
        for name in D.DESCRIBE_LAYOUTS:
            case, lay = next((c, l) for c, l in D.all_layouts() if l.name == name)
            frames = D.case_frames(case)
            img = frames[D.DESCRIBE_FRAME]
            keys = D.describe_keys(lay.w, lay.h)
            fails = self.record("describe_" + name, lay, keys=len(keys))
            oex = self.O.Extractor(case.nfeatures, D.SCALE_FACTOR, case.nlevels, D.INI_TH, D.MIN_TH)
            ptr = self.upload(lay, frames)
            for mode in CV_MODES:
                ex = self.extractor(case.w, case.h, case.nlevels, case.nfeatures, 3, "own_plans", cv_mode=mode)
                self.extract_device(ex, lay, ptr)
                for recompute in (False, True):
                    ang, d = ex.describe_keys(keys, frame=D.DESCRIBE_FRAME, recompute_angle=recompute)
                    with self.O.cv_mode(mode):
                        ek, ed = oex.describe_keys(img, keys, recompute_angle=recompute)
                    tag = "cv mode %d, %s angle" % (mode, "recomputed" if recompute else "stored")
                    bad = (d != ed).any(axis=1)
                    if bad.any():
                        fails.append("%s: descriptors differ for %d of %d keys, e.g. (x, y, octave) = %s" % (
                            tag, int(bad.sum()), len(keys), [(int(k["x"]), int(k["y"]), int(k["octave"])) for k in keys[bad][:6]]))
                    if recompute:
                        bad = ang.view(np.uint32) != ek["angle"].view(np.uint32)
                        if bad.any():
                            fails.append("%s: angles differ for %d of %d keys" % (tag, int(bad.sum()), len(keys)))
                    elif (ed[keys["octave"] == 0] == ed[0]).all():
                        fails.append("%s: the expected descriptors are all the same" % tag)

    def bench_clip(self):
        """bench.py's clip, configuration and launch: two sub-batches of two frames at p0 and p0 + 2 w h, match_batch_prev and align_batch_prev behind
        each.  One context sees the clip three times -- host, device, host -- so that the device pass and the last host pass both start from the
        clip's last frame as their carried previous frame."""
        from orb_ygz_slam_amd import make_camera, EUROC
        case = D.case_by_name("bench_clip")
        lay = case.layouts[0]
        frames = D.case_frames(case)
        w, h, nl, sub = case.w, case.h, case.nlevels, D.BENCH_SUB
        exp = self.oracle_frames(case)
        fails = self.record("bench_clip", lay, keypoints=[len(k) for k, _ in exp])
        cam = make_camera(w, h)
        scale = self.O.Extractor(*D.BENCH_CFG).tables()["scale"]
        I, z = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
        e_match = []
        for f in range(lay.n):                      # frame f against its predecessor in the walk (the clip's last frame before its first)
            (k, d), (pk, pd) = exp[f], exp[f - 1]
            world = np.stack([(pk["x"] - np.float32(EUROC["cx"])) / np.float32(EUROC["fx"]),
                              (pk["y"] - np.float32(EUROC["cy"])) / np.float32(EUROC["fy"]), np.ones(len(pk), np.float32)], -1).astype(np.float32)
            e_match.append(self.O.search_by_projection_last(k, d, scale, w, h, EUROC, pk, world, pd, I, z, I, z, 15.0))
        ptr = self.upload(lay, frames)
        for variant in VARIANTS:
            ex = self.extractor(w, h, nl, case.nfeatures, sub, variant, fast_register_staging=False)      # (bench.py leaves the FAST kernel alone)

            def walk(device):
                out = []
                for k0 in range(0, lay.n, sub):
                    if device:
                        self.extract_device(ex, lay, ptr, first=k0, n=sub)
                    else:
                        ex.extract_batch_host(frames[k0:k0 + sub])
                    ex.match_batch_prev(cam, 15.0, True, True, True)
                    ex.align_batch_prev(cam, nl - 1, 1, 10)
                    counts = ex.match_counts()
                    for f in range(sub):
                        k, d = ex.batch_fetch(f)
                        m, o = ex.match_fetch(f)
                        out.append(dict(k=k, d=d, n=int(counts[f]), m=m[:len(k)].copy(), o=o[:len(k)].copy(), align=ex.align_fetch(f)))
                return out

            walk(False)
            dev, host = walk(True), walk(False)
            for f in range(lay.n):
                tag = "%s frame %d" % (variant, f)
                a, b = dev[f], host[f]
                self.same_keys(fails, tag + " vs the host path", a["k"], a["d"], b["k"], b["d"])
                self.same_keys(fails, tag + " vs the oracle", a["k"], a["d"], *exp[f])
                if a["n"] != b["n"] or not np.array_equal(a["m"], b["m"]) or not np.array_equal(a["o"], b["o"]):
                    fails.append("%s: matches differ from the host path's (%d vs %d)" % (tag, a["n"], b["n"]))
                e_n, e_m, e_o = e_match[f]
                if len(a["k"]) == len(exp[f][0]) and (a["n"] != e_n or not np.array_equal(a["m"], e_m) or not np.array_equal(a["o"], e_o)):
                    fails.append("%s: matches differ from the oracle's (%d vs %d)" % (tag, a["n"], e_n))
                if a["align"][0] != b["align"][0]:
                    fails.append("%s: align_batch_prev returns %d, host path %d" % (tag, a["align"][0], b["align"][0]))
                self.same_bits(fails, tag + ": align_batch_prev pose vs the host path", a["align"][1], b["align"][1])
                self.same_bits(fails, tag + ": align_batch_prev info vs the host path", a["align"][2], b["align"][2])
            self.records["bench_clip"]["info"]["matches"] = [r["n"] for r in dev]

    def stereo(self):
        pair = D.stereo_pair()
        oex = self.O.Extractor(D.STEREO_FEATURES, D.SCALE_FACTOR, D.STEREO_LEVELS, D.INI_TH, D.MIN_TH)
        for lay in D.STEREO_LAYOUTS:
            fails = self.record(lay.name, lay)
            ptr = self.upload(lay, pair)
            for variant in VARIANTS:
                ex = self.extractor(lay.w, lay.h, D.STEREO_LEVELS, D.STEREO_FEATURES, 2, variant)
                ex.extract_batch_host(pair)
                ex.stereo_batch(D.STEREO_MB, D.STEREO_MBF)
                hur, hdp = ex.stereo_fetch(0)
                self.extract_device(ex, lay, ptr)
                ex.stereo_batch(D.STEREO_MB, D.STEREO_MBF)
                ur, dp = ex.stereo_fetch(0)
                (kl, dl), (kr, dr) = ex.batch_fetch(0), ex.batch_fetch(1)
                n = len(kl)
                self.same_bits(fails, "%s: mvuRight vs the host path" % variant, ur[:n], hur[:n])
                self.same_bits(fails, "%s: mvDepth vs the host path" % variant, dp[:n], hdp[:n])
                our, odp = oex.compute_stereo_matches(pair[0], pair[1], kl, dl, kr, dr, D.STEREO_MB, D.STEREO_MBF)
                self.same_bits(fails, "%s: mvuRight vs the oracle" % variant, ur[:n], our)
                self.same_bits(fails, "%s: mvDepth vs the oracle" % variant, dp[:n], odp)
                octave0 = int(((ur[:n] >= 0) & (kl["octave"] == 0)).sum())
                self.records[lay.name]["info"]["octave0_matches"] = octave0
                if octave0 < D.STEREO_MIN_OCTAVE0:
                    fails.append("%s: only %d matched keypoints of octave 0 read the caller's level 0" % (variant, octave0))

    def held_frame_switching(self):
        """ygzf_describe_keys reads the frames of the LAST extraction, whichever entry point it came through"""
        from orb_ygz_slam_amd.synth import synth_frame
        case = D.case_by_name("tight4")
        lay = case.layouts[0]
        frames = D.case_frames(case)
        other = synth_frame(4190, case.w, case.h)
        keys = D.describe_keys(case.w, case.h)
        oex = self.O.Extractor(case.nfeatures, D.SCALE_FACTOR, case.nlevels, D.INI_TH, D.MIN_TH)
        want_dev = oex.describe_keys(frames[0], keys, recompute_angle=True)
        want_host = oex.describe_keys(other, keys, recompute_angle=True)
        assert (want_dev[1] != want_host[1]).any(axis=1).mean() > 0.9
        ex = self.extractor(case.w, case.h, case.nlevels, case.nfeatures, 3)
        ptr = self.upload(lay, frames)
        for name, order, want in (("switch_device_then_host", ("device", "host"), want_host), ("switch_host_then_device", ("host", "device"), want_dev)):
            fails = self.record(name, lay)
            for step in order:
                if step == "device":
                    self.extract_device(ex, lay, ptr)
                else:
                    ex.extract(other)
            ang, d = ex.describe_keys(keys, frame=0, recompute_angle=True)
            self.same_bits(fails, "descriptors after %s then %s" % order, d, want[1])
            self.same_bits(fails, "angles after %s then %s" % order, ang, want[0]["angle"])

    def argument_errors(self):
        """rejected on the arguments alone: the error comes back, and the context still holds the batch it held before"""
        from orb_ygz_slam_amd.capi import YgzfError
        case = D.case_by_name("tight0")
        lay = case.layouts[0]
        frames = D.case_frames(case)
        fails = self.record("argument_errors")
        ex = self.extractor(case.w, case.h, case.nlevels, case.nfeatures, 3)
        ptr = self.upload(lay, frames)
        self.extract_device(ex, lay, ptr)
        before = [ex.batch_fetch(f) for f in range(lay.n)]
        w, h = lay.w, lay.h
        for what, pitch, stride in (("row_pitch < w", w - 4, w * h), ("row_pitch % 4 != 0", w + 2, (w + 2) * h), ("frame_stride % 4 != 0", w, w * h + 2)):
            try:
                ex.extract_batch_device(ptr, lay.n, w, h, pitch, stride)
                fails.append("%s was accepted" % what)
            except YgzfError:
                pass
            for f in range(lay.n):
                self.same_keys(fails, "%s: held frame %d afterwards" % (what, f), *ex.batch_fetch(f), *before[f])


def child_main(out_path):
    """(called in the child, after torch has initialised the device)"""
    import time
    c = _Child()
    timing = {}
    try:
        for step in (c.argument_errors, c.layouts, c.pitch_sequence, c.describe_window, c.held_frame_switching, c.stereo, c.bench_clip):
            t0 = time.perf_counter()
            step()
            timing[step.__name__] = round(time.perf_counter() - t0, 2)
    finally:                                        # what ran so far is on record also when a step raised: nothing more runs on the device then
        c.records["_timing"] = {"failures": [], "info": timing}
        with open(out_path, "w") as f:
            json.dump(c.records, f, indent=1, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    for ex in c.ctx.values():
        ex.close()
    print("OK")


# ---- the parent -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def records(oracle, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("device_frames") / "records.json")
    code = ("import torch\n"
            "torch.cuda.init()            # before the library creates its own HIP context (as bench.py does)\n"
            "import sys\n"
            "sys.path.insert(0, %r)\n"
            "from tests.test_gpu_device_frames import child_main\n"
            "child_main(%r)\n") % (ROOT, out)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=300)
    rec = json.load(open(out)) if os.path.exists(out) else {}
    print(json.dumps({k: v["info"] for k, v in rec.items()}))
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return rec


def _clean(records, name):
    assert name in records, "the child wrote no record for %s" % name
    assert not records[name]["failures"], "\n".join(records[name]["failures"][:40])


def test_every_case_ran(records):
    assert set(records) - {"_timing"} == set(LAYOUT_IDS + DESCRIBE_IDS + STEREO_IDS + OTHER_IDS)


@pytest.mark.parametrize("name", LAYOUT_IDS)
def test_device_frames_equal_host_frames_and_the_oracle(records, name):
    """extract_batch_device + batch_fetch of every frame == extract_batch_host of the tight frames on the same context == the oracle, keypoints
    field by field and all descriptor bytes; every level == the host path's, level 0 == the tight frame; under both plan variants"""
    _clean(records, name)
    assert min(records[name]["info"]["keypoints"]) > 100


def test_one_context_three_pitches_then_host_then_device(records):
    _clean(records, "pitch_sequence")


@pytest.mark.parametrize("name", DESCRIBE_IDS)
def test_describe_window_at_every_row_offset(records, name):
    """describe_keys on frame 1: keys at every rowOff0 and on both sides of every term of `interior`, stored and recomputed angles, cv modes 0 and 2,
    against oracle.Extractor.describe_keys on the tight image"""
    _clean(records, name)


def test_bench_clip_through_the_device_entry(records):
    """what bench.py times, as bench.py launches it: keypoints, descriptors, match counts, matches and orientation flags == the host-path run == the
    oracle (as test_gpu_extract.py::test_bench_clip_parity checks the host entry); align_batch_prev bit-identical to the host-path run"""
    _clean(records, "bench_clip")
    assert min(records["bench_clip"]["info"]["keypoints"]) > 900 and min(records["bench_clip"]["info"]["matches"]) > 100


@pytest.mark.parametrize("name", STEREO_IDS)
def test_stereo_batch_reads_the_callers_frames(records, name):
    _clean(records, name)
    assert records[name]["info"]["octave0_matches"] >= D.STEREO_MIN_OCTAVE0


@pytest.mark.parametrize("name", ["switch_device_then_host", "switch_host_then_device"])
def test_held_frame_switching(records, name):
    _clean(records, name)


def test_argument_errors_leave_the_context_alone(records):
    _clean(records, "argument_errors")
