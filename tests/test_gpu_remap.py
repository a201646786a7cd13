"""The undistortion on the GPU (cv::remap's fixed-point bilinear path, src/Frame.cc:775-805): every constructed case of tests/remap_cases.py through
ygzf_remap_batch_device under the three path settings, and the host, pyramid and extraction forms against the numpy restatement.  All expectations
are exact.

Device memory comes from torch, as in bench.py, so the work runs in ONE child process for the module (torch initialises the device before the
library does); the child writes one record per check -- the list of what differed, empty when nothing did -- and the parametrised tests read them.

Layouts: source and destination frames lie between seeded garbage at four pitch classes -- `tight` (pitch = width), `round4`, `align64` and `odd`
(pitch = width + 1 from an odd base: no side is word-aligned) -- and the garbage, row padding included, must be unchanged afterwards."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import remap_cases as R
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

CASE_IDS = [c.name for c in R.CASES]
PATHS = (("auto", 0), ("lds", 1), ("gather", 2))
LAYOUTS = ("tight", "round4", "align64", "odd")
OTHER_IDS = ["three_maps_two_ids", "host_form", "pyramid_remapped", "extract_after_remap", "batch_device_chain", "errors"]
PREFIX = 256


def layout(name, w, h, n):
    """(pitch, frame stride, first frame's offset, bytes) of n frames of w x h"""
    if name == "tight":
        pitch, gap, off = w, 0, PREFIX
    elif name == "round4":
        pitch, gap, off = (w + 3) & ~3, 64, PREFIX
    elif name == "align64":
        pitch, gap, off = (w + 63) & ~63, 128, PREFIX
    else:
        pitch, gap, off = w + 1, 7, PREFIX + 1
    stride = pitch * h + gap
    return pitch, stride, off, off + stride * n + PREFIX


def place(buf, frames, pitch, stride, off):
    for f, img in enumerate(frames):
        h, w = img.shape
        rows = buf[off + f * stride: off + f * stride + pitch * h].reshape(h, pitch)
        rows[:, :w] = img


class _Child:
    def __init__(self):
        import torch
        self.torch = torch
        self.records = {}
        self.keep = []
        self.frames = {}
        self.want = {}
        self.garbage = np.random.RandomState(5).randint(0, 256, 16 << 20).astype(np.uint8)

    def fails(self, name, **info):
        r = self.records.setdefault(name, {"failures": [], "info": {}})
        r["info"].update(info)
        return r["failures"]

    def sources(self, case, n):
        key = case.name
        if key not in self.frames or len(self.frames[key]) < n:
            self.frames[key] = R.case_frames(case, n)
            self.want[key] = np.stack([R.expected(case)] + [R.remap_ref(f, case.map_xy, case.map_tab) for f in self.frames[key][1:]])
        return self.frames[key][:n], self.want[key][:n]

    def run_layout(self, fails, tag, ex, map_id, frames, want, lay):
        """remap_batch_device of `frames` laid out as `lay` on both sides; compares every byte of the destination and of the source"""
        torch = self.torch
        n, (sh, sw), (dh, dw) = len(frames), frames[0].shape, want[0].shape
        sp, ss, so, sbytes = layout(lay, sw, sh, n)
        dp, ds, do, dbytes = layout(lay, dw, dh, n)
        k = (len(tag) * 131 + n) % 4096             # seeded garbage, another stretch of it per run
        src, dst = self.garbage[k: k + sbytes].copy(), self.garbage[k + 4096: k + 4096 + dbytes].copy()
        place(src, frames, sp, ss, so)
        exp = dst.copy()
        place(exp, want, dp, ds, do)
        ts, td = torch.from_numpy(src).to("cuda:0"), torch.from_numpy(dst).to("cuda:0")
        assert ts.data_ptr() % 256 == 0 and td.data_ptr() % 256 == 0
        ex.remap_batch_device(map_id, ts.data_ptr() + so, n, sp, ss, td.data_ptr() + do, dp, ds)
        ex.sync()
        got, src_after = td.cpu().numpy(), ts.cpu().numpy()
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            inside = 0
            for f in range(n):
                g = got[do + f * ds: do + f * ds + dp * dh].reshape(dh, dp)[:, :dw]
                inside += int((g != want[f]).sum())
            fails.append("%s: %d destination bytes differ (%d of them pixels, the rest garbage that was overwritten), first at %d" % (
                tag, len(bad), inside, int(bad[0])))
        if not np.array_equal(src_after, src):
            fails.append("%s: the source buffer changed" % tag)

    def cases(self):
        from orb_ygz_slam_amd import Extractor
        from orb_ygz_slam_amd.capi import remap_plan_host
        ex = Extractor(500, 1.2, 4, 20, 7, max_width=752, max_height=480, max_batch=1)
        self.small = ex
        for case in R.CASES:
            fails = self.fails(case.name)
            sh, sw = case.src.shape
            ex.remap_set(0, sw, sh, case.map_xy, case.map_tab)
            info = ex.remap_info(0)
            P = remap_plan_host(sw, sh, case.map_xy, case.map_tab)
            G = info["frames_per_run"]
            if info["count"] != P["count"] or info["src"] != (sw, sh) or info["dst"] != case.map_tab.shape[::-1] or G != P["frames_per_run"]:
                fails.append("remap_info %r differs from the plan %r" % (info, P["count"]))
            counts = (1, 2, 3, 5, G + 1)
            frames, want = self.sources(case, max(counts))
            nt = P["tiles"][0] * P["tiles"][1]
            c = P["count"]
            self.records[case.name]["info"].update(count=c, frames_per_run=G)
            for pname, path in PATHS:
                ex.remap_set_path(path)
                for n in counts:
                    for lay in LAYOUTS:
                        tag = "%s n=%d %s" % (pname, n, lay)
                        self.run_layout(fails, tag, ex, 0, frames[:n], want[:n], lay)
                        st = ex.remap_stats()
                        exp_st = dict(staged=0, zeroed=0, gathered=nt, runs=-(-n // G)) if path == 2 else dict(staged=c[0] + c[1], zeroed=c[3], gathered=c[2], runs=-(-n // G))
                        if st != exp_st:
                            fails.append("%s: remap_stats %r, the plan says %r" % (tag, st, exp_st))
            ex.remap_set_path(0)

    def three_maps_two_ids(self):
        from orb_ygz_slam_amd.capi import YgzfError
        fails = self.fails("three_maps_two_ids")
        ex = self.small
        a, b, c = (R.case_by_name(n) for n in ("radial_k1_positive", "width_37", "mixed_classes"))

        def check(tag, map_id, case):
            frames, want = self.sources(case, 2)
            self.run_layout(fails, tag, ex, map_id, frames, want, "round4")
        ex.remap_set(0, 96, 64, a.map_xy, a.map_tab)
        ex.remap_set(1, 96, 64, b.map_xy, b.map_tab)
        check("id 0 = a", 0, a)
        check("id 1 = b", 1, b)
        check("id 0 again", 0, a)
        ex.remap_set(0, 96, 64, c.map_xy, c.map_tab)
        check("id 0 = c", 0, c)
        check("id 1 = b after id 0 was replaced", 1, b)
        ex.remap_clear(0)
        try:
            ex.remap_info(0)
            fails.append("remap_info of a cleared id succeeded")
        except YgzfError:
            pass
        check("id 1 = b after id 0 was cleared", 1, b)
        ex.remap_clear(1)

    def host_form(self):
        fails = self.fails("host_form")
        ex = self.small
        for name in ("other_size", "width_37", "scatter", "euroc_752x480"):
            case = R.case_by_name(name)
            ex.remap_set(1, case.src.shape[1], case.src.shape[0], case.map_xy, case.map_tab)
            for pname, path in PATHS:
                ex.remap_set_path(path)
                if not np.array_equal(ex.remap_host(1, case.src), R.expected(case)):
                    fails.append("%s %s: remap_host differs from the restatement" % (name, pname))
                padded = np.zeros((case.src.shape[0], case.src.shape[1] + 5), np.uint8)
                padded[:, :case.src.shape[1]] = case.src
                if not np.array_equal(ex.remap_host(1, padded[:, :case.src.shape[1]]), R.expected(case)):
                    fails.append("%s %s: remap_host of a strided view differs" % (name, pname))
            ex.remap_set_path(0)
        ex.remap_clear(1)

    def full_size(self):
        """a synthetic scene through the EuRoC map and through the k1 > 0 map (border on all sides), restated"""
        from orb_ygz_slam_amd.synth import synth_frame
        out = []
        for name in ("euroc_752x480", "radial_k1_positive_752x480"):
            case = R.case_by_name(name)
            raw = [synth_frame(70 + k, 752, 480) for k in range(3)]
            out.append((case, raw, [R.remap_ref(r, case.map_xy, case.map_tab) for r in raw]))
        return out

    def pyramid_and_extraction(self):
        from orb_ygz_slam_amd import Extractor
        fp, fe, fb = self.fails("pyramid_remapped"), self.fails("extract_after_remap"), self.fails("batch_device_chain")
        torch = self.torch
        ex = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=3)
        ref = Extractor(1000, 1.2, 8, 20, 7, max_width=752, max_height=480, max_batch=3)
        nkp = []
        for case, raw, und in self.full_size():
            ex.remap_set(0, 752, 480, case.map_xy, case.map_tab)
            for ahead in (0, 1):
                ex.set_extract_ahead(ahead)
                for k in range(2):
                    tag = "%s frame %d ahead=%d" % (case.name, k, ahead)
                    lv = ex.compute_pyramid_remapped(0, raw[k])
                    if not np.array_equal(lv[0], und[k]):
                        fp.append("%s: level 0 differs from the restatement in %d pixels" % (tag, int((lv[0] != und[k]).sum())))
                    want = ref.compute_pyramid(und[k])
                    for l in range(1, 8):
                        if not np.array_equal(lv[l], want[l]):
                            fp.append("%s: level %d differs from compute_pyramid of the restated image" % (tag, l))
                    kp, d = ex.extract_resident(752, 480)
                    ek, ed = ref.extract(und[k])
                    nkp.append(len(ek))
                    if len(kp) != len(ek) or kp.tobytes() != ek.tobytes() or not np.array_equal(d, ed):
                        fe.append("%s: extract_resident differs from extract of the restated image (%d vs %d keypoints)" % (tag, len(kp), len(ek)))
            ex.set_extract_ahead(0)
            # device to device, then extraction from the remapped frames where they lie (pitch 768: 4-aligned, as ygzf_extract_batch_device asks)
            sp, ss, so, sbytes = layout("tight", 752, 480, 3)
            dp, ds, do, dbytes = layout("align64", 752, 480, 3)
            src = np.zeros(sbytes, np.uint8)
            place(src, raw, sp, ss, so)
            ts = torch.from_numpy(src).to("cuda:0")
            td = torch.zeros(dbytes, dtype=torch.uint8, device="cuda:0")
            self.keep += [ts, td]
            ex.remap_batch_device(0, ts.data_ptr() + so, 3, sp, ss, td.data_ptr() + do, dp, ds)
            ex.extract_batch_device(td.data_ptr() + do, 3, 752, 480, dp, ds)
            ref.extract_batch_host(np.stack(und))
            for f in range(3):
                (kp, d), (ek, ed) = ex.batch_fetch(f), ref.batch_fetch(f)
                if len(kp) != len(ek) or kp.tobytes() != ek.tobytes() or not np.array_equal(d, ed):
                    fb.append("%s frame %d: extraction of the remapped device frame differs (%d vs %d keypoints)" % (case.name, f, len(kp), len(ek)))
                if not np.array_equal(ex.batch_fetch_level(f, 0), und[f]):
                    fb.append("%s frame %d: level 0 of the batch differs from the restatement" % (case.name, f))
        self.records["extract_after_remap"]["info"]["keypoints"] = nkp
        ex.close()
        ref.close()

    def errors(self):
        import ctypes as C
        from orb_ygz_slam_amd.capi import YgzfError
        fails = self.fails("errors")
        ex = self.small
        good = R.case_by_name("radial_k1_negative")
        frames, want = self.sources(good, 2)
        ex.remap_set(0, 96, 64, good.map_xy, good.map_tab)
        bad_tab = good.map_tab.copy()
        bad_tab[10, 10] = 1024
        big = R.case_by_name("identity")
        vp = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)
        attempts = (("tab > 1023", lambda: ex.remap_set(0, 96, 64, good.map_xy, bad_tab)),
                    ("source beyond the context", lambda: ex.remap_set(0, 753, 64, good.map_xy, good.map_tab)),
                    ("destination beyond the context", lambda: ex.remap_set(0, 96, 64, np.zeros((481, 8, 2), np.int16), np.zeros((481, 8), np.uint16))),
                    ("map id 2", lambda: ex.remap_set(2, 96, 64, big.map_xy, big.map_tab)),
                    ("null map_xy", lambda: ex._ck(ex.L.ygzf_remap_set(ex.h, 0, 96, 64, 96, 64, None, vp(good.map_tab)))),
                    ("null map_tab", lambda: ex._ck(ex.L.ygzf_remap_set(ex.h, 0, 96, 64, 96, 64, vp(good.map_xy), None))),
                    ("path 3", lambda: ex.remap_set_path(3)),
                    ("pitch below the width", lambda: ex.remap_batch_device(0, 256, 1, 95, 96 * 64, 256, 96, 96 * 64)),
                    ("no map at id 1", lambda: ex.remap_host(1, good.src)))
        for what, call in attempts:
            try:
                call()
                fails.append("%s was accepted" % what)
            except YgzfError:
                pass
            self.run_layout(fails, "after '%s'" % what, ex, 0, frames, want, "round4")
        ex.remap_clear(0)


def child_main(out_path):
    """(called in the child, after torch has initialised the device)"""
    import time
    c = _Child()
    timing = {}
    try:
        for step in (c.cases, c.three_maps_two_ids, c.host_form, c.errors, c.pyramid_and_extraction):
            t0 = time.perf_counter()
            step()
            timing[step.__name__] = round(time.perf_counter() - t0, 2)
    finally:                                        # what ran so far is on record also when a step raised: nothing more runs on the device then
        c.records["_timing"] = {"failures": [], "info": timing}
        with open(out_path, "w") as f:
            json.dump(c.records, f, indent=1, default=lambda o: o.tolist() if hasattr(o, "tolist") else str(o))
    c.small.close()
    print("OK")


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("remap") / "records.json")
    code = ("import torch\n"
            "torch.cuda.init()            # before the library creates its own HIP context (as bench.py does)\n"
            "import sys\n"
            "sys.path.insert(0, %r)\n"
            "from tests.test_gpu_remap import child_main\n"
            "child_main(%r)\n") % (ROOT, out)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=300)
    rec = json.load(open(out)) if os.path.exists(out) else {}
    print(json.dumps({k: v["info"] for k, v in rec.items()}))
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return rec


def _clean(records, name):
    assert name in records, "the child wrote no record for %s" % name
    assert not records[name]["failures"], "\n".join(records[name]["failures"][:40])


def test_every_check_ran(records):
    assert set(records) - {"_timing"} == set(CASE_IDS + OTHER_IDS)


@pytest.mark.parametrize("name", CASE_IDS)
def test_case_under_every_path_count_and_layout(records, name):
    """remap_batch_device == the restatement for 1, 2, 3, 5 and G + 1 frames, under AUTO, LDS and GATHER, at four pitch classes; nothing but the
    pixels is written; remap_stats reports the tiles the plan assigns to each kernel"""
    _clean(records, name)


def test_paths_were_taken(records):
    """the named cases ran where they say: scatter through the gather kernel under AUTO, the EuRoC map staged, the mixed map on all four classes"""
    assert records["scatter"]["info"]["count"][2] > 0 and records["scatter"]["info"]["count"][0] + records["scatter"]["info"]["count"][1] == 0
    assert records["euroc_752x480"]["info"]["count"][2] == 0 and records["euroc_752x480"]["info"]["count"][0] > 300
    assert min(records["mixed_classes"]["info"]["count"]) > 0


def test_one_context_three_maps_two_ids(records):
    _clean(records, "three_maps_two_ids")


def test_host_form_equals_the_restatement(records):
    _clean(records, "host_form")


def test_pyramid_of_the_remapped_image(records):
    """compute_pyramid_remapped: level 0 == the restatement, levels >= 1 == compute_pyramid of the restated image; with and without extract-ahead"""
    _clean(records, "pyramid_remapped")


def test_extract_resident_after_the_remapped_pyramid(records):
    _clean(records, "extract_after_remap")
    assert min(records["extract_after_remap"]["info"]["keypoints"]) > 500


def test_remapped_device_frames_feed_the_batch_extraction(records):
    _clean(records, "batch_device_chain")


def test_errors_leave_the_previous_map_working(records):
    _clean(records, "errors")
