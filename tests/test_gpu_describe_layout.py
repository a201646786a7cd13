"""describe_window's padded LDS window on the device: angles and descriptors of an explicit key list equal the oracle's, at every class of
level-0 row pitch (pitch & 15 = 0, 4, 8, 12: the offset of a window row inside its 16-byte aligned span then changes from row to row by that much)
and in every cv_mode.

A 160 x 120 image of random bytes, 2 levels, handed over as a caller-owned device frame at row pitches 160, 164, 168 and 172.  The keys:
  * sixteen consecutive kx on one row of level 0, and of level 1 (every (kx - 21) & 15, i.e. every offset of the window's first byte);
  * the first and last interior positions (kx = 21, kx + 21 = gw - 1, ky = 21, ky + 22 = gh - 1), alone and in the corners, on both levels: the
    LDS-DMA's first and last rows and quarters;
  * one pixel outside each of them: the border path's byte stores into the same layout;
  * 16 px from every edge of level 0: windows that reach 5 px past the image.  The reference never has a key closer than 19 px to an edge and its
    descriptor would sample outside the image there, so these keys are compared with the oracle on the image extended by 32 px of
    BORDER_REFLECT_101 -- what the reference's blur sees past an edge, and what the border path stages.
One more call has two keys only, one per level: the two waves of a workgroup then work at different pitch classes.

Device memory comes from torch, which has to initialise the device before the library does: the work runs in ONE child process for the module (as
tests/test_gpu_device_frames.py does), which writes what differed per (pitch, cv_mode); the tests read that record."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import device_frame_cases as D
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

W, H, NLEVELS, NFEATURES = 160, 120, 2, 300
PITCHES = (160, 164, 168, 172)
CV_MODES = (0, 1, 2)
PAD = 32


def image():
    return np.random.default_rng(160120).integers(0, 256, (H, W), dtype=np.uint8)


def make_keys(points):
    """points: (x, y, level) in level coordinates -> cv::KeyPoint records (pt in level-0 coordinates, as the reference stores them)"""
    k = np.zeros(len(points), np.dtype(D.KP_FIELDS))
    for i, (x, y, l) in enumerate(points):
        s = np.float32(D.SCALE_FACTOR) if l else np.float32(1.0)
        k[i] = (np.float32(x) * s, np.float32(y) * s, np.float32(31.0) * s, 0.0, 0.0, l, -1)
    return k


def key_points():
    inside, edge16 = [], []
    for l in range(NLEVELS):
        gw, gh = D.level_size(W, H, l)
        x0, x1, y0, y1 = 21, gw - 22, 21, gh - 23                      # first and last interior positions
        inside += [(x, 40, l) for x in range(21, 37)]
        inside += [(x, y, l) for x in (x0, gw // 2, x1) for y in (y0, gh // 2, y1) if (x, y) != (gw // 2, gh // 2)]
        inside += [(x0 - 1, gh // 2, l), (x1 + 1, gh // 2, l), (gw // 2, y0 - 1, l), (gw // 2, y1 + 1, l),      # one pixel outside: the border path
                   (x0 - 1, y0 - 1, l), (x1 + 1, y1 + 1, l), (x0 - 1, y1, l), (x1, y0 - 1, l)]
    edge16 += [(16, H // 2, 0), (W - 17, H // 2, 0), (W // 2, 16, 0), (W // 2, H - 17, 0), (16, 16, 0), (W - 17, H - 17, 0)]
    return inside, edge16


def expected(O):
    """keys, {cv_mode: (angles, descriptors)} of all keys from the oracle, once"""
    img = image()
    inside, edge16 = key_points()
    keys = make_keys(inside + edge16)
    ext = np.pad(img, PAD, mode="reflect")                             # numpy's 'reflect' is BORDER_REFLECT_101
    shifted = make_keys([(x + PAD, y + PAD, l) for x, y, l in edge16])
    oex = O.Extractor(NFEATURES, D.SCALE_FACTOR, NLEVELS, D.INI_TH, D.MIN_TH)
    out = {}
    for mode in CV_MODES:
        with O.cv_mode(mode):
            ek, ed = oex.describe_keys(img, keys[:len(inside)], recompute_angle=True)
            xk, xd = oex.describe_keys(ext, shifted, recompute_angle=True)
        out[mode] = (np.concatenate([ek["angle"], xk["angle"]]), np.concatenate([ed, xd]))
    return keys, out


def differences(fails, ang, d, eang, ed, keys, tag):
    bad = (d != ed).any(axis=1)
    if bad.any():
        fails.append("%s: descriptors differ for %d of %d keys, e.g. (x, y, octave) = %s" % (
            tag, int(bad.sum()), len(keys), [(float(k["x"]), float(k["y"]), int(k["octave"])) for k in keys[bad][:6]]))
    bad = ang.view(np.uint32) != eang.view(np.uint32)
    if bad.any():
        fails.append("%s: angles differ for %d of %d keys" % (tag, int(bad.sum()), len(keys)))


def child_main(out_path):
    """(called in the child, after torch has initialised the device)"""
    import torch
    from oracle import oracle_py as O
    from orb_ygz_slam_amd import Extractor
    O.build()
    records = {}
    try:
        keys, exp = expected(O)
        records["keys"] = {"n": len(keys), "distinct_descriptors": {str(m): len(np.unique(exp[m][1], axis=0)) for m in CV_MODES}}
        img = image()
        pair = np.array([0, next(i for i, k in enumerate(keys) if k["octave"] == 1)])      # level 0 (the caller's pitch) beside level 1 (the library's own)
        keep = []                                                        # (a context reads its frame until its next extraction)
        for mode in CV_MODES:
            ex = Extractor(NFEATURES, D.SCALE_FACTOR, NLEVELS, D.INI_TH, D.MIN_TH, max_width=W, max_height=H, max_batch=1, cv_mode=mode)
            for pitch in PITCHES:
                fails = []
                buf, off0 = D.build_buffer(img[None], pitch, pitch * H)
                t = torch.from_numpy(buf).to("cuda:0")
                keep.append(t)
                ex.extract_batch_device(t.data_ptr() + off0, 1, W, H, pitch, pitch * H)
                ang, d = ex.describe_keys(keys, frame=0, recompute_angle=True)
                differences(fails, ang, d, exp[mode][0], exp[mode][1], keys, "all keys")
                ang, d = ex.describe_keys(keys[pair], frame=0, recompute_angle=True)
                differences(fails, ang, d, exp[mode][0][pair], exp[mode][1][pair], keys[pair], "two keys")
                records["%d-%d" % (pitch, mode)] = fails
            ex.close()
    finally:                                                             # what ran so far is on record also when a step raised
        with open(out_path, "w") as f:
            json.dump(records, f)
    print("OK")


@pytest.fixture(scope="module")
def records(oracle, tmp_path_factory):
    out = str(tmp_path_factory.mktemp("describe_layout") / "records.json")
    code = ("import torch\n"
            "torch.cuda.init()            # before the library creates its own HIP context (as bench.py does)\n"
            "import sys\n"
            "sys.path.insert(0, %r)\n"
            "from tests.test_gpu_describe_layout import child_main\n"
            "child_main(%r)\n") % (ROOT, out)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=120)
    rec = json.load(open(out)) if os.path.exists(out) else {}
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    return rec


def test_the_expected_descriptors_differ_from_key_to_key(records):
    assert all(n > records["keys"]["n"] // 2 for n in records["keys"]["distinct_descriptors"].values())


@pytest.mark.parametrize("mode", CV_MODES)
@pytest.mark.parametrize("pitch", PITCHES)
def test_keys_at_every_row_offset_and_on_both_staging_paths(records, pitch, mode):
    name = "%d-%d" % (pitch, mode)
    assert name in records, "the child wrote no record for %s" % name
    assert not records[name], "\n".join(records[name])
