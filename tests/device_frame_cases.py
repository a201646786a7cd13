"""Layouts of caller-owned device frames for ygzf_extract_batch_device (include/ygzf.h), pure numpy.

Every host entry point copies level 0 into the context's own buffer: pitch = width rounded up to 64, a 256-byte aligned base, frames pitch * h
apart.  The device entry hands the kernels the CALLER's layout instead, and these branches exist only for it (csrc/extract_kernels.hip):

  describe_window   the wide (LDS-DMA) staging runs when row_pitch % 4 == 0 and addresses window row r at ((rowOff0 + r * rowOffStep) & 15) with
                    rowOffStep = row_pitch & 15 (0 at the library's own pitch) and rowOff0 = (address of the window's first byte) & 15, which depends
                    on the frame's base, i.e. on the caller's pointer and frame_stride;
  pyr_tile          level 0 -> 1 in 16-byte chunks; a chunk that would cross row_pitch * h goes through pyr_tail_chunk -- only a tight buffer whose last
                    staged chunk sticks out of the last row gets there;
  fast_cell / fast_tab_cell, k_pyr_strips   row addresses at the caller's pitch.

build_buffer() lays tight frames out in one byte buffer under such a layout, with seeded random garbage wherever no pixel is, and enough of it before
frame 0 and behind the last frame that an aligned over-read of a kernel stays inside the allocation: it can only show as a wrong result.
layout_classes() says which of the branches above a layout reaches; tests/test_device_frame_cases.py checks that the case list reaches all of them,
tests/test_gpu_device_frames.py runs the list on the device."""
from collections import namedtuple

import numpy as np

from orb_ygz_slam_amd.synth import synth_frame

SCALE_FACTOR = 1.2
INI_TH, MIN_TH = 20, 7
SMALL_FEATURES = 300
BENCH_CFG = (1000, 1.2, 8, 20, 7)          # bench.py's euroc752x480_8lvl_1000feat
BUFFER_ALIGN = 256                          # frame 0 lies base_offset bytes past a multiple of this inside the buffer (the allocator gives at least that)

# one layout = one ygzf_extract_batch_device call: n frames of w x h, frame f at base_offset + f * frame_stride past an aligned address
Layout = namedtuple("Layout", "name w h n row_pitch frame_stride base_offset")
# one case = layouts of ONE geometry that share their frames (synth_frame(seed + i, w, h), or the bench clip) and their extractor configuration
Case = namedtuple("Case", "name w h nlevels nfeatures seed layouts expect")


def align_up(x, a):
    return (x + a - 1) // a * a


def required_slack(row_pitch):
    return row_pitch + 64


def build_buffer(frames, row_pitch, frame_stride, base_offset=0, slack=0, garbage_seed=0x5EED):
    """frames (n, h, w) uint8 -> (buf, off0): frame f's pixel (y, x) is buf[off0 + f * frame_stride + y * row_pitch + x]; every other byte of buf is
    seeded random garbage.  At least max(slack, row_pitch + 64) bytes lie in front of frame 0 and behind the last pixel of the last frame, and
    off0 - base_offset is a multiple of BUFFER_ALIGN: uploaded to an allocation aligned that far, frame 0's address is base_offset modulo 16."""
    frames = np.asarray(frames)
    assert frames.dtype == np.uint8 and frames.ndim == 3
    n, h, w = frames.shape
    assert row_pitch >= w and base_offset >= 0
    assert n == 1 or frame_stride >= (h - 1) * row_pitch + w, "frames overlap"
    slack = max(slack, required_slack(row_pitch))
    off0 = align_up(slack, BUFFER_ALIGN) + base_offset
    end = off0 + (n - 1) * frame_stride + (h - 1) * row_pitch + w
    size = align_up(end + slack, BUFFER_ALIGN)
    buf = garbage(size, garbage_seed)
    frame_views(buf, off0, n, h, w, row_pitch, frame_stride)[...] = frames
    return buf, off0


def garbage(size, seed):
    return np.random.default_rng(seed).integers(0, 256, size, dtype=np.uint8)


def frame_views(buf, off0, n, h, w, row_pitch, frame_stride):
    """The (n, h, w) view of the frames inside buf (writable, no copy)."""
    assert off0 + (n - 1) * frame_stride + (h - 1) * row_pitch + w <= buf.size
    return np.lib.stride_tricks.as_strided(buf[off0:], shape=(n, h, w), strides=(frame_stride, row_pitch, 1))


def pixel_mask(size, off0, n, h, w, row_pitch, frame_stride):
    m = np.zeros(size, bool)
    frame_views(m, off0, n, h, w, row_pitch, frame_stride)[...] = True
    return m


def layout_buffer(lay, frames, garbage_seed=0x5EED):
    assert frames.shape == (lay.n, lay.h, lay.w)
    return build_buffer(frames, lay.row_pitch, lay.frame_stride, lay.base_offset, garbage_seed=garbage_seed)


# ---- reach predicates ---------------------------------------------------------------------------------------------------------------------------
def level_size(w, h, level, scale_factor=SCALE_FACTOR):
    """Tables::levelSize (csrc/ygzf_plan.hip): cvRound of float products, the scale accumulated in float."""
    s = np.float32(1.0)
    for _ in range(level):
        s = np.float32(s * np.float32(scale_factor))
    inv = np.float32(1.0) / s
    return int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))


def _resize_ofs(dst, src):
    """xofs / yofs of cv::resize INTER_LINEAR as build_geometry computes them: floor((float) ((d + 0.5) * scale - 0.5)), unclamped."""
    scale = 1.0 / (dst / src)
    return [int(np.floor(np.float32((d + 0.5) * scale - 0.5))) for d in range(dst)]


def pyr_tile_chunks(w, h, scale_factor=SCALE_FACTOR):
    """What pyr_tile stages of level 0 for level 1, restated from build_geometry's tile loop: [(first staged column sxa, 16-byte chunks nc)] per tile
    column, and the last source row any tile stages."""
    w1, h1 = level_size(w, h, 1, scale_factor)
    xofs = [min(max(s, 0), w - 1) for s in _resize_ofs(w1, w)]            # (sx < 0 -> 0, sx >= w - 1 -> w - 1)
    yofs = _resize_ofs(h1, h)
    cols = []
    x0 = 0
    while x0 < w1:
        rest = w1 - x0
        fl = 0
        if rest <= 224:
            units = (rest + 31) // 32
            fl = 1 if units >= 4 else 2 if units >= 2 else 3
        tw = 256 >> fl
        xl = min(x0 + tw, w1) - 1
        sxa, sxb = xofs[x0] & ~3, min(xofs[xl] + 1, w - 1)
        cols.append((sxa, (sxb - sxa) // 16 + 1))
        x0 += tw
    last_row = min(max(yofs[h1 - 1] + 1, 0), h - 1)
    return cols, last_row


def pyr_tail_reachable(w, h, row_pitch, scale_factor=SCALE_FACTOR):
    """pyr_tile's own condition: the chunk at byte offset oo of the frame takes pyr_tail_chunk when oo + 16 > h * row_pitch.  Chunks start at
    row * row_pitch + sxa + 16 c, c < nc, so only the last row's last chunk can get there."""
    cols, last_row = pyr_tile_chunks(w, h, scale_factor)
    return any(last_row * row_pitch + sxa + 16 * (nc - 1) + 16 > h * row_pitch for sxa, nc in cols)


def layout_classes(lay, scale_factor=SCALE_FACTOR):
    return dict(base_mod16=tuple((lay.base_offset + f * lay.frame_stride) % 16 for f in range(lay.n)),
                pitch_mod16=lay.row_pitch % 16, pitch_mod64=lay.row_pitch % 64, stride_mod16=lay.frame_stride % 16,
                pyr_tail=pyr_tail_reachable(lay.w, lay.h, lay.row_pitch, scale_factor),
                wide_window=lay.row_pitch % 4 == 0,
                own_layout=lay.row_pitch == align_up(lay.w, 64) and lay.frame_stride == lay.row_pitch * lay.h and lay.base_offset % BUFFER_ALIGN == 0)


# ---- the case list ------------------------------------------------------------------------------------------------------------------------------
def _tight(name, w, h, n=3):
    return Layout(name, w, h, n, w, w * h, 0)


def _pitched(name, w, h, pitch, n=3, base=0, extra=0):
    return Layout(name, w, h, n, pitch, pitch * h + extra, base)


CROP_IMAGE_W, CROP_IMAGE_H, CROP_X0, CROP_Y0 = 1024, 260, 44, 7       # x0 % 4 == 0, x0 % 16 == 12

# `expect`: the classes the case is named for, checked per layout by tests/test_device_frame_cases.py (base_mod16: of frame 0)
CASES = [
    Case("tight4", 164, 120, 4, SMALL_FEATURES, 4100, [_tight("tight4", 164, 120)], dict(pitch_mod16=4, pyr_tail=True)),
    Case("tight8", 168, 120, 4, SMALL_FEATURES, 4110, [_tight("tight8", 168, 120)], dict(pitch_mod16=8)),
    Case("tight12", 172, 121, 3, SMALL_FEATURES, 4120, [_tight("tight12", 172, 121)], dict(pitch_mod16=12, stride_mod16=172 * 121 % 16)),
    Case("tight0", 176, 120, 4, SMALL_FEATURES, 4130, [_tight("tight0", 176, 120)], dict(pitch_mod16=0, pitch_mod64=48)),
    # row_pitch > w.  (a: the last tile's chunk [152, 168) still crosses the 164-byte last row -- pitched, and on the tail path all the same; b: inside 172)
    Case("oddwidth_a", 161, 120, 3, SMALL_FEATURES, 4140, [_pitched("oddwidth_a", 161, 120, 164)], dict(pitch_mod16=4, pyr_tail=True)),
    Case("oddwidth_b", 163, 120, 4, SMALL_FEATURES, 4150, [_pitched("oddwidth_b", 163, 120, 172)], dict(pitch_mod16=12, pyr_tail=False)),
    # consecutive frames fall into different mod-16 classes: frame_stride = pitch * h + 4
    Case("offset_base", 164, 120, 4, SMALL_FEATURES, 4100,
         [_pitched("offset_base%d" % b, 164, 120, 164, base=b, extra=4) for b in (4, 8, 12)], dict(pitch_mod16=4, stride_mod16=4)),
    # a w x h window of larger device images (1024 x 260 each), first pixel at (x0, y0)
    Case("crop", 200, 150, 4, SMALL_FEATURES, 4160,
         [Layout("crop", 200, 150, 3, CROP_IMAGE_W, CROP_IMAGE_W * CROP_IMAGE_H, CROP_Y0 * CROP_IMAGE_W + CROP_X0)],
         dict(base_mod16=CROP_X0 % 16, pitch_mod16=0, pyr_tail=False)),
    # one geometry at three pitches in a row on one context (a plan record must not remember a pitch): every pitch % 16 that is not the library's
    Case("pitch_sequence", 164, 120, 4, SMALL_FEATURES, 4100,
         [_pitched("pitch_sequence%d" % p, 164, 120, p) for p in (164, 168, 188)], dict()),
    # bench.py's clip and configuration, launched as bench.py's SubPipe does: row_pitch = w, frame_stride = w * h, sub-batches at p0 + k * sub * w * h
    Case("bench_clip", 752, 480, BENCH_CFG[2], BENCH_CFG[0], None, [_tight("bench_clip", 752, 480, n=4)], dict(pitch_mod16=0, pitch_mod64=48)),
]
BENCH_SUB = 2                                                             # frames per sub-batch of the bench clip


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def all_layouts():
    return [(c, lay) for c in CASES for lay in c.layouts]


_frames_cache = {}


def case_frames(case):
    """The case's tight frames, (n, h, w); computed once per process and not to be written to."""
    if case.name not in _frames_cache:
        n = case.layouts[0].n
        if case.seed is None:
            from bench import make_frames
            f = make_frames(n, case.w, case.h)
        else:
            f = np.stack([synth_frame(case.seed + i, case.w, case.h) for i in range(n)])
        f.setflags(write=False)
        _frames_cache[case.name] = f
    return _frames_cache[case.name]


# ---- describe_window keys -----------------------------------------------------------------------------------------------------------------------
DESCRIBE_LAYOUTS = ("tight4", "tight8", "tight12", "offset_base4", "offset_base8", "offset_base12")
DESCRIBE_FRAME = 1
DESCRIBE_ANGLES = (0.0, 33.0, 217.5)
KP_FIELDS = [("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")]


def describe_keys(w, h, scale_factor=SCALE_FACTOR):
    """Keys for ygzf_describe_keys on a w x h frame.  Level 0: sixteen consecutive x from 21 (every rowOff0) at the y on both sides of every term of
    describe_window's `interior` (ky >= 21, ky + 22 < gh -- asymmetric --, and the domain's edge 19 px from the border); x on both sides of
    kx >= 21 and kx + 21 < gw for three y; a few keys on level 1 as a control.  All at least 19 px from every border of their level."""
    ys = (19, 20, 21, 22, h - 24, h - 23, h - 22, h - 20)
    xy = [(x, y) for x in range(21, 37) for y in ys]
    xy += [(x, y) for x in (19, 20, w - 23, w - 22, w - 21, w - 20) for y in (20, h // 2, h - 22)]
    assert all(19 <= x <= w - 20 and 19 <= y <= h - 20 for x, y in xy)
    k = np.zeros(len(xy) + 6, np.dtype(KP_FIELDS))
    k["size"], k["class_id"] = 31.0, -1
    k["x"][:len(xy)], k["y"][:len(xy)] = np.array(xy, np.float32).T
    w1, h1 = level_size(w, h, 1, scale_factor)
    s1 = np.float32(scale_factor)
    lvl1 = [(21, 21), (22, h1 - 23), (w1 - 22, 22), (w1 // 2, h1 // 2), (w1 - 23, h1 - 24), (30, h1 // 2)]
    for i, (x, y) in enumerate(lvl1):                                  # stored in level-0 coordinates, as cv::KeyPoint::pt is
        k[len(xy) + i] = (np.float32(x) * s1, np.float32(y) * s1, np.float32(31.0) * s1, 0.0, 0.0, 1, -1)
    k["angle"] = np.resize(np.array(DESCRIBE_ANGLES, np.float32), len(k))
    return k


# ---- stereo pairs -------------------------------------------------------------------------------------------------------------------------------
STEREO_W, STEREO_H, STEREO_LEVELS, STEREO_FEATURES, STEREO_SEED, STEREO_DISPARITY = 328, 200, 3, 500, 4200, 24
STEREO_MB, STEREO_MBF = 0.11, 47.9
STEREO_MIN_OCTAVE0 = 20                    # matched keypoints of octave 0 the scene must give: only those read the caller's level 0
STEREO_LAYOUTS = [_tight("stereo_tight", STEREO_W, STEREO_H, n=2), _pitched("stereo_pitch1024", STEREO_W, STEREO_H, 1024, n=2)]


def stereo_pair(seed=STEREO_SEED, w=STEREO_W, h=STEREO_H, d=STEREO_DISPARITY):
    """(2, h, w): left, and the left image seen d px to the side (as bench.py --stereo builds its right eyes: the last d columns are another scene's)."""
    left, right = synth_frame(seed, w, h), synth_frame(seed + 1, w, h)
    right[:, :w - d] = left[:, d:]
    return np.stack([left, right])
