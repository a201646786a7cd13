"""cv::remap's fixed-point bilinear path (8-bit, one channel, INTER_LINEAR, BORDER_CONSTANT 0, CV_16SC2 + CV_16UC1 maps) restated in numpy, its
plausible wrong forms behind a switch each, and constructed cases with a reach predicate each (src/Frame.cc:775-805; include/ygzf.h states the
arithmetic).  No device and no library: tests/test_remap_cases.py holds the cases to their claims, tests/test_gpu_remap.py runs them on the GPU,
tools/make_golden_remap_opencv.py runs them through cv2.remap on a machine that has it.

    map_xy[y, x] = (sx, sy) int16        map_tab[y, x] = fy * 32 + fx, fx, fy in 0..31
    dst = (sum_jk b_j a_k src(sy + j, sx + k) + 512) >> 10,  a = (32 - fx, fx), b = (32 - fy, fy), taps outside the source count 0
"""
import collections

import numpy as np

WRONG_FORMS = ("no_round", "round_minus_1", "border_replicate", "row_wrap", "swap_fxfy", "swap_xy", "int16_wrap", "tab0_32767")


def _wrap16(v):
    return ((v + 32768) & 0xFFFF) - 32768


def remap_ref(src, map_xy, map_tab, wrong=None):
    """The restatement.  wrong: None or one of WRONG_FORMS --
    no_round          no rounding term: S >> 10
    round_minus_1     OpenCV's sum with + 2^14 - 1 in the place of + 2^14
    border_replicate  a tap outside the source reads the nearest source pixel
    row_wrap          a tap at sx + 1 == src_w reads the byte that follows the row in a tight image: the next row's first (0 after the last row)
    swap_fxfy         fx = tab >> 5, fy = tab & 31
    swap_xy           sx = map_xy[..., 1], sy = map_xy[..., 0]
    int16_wrap        sx + 1 and sy + 1 formed in int16, the second tap's lower bound taken from the first coordinate (sx >= -1): at 32767 the tap
                      wraps to -32768, passes for inside and reads some byte of the image (here: the flat index modulo the image's size)
    tab0_32767        the tab == 0 entry as OpenCV's table holds it before the sum correction: weight 32767 on p00, nothing on the other taps
    """
    assert wrong is None or wrong in WRONG_FORMS
    src = np.asarray(src, np.uint8)
    sh, sw = src.shape
    xy = np.asarray(map_xy).astype(np.int64)
    tab = np.asarray(map_tab).astype(np.int64)
    assert tab.max() <= 1023
    sx, sy = (xy[..., 1], xy[..., 0]) if wrong == "swap_xy" else (xy[..., 0], xy[..., 1])
    fx, fy = (tab >> 5, tab & 31) if wrong == "swap_fxfy" else (tab & 31, tab >> 5)
    flat = src.reshape(-1).astype(np.int64)

    def tap(j, k):
        x, y = sx + k, sy + j
        if wrong == "border_replicate":
            return src[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)].astype(np.int64)
        if wrong == "int16_wrap":
            x, y = _wrap16(x), _wrap16(y)
            xin = (x < sw) & ((sx >= -1) if k else (x >= 0))
            yin = (y < sh) & ((sy >= -1) if j else (y >= 0))
            return np.where(xin & yin, flat[(y * sw + x) % flat.size], 0)
        inside = (x >= 0) & (x < sw) & (y >= 0) & (y < sh)
        v = np.where(inside, src[np.clip(y, 0, sh - 1), np.clip(x, 0, sw - 1)], 0).astype(np.int64)
        if wrong == "row_wrap" and k == 1:
            spill = (x == sw) & (y >= 0) & (y < sh)
            nxt = np.where(y + 1 < sh, src[np.clip(y + 1, 0, sh - 1), 0], 0).astype(np.int64)
            v = np.where(spill, nxt, v)
        return v
    p00, p01, p10, p11 = tap(0, 0), tap(0, 1), tap(1, 0), tap(1, 1)
    S = (32 - fy) * ((32 - fx) * p00 + fx * p01) + fy * ((32 - fx) * p10 + fx * p11)
    if wrong == "no_round":
        out = S >> 10
    elif wrong == "round_minus_1":
        out = (32 * S + (1 << 14) - 1) >> 15
    else:
        out = (S + 512) >> 10
    if wrong == "tab0_32767":
        out = np.where(tab == 0, (32767 * p00 + (1 << 14)) >> 15, out)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------
# moved_by: the wrong forms under which the restatement gives another image for this case (every other form must give the same one).
# reach: what the case is there for, as a predicate on (case, expected image).
Case = collections.namedtuple("Case", "name src map_xy map_tab moved_by reach")
SRC_W, SRC_H = 96, 64


def noise(seed, w=SRC_W, h=SRC_H, lo=1):
    """seeded bytes lo..255 (no zero: a tap that wrongly reads the image instead of the border shows)"""
    return np.random.RandomState(seed).randint(lo, 256, (h, w)).astype(np.uint8)


def maps(sx, sy, fx, fy):
    sx, sy, fx, fy = np.broadcast_arrays(np.asarray(sx), np.asarray(sy), np.asarray(fx), np.asarray(fy))
    assert sx.min() >= -32768 and sx.max() <= 32767 and sy.min() >= -32768 and sy.max() <= 32767 and fx.min() >= 0 and fx.max() < 32
    return np.stack([sx, sy], -1).astype(np.int16), (fy * 32 + fx).astype(np.uint16)


def grid(w, h):
    return np.meshgrid(np.arange(w), np.arange(h))


def fixed_point(u, v):
    """float source coordinates as cv::initUndistortRectifyMap / cv::convertMaps round them: rint(u * 32), >> 5, & 31"""
    iu, iv = np.rint(u * 32).astype(np.int64), np.rint(v * 32).astype(np.int64)
    return maps(iu >> 5, iv >> 5, iu & 31, iv & 31)


def radial_maps(w, h, fx, fy, cx, cy, k1, k2):
    """initUndistortRectifyMap(K, (k1, k2, 0, 0), R = I, newK = K) in double"""
    x, y = grid(w, h)
    xn, yn = (x - cx) / fx, (y - cy) / fy
    r2 = xn * xn + yn * yn
    d = 1 + k1 * r2 + k2 * r2 * r2
    return fixed_point(fx * xn * d + cx, fy * yn * d + cy)


def taps_inside(case):
    """per pixel and tap: inside the source (bool [h, w, 2, 2] indexed j, k)"""
    sh, sw = case.src.shape
    sx, sy = case.map_xy[..., 0].astype(np.int64), case.map_xy[..., 1].astype(np.int64)
    out = np.zeros(sx.shape + (2, 2), bool)
    for j in (0, 1):
        for k in (0, 1):
            out[..., j, k] = (sx + k >= 0) & (sx + k < sw) & (sy + j >= 0) & (sy + j < sh)
    return out


EUROC_CAM = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, k1=-0.28340811, k2=0.07395907)


def _build():
    C = []

    def add(name, src, m, moved_by, reach):
        C.append(Case(name, src, m[0], m[1], tuple(moved_by), reach))
    X, Y = grid(SRC_W, SRC_H)
    ins = lambda c: taps_inside(c)
    add("identity", noise(1), maps(X, Y, 0, 0), ("swap_xy",), lambda c, e: np.array_equal(e, c.src))
    add("half_pixel", noise(2), maps(X, Y, 16, 16), ("no_round", "round_minus_1", "border_replicate", "row_wrap", "swap_xy"),
        lambda c, e: (c.map_tab == 16 * 32 + 16).all() and not np.array_equal(e, c.src))
    ch = (((np.arange(40)[:, None] + np.arange(40)[None, :]) & 1) * 255).astype(np.uint8)
    i, j = grid(32, 32)
    # (on a checkerboard p00 == p11 and p01 == p10: the sum is symmetric in fx and fy, and the map is symmetric in x and y)
    add("all_tab_entries", ch, maps(i + 3, j + 4, i, j), ("no_round", "round_minus_1"),
        lambda c, e: len(np.unique(c.map_tab)) == 1024 and ins(c).all() and set(np.unique(c.src)) == {0, 255} and e.max() == 255 and len(np.unique(e)) > 100)
    for axis in "xy":
        n = SRC_W if axis == "x" else SRC_H
        for d, tag in ((1, "1"), (2, "2"), (n, "all")):
            for sign in (1, -1):
                m = maps(X + sign * d, Y, 0, 0) if axis == "x" else maps(X, Y + sign * d, 0, 0)
                outside = d * (SRC_H if axis == "x" else SRC_W)
                # (with every pixel outside on the x side, or above the first row, the transposed reading lies outside as well)
                moved = ("border_replicate",) if d == n and (axis == "x" or sign < 0) else ("border_replicate", "swap_xy")
                add("shift_%s_%s%s" % (axis, "plus" if sign > 0 else "minus", tag), noise(10 + d + sign), m, moved,
                    lambda c, e, outside=outside: int((~ins(c)[..., 0, 0]).sum()) == outside and int((e == 0).sum()) == outside)
    xs = np.array([-1, SRC_W - 1, SRC_W])[np.arange(SRC_W) % 3]
    add("sx_edges", noise(20), maps(xs[None, :], Y, (X * 7 + Y) % 32, (Y * 5 + X) % 32),
        ("no_round", "round_minus_1", "border_replicate", "row_wrap", "swap_fxfy", "swap_xy"),
        lambda c, e: set(np.unique(c.map_xy[..., 0])) == {-1, SRC_W - 1, SRC_W} and (e[:, 2::3] == 0).all() and (e[:, 1::3] != 0).any())
    ys = np.array([-1, SRC_H - 1, SRC_H])[np.arange(SRC_H) % 3]
    add("sy_edges", noise(21), maps(X, ys[:, None], (X * 7 + Y) % 32, (Y * 5 + X) % 32),
        ("no_round", "round_minus_1", "border_replicate", "row_wrap", "swap_fxfy", "swap_xy"),
        lambda c, e: set(np.unique(c.map_xy[..., 1])) == {-1, SRC_H - 1, SRC_H} and (e[2::3] == 0).all() and (e[1::3] != 0).any())
    ext = np.array([32767, -32767, -32768, 5])
    add("extreme_coordinates", noise(22), maps(ext[(X + Y) % 4], ext[(X // 4 + Y) % 4], (X * 3) % 32, (Y * 3) % 32),
        ("no_round", "border_replicate", "swap_fxfy", "int16_wrap"),
        lambda c, e: {32767, -32767, -32768} <= set(np.unique(c.map_xy)) and (e != 0).any() and (e == 0).any())
    add("constant_map", noise(23), maps(np.full((SRC_H, SRC_W), 40), 20, 11, 23), ("swap_fxfy", "swap_xy"),
        lambda c, e: len(np.unique(e)) == 1)
    Xt, Yt = grid(SRC_H, SRC_W)
    add("transpose", noise(24), maps(Yt, Xt, 0, 0), ("swap_xy",), lambda c, e: np.array_equal(e, c.src.T))
    rs = np.random.RandomState(25)
    add("scatter", noise(25), maps(rs.randint(-3, SRC_W + 2, (SRC_H, SRC_W)), rs.randint(-3, SRC_H + 2, (SRC_H, SRC_W)), rs.randint(0, 32, (SRC_H, SRC_W)),
                                   rs.randint(0, 32, (SRC_H, SRC_W))),
        ("no_round", "round_minus_1", "border_replicate", "row_wrap", "swap_fxfy", "swap_xy"),
        lambda c, e: c.map_xy[..., 0].min() < 0 and c.map_xy[..., 0].max() >= SRC_W and c.map_xy[..., 1].min() < 0 and c.map_xy[..., 1].max() >= SRC_H)
    # four 64 x 16 bands of one 64 x 64 destination: smooth inside the source | shifted over the left border | scattered | wholly outside
    Xm, Ym = grid(64, 64)
    rs = np.random.RandomState(26)
    band = Ym // 16
    sxm = np.select([band == 0, band == 1, band == 2], [Xm + 10, Xm - 20, rs.randint(0, SRC_W, (64, 64))], SRC_W + 5 + Xm)
    sym = np.select([band == 0, band == 1, band == 2], [Ym + 5, Ym, rs.randint(0, SRC_H, (64, 64))], Ym)
    add("mixed_classes", noise(26), maps(sxm, sym, (Xm * 5 + Ym) % 32, (Ym * 11 + Xm) % 32),
        ("no_round", "round_minus_1", "border_replicate", "row_wrap", "swap_fxfy", "swap_xy"),
        lambda c, e: ins(c)[:16].all() and not ins(c)[16:32].all() and ins(c)[16:32].any() and not ins(c)[48:].any() and (e[48:] == 0).all())
    for wd in (70, 37):
        Xw, Yw = grid(wd, 40)
        add("width_%d" % wd, noise(30 + wd), fixed_point(Xw * 1.3 + 0.37 * Yw / 40.0, Yw * 1.5 + 0.2 + 0.11 * Xw / wd),
            ("no_round", "round_minus_1", "swap_fxfy", "swap_xy"), lambda c, e, wd=wd: e.shape == (40, wd) and ins(c).all())
    Xs, Ys = grid(50, 30)
    add("other_size", noise(40), fixed_point(Xs * 96.0 / 50 - 0.8, Ys * 64.0 / 30 - 0.6),
        ("no_round", "round_minus_1", "border_replicate", "swap_fxfy", "swap_xy"), lambda c, e: e.shape == (30, 50) and c.src.shape == (64, 96))

    def border_sides(c):
        o = ~ins(c).all(axis=(2, 3))
        return bool(o[0].any() and o[-1].any() and o[:, 0].any() and o[:, -1].any())
    small = dict(w=SRC_W, h=SRC_H, fx=60.0, fy=58.0, cx=47.3, cy=31.6)
    add("radial_k1_positive", noise(41), radial_maps(k1=0.35, k2=0.05, **small), ("no_round", "round_minus_1", "border_replicate", "row_wrap", "swap_fxfy", "swap_xy"),
        lambda c, e: border_sides(c) and (e[1:-1, 1:-1] != 0).any())
    add("radial_k1_negative", noise(42), radial_maps(k1=-0.28, k2=0.07, **small), ("no_round", "round_minus_1", "swap_fxfy", "swap_xy"),
        lambda c, e: ins(c).all())
    add("radial_k1_positive_752x480", noise(43, 752, 480), radial_maps(752, 480, EUROC_CAM["fx"], EUROC_CAM["fy"], EUROC_CAM["cx"], EUROC_CAM["cy"], 0.283, 0.074),
        ("no_round", "round_minus_1", "border_replicate", "row_wrap", "swap_fxfy", "swap_xy"), lambda c, e: border_sides(c))
    add("euroc_752x480", noise(44, 752, 480), radial_maps(752, 480, **EUROC_CAM), ("no_round", "round_minus_1", "swap_fxfy", "swap_xy"),
        lambda c, e: ins(c).all() and e.shape == (480, 752))
    return C


CASES = _build()
_expected = {}


def case_by_name(name):
    return next(c for c in CASES if c.name == name)


def expected(case):
    """the restated image of the case's own source, computed once"""
    if case.name not in _expected:
        e = remap_ref(case.src, case.map_xy, case.map_tab)
        e.setflags(write=False)
        _expected[case.name] = e
    return _expected[case.name]


def case_frames(case, n):
    """n source frames of the case's size: frame 0 is the case's own source, the others are seeded noise"""
    h, w = case.src.shape
    return np.stack([case.src] + [noise(1000 + 17 * f + len(case.name), w, h, lo=0) for f in range(1, n)])
