"""Constructed inputs for ORBmatcher::FindDirectProjection (GetWarpAffineMatrix, GetBestSearchLevel, WarpAffine, ygz::Align2D: src/ORBmatcher.cc:
1525-1602, include/ORBmatcher.h:185-211, src/Align.cc:8-104) and for Frame::isInFrustum + MapPoint::PredictScale (src/Frame.cc:363-422,
src/MapPoint.cc:359-373), with a plain numpy restatement of both (np.float32 in source order, ints where the source has ints, doubles where it
has doubles) that carries mutation switches.  No GPU, no extractor, no fixture file: every image is generated from a fixed seed with integer
arithmetic.  Shared by tests/test_direct_cases.py (CPU: the restatement equals the oracle bit for bit, every case is what it claims, every
mutation moves exactly the labels declared for it, the oracle equals the reference's own code) and tests/test_gpu_direct_cases.py
(k_direct_projection and k_frustum equal the oracle bit for bit, twice in a row on one context per configuration).

Cameras and poses.  fx = fy = 256 and cx = w / 2, cy = h / 2; depths and translations are small dyadic numbers and rotations are the identity
(the `rotation` family apart), so that the back-projection of an integer pixel, its projections and A_cur_ref are exact in float: a case can
claim A == s * I (key "A" of its expectation) and the CPU tier checks the claim on the restatement's trace.

Configurations (scale factor, levels, frame): "L8" 1.2 / 8 / 192 x 144 (level 7 is 54 x 40: a 10 x 10 patch and the 8 x 8 window fit with room
to place them); "P4" 2.0 / 4 / 192 x 144, whose scales 1, 2, 4, 8 are exact (level 3 is 24 x 18); "L2" 1.2 / 2 / 96 x 72 and "L1" 1.2 / 1 /
96 x 72 for the search-level cap (with one level ygzf_find_direct_projection_batch passes invLevelSigma2[0]; the loop never runs, so the value
is never read -- as in the reference, whose mvInvLevelSigma2[1] would lie outside the vector).  The frustum cases add "L12" (12 levels of 1.2).

The image.  base_image() is integer noise box-filtered twice and stretched to 16..225 (so that + 30 never clips), with five 24 x 24 blocks painted
into its upper half for the 192 x 144 frames: a 0 / 255 checkerboard of 2 x 2 cells (the central differences of a period-4 pattern are +-127.5 on
every pixel, the Hessian's largest terms: 64 * 127.5^2 = 1040400 < 2^22), a flat block, vertical stripes, horizontal stripes, and a black block
with a white quadrant.

Direct-path families (a case = a batch of candidates; `expect` maps a label to what must happen to that candidate):
  warp_border   identity poses, integer px_ref: A == I (octave 0) or 2 I (octave 1 of P4), so the warped patch is an integer crop of the
                reference level with zeros where the sample column / row is < 0 or >= w - 1 / h - 1.  The patch starts on column / row 0
                (sampled), one pixel outside (zero), ends on w - 2 (sampled), on w - 1 (zero); both axes at two corners; the same at octave 1
                where px_ref / 2 carries the edge.  expect gives the crop from first principles (key "crop").
  align_border  identical images, the start pixel on the reference keypoint, so that an Align2D that runs has residual 0, computes one zero
                update and converges in iteration 0 with the pixel unchanged, while one that stops at the window gate returns success 0 and
                (px0 * invScale[sl]) * scale[sl]: floor(u) == 4 / w - 5 run, 3 / w - 4 stop, the same for v, for a search level above 0 (P4,
                octave 1), and u one float below 4.0.  walks_out: the current image is the reference moved 4 px to the left, the reference keypoint
                is at x = 7 and the start at u = 5.0: the first update carries the iterate to 3.84 and iteration 1 stops at the gate.
                ten_iterations: the reference patch comes from an unrelated texture, so no alignment exists; the iterate wanders a few pixels
                and neither the stop rule nor the gate ends the loop before its tenth iteration.  (On a periodic texture a start outside the
                basin is pulled into the neighbouring period and converges there, and a start in anti-phase sees res * dx cancel and
                "converges" at once: neither exhausts the loop.)
  align_values  identical images and an exact start (first update exactly 0); the current image moved by (1, 1); the current image + 30 (the
                mean-difference term carries it) from an exact start and from two starts off the alignment; the checkerboard at an exact start
                and a quarter pixel off; the white quadrant moved by (1, 1): residuals of 255; stop_threshold: two starts whose first update
                squares to float(0.03 * 0.03) exactly (the stop rule is `<`: a second iteration runs) and their lattice neighbour just inside.
  singular      det H == 0: a flat patch, vertical stripes only, horizontal stripes only, and a reference keypoint 20 px outside the image
                (the patch is all zeros).  Hinv is inf / NaN, the first update and the pixel are NaN, iteration 1 stops at the window gate
                (int(floor(NaN)) is below 4 on the host and on the device) and the pixel comes back NaN with success 0.  Device and oracle are
                compared on NaN-ness there, not on NaN bits.  The `isnan` test behind the gate (src/Align.cc:59-61) can therefore not be
                reached and no case is owed for it.
  search_level  P4: octaves 0..3 at identity give D == 1, 4, 16, 64 exactly and sl == 0, 1, 2, 3; a forward translation that halves the depth
                magnifies by 2 (D == 4 at octave 0); the cap: D == 16 with 2 levels, D == 16 with 1 level, D == 256 at octave 3 of P4 all stop at
                nlevels - 1 with D still above 3; the threshold on the 1.2 pyramid: octave 3 (s = 1.728, D = 2.985984) at depth 4 and a forward
                translation of k / 4096: k = 38 gives the largest D below 3.0 (2.9998846) and k = 39 the smallest above it (3.0002546) among
                k = 0 .. 63 (threshold_search; the CPU tier repeats the search).  No dyadic (Z, tz) gives D == 3.0f: with identity rotations A is
                s * Z / (Z + tz) * I and its square rounds to 3.0f for A == float(sqrt(3)) alone.  determinant_3 reaches that float with a
                principal point at (0, 0), a reference keypoint at (0.5, 0.5) and a tz found by stepping through neighbouring floats (D == 3.0f
                stays on level 0: the test is D > 3.0); determinant_3_next is the neighbouring tz whose D is 3.0000007 (level 1).  A negative
                determinant needs a mirror, which needs a rotation: it is the third case of the `rotation` family.
  rotation      an in-plane plus out-of-plane rotation of the current frame, one of the reference frame, and the mirror (the current camera
                turned by pi about y: A = diag(-1, 1), D = -1, sl == 0).  restated=False: the restatement's GetWarpAffineMatrix covers identity
                rotations only; these three cases are held by the oracle, the reference's own code and the device.
  batch         n = 1, 3, 4, 5, 8, 9 (kDirWaves = 4 candidates per workgroup); one candidate at every even, then every odd position of a
                9-batch between candidates that stop at the gate, run 10 iterations or go singular -- every copy returns the same bits;
                candidates of two reference slots; cur_slot == ref_slot.  The GPU tier runs these with and without want_patches.

Frustum families (Rcw = I, tcw = 0, Ow = 0, dyadic points unless noted; minX = minY = 0, maxX = w, maxY = h as make_camera sets them):
  depth     PcZ == -0.0 and +0.0 with PcX != 0 (u is -+inf: out), the smallest positive normal (dist underflows to 0 < minDistance: out), -tiny.
  image     u == minX, u == maxX, v == minY, v == maxY (in view) and the nearest projection outside each (192 + 2^-16, -2^-17, ...: out).
  distance  dist == minDistance and == maxDistance (in view), one ulp outside each (out).
  angle     viewCos == limit exactly (PO = (0,0,2), Pn = (0,0,0.5), limit 0.5; Pn = 0, limit 0.0) and one ulp below.
  level     dist == 1 and mfMaxDistance on every step of ceil(log(ratio) / logScaleFactor), the float below each step, ratio < 1 (clamps to
            0) and 1e30 (clamps to nlevels - 1), for 8 and 12 levels of 1.2, 4 levels of 2.0 and 1 level.  The steps come from a bisection
            over oracle.predict_scale (the host's libm), never from ygzf_predict_scale_steps.
  mask      candidate[i] == 0 on points that are in view otherwise.
  batch     n = 1, 255, 256, 257 (the block is 256 threads), mbf = 32 so that projXR differs from projX, and one pose with a rotation and a
            translation so that the three-term sums round.
  fused     search_local_points: MapPoints projecting exactly onto maxX and maxY (and their corner) with a keypoint inside the radius: the
            edge cell of the feature grid on the path that chains k_frustum into the matcher.

Undefined in the reference, no case built: det(A_cur_ref) == 0 or NaN (depth 0 in the reference frame, or a point on the current camera's plane
c[2] == 0): the reference then indexes the image with int(NaN); and dist == 0 with minDistance <= 0, which gives int(ceil(inf)).  reach() of
every direct case asserts a finite non-zero determinant, and of every frustum case dist > 0 wherever the distance gate is reached.

MUTATIONS / MOVES: per wrong form and case, the labels whose answer it changes; every other label of the mutation's family keeps its answer.
  EQUIVALENT  z_le (PcZ <= 0 instead of < 0): the two differ for PcZ == +-0 alone.  Then invz is +-inf and u = fx * PcX * invz + cx is +-inf for
              PcX != 0 (out at the u gate either way), likewise v for PcY != 0; PcX == PcY == PcZ == 0 is the point at the camera centre, whose
              dist is 0 up to the rounding of Ow: the second undefined situation above.  No defined input tells the two forms apart.
  MAY_MOVE    level_floor moves every step label (at a step ceil() has just left a whole number); one float below a step the quotient may or
              may not be that whole number exactly, depending on the host's logf: those labels are free to move or stay."""
import ctypes
import ctypes.util
import math

import numpy as np

from tests.matcher_cases import flip, make_keys

f32 = np.float32
CONFIGS = dict(L8=(1.2, 8, 192, 144), P4=(2.0, 4, 192, 144), L2=(1.2, 2, 96, 72), L1=(1.2, 1, 96, 72), L12=(1.2, 12, 192, 144))
DIRECT_MUTATIONS = ("warp_lt_w", "warp_le_0", "warp_gt", "align_lo_3", "align_lo_5", "align_hi_open", "level_ge", "level_uncapped",
                    "level_sigma_octave", "no_mean_diff", "iters_9", "stop_le", "patch_scale_octave", "hessian_unit_missing")
FRUSTUM_MUTATIONS = ("u_open", "v_open", "dist_open", "cos_le", "level_floor", "level_unclamped_low", "level_unclamped_high", "xr_plus")
EQUIVALENT = ("z_le",)
# labels a mutation may move or keep, depending on the host's libm: whether log(ratio) / logScaleFactor is a whole number one float below a step
MAY_MOVE = {"level_floor": "below"}
MUTATION_FAMILY = dict(warp_lt_w="warp_border", warp_le_0="warp_border", warp_gt="warp_border", align_lo_3="align_border",
                       align_lo_5="align_border", align_hi_open="align_border", iters_9="align_border", level_ge="search_level",
                       level_uncapped="search_level", level_sigma_octave="search_level", patch_scale_octave="search_level",
                       no_mean_diff="align_values", hessian_unit_missing="align_values", stop_le="align_values",
                       z_le="depth", u_open="image", v_open="image", dist_open="distance", cos_le="angle", level_floor="level",
                       level_unclamped_low="level", level_unclamped_high="level", xr_plus="batch")
# mutation -> case -> labels it moves.  Why: the three warp forms move the patches whose first / last sample sits on column or row 0 / w - 1 / h - 1
# (<= 0 also zeroes column 0 of the patches that start one pixel outside; >= w and > w - 1 both sample column w - 1); the gate forms move the starts
# that sit on 3, 4 and w - 4 (walks_out stops at floor(u) == 3, which < 3 lets run on; it starts on 5, which < 5 lets run too); nine iterations end
# ten_iterations one update early; without the cap the capped cases climb on; the octave's sigma stalls at octave 0 (factor 1: D > 3 climbs to the
# cap) and overshoots above octave 1, octave 1 itself and D <= 3 are untouched; pp scaled by the reference octave differs wherever sl != octave.
# no_mean_diff: in exact arithmetic the mean difference does not reach u and v at all -- a constant m added to every residual changes Jres by
# -m * H[:, 2] and the update by -m * Hinv * H[:, 2] = (0, 0, -m) -- so dropping it shows through the rounding of res * dx alone: of the + 30
# cases that start off the alignment (small coordinates, where an ulp of u is 2^-20) one ends on other bits, the other, like the exact start and
# the moved images, does not.  Without H[8] = 64 every Hinv differs, and the answer with it unless Jres is exactly 0 and Hinv stays finite (the
# checkerboard's H is diagonal: without H[8] it is singular).
MOVES = {
    "warp_lt_w": {"warp_border_L8": "col_end_w-1 row_end_h-1 corner_br", "warp_border_octave1": "col_end_w-1 row_end_h-1"},
    "warp_gt": {"warp_border_L8": "col_end_w-1 row_end_h-1 corner_br", "warp_border_octave1": "col_end_w-1 row_end_h-1"},
    "warp_le_0": {"warp_border_L8": "col_start_0 col_start_-1 row_start_0 row_start_-1 corner_tl",
                  "warp_border_octave1": "col_start_0 col_start_-1 row_start_0 row_start_-1"},
    "align_lo_3": {"gate_L8": "u3 v3 u_below_4", "gate_level1": "u3 v3", "walks_out": "left"},
    "align_lo_5": {"gate_L8": "u4 v4", "gate_level1": "u4 v4"},
    "align_hi_open": {"gate_L8": "u_w-4 v_h-4", "gate_level1": "u_w-4 v_h-4"},
    "iters_9": {"ten_iterations": "p"},
    "level_ge": {"determinant_3": "p"},
    "stop_le": {"stop_threshold": "on on2"},
    "level_floor": {"steps_L8": " ".join("step%d" % k for k in range(1, 8)), "steps_L12": " ".join("step%d" % k for k in range(1, 12)),
                    "steps_P4": "step1 step2 step3"},
    "level_unclamped_low": {"steps_%s" % c: "ratio_half" for c in ("L8", "L12", "P4", "L1")},
    "level_unclamped_high": {"steps_%s" % c: "ratio_huge" for c in ("L8", "L12", "P4", "L1")},
    "xr_plus": {"n_1": "p0", "n_255": "p0 p1 p253", "n_256": "p0 p1", "n_257": "p0 p1 p256", "posed_257": "p0 p1 p256"},
    "level_uncapped": {"cap_L2": "d16", "cap_L1": "d16", "cap_P4_octave3": "d256"},
    "level_sigma_octave": {"octaves_P4": "o2 o3", "magnified_P4": "o0_P4", "magnified_L8": "o0_L8", "cap_P4_octave3": "d256",
                           "determinant_3_next": "p"},
    "patch_scale_octave": {"magnified_P4": "o0_P4 o1_P4", "magnified_L8": "o0_L8", "cap_L2": "d16", "threshold_below": "p", "threshold_above": "p",
                           "determinant_3_next": "p"},
    "no_mean_diff": {"brightness_offset": "off2"},
    "hessian_unit_missing": {"brightness_offset": "p off off2", "moved_1_1": "p", "saturated_moved": "p", "identical": "checker_exact checker_quarter",
                             "stop_threshold": "on on2 inside"},
    "u_open": {"image_edges": "u_min u_max corner"},
    "v_open": {"image_edges": "v_min v_max corner"},
    "dist_open": {"distance_edges": "min_eq max_eq both_eq"},
    "cos_le": {"angle_limit_0.5": "eq", "angle_limit_0": "eq"},
}


def scale_tables(scale_factor, nlevels):
    """ORBextractor's mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2 (tests/test_direct_cases.py checks them against the oracle's)"""
    s = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        s[i] = s[i - 1] * f32(scale_factor)
    s2 = (s * s).astype(f32)
    return dict(scale=s, inv_scale=(f32(1) / s).astype(f32), sigma2=s2, inv_sigma2=(f32(1) / s2).astype(f32))


def camera(cfg, mbf=0.0):
    _, _, w, h = CONFIGS[cfg]
    return dict(fx=256.0, fy=256.0, cx=w / 2.0, cy=h / 2.0, mb=0.0, mbf=mbf)


# ---- images -----------------------------------------------------------------------------------------------------------------------------------
BLOCKS = dict(checker=(24, 24), flat=(60, 24), vstripes=(96, 24), hstripes=(132, 24), quadrant=(24, 96))   # top-left corners of the 24 x 24 blocks


def block_centre(name):
    x, y = BLOCKS[name]
    return x + 12, y + 12


def base_image(w, h, seed, blocks=True):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h + 16, w + 16)).astype(np.int64)
    for _ in range(2):                                           # 5 x 5 box sums, twice
        c = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), axis=0), axis=1)
        a = c[5:, 5:] - c[:-5, 5:] - c[5:, :-5] + c[:-5, :-5]
    a = a[:h, :w]
    a = np.clip((a - int(a.mean())) * 10 // 625 + 120, 16, 225).astype(np.uint8)
    if blocks and w >= 192:
        yy, xx = np.mgrid[0:24, 0:24]
        x, y = BLOCKS["checker"]; a[y:y + 24, x:x + 24] = (((xx // 2 + yy // 2) % 2) * 255).astype(np.uint8)
        x, y = BLOCKS["flat"]; a[y:y + 24, x:x + 24] = 100
        x, y = BLOCKS["vstripes"]; a[y:y + 24, x:x + 24] = (40 + 160 * ((xx // 2) % 2)).astype(np.uint8)
        x, y = BLOCKS["hstripes"]; a[y:y + 24, x:x + 24] = (40 + 160 * ((yy // 2) % 2)).astype(np.uint8)
        x, y = BLOCKS["quadrant"]; a[y:y + 24, x:x + 24] = (255 * ((xx >= 12) & (yy >= 12))).astype(np.uint8)
    return a


def moved(img, dx, dy):
    """out[y, x] = img[y - dy, x - dx]: the content moves by (+dx, +dy); rows / columns that enter repeat the edge"""
    h, w = img.shape
    ys = np.clip(np.arange(h) - dy, 0, h - 1)
    xs = np.clip(np.arange(w) - dx, 0, w - 1)
    return np.ascontiguousarray(img[ys][:, xs])


def crop_with_zeros(level_img, x0, y0):
    """WarpAffine from first principles when the samples are the integers x0 .. x0 + 9, y0 .. y0 + 9: the pixel, or 0 outside [0, w - 1) x [0, h - 1)"""
    h, w = level_img.shape
    out = np.zeros((10, 10), np.uint8)
    for y in range(10):
        for x in range(10):
            c, r = x0 + x, y0 + y
            if 0 <= c < w - 1 and 0 <= r < h - 1:
                out[y, x] = level_img[r, c]
    return out.reshape(100)


# ---- the restatement: FindDirectProjection -------------------------------------------------------------------------------------------------------
INT_MIN = -2 ** 31


def _inverse3(m):
    """Matrix3f::inverse() as oracle_direct.cpp writes it out: cofactors, the determinant from the first column"""
    M = lambda i, j: m[3 * (i % 3) + (j % 3)]
    cof = lambda i, j: M(i + 1, j + 1) * M(i + 2, j + 2) - M(i + 1, j + 2) * M(i + 2, j + 1)
    c00, c10, c20 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = (c00 * M(0, 0) + c10 * M(1, 0)) + c20 * M(2, 0)
    invdet = f32(1) / det
    return [c00 * invdet, c10 * invdet, c20 * invdet, cof(0, 1) * invdet, cof(1, 1) * invdet, cof(2, 1) * invdet,
            cof(0, 2) * invdet, cof(1, 2) * invdet, cof(2, 2) * invdet]


def warp_matrix_identity(kp, ref_t, cur_t, mp, scale, cam):
    """GetWarpAffineMatrix (:1525-1548) for poses whose rotations are the identity: T * p = p + t and T_cur_ref.t = (-t_ref) + t_cur"""
    fx, fy, cx, cy = f32(cam["fx"]), f32(cam["fy"]), f32(cam["cx"]), f32(cam["cy"])
    px, py, s = f32(kp["x"]), f32(kp["y"]), scale[int(kp["octave"])]
    tr, tc = [f32(v) for v in ref_t], [f32(v) for v in cur_t]
    pt = [f32(mp[k]) + tr[k] for k in range(3)]
    depth = pt[2]
    du = (px + f32(4) * s, py + f32(0) * s)
    dv = (px + f32(0) * s, py + f32(4) * s)
    p_du = ((du[0] - cx) * depth / fx, (du[1] - cy) * depth / fy, depth)
    p_dv = ((dv[0] - cx) * depth / fx, (dv[1] - cy) * depth / fy, depth)
    tcr = [(-tr[k]) + tc[k] for k in range(3)]

    def w2p(p):
        c = [p[k] + tcr[k] for k in range(3)]
        return fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy
    pc, pu, pv = w2p(pt), w2p(p_du), w2p(p_dv)
    return [(pu[0] - pc[0]) / f32(4), (pv[0] - pc[0]) / f32(4), (pu[1] - pc[1]) / f32(4), (pv[1] - pc[1]) / f32(4)]   # row-major A_cur_ref


def _pad(img, n):
    return np.pad(img, n, mode="edge")


def direct_from_A(A, kp, px0, ref_pyr, cur_pyr, tabs, mutation=None, trace=None):
    """GetBestSearchLevel, WarpAffine and Align2D from A_cur_ref onward -> (px (2,) f32, search_level, success, patch_with_border (100,) u8)"""
    mut = mutation
    scale, inv_scale = tabs["scale"], tabs["inv_scale"]
    n = len(scale)
    octave = int(kp["octave"])
    t = dict(A=[float(a) for a in A])
    # GetBestSearchLevel include/ORBmatcher.h:185-197
    D = A[0] * A[3] - A[2] * A[1]
    t["D"] = float(D)
    sl = 0
    k = tabs["inv_sigma2"][octave if mut == "level_sigma_octave" else (1 if n > 1 else 0)]
    while ((D >= f32(3)) if mut == "level_ge" else (D > f32(3))) and (sl < n - 1 or (mut == "level_uncapped" and sl < 31)):
        sl += 1
        D = D * k
    t["sl"], t["D_end"] = sl, float(D)
    if sl >= n:                        # (level_uncapped alone) there is no such level: the answer differs already
        t.update(code="NO_LEVEL", updates=0)
        if trace is not None:
            trace.append(t)
        return np.full(2, np.nan, f32), sl, 0, np.zeros(100, np.uint8)
    # WarpAffine :1550-1572, half_patch_size = 5
    det = A[0] * A[3] - A[2] * A[1]
    invdet = f32(1) / det
    ARC = [A[3] * invdet, -A[1] * invdet, -A[2] * invdet, A[0] * invdet]
    img = ref_pyr[octave]
    h, w = img.shape
    imgp = _pad(img, ((0, 2), (0, 2)))                              # the wrong forms sample column w - 1 / row h - 1, whose neighbours lie outside
    pr = (f32(kp["x"]) / scale[octave], f32(kp["y"]) / scale[octave])
    pscale = scale[octave] if mut == "patch_scale_octave" else scale[sl]
    pwb = np.zeros(100, np.uint8)
    for y in range(10):
        for x in range(10):
            pp0, pp1 = f32(x - 5) * pscale, f32(y - 5) * pscale
            p0 = (ARC[0] * pp0 + ARC[1] * pp1) + pr[0]
            p1 = (ARC[2] * pp0 + ARC[3] * pp1) + pr[1]
            if mut == "warp_lt_w":
                out = p0 < 0 or p1 < 0 or p0 >= w or p1 >= h
            elif mut == "warp_le_0":
                out = p0 <= 0 or p1 <= 0 or p0 >= w - 1 or p1 >= h - 1
            elif mut == "warp_gt":
                out = p0 < 0 or p1 < 0 or p0 > w - 1 or p1 > h - 1
            else:
                out = p0 < 0 or p1 < 0 or p0 >= w - 1 or p1 >= h - 1
            if out:
                continue
            X, Y = float(p0), float(p1)
            xx, yy = X - math.floor(X), Y - math.floor(Y)
            d = imgp[int(Y):int(Y) + 2, int(X):int(X) + 2]
            pwb[10 * y + x] = int((1 - xx) * (1 - yy) * float(d[0, 0]) + xx * (1 - yy) * float(d[0, 1]) + (1 - xx) * yy * float(d[1, 0])
                                  + xx * yy * float(d[1, 1]))
    t["zeros"] = int((pwb == 0).sum())
    # Align2D src/Align.cc:8-104 on the current frame's level sl
    P = pwb.reshape(10, 10).astype(np.int64)
    ref = P[1:9, 1:9].astype(f32).reshape(64)
    dx = (0.5 * (P[1:9, 2:10] - P[1:9, 0:8])).astype(f32).reshape(64)
    dy = (0.5 * (P[2:10, 1:9] - P[0:8, 1:9])).astype(f32).reshape(64)
    J = (dx, dy, np.ones(64, f32))
    H = [np.add.accumulate((J[a] * J[b]).astype(f32), dtype=f32)[-1] for a in range(3) for b in range(3)]   # += in raster order
    if mut == "hessian_unit_missing":
        H[8] = f32(0)
    t["H"] = [float(v) for v in H]
    Hinv = _inverse3(H)
    cur = cur_pyr[sl]
    ch, cw = cur.shape
    curp = _pad(cur, 2).astype(f32)                                  # the wrong gate forms read one pixel outside the level
    u0, v0 = f32(px0[0]) * inv_scale[sl], f32(px0[1]) * inv_scale[sl]
    u, v = u0, v0
    mean_diff = f32(0)
    min_update_squared = f32(0.03 * 0.03)
    lo = {"align_lo_3": 3, "align_lo_5": 5}.get(mut, 4)
    converged, code, updates = False, "EXHAUSTED", 0
    for it in range(9 if mut == "iters_9" else 10):
        u_r = int(math.floor(u)) if math.isfinite(u) else INT_MIN     # (int) of a NaN or an out-of-range float on the host
        v_r = int(math.floor(v)) if math.isfinite(v) else INT_MIN
        if mut == "align_hi_open":
            gate = u_r < lo or v_r < lo or u_r > cw - 4 or v_r > ch - 4
        else:
            gate = u_r < lo or v_r < lo or u_r >= cw - 4 or v_r >= ch - 4
        if gate:
            code = "GATE"
            break
        sx, sy = u - f32(u_r), v - f32(v_r)
        wTL = f32((1.0 - float(sx)) * (1.0 - float(sy)))
        wTR = f32(float(sx) * (1.0 - float(sy)))
        wBL = f32((1.0 - float(sx)) * float(sy))
        wBR = sx * sy
        y0, x0 = v_r - 4 + 2, u_r - 4 + 2
        a, b = curp[y0:y0 + 8, x0:x0 + 8].reshape(64), curp[y0:y0 + 8, x0 + 1:x0 + 9].reshape(64)
        c, d = curp[y0 + 1:y0 + 9, x0:x0 + 8].reshape(64), curp[y0 + 1:y0 + 9, x0 + 1:x0 + 9].reshape(64)
        search = ((wTL * a + wTR * b) + wBL * c) + wBR * d
        res = (search - ref) + mean_diff
        Jres = [-np.add.accumulate((res * dx).astype(f32), dtype=f32)[-1], -np.add.accumulate((res * dy).astype(f32), dtype=f32)[-1],
                -np.add.accumulate(res.astype(f32), dtype=f32)[-1]]   # Jres -= product, in raster order
        up = [(Hinv[3 * r] * Jres[0] + Hinv[3 * r + 1] * Jres[1]) + Hinv[3 * r + 2] * Jres[2] for r in range(3)]
        u = u + up[0]
        v = v + up[1]
        if mut != "no_mean_diff":
            mean_diff = mean_diff + up[2]
        updates += 1
        t.setdefault("first_update", [float(x) for x in up])
        n2 = up[0] * up[0] + up[1] * up[1]
        t.setdefault("first_n2", n2)
        if (n2 <= min_update_squared) if mut == "stop_le" else (n2 < min_update_squared):
            converged, code = True, "CONVERGED"
            break
    t.update(code=code, updates=updates, start=(float(u0 * scale[sl]), float(v0 * scale[sl])), mean_diff=float(mean_diff))
    if trace is not None:
        trace.append(t)
    return np.array([u * scale[sl], v * scale[sl]], f32), sl, int(converged), pwb


class DirectCase:
    """images[slot]; candidate i = (ref_slot[i], ref_T7[i], ref_kp[i], world[i], px0[i]); the current frame is images[cur_slot] at pose cur_T7"""

    def __init__(self, name, family, cfg, images, cur_slot, cur_t=(0, 0, 0), cur_q=(0, 0, 0, 1), restated=True, cam=None):
        self.name, self.family, self.cfg, self.images, self.cur_slot, self.restated = name, family, cfg, images, cur_slot, restated
        self.cur_T7 = np.array(list(cur_q) + list(cur_t), f32)
        self.cam = cam or camera(cfg)
        self.labels, self.expect, self.undefined = {}, {}, None
        self._rows = []

    def add(self, label, xy, octave, px0, Z=2.0, ref_slot=0, ref_t=(0, 0, 0), ref_q=(0, 0, 0, 1), **expect):
        """a reference keypoint at pixel xy whose MapPoint lies at depth Z on its viewing ray in the reference frame"""
        c = self.cam
        p_ref = np.array([(f32(xy[0]) - f32(c["cx"])) * f32(Z) / f32(c["fx"]), (f32(xy[1]) - f32(c["cy"])) * f32(Z) / f32(c["fy"]), f32(Z)], np.float64)
        R = quat_to_R(ref_q)
        world = R.T @ (p_ref - np.array(ref_t, np.float64))           # exact for identity rotations and dyadic numbers
        self.labels[label] = len(self._rows)
        self.expect[label] = expect
        self._rows.append((xy, octave, px0, world, ref_slot, list(ref_q) + list(ref_t)))
        return self

    def done(self):
        r = self._rows
        self.ref_kp = make_keys(np.array([x[0] for x in r], f32), np.array([x[1] for x in r], np.int32))
        self.px0 = np.array([x[2] for x in r], f32).reshape(-1, 2)
        self.world = np.array([x[3] for x in r], f32).reshape(-1, 3)
        self.ref_slot = np.array([x[4] for x in r], np.int32)
        self.ref_T7 = np.array([x[5] for x in r], f32).reshape(-1, 7)
        return self

    def __repr__(self):
        return "%s:%s" % (self.family, self.name)

    def reach(self):
        """None, or why the case lies in what the reference leaves undefined: det(A_cur_ref) finite and non-zero, in double from the poses"""
        for label, i in self.labels.items():
            A = warp_matrix_f64(self, i)
            det = A[0] * A[3] - A[1] * A[2]
            if not (math.isfinite(det) and det != 0):
                return "%s: det(A_cur_ref) = %r" % (label, det)
        return None


def quat_to_R(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def warp_matrix_f64(case, i):
    """A_cur_ref of candidate i in double, rotations included (for reach() and for the claims of the rotation family; never compared bit for bit)"""
    c = case.cam
    s = float(scale_tables(*CONFIGS[case.cfg][:2])["scale"][int(case.ref_kp["octave"][i])])
    Rr, tr = quat_to_R(case.ref_T7[i, :4]), case.ref_T7[i, 4:].astype(np.float64)
    Rc, tc = quat_to_R(case.cur_T7[:4]), case.cur_T7[4:].astype(np.float64)
    pt = Rr @ case.world[i].astype(np.float64) + tr
    x, y, depth = float(case.ref_kp["x"][i]), float(case.ref_kp["y"][i]), pt[2]
    bp = lambda a, b: np.array([(a - c["cx"]) * depth / c["fx"], (b - c["cy"]) * depth / c["fy"], depth])

    def w2p(p):
        with np.errstate(all="ignore"):
            q = Rc @ (Rr.T @ (p - tr)) + tc
            return np.array([c["fx"] * q[0] / q[2] + c["cx"], c["fy"] * q[1] / q[2] + c["cy"]])
    pc, pu, pv = w2p(pt), w2p(bp(x + 4 * s, y)), w2p(bp(x, y + 4 * s))
    return [(pu[0] - pc[0]) / 4, (pv[0] - pc[0]) / 4, (pu[1] - pc[1]) / 4, (pv[1] - pc[1]) / 4]


def run_restatement(oracle, case, mutation=None, trace=None):
    """the restatement over the oracle's pyramids (the pyramid is the extractor's, tested elsewhere) -> (px n x 2, search_level, success, patches)"""
    assert case.restated
    sf, nl, _, _ = CONFIGS[case.cfg]
    tabs = scale_tables(sf, nl)
    oex = oracle.Extractor(1000, sf, nl, 20, 7)
    pyr = [oex.pyramid(im) for im in case.images]
    n = len(case.ref_kp)
    px, sl, ok, pt = np.zeros((n, 2), f32), np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 100), np.uint8)
    with np.errstate(all="ignore"):
        for i in range(n):
            assert (case.ref_T7[i, :4] == (0, 0, 0, 1)).all() and (case.cur_T7[:4] == (0, 0, 0, 1)).all()
            A = warp_matrix_identity(case.ref_kp[i], case.ref_T7[i, 4:], case.cur_T7[4:], case.world[i], tabs["scale"], case.cam)
            px[i], sl[i], ok[i], pt[i] = direct_from_A(A, case.ref_kp[i], case.px0[i], pyr[case.ref_slot[i]], pyr[case.cur_slot], tabs, mutation, trace)
    return px, sl, ok, pt


def run_oracle(oracle, case, fn=None):
    """-> the oracle's answer; fn: another implementation with the oracle's signature after the extractor (the reference's own code)"""
    sf, nl, _, _ = CONFIGS[case.cfg]
    oex = oracle.Extractor(1000, sf, nl, 20, 7)
    args = (case.images, case.images[case.cur_slot], case.cur_T7, case.cam, case.ref_slot, case.ref_T7, case.ref_kp, case.world, case.px0)
    return fn(oex, *args) if fn else oex.find_direct_projection_batch(*args)


def run_device(ex, case, want_patches=True):
    """ex: an Extractor of the case's configuration whose image cache was reserved for its frame size and at least len(images) slots"""
    from orb_ygz_slam_amd import make_camera
    _, _, w, h = CONFIGS[case.cfg]
    c = case.cam
    for s, im in enumerate(case.images):
        ex.image_cache_put(s, im)
    return ex.find_direct_projection_batch(make_camera(w, h, fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"]), case.cur_slot, case.cur_T7,
                                           case.ref_slot, case.ref_T7, case.ref_kp, case.world, case.px0, want_patches=want_patches)


def same_direct(a, b):
    """pixels bit-identical where b's are not NaN and NaN where they are; level, flag (and patches when both carry them) equal"""
    nan = np.isnan(b[0])
    ok = np.array_equal(np.isnan(a[0]), nan) and np.array_equal(a[0].view(np.uint32)[~nan], b[0].view(np.uint32)[~nan])
    ok = ok and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    if len(a) > 3 and len(b) > 3:
        ok = ok and np.array_equal(a[3], b[3])
    return bool(ok)


def moved_labels(case, a, b):
    """the labels whose answer differs between a and b (patch included)"""
    out = []
    for label, i in case.labels.items():
        if not same_direct(tuple(x[i:i + 1] for x in a), tuple(x[i:i + 1] for x in b)):
            out.append(label)
    return sorted(out)


# ---- the direct cases ----------------------------------------------------------------------------------------------------------------------------
THRESHOLD_K = (38, 39)      # forward translation k / 4096 at depth 4, octave 3 of the 1.2 pyramid: D just below / just above 3.0 (see threshold_search)


def threshold_search(ks=range(64), octave=3, Z=4.0):
    """-> {k: D} of the restatement's float D for a forward translation of k / 4096 at depth Z"""
    tabs = scale_tables(1.2, 8)
    cam = camera("L8")
    out = {}
    kp = make_keys(np.array([[96, 72]], f32), octave)[0]
    for k in ks:
        A = warp_matrix_identity(kp, (0, 0, 0), (0, 0, -k / 4096.0), (0, 0, Z), tabs["scale"], cam)
        out[k] = float(A[0] * A[3] - A[2] * A[1])
    return out


def direct_cases():
    out = []
    T = base_image(192, 144, 11)
    T2 = base_image(192, 144, 12)
    S = np.random.default_rng(13).integers(16, 226, (72, 96)).astype(np.uint8)      # raw noise: a patch magnified 4 times still has gradients
    w, h = 192, 144
    mid = (96.0, 72.0)

    # -- warp_border: the patch covers columns x - 5 .. x + 4 and rows y - 5 .. y + 4 of the reference level
    c = DirectCase("warp_border_L8", "warp_border", "L8", [T, T], 1)
    for label, (x, y) in (("col_start_0", (5, 70)), ("col_start_-1", (4, 70)), ("col_end_w-2", (w - 6, 70)), ("col_end_w-1", (w - 5, 70)),
                          ("row_start_0", (90, 5)), ("row_start_-1", (90, 4)), ("row_end_h-2", (90, h - 6)), ("row_end_h-1", (90, h - 5)),
                          ("corner_tl", (4, 4)), ("corner_br", (w - 5, h - 5)), ("inside", (90, 70))):
        c.add(label, (x, y), 0, mid, A=1.0, sl=0, crop=(0, 0, x - 5, y - 5))
    out.append(c.done())
    c = DirectCase("warp_border_octave1", "warp_border", "P4", [T, T], 1)
    w1, h1 = 96, 72
    for label, (x, y) in (("col_start_0", (5, 35)), ("col_start_-1", (4, 35)), ("col_end_w-2", (w1 - 6, 35)), ("col_end_w-1", (w1 - 5, 35)),
                          ("row_start_0", (45, 5)), ("row_start_-1", (45, 4)), ("row_end_h-2", (45, h1 - 6)), ("row_end_h-1", (45, h1 - 5))):
        c.add(label, (2 * x, 2 * y), 1, mid, A=2.0, sl=1, crop=(0, 1, x - 5, y - 5))
    out.append(c.done())

    # -- align_border
    run = dict(A=1.0, sl=0, code="CONVERGED", updates=1, ok=1, px="unchanged")
    stop = dict(A=1.0, sl=0, code="GATE", updates=0, ok=0, px="start")
    c = DirectCase("gate_L8", "align_border", "L8", [T, T], 1)
    for label, xy, e in (("u4", (4, 72), run), ("u3", (3, 72), stop), ("u_w-5", (w - 5, 72), run), ("u_w-4", (w - 4, 72), stop),
                         ("v4", (100, 4), run), ("v3", (100, 3), stop), ("v_h-5", (100, h - 5), run), ("v_h-4", (100, h - 4), stop)):
        c.add(label, xy, 0, xy, **e)
    c.add("u_below_4", (4, 80), 0, (float(np.nextafter(f32(4), f32(0))), 80.0), **stop)
    out.append(c.done())
    c = DirectCase("gate_level1", "align_border", "P4", [T, T], 1)
    for label, (x, y), e in (("u4", (4, 36), run), ("u3", (3, 36), stop), ("u_w-5", (w1 - 5, 36), run), ("u_w-4", (w1 - 4, 36), stop),
                             ("v4", (50, 4), run), ("v3", (50, 3), stop), ("v_h-5", (50, h1 - 5), run), ("v_h-4", (50, h1 - 4), stop)):
        c.add(label, (2 * x, 2 * y), 1, (2 * x, 2 * y), **dict(e, A=2.0, sl=1))
    out.append(c.done())
    c = DirectCase("walks_out", "align_border", "L8", [T, moved(T, -4, 0)], 1)
    c.add("left", (7, 100), 0, (5.0, 100.0), A=1.0, sl=0, code="GATE", updates=">=1", ok=0)
    out.append(c.done())
    c = DirectCase("ten_iterations", "align_border", "L8", [T2, T], 1)
    c.add("p", (96, 100), 0, (96, 100), A=1.0, sl=0, code="EXHAUSTED", updates=10, ok=0)
    out.append(c.done())

    # -- align_values
    c = DirectCase("identical", "align_values", "L8", [T, T], 1)
    c.add("exact", (96, 100), 0, (96, 100), A=1.0, sl=0, code="CONVERGED", updates=1, ok=1, px="unchanged")
    ck = block_centre("checker")
    c.add("checker_exact", ck, 0, ck, A=1.0, sl=0, code="CONVERGED", updates=1, ok=1, px="unchanged", H=(1040400.0, 1040400.0))
    c.add("checker_quarter", ck, 0, (ck[0] + 0.25, ck[1] + 0.25), A=1.0, sl=0, H=(1040400.0, 1040400.0))
    out.append(c.done())
    c = DirectCase("moved_1_1", "align_values", "L8", [T, moved(T, 1, 1)], 1)
    c.add("p", (96, 100), 0, (96, 100), A=1.0, sl=0, code="CONVERGED", updates=">=2", ok=1)
    out.append(c.done())
    c = DirectCase("brightness_offset", "align_values", "L8", [T, (T.astype(np.int64) + 30).astype(np.uint8)], 1)
    c.add("p", (96, 100), 0, (96, 100), A=1.0, sl=0, code="CONVERGED", updates=1, ok=1, mean_diff=-30)
    c.add("off", (8, 9), 0, (8.3, 9.4), A=1.0, sl=0, code="CONVERGED", updates=">=2", ok=1)
    c.add("off2", (9, 8), 0, (8.6, 8.3), A=1.0, sl=0, code="CONVERGED", updates=">=2", ok=1)
    out.append(c.done())
    c = DirectCase("saturated_moved", "align_values", "L8", [T, moved(T, 1, 1)], 1)
    c.add("p", block_centre("quadrant"), 0, block_centre("quadrant"), A=1.0, sl=0, updates=">=1")
    out.append(c.done())

    # the first update lands on the stop rule's threshold: update[0]^2 + update[1]^2 == float(0.03 * 0.03) exactly, so `<` runs a second iteration.
    # (Found by a search over the 2^-21 lattice of start pixels around the reference keypoint at (6, 6): for a column offset i the row offset j
    # where the squared update crosses the threshold is bisected and its neighbours are tested for equality; about one column in 250 has one.)
    c = DirectCase("stop_threshold", "align_values", "L8", [T, T], 1)
    c.add("on", (6, 6), 0, (6 + 51265 * 2.0 ** -21, 6 + 57791 * 2.0 ** -21), A=1.0, sl=0, first_n2=float(f32(0.03 * 0.03)), code="CONVERGED", updates=2, ok=1)
    c.add("on2", (6, 6), 0, (6 + 57370 * 2.0 ** -21, 6 + 45001 * 2.0 ** -21), A=1.0, sl=0, first_n2=float(f32(0.03 * 0.03)), code="CONVERGED", updates=2, ok=1)
    c.add("inside", (6, 6), 0, (6 + 51265 * 2.0 ** -21, 6 + 57790 * 2.0 ** -21), A=1.0, sl=0, code="CONVERGED", updates=1, ok=1)
    out.append(c.done())

    # -- singular
    nan = dict(A=1.0, sl=0, code="GATE", updates=1, ok=0, px="nan", det_H=0.0)
    c = DirectCase("singular", "singular", "L8", [T, T], 1)
    for name in ("flat", "vstripes", "hstripes"):
        c.add(name, block_centre(name), 0, block_centre(name), **nan)
    c.add("outside", (-20, 72), 0, mid, **dict(nan, zeros=100))
    out.append(c.done())

    # -- search_level
    c = DirectCase("octaves_P4", "search_level", "P4", [T, T], 1)
    for o in range(4):
        c.add("o%d" % o, mid, o, mid, A=float(2 ** o), D=float(4 ** o), sl=o)
    out.append(c.done())
    c = DirectCase("magnified_P4", "search_level", "P4", [T, T], 1, cur_t=(0, 0, -1))
    c.add("o0_P4", mid, 0, mid, Z=2.0, A=2.0, D=4.0, sl=1)
    c.add("o1_P4", mid, 1, mid, Z=2.0, A=4.0, D=16.0, sl=2)
    out.append(c.done())
    c = DirectCase("magnified_L8", "search_level", "L8", [T, T], 1, cur_t=(0, 0, -1))
    c.add("o0_L8", mid, 0, mid, Z=2.0, A=2.0, D=4.0, sl=1)
    out.append(c.done())
    c = DirectCase("cap_L2", "search_level", "L2", [S, S], 1, cur_t=(0, 0, -3))
    c.add("d16", (48, 36), 0, (48, 36), Z=4.0, A=4.0, D=16.0, sl=1, D_end_gt_3=True)
    out.append(c.done())
    c = DirectCase("cap_L1", "search_level", "L1", [S, S], 1, cur_t=(0, 0, -3))
    c.add("d16", (48, 36), 0, (48, 36), Z=4.0, A=4.0, D=16.0, sl=0, D_end_gt_3=True)
    out.append(c.done())
    c = DirectCase("cap_P4_octave3", "search_level", "P4", [T, T], 1, cur_t=(0, 0, -1))
    c.add("d256", mid, 3, mid, Z=2.0, A=16.0, D=256.0, sl=3, D_end_gt_3=True)
    out.append(c.done())
    for label, k, sl in (("below", THRESHOLD_K[0], 0), ("above", THRESHOLD_K[1], 1)):
        c = DirectCase("threshold_%s" % label, "search_level", "L8", [T, T], 1, cur_t=(0, 0, -k / 4096.0))
        c.add("p", mid, 3, mid, Z=4.0, sl=sl, threshold_k=k)
        out.append(c.done())

    # D == 3.0f exactly: cx = cy = 0 and a reference keypoint at (0.5, 0.5) keep the three projections below 8, where a float has the 2^-21 that
    # A = (px_du - px_cur) / 4 needs to reach float(sqrt(3)) = 1.7320508, the one float whose square rounds to 3.0f; tz was found by stepping through
    # the floats next to 2 / sqrt(3) - 2 (three neighbours give it).  One float further the magnification is two ulps more and D is 3.0000007.
    cam0 = dict(camera("L8"), cx=0.0, cy=0.0)
    for name, tz, e in (("determinant_3", -0.845299482345581, dict(D=3.0, sl=0)), ("determinant_3_next", -0.8452996015548706, dict(D_above_3=True, sl=1))):
        c = DirectCase(name, "search_level", "L8", [T, T], 1, cur_t=(0, 0, tz), cam=cam0)
        c.add("p", (0.5, 0.5), 0, mid, Z=2.0, **e)
        out.append(c.done())

    # -- rotation (not restated)
    c = DirectCase("cur_rotated", "rotation", "L8", [T, T2], 1, cur_t=(0.0625, -0.03125, 0.125), cur_q=_quat((0.05, -0.04, 0.3)), restated=False)
    c.add("a", (96, 100), 0, (100, 96), Z=2.0, A_entries_nonzero=True)
    c.add("b", (60, 90), 2, (70, 80), Z=4.0, A_entries_nonzero=True)
    out.append(c.done())
    c = DirectCase("ref_rotated", "rotation", "L8", [T, T2], 1, restated=False)
    c.add("a", (110, 80), 1, (105, 85), Z=2.0, ref_q=_quat((-0.03, 0.06, -0.2)), ref_t=(0.125, 0.0625, -0.25), A_entries_nonzero=True)
    out.append(c.done())
    c = DirectCase("mirror_negative_det", "rotation", "L8", [T, T2], 1, cur_t=(0, 0, 4), cur_q=(0, 1, 0, 0), restated=False)
    c.add("m", (104, 80), 0, (88, 80), Z=2.0, det_negative=True, sl=0)
    out.append(c.done())

    # -- batch
    def pool(c, order):
        items = dict(
            X=lambda l: c.add(l, (96, 100), 0, (96.25, 100.5), same="X"),
            stop=lambda l: c.add(l, (3, 72), 0, (3, 72), code="GATE", updates=0, ok=0),
            ten=lambda l: c.add(l, (96, 100), 0, (96, 100), ref_slot=2, code="EXHAUSTED", updates=10, ok=0),
            sing=lambda l: c.add(l, block_centre("flat"), 0, block_centre("flat"), px="nan", ok=0))
        for j, name in enumerate(order):
            items[name]("%s%d" % (name, j))
        return c.done()
    # slot 0: T (reference), slot 1: T (current), slot 2: the unrelated texture as a second reference (its candidates run all 10 iterations)
    for n in (1, 3, 4, 5, 8, 9):
        out.append(pool(DirectCase("n_%d" % n, "batch", "L8", [T, T, T2], 1), ("X", "stop", "ten", "sing", "X", "ten", "stop", "sing", "X")[:n]))
    out.append(pool(DirectCase("copies_even", "batch", "L8", [T, T, T2], 1), ("X", "stop", "X", "ten", "X", "sing", "X", "stop", "X")))
    out.append(pool(DirectCase("copies_odd", "batch", "L8", [T, T, T2], 1), ("ten", "X", "sing", "X", "stop", "X", "ten", "X", "sing")))
    c = DirectCase("two_ref_slots", "batch", "L8", [T, T2, T], 2)
    c.add("slot0", (96, 100), 0, (96, 100), ref_slot=0, code="CONVERGED", ok=1, px="unchanged")
    c.add("slot1", (96, 100), 0, (96, 100), ref_slot=1)
    c.add("slot0_again", (96, 100), 0, (96, 100), ref_slot=0, same="s0")
    c.add("slot0_third", (96, 100), 0, (96, 100), ref_slot=0, same="s0")
    out.append(c.done())
    c = DirectCase("cur_is_ref_slot", "batch", "L8", [T], 0)
    c.add("p", (96, 100), 0, (96, 100), code="CONVERGED", ok=1, px="unchanged")
    c.add("q", (60, 90), 0, (60.5, 90.25))
    out.append(c.done())
    return out


def _quat(rotvec):
    r = np.array(rotvec, np.float64)
    a = np.linalg.norm(r)
    q = np.concatenate([np.sin(a / 2) * r / a, [np.cos(a / 2)]])
    return tuple(float(v) for v in q.astype(f32))


# ---- the restatement: isInFrustum + PredictScale ------------------------------------------------------------------------------------------------
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def _logf(x):
    """std::log(float) of the host's libm, the one the oracle and ygzf_predict_scale_steps call"""
    return f32(_libm.logf(float(x)))


def _c_int(x):
    """(int) of a float on the host: INT_MIN for NaN and for what lies outside int"""
    x = float(x)
    return int(x) if math.isfinite(x) and -2.0 ** 31 <= x < 2.0 ** 31 else INT_MIN


def ref_frustum(case, mutation=None):
    """src/Frame.cc:363-422 + src/MapPoint.cc:359-373 -> (in_view, projX, projY, projXR, level, viewCos); zeros where the point is out"""
    mut = mutation
    a = case.a
    w, h = case.frame
    c = case.cam
    fx, fy, cx, cy, mbf = f32(c["fx"]), f32(c["fy"]), f32(c["cx"]), f32(c["cy"]), f32(c["mbf"])
    minX, minY, maxX, maxY = f32(0), f32(0), f32(w), f32(h)
    R, tc, Ow = a["Rcw"].reshape(9).astype(f32), a["tcw"].astype(f32), a["Ow"].astype(f32)
    limit, lsf, nl = f32(case.limit), f32(case.lsf), case.nlevels
    M = len(a["world"])
    iv, lv = np.zeros(M, np.uint8), np.zeros(M, np.int32)
    px, py, pxr, vcs = (np.zeros(M, f32) for _ in range(4))
    with np.errstate(all="ignore"):
        for i in range(M):
            P = a["world"][i].astype(f32)
            Pc = [((R[3 * r] * P[0] + R[3 * r + 1] * P[1]) + R[3 * r + 2] * P[2]) + tc[r] for r in range(3)]
            if (Pc[2] <= f32(0)) if mut == "z_le" else (Pc[2] < f32(0)):
                continue
            invz = f32(1) / Pc[2]
            u = fx * Pc[0] * invz + cx
            v = fy * Pc[1] * invz + cy
            if (u <= minX or u >= maxX) if mut == "u_open" else (u < minX or u > maxX):
                continue
            if (v <= minY or v >= maxY) if mut == "v_open" else (v < minY or v > maxY):
                continue
            PO = [P[k] - Ow[k] for k in range(3)]
            dist = np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2])
            mn, mx = a["min_dist"][i], a["max_dist"][i]
            if (dist <= mn or dist >= mx) if mut == "dist_open" else (dist < mn or dist > mx):
                continue
            Pn = a["normal"][i].astype(f32)
            vc = ((PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2]) / dist
            if (vc <= limit) if mut == "cos_le" else (vc < limit):
                continue
            ratio = a["mf_max"][i] / dist
            q = _logf(ratio) / lsf
            ns = _c_int(np.floor(q) if mut == "level_floor" else np.ceil(q))
            if ns < 0:
                if mut != "level_unclamped_low":
                    ns = 0
            elif ns >= nl and mut != "level_unclamped_high":
                ns = nl - 1
            iv[i], px[i], py[i], lv[i], vcs[i] = 1, u, v, ns, vc
            pxr[i] = (u + mbf * invz) if mut == "xr_plus" else (u - mbf * invz)
    if a.get("candidate") is not None:
        keep = a["candidate"].astype(bool)
        iv, lv = iv * keep, lv * keep
        px, py, pxr, vcs = px * keep, py * keep, pxr * keep, vcs * keep
    return iv, px, py, pxr, lv, vcs


class FrustumCase:
    def __init__(self, name, family, cfg, limit=0.5, mbf=0.0, Rcw=None, tcw=(0, 0, 0), Ow=(0, 0, 0)):
        self.name, self.family, self.cfg, self.limit = name, family, cfg, limit
        sf, self.nlevels, w, h = CONFIGS[cfg]
        self.frame = (w, h)
        self.cam = camera(cfg, mbf)
        self.lsf = np.log(f32(sf), dtype=f32)                       # mfLogScaleFactor = log(mfScaleFactor) in float
        self.scale = scale_tables(sf, self.nlevels)["scale"]
        self.Rcw = np.eye(3, dtype=f32) if Rcw is None else np.array(Rcw, f32)
        self.tcw, self.Ow = np.array(tcw, f32), np.array(Ow, f32)
        self.labels, self.expect, self.undefined, self._rows, self.candidate = {}, {}, None, [], None

    def add(self, label, P, Pn=(0, 0, 1), mn=0.25, mx=64.0, mf=1.0, cand=1, **expect):
        if label is not None:
            self.labels[label] = len(self._rows)
            self.expect[label] = expect
        self._rows.append((P, Pn, mn, mx, mf, cand))
        return self

    def done(self):
        r = self._rows
        cand = np.array([x[5] for x in r], np.uint8)
        self.a = dict(world=np.array([x[0] for x in r], f32).reshape(-1, 3), normal=np.array([x[1] for x in r], f32).reshape(-1, 3),
                      min_dist=np.array([x[2] for x in r], f32), max_dist=np.array([x[3] for x in r], f32), mf_max=np.array([x[4] for x in r], f32),
                      Rcw=self.Rcw, tcw=self.tcw, Ow=self.Ow, candidate=None if cand.all() else cand)
        return self

    def __repr__(self):
        return "frustum_%s:%s" % (self.family, self.name)

    def reach(self):
        """None, or why the case lies in what the reference leaves undefined: dist > 0 wherever minDistance <= 0 would let it through"""
        a = self.a
        d = np.linalg.norm(a["world"].astype(np.float64) - a["Ow"].astype(np.float64), axis=1)
        bad = np.nonzero((d.astype(f32) == 0) & (a["min_dist"] <= 0))[0]
        return None if len(bad) == 0 else "point %d: dist == 0 with minDistance <= 0" % bad[0]


def frustum_args(case):
    a = case.a
    return (a["world"], a["normal"], a["max_dist"], a["min_dist"], a["mf_max"], a["Rcw"], a["tcw"], a["Ow"], case.lsf, case.limit)


def run_frustum_oracle(oracle, case):
    """-> (in_view, projX, projY, projXR, level, viewCos), the mask applied as the device applies it (the reference has no mask: its caller skips)"""
    w, h = case.frame
    k = make_keys(np.zeros((0, 2), f32))
    r = oracle.is_in_frustum(k, np.zeros((0, 32), np.uint8), case.scale, w, h, case.cam, *frustum_args(case))
    if case.a["candidate"] is not None:
        r = (r[0] & case.a["candidate"],) + tuple(r[1:])
    return r


def run_frustum_device(ex, case):
    from orb_ygz_slam_amd import make_camera
    w, h = case.frame
    c = case.cam
    cam = make_camera(w, h, fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"], mbf=c["mbf"])
    return ex.is_in_frustum_batch(cam, *frustum_args(case), candidate=case.a["candidate"])


def same_frustum(a, b):
    """in_view equal everywhere, the five fields bit-identical where the point is in view (elsewhere they are unspecified)"""
    iv = b[0].astype(bool)
    if not np.array_equal(a[0], b[0]):
        return False
    return all(np.array_equal(np.asarray(x)[iv].view(np.uint32), np.asarray(y)[iv].view(np.uint32)) for x, y in zip(a[1:], b[1:]))


def moved_frustum_labels(case, a, b):
    return sorted(l for l, i in case.labels.items() if not same_frustum(tuple(x[i:i + 1] for x in a), tuple(x[i:i + 1] for x in b)))


def level_steps(oracle, lsf, nlevels):
    """step[k] (k = 1 .. nlevels - 1) = the smallest positive float ratio whose PredictScale is >= k, by bisection over oracle.predict_scale"""
    steps = {}
    for k in range(1, nlevels):
        lo, hi = 0x00800000, 0x7F7FFFFF
        lvl = lambda b: int(oracle.predict_scale(np.array([b], np.uint32).view(f32), float(lsf), nlevels)[0])
        assert lvl(hi) >= k
        while lo < hi:
            m = (lo + hi) // 2
            if lvl(m) >= k:
                hi = m
            else:
                lo = m + 1
        steps[k] = np.array([lo], np.uint32).view(f32)[0]
    return steps


def frustum_cases(oracle):
    out = []
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    dn = lambda v: np.nextafter(f32(v), f32(-np.inf))
    tiny = np.finfo(f32).tiny
    IN, OUT = dict(in_view=1), dict(in_view=0)

    c = FrustumCase("zero_and_tiny_depth", "depth", "L8")
    c.add("neg_zero", (0.25, 0, -0.0), **OUT).add("pos_zero", (0.25, 0, 0.0), **OUT).add("pos_zero_left", (-0.25, 0, 0.0), **OUT)
    c.add("tiny", (0, 0, tiny), **OUT).add("neg_tiny", (0, 0, -tiny), **OUT).add("front", (0, 0, 1), in_view=1, u=96.0, v=72.0)
    out.append(c.done())

    # u = 256 * X + 96 at Z = 1: X = +-0.375 lands on 192 / 0; v = 256 * Y + 72: Y = +-0.28125 lands on 144 / 0
    c = FrustumCase("image_edges", "image", "L8")
    c.add("u_min", (-0.375, 0, 1), in_view=1, u=0.0).add("u_max", (0.375, 0, 1), in_view=1, u=192.0)
    c.add("v_min", (0, -0.28125, 1), in_view=1, v=0.0).add("v_max", (0, 0.28125, 1), in_view=1, v=144.0)
    # one ulp of X more gives 192 + 2^-17, which rounds back onto 192 (a tie, to even): two ulps give 192 + 2^-16, the next float
    c.add("u_below", (float(dn(-0.375)), 0, 1), **OUT).add("u_above", (0.375 + 2.0 ** -24, 0, 1), **OUT)
    c.add("v_below", (0, float(dn(-0.28125)), 1), **OUT).add("v_above", (0, 0.28125 + 2.0 ** -24, 1), **OUT)
    c.add("corner", (0.375, 0.28125, 1), in_view=1, u=192.0, v=144.0)
    out.append(c.done())

    c = FrustumCase("distance_edges", "distance", "L8")
    c.add("min_eq", (0, 0, 2), mn=2.0, **IN).add("max_eq", (0, 0, 2), mx=2.0, **IN)
    c.add("min_above", (0, 0, 2), mn=float(up(2)), **OUT).add("max_below", (0, 0, 2), mx=float(dn(2)), **OUT)
    c.add("both_eq", (0, 0, 2), mn=2.0, mx=2.0, **IN).add("inside", (0, 0, 2), **IN)
    out.append(c.done())

    c = FrustumCase("angle_limit_0.5", "angle", "L8", limit=0.5)
    c.add("eq", (0, 0, 2), Pn=(0, 0, 0.5), in_view=1, cos=0.5).add("below", (0, 0, 2), Pn=(0, 0, float(dn(0.5))), **OUT)
    c.add("above", (0, 0, 2), Pn=(0, 0, float(up(0.5))), **IN)
    out.append(c.done())
    c = FrustumCase("angle_limit_0", "angle", "L8", limit=0.0)
    c.add("eq", (0, 0, 2), Pn=(0, 0, 0), in_view=1, cos=0.0).add("below", (0, 0, 2), Pn=(0, 0, -float(tiny)), **OUT)
    c.add("above", (0, 0, 2), Pn=(0, 0, float(tiny)), **IN)
    out.append(c.done())

    for cfg in ("L8", "L12", "P4", "L1"):
        c = FrustumCase("steps_%s" % cfg, "level", cfg)
        nl = c.nlevels
        st = level_steps(oracle, c.lsf, nl)
        for k in range(1, nl):
            c.add("step%d" % k, (0, 0, 1), mf=float(st[k]), in_view=1, level=k)
            c.add("below%d" % k, (0, 0, 1), mf=float(dn(st[k])), in_view=1, level=k - 1)
        c.add("ratio_half", (0, 0, 1), mf=0.5, in_view=1, level=0)
        c.add("ratio_one", (0, 0, 1), mf=1.0, in_view=1, level=0)
        c.add("ratio_huge", (0, 0, 1), mf=1e30, in_view=1, level=nl - 1)
        c.steps = st
        out.append(c.done())

    c = FrustumCase("masked", "mask", "L8")
    c.add("kept", (0, 0, 1), in_view=1).add("masked", (0, 0, 1), cand=0, **OUT).add("masked_edge", (0.375, 0, 1), cand=0, **OUT)
    c.add("kept_edge", (0.375, 0, 1), in_view=1)
    out.append(c.done())

    def grid_points(c, n):
        for i in range(n):                                          # a dyadic lattice, every eighth point outside the image, the masked and the far ones apart
            X, Y, Z = ((i % 16) - 5.5) / 16.0, ((i // 16 % 16) - 7.5) / 32.0, 1.0 + (i % 5) * 0.5
            if i % 8 == 3:
                X += 4.0
            c.add("p%d" % i if i in (0, 1, n - 2, n - 1) else None, (X, Y, Z), Pn=(0, 0, 1), mn=0.5, mx=2.75, mf=1.0 + (i % 11))
        return c.done()
    for n in (1, 255, 256, 257):
        out.append(grid_points(FrustumCase("n_%d" % n, "batch", "L8", mbf=32.0), n))
    ang = 0.3
    Rcw = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], f32)
    tcw = np.array([0.0625, -0.03125, 0.125], f32)
    Ow = (-(Rcw.astype(np.float64).T @ tcw.astype(np.float64))).astype(f32)
    out.append(grid_points(FrustumCase("posed_257", "batch", "L8", mbf=32.0, Rcw=Rcw, tcw=tcw, Ow=Ow), 257))
    return out


# ---- the fused case: Tracking::SearchLocalPoints with projections exactly on maxX / maxY --------------------------------------------------------
def fused_case():
    """-> dict of the arguments shared by oracle.is_in_frustum + oracle.search_by_projection_mappoints and Extractor.search_local_points"""
    rng = np.random.default_rng(5)
    base = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(4)]
    c = FrustumCase("edge_cells", "fused", "L8")
    # MapPoints at Z = 1: on maxX, on maxY, on both, and one in the middle; level 0 (ratio 1), viewCos 1 -> radius 2.5 * th
    for P in ((0.375, 0.0, 1), (0.0, 0.28125, 1), (0.375, 0.28125, 1), (0.0, 0.0, 1)):
        c.add("mp%d" % len(c._rows), P)
    c.done()
    kxy = [(190, 72), (96, 142), (190, 142), (96, 72), (150, 30)]       # keypoints 2 px inside the edges, one unrelated
    keys = make_keys(np.array(kxy, f32), 0)
    desc = np.array([flip(base[0], [1]), flip(base[1], [2, 3]), flip(base[2], []), flip(base[3], [7]), rng.integers(0, 256, 32, dtype=np.uint8)], np.uint8)
    return dict(case=c, keys=keys, desc=desc, mp_desc=np.array(base, np.uint8), th=1.0, expect_match={0: 0, 1: 1, 2: 2, 3: 3, 4: -1})
