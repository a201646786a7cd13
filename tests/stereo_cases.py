"""Constructed inputs for Frame::ComputeStereoMatches (no GPU, no extractor) and a plain numpy / Python restatement of src/Frame.cc:509-682
with mutation switches: descriptor ties, crowded rows, band and bin edges, the inclusive gates met with equality, half-integer rounding, ties and
edges of the 11 SADs, the disparity gates and the median cut at its histogram-bin and float edges -- inputs that keypoints out of the extractor
on rendered pairs never produce.  Shared by tests/test_stereo_cases.py (CPU: the restatement equals the oracle bit for bit, every case is what it
claims, every mutation moves the keypoints its family labels, the oracle equals the reference's own Frame.cc) and tests/test_gpu_stereo_cases.py
(the device equals the oracle bit for bit, twice in a row).

Images.  The left image is seeded noise; the right image is the left one shifted by an integer disparity, so that every left keypoint finds its
texture `disp` pixels to the left at SAD 0, plus a lattice of +8 pixels (one per 11 x 11 window, never a window's centre for the keypoints used
here) that makes the SAD at alignment 8 everywhere: a median of 0 would cut every match.  Cases that need an exact SAD switch the lattice off
and raise single non-centre-row pixels of the right window (set_sad); cases that need ties between the 11 sums paint flat regions with single
marked pixels.  Left keypoints may be duplicated (every left keypoint is independent): that is how lists of more than 1024 SADs come out of a
small frame.  Descriptors are bit-flips of a base at exact Hamming distances.

Configurations.  "L8": 8 levels of 1.2 on 512 x 384 ("L8S": the same on 416 x 312, for two cases between which a context changes size).
"L12": 12 levels of 1.2 on 384 x 288.  The context's geometry accepts every frame whose levels are non-empty (12 levels: from 4 x 4 px), so the
size is set by what the octave-11 cases need: level 11 is 52 x 39 px, which holds an 11 x 11 patch and the 21-column search window with room to
place them, and 288 rows hold the 32-row bands of octave 11 (r = 2 * 1.2^11 = 14.86) at two different offsets inside the 8-row bins.

Every case carries `expect` (label -> what the restatement's trace must say of that left keypoint: the step that ended it, and optionally the
best right index, the winning incR and the SAD), and `undefined`: None, or which of the four situations the reference leaves undefined the case
is in ("left_row", "clipped_band", "empty_list", "right_window_left"); oracle_stereo.cpp states the defined behaviour for them.

deltaR < -1 || deltaR > 1 (:649) cannot trigger and no case is owed for it: the strict scan makes dist1 > dist2 and dist3 >= dist2, so the
denominator 2 (dist1 + dist3 - 2 dist2) is positive and |dist1 - dist3| <= dist1 + dist3 - 2 dist2, that is |deltaR| <= 0.5.
The SAD ceiling: a sum is at most 120 * 510 = 61200 and an accepted one must be strictly below the sum at incR = -5.  _large_sad_case builds
accepted SADs up to 58010 (bin 226 of the 256-wide histogram that k_stereo_cut selects the median with): alone, as a median with SADs either
side, and kept / cut by a median of 27624 / 27623.  2.1 times a median that high is above every SAD there is, so such a median cuts nothing.
uL - 0.01 in double (:661) against uL - 0.01f in float: both subtract from a uL that is a multiple of the result's ulp u = 2^-k, so they round
differently only if an odd multiple of u / 2 lies in [0.01f, 0.01], the tie itself included.  0.01f is m * 2^-30 with m = 10737418 = 2 * 5368709
and 0.01 is (m + 0.24) * 2^-30: for k <= 29 the multiples of u / 2 are multiples of 2^-30 spaced at least 2^-30 apart, none lies strictly inside,
and m * 2^-30 is an odd multiple of u / 2 for k = 28 alone, that is for a result in [2^-5, 2^-4).  A left keypoint whose patch is inside its
level has uL >= 4.5 (k <= 21): no uL a case can use tells the two forms apart, whatever deltaR made the disparity zero, and none is owed.
thDist: 1.5f * 1.4f is 2.0999999 in float and times 10 is the exact tie between 20.999998 and 21, which rounds to even: 21.0 (numpy and the
compiled reference agree).  A threshold computed in double, or exactly (`thdist_double`: SAD < 21 * median / 10 in integers), gives the same
verdict on every integer SAD and is listed under EQUIVALENT, not MUTATIONS: the float product c * median with c = 2.0999999 is never above
2.1 * median after rounding when that is an integer (an integer of this size is a float), and it is below it by less than 1e-6 * median, while
2.1 * median lies at least 0.1 above the next lower integer unless it is one itself: no integer SAD separates the two thresholds."""
import math

import numpy as np

from orb_ygz_slam_amd.capi import KP_DTYPE
from tests.matcher_cases import flip, ham   # noqa: F401 (ham: for whoever checks a case by hand)

f32 = np.float32
TH_HIGH, TH_LOW = 100, 50
CODES = ("ROW_OUT", "NO_CANDIDATE", "MAXU_NEG", "DESC_FAR", "PATCH_OUT", "RIGHT_OUT", "EDGE_INC", "DISP_OUT", "ACCEPT", "ACCEPT_ZERO_DISP", "CUT")
UNDEFINED = ("left_row", "clipped_band", "empty_list", "right_window_left")
MUTATIONS = ("dist_le", "th_orb_le", "band_open", "band_round", "octave_same_only", "octave_any", "u_open", "no_right_centre", "patch_level0",
             "round_half_even", "round_trunc", "sad_le", "edge_inc_kept", "disp_le_max", "disp_zero_refused", "median_lower", "cut_gt",
             "index_15bit")
# wrong forms that no input can tell from the right one (see the module's docstring); the tests hold that they move nothing
EQUIVALENT = ("thdist_double",)
# the case families whose labelled keypoints a mutation must move (and no others of that family's cases)
MUTATION_FAMILY = dict(dist_le="scan", th_orb_le="scan", octave_same_only="scan", octave_any="scan", u_open="scan", index_15bit="index",
                       band_open="band", band_round="band", no_right_centre="sad", patch_level0="sad", round_half_even="sad", round_trunc="sad",
                       sad_le="sad", edge_inc_kept="sad", disp_le_max="disp", disp_zero_refused="disp", median_lower="median", cut_gt="median",
                       thdist_double="median")
# mutation -> case -> the labelled left keypoints whose answer it changes (every other keypoint of the family's cases keeps its answer).  Why:
# dist_le lets the later of two equal distances win; th_orb_le lets 75 through; band_open drops a band's first and last row, band_round turns
# ceil(102.3) = 103 into 102 and the 32-row band into 31 rows; the octave and u gates move what sits on them; no_right_centre changes every SAD
# profile that is not symmetric (all of them; the ballast pairs too); patch_level0 reads level 0 at level-l coordinates; the roundings differ at
# .5 (half even: 100.5 -> 100 but 101.5 -> 102) and at .51 (truncation); sad_le lets the later of two equal sums win; edge_inc_kept keeps +-5;
# the disparity gates move what sits on 0 and on maxD; median_lower reads element (n - 1) / 2 (differs for even n alone); cut_gt keeps SAD == thDist;
# index_15bit loses right indices from 32768 on.
MOVES = {
    "dist_le": {"tie_partner_first": "q", "tie_partner_second": "q", "tie_64_apart": "q"},
    "th_orb_le": {"distance_74_75": "d75"},
    "band_open": {"band_rows_integer_y": "dy0 dy1 dy2", "band_rows_fractional_y": "v0 v1", "band_32_rows_octave_11": "first0 first1 last0 last1"},
    "band_round": {"band_rows_fractional_y": "v1", "band_32_rows_octave_11": "first0 first1 last0 last1"},
    "octave_same_only": {"octave_gate": "oct1 oct3"},
    "octave_any": {"octave_gate": "oct0 oct4"},
    "u_open": {"u_min": "on", "u_max": "on"},
    "no_right_centre": {"brightness_offset": "ballast0 ballast1 p", "upper_octaves": "ballast0 ballast1 o1 o3 o7",
                        "rounding": "ballast0 ballast1 x0 x1 x2 x3 y_half", "sad_ties": "ballast0 ballast1 half tie",
                        "edge_inc": "ballast0 ballast1 inc+4 inc-4", "right_and_level_edges": "endu_cols_1 touch_bottom touch_right touch_top",
                        "right_window_at_10": "ballast0 ballast1 r10", "right_window_off_the_left_edge": "ballast0 ballast1"},
    "patch_level0": {"upper_octaves": "o1 o3"},
    "round_half_even": {"rounding": "x0 y_half"},
    "round_trunc": {"upper_octaves": "o3 o7", "rounding": "x0 x2 x3 y_half"},
    "sad_le": {"sad_ties": "tie"},
    "edge_inc_kept": {"edge_inc": "inc+5 inc-5"},
    "disp_le_max": {"disparity_max": "maxd0"},
    "disp_zero_refused": {"disparity_zero": "zero"},
    "median_lower": {"list_2": "s20", "list_4": "s20", "list_1024": "s41", "list_2500": "s41", "median_alone_in_a_high_bin": "s2000"},
    "cut_gt": {"list_1024": "s42", "list_1025": "s42", "list_2500": "s42", "median_0": "s0 s0_again",
               "thdist_median_10": "s21","thdist_median_20": "s42", "equal_sads_share_the_verdict": "s21 s21_again"},
    "index_15bit": {"n_right_65535": "i32768 i65534"},
}
CONFIGS = dict(L8=(8, 512, 384), L8S=(8, 416, 312), L12=(12, 384, 288))
MB, MBF = 0.5, 32.0          # maxD = 64 exactly


def scale_tables(nlevels):
    """ORBextractor's mvScaleFactor / mvInvScaleFactor (float products and float reciprocals; test_stereo_cases.py checks them against the oracle's)"""
    s = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        s[i] = s[i - 1] * f32(1.2)
    return s, (f32(1) / s).astype(f32)


def c_round(v):
    """round() of <cmath>: half away from zero"""
    v = float(v)
    return f32(math.floor(abs(v) + 0.5) * (1.0 if v >= 0 else -1.0))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def ref_stereo(pyr_l, pyr_r, keys_l, desc_l, keys_r, desc_r, scale, inv_scale, mb, mbf, mutation=None, trace=None):
    """src/Frame.cc:509-682 -> (mvuRight, mvDepth).  Float expressions in np.float32 in source order, SAD in integers, the situations the
    reference leaves undefined as oracle_stereo.cpp defines them.  mutation: one of MUTATIONS (tests only).  trace: a list that receives one dict
    per left keypoint: code (the step that ended it), best (right index), best_dist, inc, sums (the 11 SADs), sad."""
    assert mutation is None or mutation in MUTATIONS or mutation in EQUIVALENT
    mut = mutation
    N, Nr = len(keys_l), len(keys_r)
    u_right, depth = np.full(N, -1, f32), np.full(N, -1, f32)
    th_orb = (TH_HIGH + TH_LOW) // 2
    n_rows = pyr_l[0].shape[0]
    scale, inv_scale = np.asarray(scale, f32), np.asarray(inv_scale, f32)
    desc_l, desc_r = np.asarray(desc_l, np.uint8).reshape(-1, 32), np.asarray(desc_r, np.uint8).reshape(-1, 32)
    # :526-536 the row table (clipped to the image: the reference indexes outside the table there)
    rows = [[] for _ in range(n_rows)]
    if Nr:
        ky = keys_r["y"].astype(f32)
        r = (f32(2.0) * scale[keys_r["octave"]]).astype(f32)
        hi, lo = (ky + r).astype(f32), (ky - r).astype(f32)
        if mut == "band_round":
            maxr, minr = np.floor(hi.astype(np.float64) + 0.5), np.floor(lo.astype(np.float64) + 0.5)
        else:
            maxr, minr = np.ceil(hi), np.floor(lo)
        if mut == "band_open":
            maxr, minr = maxr - 1, minr + 1
        maxr = np.minimum(np.nan_to_num(maxr, nan=-1.0), n_rows - 1).astype(np.int64)
        minr = np.maximum(np.nan_to_num(minr, nan=float(n_rows)), 0).astype(np.int64)
        for i in range(Nr):
            for yi in range(minr[i], maxr[i] + 1):
                rows[yi].append(i)
    rows = [np.array(c, np.int64) for c in rows]
    rx, roct = keys_r["x"].astype(f32), keys_r["octave"].astype(np.int64)
    max_d = f32(mbf) / f32(mb)
    min_d = f32(0)
    accepted = []
    info = [None] * N
    memo = {}

    def one(iL):
        kp = keys_l[iL]
        level, vL, uL = int(kp["octave"]), f32(kp["y"]), f32(kp["x"])
        t = dict(code=None, best=None, best_dist=None, inc=None, sums=None, sad=None)
        if not (vL >= 0 and vL < f32(n_rows)):
            return dict(t, code="ROW_OUT")
        cands = rows[int(vL)]
        if len(cands) == 0:
            return dict(t, code="NO_CANDIDATE")
        min_u, max_u = uL - max_d, uL - min_d
        if max_u < 0:
            return dict(t, code="MAXU_NEG")
        oc, ux = roct[cands], rx[cands]
        if mut == "octave_same_only":
            gate = oc == level
        elif mut == "octave_any":
            gate = np.ones(len(cands), bool)
        else:
            gate = ~((oc < level - 1) | (oc > level + 1))
        gate &= ((ux > min_u) & (ux < max_u)) if mut == "u_open" else ((ux >= min_u) & (ux <= max_u))
        live = cands[gate]
        dist = np.unpackbits(desc_r[live] ^ desc_l[iL][None, :], axis=1).sum(axis=1) if len(live) else np.zeros(0, np.int64)
        best_dist, best = TH_HIGH, 0
        for d, iR in zip(dist.tolist(), live.tolist()):
            if (d <= best_dist) if mut == "dist_le" else (d < best_dist):
                best_dist, best = d, iR
        if mut == "index_15bit":
            best &= 0x7FFF
        t.update(best=best, best_dist=best_dist)
        if not ((best_dist <= th_orb) if mut == "th_orb_le" else (best_dist < th_orb)):
            return dict(t, code="DESC_FAR")
        rnd = {"round_half_even": lambda v: f32(np.rint(v)), "round_trunc": lambda v: f32(int(v))}.get(mut, c_round)
        uR0 = rx[best]
        sf = inv_scale[level]
        su, sv, sr = rnd(uL * sf), rnd(vL * sf), rnd(uR0 * sf)
        w = L = 5
        imL, imR = (pyr_l[0], pyr_r[0]) if mut == "patch_level0" else (pyr_l[level], pyr_r[level])
        cxL, cyL, cxR0 = int(su), int(sv), int(sr)
        if cxL - w < 0 or cyL - w < 0 or cxL + w >= imL.shape[1] or cyL + w >= imL.shape[0] or cyL + w >= imR.shape[0]:
            return dict(t, code="PATCH_OUT")
        IL = imL[cyL - w:cyL + w + 1, cxL - w:cxL + w + 1].astype(np.int64)
        IL = IL - IL[w, w]
        iniu, endu = sr + f32(L) - f32(w), sr + f32(L) + f32(w) + f32(1)
        if iniu < 0 or endu >= imR.shape[1] or cxR0 - L - w < 0:
            return dict(t, code="RIGHT_OUT")
        best_s, best_inc, sums = 2 ** 31 - 1, 0, []
        for inc in range(-L, L + 1):
            cx = cxR0 + inc
            IR = imR[cyL - w:cyL + w + 1, cx - w:cx + w + 1].astype(np.int64)
            if mut != "no_right_centre":
                IR = IR - IR[w, w]
            s = int(np.abs(IL - IR).sum())
            if (s <= best_s) if mut == "sad_le" else (s < best_s):
                best_s, best_inc = s, inc
            sums.append(s)
        t.update(inc=best_inc, sums=sums, sad=best_s)
        if best_inc == -L or best_inc == L:
            if mut != "edge_inc_kept":
                return dict(t, code="EDGE_INC")
        k = L + best_inc
        d1, d2, d3 = f32(sums[max(k - 1, 0)]), f32(sums[k]), f32(sums[min(k + 1, 2 * L)])   # (clamped for edge_inc_kept alone)
        with np.errstate(divide="ignore", invalid="ignore"):
            delta = (d1 - d3) / (f32(2.0) * (d1 + d3 - f32(2.0) * d2))
        if delta < -1 or delta > 1:
            return dict(t, code="DELTA_OUT")         # unreachable without a mutation, see the module's docstring
        best_u = scale[level] * (f32(sr) + f32(best_inc) + delta)
        disparity = uL - best_u
        lower = (disparity > min_d) if mut == "disp_zero_refused" else (disparity >= min_d)
        upper = (disparity <= max_d) if mut == "disp_le_max" else (disparity < max_d)
        if not (lower and upper):
            return dict(t, code="DISP_OUT")
        code = "ACCEPT"
        if disparity <= 0:
            disparity = f32(0.01)
            best_u = f32(np.float64(uL) - 0.01)
            code = "ACCEPT_ZERO_DISP"
        t["u"], t["d"] = best_u, f32(mbf) / disparity
        return dict(t, code=code)

    for iL in range(N):
        key = keys_l[iL].tobytes() + desc_l[iL].tobytes()
        if key not in memo:
            memo[key] = one(iL)
        t = dict(memo[key])
        info[iL] = t
        if t["code"] in ("ACCEPT", "ACCEPT_ZERO_DISP"):
            u_right[iL], depth[iL] = t["u"], t["d"]
            accepted.append((t["sad"], iL))
    if accepted:                                     # (empty: the reference reads element 0 of an empty vector; defined: nothing to cut)
        accepted.sort()
        n = len(accepted)
        median = f32(accepted[(n - 1) // 2 if mut == "median_lower" else n // 2][0])
        th = f32(1.5) * f32(1.4) * median
        for s, iL in reversed(accepted):
            if mut == "thdist_double":
                keep = 10 * s < 21 * int(median)
            else:
                keep = (s <= th) if mut == "cut_gt" else (s < th)
            if keep:
                break
            u_right[iL] = depth[iL] = -1
            info[iL]["code"] = "CUT"
    if trace is not None:
        trace.extend(info)
    return u_right, depth


# ---- models of two of the kernels' shortcuts.  They check the CASES, not the kernels: written from a reading of k_stereo_prep / k_stereo_match /
# k_stereo_cut, they say whether a case's inputs stay inside what those shortcuts assume (bandMax, the clamped bin index, SAD >> 8 below 256);
# the kernels themselves are held by tests/test_gpu_stereo_cases.py alone -------------------------------------------------------------------------
def model_bin_scan(keys_r, scale, n_rows, row):
    """k_stereo_prep / k_stereo_match: right keypoints sorted by the 8-row bin of their clipped band's first row; a left keypoint on `row` reads
    the bins of rows [row - bandMax, row], bandMax = ceil(4 * max scale) + 2 -> (the records it compares, the records whose band covers the row)"""
    band_max, shift = int(math.ceil(4.0 * float(np.max(scale)))) + 2, 3
    n_bins = ((n_rows - 1) >> shift) + 1
    r = (f32(2.0) * np.asarray(scale, f32)[keys_r["octave"]]).astype(f32)
    maxr = np.minimum(np.ceil((keys_r["y"] + r).astype(f32)).astype(np.int64), n_rows - 1)
    minr = np.maximum(np.floor((keys_r["y"] - r).astype(f32)).astype(np.int64), 0)
    covers = (maxr >= minr) & (row >= minr) & (row <= maxr)
    b = np.minimum(np.minimum(minr, n_rows - 1) >> shift, n_bins - 1)
    b0, b1 = max(row - band_max, 0) >> shift, min(row >> shift, n_bins - 1)
    return set(np.nonzero(covers & (b >= b0) & (b <= b1))[0].tolist()), set(np.nonzero(covers)[0].tolist())


def model_histogram_median(sads):
    """k_stereo_cut: element n / 2 of the sorted list by two 256-bin histograms (SAD >> 8, then SAD & 255 inside the selected bin)"""
    a = np.asarray(sads, np.int64)
    hi = np.minimum(a >> 8, 255)

    def select(hist, k):
        acc = 0
        for b in range(256):
            if k < acc + hist[b]:
                return b, k - acc
            acc += hist[b]
    hb, kin = select(np.bincount(hi, minlength=256), len(a) // 2)
    lb, _ = select(np.bincount(a[hi == hb] & 255, minlength=256), kin)
    return (hb << 8) | lb


# ---- building a case ------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, family, cfg, left, right, keys_l, desc_l, keys_r, desc_r, labels, expect, undefined, mb, mbf):
        self.name, self.family, self.cfg, self.left, self.right = name, family, cfg, left, right
        self.keys_l, self.desc_l, self.keys_r, self.desc_r = keys_l, desc_l, keys_r, desc_r
        self.labels, self.expect, self.undefined, self.mb, self.mbf = labels, expect, undefined, mb, mbf
        self.nlevels = CONFIGS[cfg][0]
        self.ref_defined = undefined is None

    def __repr__(self):
        return "%s:%s" % (self.family, self.name)

    def reach(self, trace):
        """None, or what the restatement's trace says otherwise than the case claims"""
        for label, want in self.expect.items():
            t = trace[self.labels[label]]
            for k, v in want.items():
                if k == "past_scan":
                    if t["code"] in ("ROW_OUT", "NO_CANDIDATE", "MAXU_NEG", "DESC_FAR"):
                        return "%s: ended at %s" % (label, t["code"])
                elif t[k] != v:
                    return "%s: %s is %r, not %r" % (label, k, t[k], v)
        return None


def _keys(rows):
    k = np.zeros(len(rows), KP_DTYPE)
    if rows:
        a = np.array(rows, np.float64)
        k["x"], k["y"], k["octave"] = a[:, 0].astype(f32), a[:, 1].astype(f32), a[:, 2].astype(np.int32)
    k["size"], k["angle"], k["response"], k["class_id"] = 31.0, 0.0, 1.0, -1
    return k


class Build:
    """One frame pair under construction.  disp: the right image is the left one shifted `disp` px to the left (right[y, x] = left[y, x + disp]);
    lattice: +8 on one pixel of every 11 x 11 window of the right image (x % 11 == 3 and y % 11 == 3); bright: added to the whole right image;
    smooth: 8 x 8 blocks under the noise, for patches taken on the upper levels."""
    BALLAST = ((443, 345), (443, 367))          # two plain pairs (SAD 8) that keep the accepted list non-empty and its median off 0

    def __init__(self, cfg="L8", seed=1, disp=20, lattice=True, bright=0, smooth=False):
        self.cfg = cfg
        _, w, h = CONFIGS[cfg]
        self.w, self.h, self.disp = w, h, disp
        rng = np.random.default_rng(seed)
        left = rng.integers(40, 216, (h, w)).astype(np.int64)
        if smooth:
            left = (left // 4 + np.kron(rng.integers(30, 160, (h // 8, w // 8)), np.ones((8, 8), np.int64))).astype(np.int64)
        right = rng.integers(40, 216, (h, w)).astype(np.int64)
        if disp >= 0:
            right[:, :w - disp] = left[:, disp:]
        else:
            right[:, -disp:] = left[:, :w + disp]
        if lattice:
            right[3::11, 3::11] += 8
        self.left, self.right = left, right + bright
        self.base = rng.integers(0, 256, 32).astype(np.uint8)
        self.kl, self.dl, self.kr, self.dr, self.labels, self.expect = [], [], [], [], {}, {}

    def near(self, n, lo=0):
        """the base descriptor with bits lo .. lo + n - 1 flipped: Hamming distance n"""
        return flip(self.base, range(lo, lo + n))

    def L(self, x, y, octave=0, desc=None, label=None, **expect):
        self.kl.append((x, y, octave))
        self.dl.append(self.base if desc is None else desc)
        if label is not None:
            self.labels[label] = len(self.kl) - 1
            self.expect[label] = expect
        return len(self.kl) - 1

    def R(self, x, y, octave=0, desc=None):
        self.kr.append((x, y, octave))
        self.dr.append(self.base if desc is None else desc)
        return len(self.kr) - 1

    def pair(self, x, y, octave=0, dist=3, label=None, **expect):
        """a left keypoint and its right partner `disp` px to the left, at Hamming distance `dist` -> (left index, right index)"""
        return self.L(x, y, octave, None, label, **expect), self.R(x - self.disp, y, octave, self.near(dist))

    def set_sad(self, x, y, sad):
        """raise pixels of the right 11 x 11 window around (x, y), none of them on its centre row, by `sad` in all"""
        rem = sad
        for r in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5):
            for c in range(-5, 6):
                if rem <= 0:
                    return
                step = min(rem, 39)
                self.right[y + r, x + c] += step
                rem -= step
        assert rem <= 0

    def flat(self, img, x, y, hw, val=100):
        img[y - 5:y + 6, x - hw:x + hw + 1] = val

    def case(self, name, family, undefined=None, ballast=True, mb=MB, mbf=MBF):
        if ballast:
            assert self.cfg == "L8" and self.disp == 20
            for i, (x, y) in enumerate(self.BALLAST):
                self.L(x, y, 0, flip(self.base, range(128, 256)), label="ballast%d" % i, code="ACCEPT", sad=8)
                self.R(x - 20, y, 0, flip(self.base, range(128, 256)))
        assert self.left.min() >= 0 and self.left.max() <= 255 and self.right.min() >= 0 and self.right.max() <= 255
        return Case(name, family, self.cfg, self.left.astype(np.uint8), self.right.astype(np.uint8), _keys(self.kl),
                    np.array(self.dl, np.uint8).reshape(-1, 32), _keys(self.kr), np.array(self.dr, np.uint8).reshape(-1, 32), self.labels,
                    self.expect, undefined, mb, mbf)


def _scan_cases():
    out = []
    # ---- ties at equal distance: the lower right index wins whatever the storage order (the partner that lines up is stored first / second)
    for name, order in (("tie_partner_first", 0), ("tie_partner_second", 1)):
        b = Build(seed=11)
        b.L(200, 100, label="q", best=0, best_dist=10, code="ACCEPT" if order == 0 else None)
        spots = [(180, 100), (168, 100)]
        for k in (0, 1):
            x, y = spots[k ^ order]
            b.R(x, y, 0, b.near(10, 20 * k))
        if order == 1:
            del b.expect["q"]["code"]
        out.append(b.case(name, "scan"))
    # the same tie with the two 64 positions apart in the candidate list: different lanes' minima
    b = Build(seed=12)
    b.L(200, 100, label="q", best=0, best_dist=10, code="ACCEPT")
    b.R(180, 100, 0, b.near(10))
    for i in range(63):
        b.R(140 + (i % 50), 101, 0, b.near(90, 100))
    b.R(168, 100, 0, b.near(10, 40))
    out.append(b.case("tie_64_apart", "scan"))
    # 1, 63, 64, 65 and 200 candidates on one row, the partner last (every filler replaces the initial best: 90 < 100)
    for n in (1, 63, 64, 65, 200):
        b = Build(seed=13)
        b.L(200, 100, label="q", best=n - 1, best_dist=5, code="ACCEPT")
        for i in range(n - 1):
            b.R(137 + (i % 60), 99 + (i % 3), 0, b.near(90, 100))
        b.R(180, 100, 0, b.near(5))
        out.append(b.case("candidates_%d" % n, "scan"))
    # best distance 74 against 75
    b = Build(seed=14)
    b.pair(200, 100, dist=74, label="d74", best_dist=74, code="ACCEPT")
    b.pair(200, 140, dist=75, label="d75", best_dist=75, code="DESC_FAR")
    out.append(b.case("distance_74_75", "scan"))
    # the octave gate: levelL - 1 and levelL + 1 compared, +-2 not
    b = Build(seed=15, smooth=True)
    for i, (o, ok) in enumerate(((1, True), (3, True), (0, False), (4, False))):
        y = 60 + 40 * i
        b.L(200, y, 2, label="oct%d" % o, **(dict(past_scan=True, best_dist=3) if ok else dict(code="DESC_FAR", best_dist=100)))
        b.R(180, y, o, b.near(3))
    out.append(b.case("octave_gate", "scan"))
    # uR == minU and uR == maxU are compared, one float step outside is not.  minU: a flat region with marked pixels that give deltaR = 0.5
    # (as in sad_ties), so that the disparity is 63.5 and not maxD = 64; maxU: the right image is the left one, the disparity is -deltaR
    b = Build(seed=16)
    for y in (100, 140):
        b.flat(b.left, 200, y, 8)
        b.flat(b.right, 136, y, 13)
        b.left[y - 3, 200] = b.right[y - 3, 136] = b.right[y - 3, 137] = 110
    b.L(200, 100, label="on", code="ACCEPT", best_dist=3, inc=0, sad=10)
    b.R(136.0, 100, 0, b.near(3))
    b.L(200, 140, label="off", code="DESC_FAR", best_dist=100)
    b.R(np.nextafter(f32(136), f32(0)), 140, 0, b.near(3))
    out.append(b.case("u_min", "scan"))
    b = Build(seed=16, disp=0)
    b.L(200, 100, label="on", past_scan=True, best_dist=3)
    b.R(200.0, 100, 0, b.near(3))
    b.L(200, 140, label="off", code="DESC_FAR", best_dist=100)
    b.R(np.nextafter(f32(200), f32(1e9)), 140, 0, b.near(3))
    b2 = Build(seed=16)                          # the ballast pairs need the plain 20 px shift: that corner comes from a plain pair
    for img, src in ((b.left, b2.left), (b.right, b2.right)):
        img[330:, 400:] = src[330:, 400:]
    b.disp = 20
    out.append(b.case("u_max", "scan"))
    # 1, 3, 4 and 5 left keypoints (a workgroup holds four)
    for n in (1, 3, 4, 5):
        b = Build("L8S" if n in (3, 5) else "L8", seed=17)          # (and the frame size alternates: a context goes through its geometry change)
        for i in range(n):
            b.pair(120 + 50 * i, 80 + 30 * i, label="p%d" % i, code="ACCEPT", best=i)
        out.append(b.case("n_left_%d" % n, "scan", ballast=False))
    return out


def _index_cases():
    """65535 right keypoints on three rows (one bin holds them all), the partners at indices 0, 32767, 32768 and 65534: every bit of the key's index"""
    b = Build(seed=21)
    spots = {0: 100, 32767: 200, 32768: 300, 65534: 400}
    far = flip(b.base, range(128, 256))
    n = 65535
    kr = _keys([(0, 0, 0)] * n)
    i = np.arange(n)
    kr["x"], kr["y"] = (40 + (i % 400)).astype(f32), (99 + (i % 3)).astype(f32)
    dr = np.tile(far, (n, 1))
    for k, (idx, x) in enumerate(spots.items()):
        d = flip(b.base, range(8 * k, 8 * k + 4))                # four bases 8 bits apart: each partner is 3 from its own, 11 from the others
        b.L(x, 100, 0, d, label="i%d" % idx, best=idx, best_dist=3, code="ACCEPT")
        kr["x"][idx], kr["y"][idx] = x - 20, 100
        dr[idx] = flip(d, range(200, 203))
    c = b.case("n_right_65535", "index", ballast=False)
    c.keys_r, c.desc_r = kr, dr
    return [c]


def _band_cases():
    out = []
    # right y = 100: rows 98 .. 102.  first row, last row, one row outside each, and vL just below an integer
    b = Build(seed=31)
    for i, (dy, code) in enumerate(((-2.0, "ACCEPT"), (2.0, "ACCEPT"), (2.9, "ACCEPT"), (-3.0, "NO_CANDIDATE"), (3.0, "NO_CANDIDATE"),
                                    (float(np.nextafter(f32(98), f32(0))) - 100.0, "NO_CANDIDATE"))):
        x = 80 + 60 * i
        b.L(x, f32(100 + dy), label="dy%d" % i, code=code)
        b.R(x - 20, 100, 0, b.near(3))
    b.L(-3.0, 100.0, label="maxu", code="MAXU_NEG")     # a row with candidates, maxU = uL < 0 (:559)
    out.append(b.case("band_rows_integer_y", "band"))
    # right y = 100.3: floor(98.3) = 98, ceil(102.3) = 103 (rounding would give 98 .. 102)
    b = Build(seed=32)
    for i, (vl, code) in enumerate(((98.0, "ACCEPT"), (103.9, "ACCEPT"), (97.99, "NO_CANDIDATE"), (104.0, "NO_CANDIDATE"))):
        x = 80 + 60 * i
        b.L(x, f32(vl), label="v%d" % i, code=code)
        b.R(x - 20, f32(100.3), 0, b.near(3))
    out.append(b.case("band_rows_fractional_y", "band"))
    # left keypoints on row 0 and on the last row, bands that end exactly there (right y = 2 and nRows - 3): compared, too far
    b = Build(seed=33)
    b.L(200, 0.5, label="row0", code="DESC_FAR", best_dist=80)
    b.R(180, 2.0, 0, b.near(80))
    b.L(200, 383.5, label="rowlast", code="DESC_FAR", best_dist=80)
    b.R(180, 381.0, 0, b.near(80))
    out.append(b.case("left_on_first_and_last_row", "band"))
    # bands clipped at row 0 and at nRows - 1: the partner is found, the patch leaves the level
    b = Build(seed=34)
    b.L(200, 0.0, label="top", code="PATCH_OUT", best_dist=3)
    b.R(180, 1.0, 0, b.near(3))
    b.L(200, 383.0, label="bottom", code="PATCH_OUT", best_dist=3)
    b.R(180, 382.5, 0, b.near(3))
    out.append(b.case("band_clipped", "band", undefined="clipped_band"))
    # empty bands: right y outside the image
    b = Build(seed=35)
    b.L(200, 1.0, label="a", code="NO_CANDIDATE")
    b.R(180, -10.0, 0, b.near(3))
    b.L(200, 382.0, label="b", code="NO_CANDIDATE")
    b.R(180, 394.0, 0, b.near(3))
    out.append(b.case("band_empty", "band", undefined="clipped_band"))
    # left y negative and >= nRows
    b = Build(seed=36)
    b.L(200, -0.5, label="neg", code="ROW_OUT")
    b.L(200, 384.0, label="past", code="ROW_OUT")
    b.R(180, 1.0, 0, b.near(3))
    out.append(b.case("left_row_outside", "band", undefined="left_row"))
    # 12 levels: an octave-11 right keypoint on y + 0.5 has the 32-row band [y - 15, y + 16]; the left keypoint on its last row, 31 rows below
    # the band's first row, with that first row first (y - 15 = 48) and last (y - 15 = 167) in its 8-row bin; and one row further: no candidate.
    # The accepted SADs are those of level-10 and level-11 patches (hundreds): no level-0 pair is added, whose SAD of 8 would cut them all
    b = Build("L12", seed=37, smooth=True)
    for i, y in enumerate((63, 182)):
        x = 150 + 100 * i
        assert (y - 15) % 8 == (0, 7)[i]
        b.R(x - 20, y + 0.5, 11, flip(b.base, range(10 * i, 10 * i + 3)))
        b.L(x, y + 16, 11, label="last%d" % i, past_scan=True, best=i, best_dist=3)
        b.L(x, y + 17, 11, label="past%d" % i, code="NO_CANDIDATE")
        b.L(x, y - 15, 10, label="first%d" % i, past_scan=True, best=i, best_dist=3)
        b.L(x, y - 16, 10, label="before%d" % i, code="NO_CANDIDATE")
    out.append(b.case("band_32_rows_octave_11", "band", ballast=False))
    return out


def _sad_cases():
    out = []
    # a brightness offset between the eyes: the centre subtraction cancels it
    b = Build(seed=41, bright=25)
    b.pair(200, 100, label="p", code="ACCEPT", sad=8, inc=0)
    out.append(b.case("brightness_offset", "sad"))
    # octaves 1, 3 and the top one: the patch is taken on the keypoint's level
    b = Build(seed=42, smooth=True)
    for i, o in enumerate((1, 3, 7)):
        b.pair(150 + 80 * i, 90 + 60 * i, o, label="o%d" % o, past_scan=True)
    out.append(b.case("upper_octaves", "sad"))
    # half-integer x * invScale at level 0 (round half away from zero), .49 and .51; the right partner on an integer column
    b = Build(seed=43)
    for i, (x, inc) in enumerate(((100.5, 1), (100.49, 0), (100.51, 1), (101.5, 2))):
        b.L(f32(x), 60 + 40 * i, label="x%d" % i, code="ACCEPT", inc=inc, sad=8)
        b.R(80.0, 60 + 40 * i, 0, b.near(3))
    b.L(200.0, 100.5, label="y_half", code="ACCEPT", inc=0)         # row 101's texture against row 101: the rows of both eyes follow scaledvL
    b.R(180.0, 100.0, 0, b.near(3))
    out.append(b.case("rounding", "sad"))
    # flat regions with marked pixels: a tie between incR = 0 and 3 (the first wins); dist2 == dist3 (deltaR = 0.5)
    b = Build(seed=44)
    for i, (label, second, inc) in enumerate((("tie", 3, 0), ("half", 1, 0))):
        x, y = 200, 80 + 60 * i
        b.flat(b.left, x, y, 8)
        b.flat(b.right, x - 20, y, 13)
        b.left[y - 3, x] = 110                           # on the centre column: inside the window at every incR, three rows off the centre
        b.right[y - 3, x - 20] = 110
        b.right[y - 3, x - 20 + second] = 110            # sums: 10 at incR = 0 and at incR = second, 20 or 30 elsewhere
        b.pair(x, y, label=label, code="ACCEPT", inc=inc, sad=10)
    out.append(b.case("sad_ties", "sad"))
    # best at incR = -5 and +5 refused, -4 and +4 kept
    b = Build(seed=45)
    for i, (off, code) in enumerate(((5, "EDGE_INC"), (4, "ACCEPT"), (-4, "ACCEPT"), (-5, "EDGE_INC"))):
        b.L(200, 60 + 40 * i, label="inc%+d" % -off, code=code, inc=-off)
        b.R(180 + off, 60 + 40 * i, 0, b.near(3))
    out.append(b.case("edge_inc", "sad"))
    # the right window against the level's right edge: endu == cols refused, cols - 1 kept; a left patch touching the right, top and bottom border
    b = Build(seed=46, disp=4)
    b.L(505, 100, label="endu_cols", code="RIGHT_OUT")
    b.R(501, 100, 0, b.near(3))
    b.L(504, 140, label="endu_cols_1", code="ACCEPT", inc=0)
    b.R(500, 140, 0, b.near(3))
    b.L(506, 180, label="touch_right", code="ACCEPT", inc=0)
    b.R(500, 180, 0, b.near(3))                       # (the window at 500 finds the texture of 506 - 4 = 502 at incR = 2)
    b.expect["touch_right"]["inc"] = 2
    b.L(200, 5, label="touch_top", code="ACCEPT", inc=0)
    b.R(196, 5, 0, b.near(3))
    b.L(200, 378, label="touch_bottom", code="ACCEPT", inc=0)
    b.R(196, 378, 0, b.near(3))
    out.append(b.case("right_and_level_edges", "sad", ballast=False))
    # scaleduR0 of 10 is the first column whose window is inside
    b = Build(seed=47)
    b.L(30, 100, label="r10", code="ACCEPT", inc=0)
    b.R(10, 100, 0, b.near(3))
    out.append(b.case("right_window_at_10", "sad"))
    b = Build(seed=47)
    b.L(29, 100, label="r9", code="RIGHT_OUT")
    b.R(9, 100, 0, b.near(3))
    b.L(5, 140, label="touch_left", code="RIGHT_OUT")
    b.R(5, 140, 0, b.near(3))
    out.append(b.case("right_window_off_the_left_edge", "sad", undefined="right_window_left"))
    return out


def _disp_cases():
    out = []

    def symmetric(b, xl, xr, y):
        """the same texture, symmetric about its centre column, around (xl, y) of the left and (xr, y) of the right image: deltaR == 0"""
        rng = np.random.default_rng(5)
        half = rng.integers(40, 216, (11, 14))
        tex = np.concatenate([half[:, :0:-1], half], axis=1)         # 27 columns, symmetric about column 13
        b.left[y - 5:y + 6, xl - 13:xl + 14] = tex
        b.right[y - 5:y + 6, xr - 13:xr + 14] = tex
    # disparity exactly 0: the 0.01 branch (uL - 0.01 in double)
    b = Build(seed=51)
    symmetric(b, 200, 200, 100)
    b.L(200, 100, label="zero", code="ACCEPT_ZERO_DISP", inc=0, sad=0)
    b.R(200, 100, 0, b.near(3))
    out.append(b.case("disparity_zero", "disp"))
    # disparity at maxD refused, one float step below kept
    b = Build(seed=52)
    for i, (ul, code) in enumerate(((200.0, "DISP_OUT"), (float(np.nextafter(f32(200), f32(0))), "ACCEPT"))):
        y = 100 + 60 * i
        symmetric(b, 200, 136, y)
        b.L(f32(ul), y, label="maxd%d" % i, code=code, inc=0, sad=0)
        b.R(136, y, 0, b.near(3))
    out.append(b.case("disparity_max", "disp"))
    # the texture lies to the right of the left keypoint (found at incR = +3): negative disparity is refused
    b = Build(seed=53, disp=-3)
    b.L(200, 100, label="neg", code="DISP_OUT", inc=3)
    b.R(200, 100, 0, b.near(3))
    b2 = Build(seed=53)
    for img, src in ((b.left, b2.left), (b.right, b2.right)):
        img[330:, 400:] = src[330:, 400:]
    b.disp = 20
    out.append(b.case("disparity_negative", "disp"))
    return out


def _median_case(name, sads, expect_cut, undefined=None):
    """accepted matches with exactly these SADs (one spot per distinct value, the left keypoint repeated); expect_cut: the SAD values that are cut"""
    b = Build(seed=61, lattice=False)
    values = sorted(set(sads))
    assert len(values) <= 40
    spot = {}
    for k, s in enumerate(values):
        x, y = 80 + 48 * (k % 8), 30 + 24 * (k // 8)
        b.set_sad(x - 20, y, s)
        spot[s] = (x, y, b.R(x - 20, y, 0, b.near(3)))
    seen = {}
    for s in sads:
        x, y, _ = spot[s]
        n = seen.get(s, 0)
        seen[s] = n + 1
        kw = dict(label="s%d" % s, code="CUT" if s in expect_cut else "ACCEPT", sad=s) if n == 0 else {}
        b.L(x, y, **kw)
    if sads and max(seen.values()) > 1:                 # the last copy of a repeated value gets the verdict of the first: the cut is on the value alone
        s = max(seen, key=lambda v: (seen[v] > 1, v))
        b.labels["s%d_again" % s] = max(i for i, k in enumerate(b.kl) if k[:2] == spot[s][:2])
        b.expect["s%d_again" % s] = dict(b.expect["s%d" % s])
    return b.case(name, "median", undefined=undefined, ballast=False)


def _large_sad_case(name, sads, expect_cut):
    """accepted matches with SADs of tens of thousands, one spot per value.  The left window is `a` with a centre of 0 (centred: a on 120 pixels),
    the right rows are 0 with the centre row at `c` over the 21 columns a window's centre visits (centred: -c on the 110 pixels off that row, 0
    on it): every one of the 11 sums is 120 a + 110 c.  Two right pixels of 20 three rows up, on the columns -5 and +5, are both inside the window
    at incR = 0 alone (-40 there, -20 elsewhere: a strict minimum with dist1 == dist3, deltaR = 0), and pixels on the centre column, which every
    window holds, take the remainder `t` off all 11 sums.  a = 250, c = 255, t = 0 gives 58010, the largest SAD of this construction."""
    b = Build(seed=63, lattice=False)
    for k, s in enumerate(sads):
        x, y = 120 + 150 * (k % 3), 60 + 60 * (k // 3)
        a = min(250, (s + 40 + 229) // 230)
        c = min(255, -((120 * a - s - 40) // 110))
        t = 120 * a + 110 * c - 40 - s
        assert 20 <= a + c and 0 <= c and 0 <= t <= 9 * min(255, a + c), (s, a, c, t)
        b.left[y - 5:y + 6, x - 5:x + 6] = a
        b.left[y, x] = 0
        b.right[y - 5:y + 6, x - 30:x - 9] = 0
        b.right[y, x - 30:x - 9] = c
        b.right[y - 3, x - 25] = b.right[y - 3, x - 15] = 20
        for r in (-5, -4, -2, -1, 1, 2, 3, 4, 5):
            step = min(t, 255, a + c)
            b.right[y + r, x - 20] = step
            t -= step
        b.pair(x, y, label="s%d" % s, code="CUT" if s in expect_cut else "ACCEPT", sad=s, inc=0, sums=[s + 20] * 5 + [s] + [s + 20] * 5)
    return b.case(name, "median", ballast=False)


def _median_cases():
    th10, th20 = f32(1.5) * f32(1.4) * f32(10), f32(1.5) * f32(1.4) * f32(20)
    f10, f20 = int(math.floor(th10)), int(math.floor(th20))
    # the SAD whose thDist is the first above 58010, and the one before it (27624 and 27623: bin 107 against bin 226)
    m_keep = next(m for m in range(27000, 28000) if f32(58010) < f32(1.5) * f32(1.4) * f32(m))
    assert m_keep == 27624 and not f32(58010) < f32(1.5) * f32(1.4) * f32(m_keep - 1)
    out = [
        _median_case("list_1", [5], ()),
        _median_case("list_2", [5, 20], ()),
        _median_case("list_3", [5, 9, 30], (30,)),
        _median_case("list_4", [5, 9, 20, 50], (50,)),
        _median_case("list_1024", [10] * 512 + [20] * 510 + [41, 42], (42,)),
        _median_case("list_1025", [10] * 512 + [20] * 511 + [41, 42], (42,)),
        _median_case("list_2500", [10] * 1250 + [20] * 1248 + [41, 42], (42,)),
        _median_case("median_0", [0, 0, 0, 5], (0, 5)),
        _median_case("median_256_not_255", [255] * 2 + [256] * 3 + [537, 538], (538,)),
        _median_case("median_255_not_256", [255] * 5 + [256] * 2 + [535, 536], (536,)),
        _median_case("median_512_not_511", [511] * 2 + [512] * 3 + [1075, 1076], (1076,)),
        _median_case("median_511_not_512", [511] * 5 + [512] * 2 + [1073, 1074], (1074,)),
        _median_case("median_alone_in_a_high_bin", [10, 2000], ()),
        _median_case("large_sads", [2900, 3000, 3000], ()),
        # near the ceiling (bin 226 of the 256-wide histogram): alone; as the median with SADs either side of it (2.1 * 57990 is above every
        # SAD there is, so nothing is cut); and either side of the thDist of a median in bin 107
        _large_sad_case("sad_near_ceiling_alone", [58010], ()),
        _large_sad_case("sad_near_ceiling_median", [20000, 57990, 58010], ()),
        _large_sad_case("sad_near_ceiling_kept", [m_keep, m_keep, 58010], ()),
        _large_sad_case("sad_near_ceiling_cut", [m_keep - 1, m_keep - 1, 58010], (58010,)),
        _median_case("thdist_median_10", [10, 10, 10, 10, f10 - 1, f10, f10 + 1], (f10, f10 + 1)),
        _median_case("thdist_median_20", [20, 20, 20, 20, f20 - 1, f20, f20 + 1], (f20, f20 + 1)),
        _median_case("equal_sads_share_the_verdict", [10, 10, 10, 10, 10, 21, 21, 20, 20], (21,)),
    ]
    assert (f10, f20) == (21, 42)
    # no accepted match at all
    b = Build(seed=62)
    b.pair(200, 100, dist=80, label="far", code="DESC_FAR")
    out.append(b.case("nothing_accepted", "median", undefined="empty_list", ballast=False))
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _scan_cases() + _index_cases() + _band_cases() + _sad_cases() + _disp_cases() + _median_cases()
        names = [repr(c) for c in _CASES]
        assert len(set(names)) == len(names)
    return _CASES


# ---- running a case -----------------------------------------------------------------------------------------------------------------------
_PYR = {}


def pyramids(O, c):
    """both eyes' pyramids from the oracle's extractor (the resize is pinned elsewhere), computed once per case"""
    if repr(c) not in _PYR:
        ex = O.Extractor(1000, 1.2, c.nlevels, 20, 7)
        _PYR[repr(c)] = (ex.pyramid(c.left), ex.pyramid(c.right))
    return _PYR[repr(c)]


def run_restatement(O, c, mutation=None, trace=None):
    pl, pr = pyramids(O, c)
    s, inv = scale_tables(c.nlevels)
    return ref_stereo(pl, pr, c.keys_l, c.desc_l, c.keys_r, c.desc_r, s, inv, c.mb, c.mbf, mutation, trace)


def run_oracle(O, c):
    return O.Extractor(1000, 1.2, c.nlevels, 20, 7).compute_stereo_matches(c.left, c.right, c.keys_l, c.desc_l, c.keys_r, c.desc_r, c.mb, c.mbf)


def run_device(ex, c):
    return ex.compute_stereo_matches(c.left, c.right, c.keys_l, c.desc_l, c.keys_r, c.desc_r, c.mb, c.mbf)


def same(a, b):
    return np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
