"""The loop-closing projection searches restated in numpy (src/ORBmatcher.cc:265-373, :888-1004, :1006-1216 with the cv::Mat arithmetic of
OpenCV 2.4 / 3.2 that include/ygzf.h fixes), on the oracle's GetFeaturesInArea / PredictScale / Hamming distance, and the constructed points that
sit where a wrong form of that arithmetic changes the answer.  Shared by tests/test_loop_cases.py (CPU: the scenes and constructed points do what
they claim) and tests/test_gpu_loop_search.py (the device against this restatement, bit for bit)."""
import math

import numpy as np

from orb_ygz_slam_amd.capi import KP_DTYPE
from orb_ygz_slam_amd.fuse_scene import make_kf

f32 = np.float32
TH_LOW, TH_HIGH = 50, 100
MUTATIONS = ("norm_float", "dot_float", "sim3_world_norm", "no_key_matched")


def norm_cv(v):
    """cv::norm on three floats: double accumulation in index order, double square root, cast to float."""
    s = float(v[0]) * float(v[0])
    s += float(v[1]) * float(v[1])
    s += float(v[2]) * float(v[2])
    return f32(math.sqrt(s))


def norm_float(v):
    """PM_FUSE's (Eigen's) float form."""
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def dot_cv(a, b):
    s = float(a[0]) * float(b[0])
    s += float(a[1]) * float(b[1])
    s += float(a[2]) * float(b[2])
    return s


def dot_float(a, b):
    return float((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])


def _rt(R, t, p):
    return [((R[r, 0] * p[0] + R[r, 1] * p[1]) + R[r, 2] * p[2]) + t[r] for r in range(3)]


def ref_search(oracle, kf, world, normal, maxinv, mininv, mf, desc, th, mode, skip=None, key_matched=None, n_best=1, max_dist=255, R2=None,
               t2=None, mutation=None, trace=None):
    """One keyframe row.  mode: "fuse" (Fuse(pKF, Scw, ..)), "proj" (SearchByProjection(pKF, Scw, ..): key_matched, n_best, max_dist) or "sim3"
    (one direction of SearchBySim3: R2 / t2 chained after kf's Rcw / tcw).  Returns (idx, dist), P x n_best, ascending (dist, list position),
    padded -1 / 256.  mutation: one of MUTATIONS (tests only).  trace: a list that receives, per point, the test that ended it."""
    assert mutation is None or mutation in MUTATIONS
    P = len(world)
    nb = n_best if mode == "proj" else 1
    oi = np.full((P, nb), -1, np.int32)
    od = np.full((P, nb), 256, np.int32)
    R, t, Ow, cam = np.asarray(kf["Rcw"], f32), np.asarray(kf["tcw"], f32), np.asarray(kf["Ow"], f32), kf["cam"]
    fx, fy, cx, cy = f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy)
    minX, minY, maxX, maxY = f32(cam.min_x), f32(cam.min_y), f32(cam.max_x), f32(cam.max_y)
    keys, kdesc, sf = kf["keys"], kf["desc"], kf["scale_factors"]
    if mutation == "no_key_matched":
        key_matched = None

    def note(i, what):
        if trace is not None:
            trace.append((i, what))
    for i in range(P):
        if skip is not None and skip[i]:
            note(i, "skip")
            continue
        p = np.asarray(world[i], f32)
        pc = _rt(R, t, p)
        if mode == "sim3":
            pc = _rt(np.asarray(R2, f32), np.asarray(t2, f32), pc)
        if pc[2] < f32(0):
            note(i, "behind")
            continue
        invz = f32(1) / pc[2]
        x, y = pc[0] * invz, pc[1] * invz
        u, v = fx * x + cx, fy * y + cy
        if not (u >= minX and u < maxX and v >= minY and v < maxY):
            note(i, "image")
            continue
        PO = [p[0] - Ow[0], p[1] - Ow[1], p[2] - Ow[2]]
        vec = pc if (mode == "sim3" and mutation != "sim3_world_norm") else PO
        dist = norm_float(vec) if mutation == "norm_float" else norm_cv(vec)
        if dist < mininv[i] or dist > maxinv[i]:
            note(i, "distance")
            continue
        if mode != "sim3":
            d = dot_float(PO, normal[i]) if mutation == "dot_float" else dot_cv(PO, normal[i])
            if d < 0.5 * float(dist):
                note(i, "view")
                continue
        ratio = mf[i] / dist
        pred = int(oracle.predict_scale(np.array([ratio], f32), float(kf["log_scale_factor"]), kf["nlevels"])[0])
        radius = f32(th) * sf[pred]
        idx = oracle.features_in_area(keys, sf, kf["w"], kf["h"], float(u), float(v), float(radius))
        cands = []
        for pos, j in enumerate(idx):
            if mode == "proj" and key_matched is not None and key_matched[j]:
                continue
            lvl = int(keys[j]["octave"])
            if lvl < pred - 1 or lvl > pred:
                continue
            dd = oracle.hamming(desc[i], kdesc[j])
            if dd <= max_dist and dd < 256:
                cands.append((dd, pos, int(j)))
        cands.sort()
        for k, (dd, pos, j) in enumerate(cands[:nb]):
            oi[i, k], od[i, k] = j, dd
        note(i, ("found", pred) if cands else "none")
    return oi, od


def ref_sim3(oracle, kf1, kf2, pts1, pts2, T, th, th_dist, skip1=None, skip2=None, mutation=None):
    """Both directions of SearchBySim3 and the agreement loop of :1200-1213 -> (nfound, match12, match1, match2)."""
    def direction(target, R, t, Rb, tb, pts, skip):
        row = dict(target, Rcw=R, tcw=t)
        world, mx, mn, mf, desc = pts
        bi, bd = ref_search(oracle, row, world, None, mx, mn, mf, desc, th, "sim3", skip=skip, R2=Rb, t2=tb, mutation=mutation)
        return np.where(bd[:, 0] <= th_dist, bi[:, 0], -1).astype(np.int32)
    m1 = direction(kf2, T["R1w"], T["t1w"], T["sR21"], T["t21"], pts1, skip1)
    m2 = direction(kf1, T["R2w"], T["t2w"], T["sR12"], T["t12"], pts2, skip2)
    m12 = np.full(len(m1), -1, np.int32)
    for i1, idx2 in enumerate(m1):
        if idx2 >= 0 and m2[idx2] == i1:
            m12[i1] = idx2
    return int((m12 >= 0).sum()), m12, m1, m2


# ---- constructed points ----------------------------------------------------------------------------------------------------------------------
# One keyframe at the identity (Ow = 0), one key per point right at its projection.  Each point is built so that ONE wrong form changes whether
# it finds its key (ref_search's `mutation`):
#   norm_max_in / norm_max_out   cv::norm's double form and the float form differ in the last bit and the distance limit is the smaller of
#                                the two: the larger one is beyond it                                                     -> "norm_float"
#   norm_step_in / norm_step_out mfMaxDistance sits where ratio = mf / dist reaches a PredictScale step under one norm only; the key's octave
#                                is inside [level - 1, level] for one of the two levels only                              -> "norm_float"
#   view_in / view_out           PO.Pn against 0.5 * dist decided differently by the double and the float dot               -> "dot_float"
#   masked_best / masked_only    (SearchByProjection) the nearest key is taken in key_matched: the next one / none comes back -> "no_key_matched"
# and for one direction of SearchBySim3 (first transform the identity, second 0.8 * I, (0, 0, 0.1)):
#   sim3_in / sim3_out           the distance limits admit norm(Pc) in the target camera's frame and not norm(P - Ow), and the reverse
#                                                                                                                      -> "sim3_world_norm"
def _step(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf) if k > 0 else f32(-np.inf))
    return x


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.kf = make_kf(self.rng, 752, 480, 8, 8, 1.2, np.eye(3), [0, 0, 0], dup_frac=0.0)
        self.keys, self.kdesc, self.rows = [], [], []

    def project(self, pc):
        cam = self.kf["cam"]
        invz = f32(1) / pc[2]
        return f32(cam.fx) * (pc[0] * invz) + f32(cam.cx), f32(cam.fy) * (pc[1] * invz) + f32(cam.cy)

    def add_key(self, x, y, octave, desc=None):
        k = np.zeros(1, KP_DTYPE)
        k["x"], k["y"], k["octave"], k["size"] = x, y, octave, 31
        self.keys.append(k)
        self.kdesc.append(self.rng.integers(0, 256, 32, dtype=np.uint8) if desc is None else desc)
        return len(self.keys) - 1

    def add_point(self, label, P, normal, mf, maxinv, mininv, desc):
        self.rows.append(dict(label=label, world=np.asarray(P, f32), normal=np.asarray(normal, f32), mf=f32(mf), maxinv=f32(maxinv),
                              mininv=f32(mininv), desc=desc))

    def rand_point(self):
        """A camera-frame point for the next row: rows project 60 px apart (jitter 8 px), further than any search radius here, so that a point
        only ever sees its own keys."""
        r, slot = self.rng, len(self.rows)
        z = f32(r.uniform(2.0, 8.0))
        px, py = -150 + 60 * (slot % 6) + r.uniform(-8, 8), -30 + 60 * (slot // 6) + r.uniform(-8, 8)
        return np.array([f32(px / 458.654) * z, f32(py / 457.296) * z, z], f32)

    def finish(self):
        kf = dict(self.kf)
        kf["keys"] = np.concatenate(self.keys)
        kf["desc"] = np.stack(self.kdesc)
        kf["u_right"] = None
        rows = self.rows
        pts = (np.stack([r["world"] for r in rows]), np.stack([r["normal"] for r in rows]), np.array([r["maxinv"] for r in rows], f32),
               np.array([r["mininv"] for r in rows], f32), np.array([r["mf"] for r in rows], f32), np.stack([r["desc"] for r in rows]))
        return kf, pts, [r["label"] for r in rows]


def constructed_scw(oracle, seed=0):
    """-> kf, pts, labels, key_matched for the Fuse-Scw / Proj-Scw modes."""
    b = _Builder(seed)
    rng = b.rng
    lsf, L = float(b.kf["log_scale_factor"]), b.kf["nlevels"]
    unit = lambda P: (P.astype(np.float64) / np.linalg.norm(P.astype(np.float64))).astype(f32)
    # norm at the distance limit
    want = {"norm_max_in", "norm_max_out"}
    while want:
        P = b.rand_point()
        nd, nf = norm_cv(P), norm_float(P)
        if nd == nf:
            continue
        lab = "norm_max_in" if nd < nf else "norm_max_out"
        if lab not in want:
            continue
        want.discard(lab)
        u, v = b.project(P)
        ki = b.add_key(u, v, 1)
        b.add_point(lab, P, unit(P), f32(min(nd, nf)) * f32(1.1), min(nd, nf), 0.001, b.kdesc[ki])
    # norm at a PredictScale step (the step to level 3, near ratio 1.2^2)
    want = {"norm_step_in", "norm_step_out"}
    while want:
        P = b.rand_point()
        nd, nf = norm_cv(P), norm_float(P)
        if nd == nf:
            continue
        mfs = np.array([_step(f32(1.44) * nd, k) for k in range(-400, 401)], f32)
        pd_ = oracle.predict_scale((mfs / nd).astype(f32), lsf, L).copy()
        pf_ = oracle.predict_scale((mfs / nf).astype(f32), lsf, L).copy()
        hit = np.nonzero(pd_ != pf_)[0]
        if not len(hit):
            continue
        h = hit[0]
        lab = "norm_step_in" if pd_[h] > pf_[h] else "norm_step_out"   # key at the higher of the two levels: inside [level - 1, level] for it only
        if lab not in want or abs(int(pd_[h]) - int(pf_[h])) != 1:
            continue
        want.discard(lab)
        u, v = b.project(P)
        ki = b.add_key(u, v, int(max(pd_[h], pf_[h])))   # the higher level L': under L' - 1 the window [L' - 2, L' - 1] excludes it
        b.add_point(lab, P, unit(P), mfs[h], 1000, 0.001, b.kdesc[ki])
    # the viewing test at its bound
    want = {"view_in", "view_out"}
    while want:
        P = b.rand_point()
        dist = norm_cv(P)
        half = 0.5 * float(dist)
        d = P.astype(np.float64) / np.linalg.norm(P.astype(np.float64))
        perp = np.cross(d, [1.0, 0.0, 0.0]); perp /= np.linalg.norm(perp)
        n0 = (0.5 * d + np.sqrt(0.75) * perp).astype(f32)
        for k in range(-60, 61):
            n = n0.copy()
            n[2] = _step(n[2], k)
            acc_d, acc_f = not (dot_cv(P, n) < half), not (dot_float(P, n) < half)
            if acc_d != acc_f:
                lab = "view_in" if acc_d else "view_out"
                if lab in want:
                    want.discard(lab)
                    u, v = b.project(P)
                    ki = b.add_key(u, v, 1)
                    b.add_point(lab, P, n, dist * f32(1.1), 1000, 0.001, b.kdesc[ki])
                    break
    # key_matched: the nearest key is taken
    for lab in ("masked_best", "masked_only"):
        P = b.rand_point()
        u, v = b.project(P)
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        k0 = b.add_key(u, v, 1, base.copy())
        if lab == "masked_best":
            far = base.copy()
            far[:2] ^= np.uint8(0xFF)
            b.add_key(u + f32(1.5), v, 1, far)
        b.add_point(lab, P, unit(P), norm_cv(P) * f32(1.1), 1000, 0.001, base)
        b.rows[-1]["mask_key"] = k0
    masked = [r["mask_key"] for r in b.rows if "mask_key" in r]
    kf, pts, labels = b.finish()
    km = np.zeros(len(kf["keys"]), np.uint8)
    km[masked] = 1
    return kf, pts, labels, km


SCW_EXPECT = {"norm_max_in": True, "norm_max_out": False, "norm_step_in": True, "norm_step_out": False, "view_in": True, "view_out": False,
              "masked_best": True, "masked_only": False}
SCW_FLIPS = {"norm_float": {"norm_max_in", "norm_max_out", "norm_step_in", "norm_step_out"}, "dot_float": {"view_in", "view_out"},
             "no_key_matched": {"masked_best", "masked_only"}, "sim3_world_norm": set()}   # points whose best key changes


def constructed_sim3(seed=0):
    """-> kf, pts (world, normal, maxinv, mininv, mf, desc), labels, R2, t2 for one Sim3 direction; kf's Rcw / tcw are the identity, Ow = 0."""
    b = _Builder(seed + 100)
    s, tz = f32(0.8), f32(0.1)
    R2 = (s * np.eye(3, dtype=f32)).astype(f32)
    t2 = np.array([0, 0, tz], f32)
    for lab in ("sim3_in", "sim3_out"):
        P = b.rand_point()
        pc = np.array(_rt(R2, t2, P), f32)
        u, v = b.project(pc)
        ki = b.add_key(u, v, 1)
        dc, dw = norm_cv(pc), norm_cv(P)                                 # dc < dw: the scale is 0.8 and the shift small
        assert dc < dw * f32(0.98)
        mid = f32(0.5) * (dc + dw)
        mx, mn = (mid, 0.001) if lab == "sim3_in" else (1000, mid)
        b.add_point(lab, P, [0, 0, 1], dc * f32(1.1) if lab == "sim3_in" else dw * f32(1.1), mx, mn, b.kdesc[ki])
    kf, pts, labels = b.finish()
    return kf, pts, labels, R2, t2


SIM3_EXPECT = {"sim3_in": True, "sim3_out": False}
