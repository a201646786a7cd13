"""The per-pair body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:1060-1194, KeyFrame::UnprojectStereo src/KeyFrame.cc:815-828)
restated in numpy, its plausible wrong forms behind a switch each, and constructed cases with a reach predicate each.  No device and no library:
tests/test_tri_cases.py holds the cases to their claims, tests/test_tri_host_progs.py runs csrc/tri_math.h as a host program against this
module, tests/test_gpu_tri.py runs the cases through ygzf_triangulate_pairs, bit for bit.

Every operation below is one numpy scalar operation on float32 (the two chi-square gates and the 0.9998 gate: one product / comparison on
float64, as the source's double literals make them), in the order csrc/tri_math.h writes them; both are correctly rounded, so they agree in
every bit.  What the header's comment fixes is fixed here the same way: distorted keys, KF1's mbf in KF2's right-eye term, 3-term sums left to
right, Twc * x through the quaternion, cos_stereo as a per-feature input, and Eigen::JacobiSVD<Matrix4f> as Eigen 3.3's two-sided Jacobi
(`jacobi_svd4`), whose parity with a compiled Eigen is unpinned.  The one deviation is the sweep cap MAX_SWEEPS, read from
the header.

Two kinds of cases:
    pair cases   (kf1, kf2, idx1, idx2): go through `tri_pair`, the host program and the GPU
    svd cases    a 4 x 4 matrix alone: go through `jacobi_svd4` and the host program (no pair of cameras gives a diagonal A, and the stop rule's
                 threshold is best shown on a matrix written down directly)
"""
import collections
import os
import re

import numpy as np

f32, f64 = np.float32, np.float64
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

_HERE = os.path.dirname(os.path.abspath(__file__))
_HEADER = os.path.join(os.path.dirname(_HERE), "orb_ygz_slam_amd", "csrc", "tri_math.h")
MAX_SWEEPS = int(re.search(r"^#define YGZF_TRI_MAX_SWEEPS (\d+)", open(_HEADER).read(), re.M).group(1))

ACCEPTED, LOW_PARALLAX, V33_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE_RATIO, SWEEP_CAP = range(10)
FROM_NONE, FROM_SVD, FROM_KF1, FROM_KF2 = range(4)
FLT_MIN, FLT_EPS = f32(np.finfo(f32).tiny), f32(np.finfo(f32).eps)

# one per rule a kernel could get wrong
WRONG_FORMS = ("chi2_mono1_ge", "chi2_stereo1_ge", "chi2_mono2_ge", "chi2_stereo2_ge", "kf2_own_mbf", "z1_lt", "z2_lt", "elseif_if", "min_dropped",
               "mono_gate_on_stereo", "v33_ignored", "ratio_abs", "undistorted_keys", "sort_ascending", "threshold_no_maxdiag")
# "the drop rule off" belongs to the replay (host/TriangulateApply.h, tests/cpp/tri_apply_cpu.cc), not to a pair

# The least relative distance (absolute where the bound is 0) a constructed pair case keeps from every gate it does not aim at.  A different
# but legitimate order of the fp32 roundings moves a compared quantity by a few units of 2^-24 = 6e-8 times the operation count (some tens):
# 1e-3 is three orders of magnitude beyond that, so a case decides what it claims to decide and nothing else.
MARGIN_MIN = 1.0e-3


# ---- the fixed JacobiSVD ----------------------------------------------------------------------------------------------------------------------------
def _maxf(a, b):
    return b if a < b else a


def _svd_step(W, V, p, q, maxDiag, wrong):
    """one (p, q) step; -> (maxDiag, rotated)"""
    threshold = FLT_MIN if wrong == "threshold_no_maxdiag" else _maxf(FLT_MIN, (f32(2) * FLT_EPS) * maxDiag)
    if not (abs(W[p][q]) > threshold or abs(W[q][p]) > threshold):
        return maxDiag, False
    m00, m01, m10, m11 = W[p][p], W[p][q], W[q][p], W[q][q]
    t, d = m00 + m11, m10 - m01
    if abs(d) < FLT_MIN:
        s1, c1 = f32(0), f32(1)
    else:
        u = t / d
        tmp = np.sqrt(f32(1) + u * u)
        s1, c1 = f32(1) / tmp, u / tmp
    if not (c1 == 1 and s1 == 0):
        a00, a10 = c1 * m00 + s1 * m10, -s1 * m00 + c1 * m10
        a01, a11 = c1 * m01 + s1 * m11, -s1 * m01 + c1 * m11
        m00, m10, m01, m11 = a00, a10, a01, a11
    deno = f32(2) * abs(m01)
    if deno < FLT_MIN:
        cr, sr = f32(1), f32(0)
    else:
        tau = (m00 - m11) / deno
        w = np.sqrt(tau * tau + f32(1))
        tt = f32(1) / (tau + w) if tau > 0 else f32(1) / (tau - w)
        sign_t = f32(1) if tt > 0 else f32(-1)
        n = f32(1) / np.sqrt(tt * tt + f32(1))
        sr = -sign_t * (m01 / abs(m01)) * abs(tt) * n
        cr = n
    nsr = -sr
    cl, sl = c1 * cr - s1 * nsr, c1 * nsr + s1 * cr
    if not (cl == 1 and sl == 0):
        for i in range(4):
            x, y = W[p][i], W[q][i]
            W[p][i] = cl * x + sl * y
            W[q][i] = -sl * x + cl * y
    if not (cr == 1 and nsr == 0):
        for M in (W, V):
            for i in range(4):
                x, y = M[i][p], M[i][q]
                M[i][p] = cr * x + nsr * y
                M[i][q] = -nsr * x + cr * y
    return _maxf(maxDiag, _maxf(abs(W[p][p]), abs(W[q][q]))), True


Svd = collections.namedtuple("Svd", "V sv sweeps")
_STEPS = ((1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2))


def jacobi_svd4(A, wrong=None, max_sweeps=None):
    """-> Svd(V 4 x 4 float32 (columns: right singular vectors), sv descending, the rotating sweeps used; == the cap: V / sv are not to be used)"""
    cap = MAX_SWEEPS if max_sweeps is None else max_sweeps
    with np.errstate(all="ignore"):
        A = [[f32(A[r][c]) for c in range(4)] for r in range(4)]
        scale = abs(A[0][0])
        for r in range(4):
            for c in range(4):
                if abs(A[r][c]) > scale:
                    scale = abs(A[r][c])
        if scale == 0:
            scale = f32(1)
        W = [[A[r][c] / scale for c in range(4)] for r in range(4)]
        V = [[f32(1 if r == c else 0) for c in range(4)] for r in range(4)]
        maxDiag = abs(W[0][0])
        for i in range(1, 4):
            if abs(W[i][i]) > maxDiag:
                maxDiag = abs(W[i][i])
        sweeps = 0
        for _ in range(cap):
            rotated = False
            for p, q in _STEPS:
                maxDiag, r = _svd_step(W, V, p, q, maxDiag, wrong)
                rotated = rotated or r
            if not rotated:
                break
            sweeps += 1
        sv = [abs(W[i][i]) * scale for i in range(4)]
        for i in range(3):
            best, pos = sv[i], i
            for j in range(i + 1, 4):
                if (sv[j] < best) if wrong == "sort_ascending" else (sv[j] > best):
                    best, pos = sv[j], j
            if pos != i:
                sv[i], sv[pos] = sv[pos], sv[i]
                for r in range(4):
                    V[r][i], V[r][pos] = V[r][pos], V[r][i]
    return Svd(np.array(V, f32), np.array(sv, f32), sweeps)


# ---- one pair -------------------------------------------------------------------------------------------------------------------------------------------
Feat = collections.namedtuple("Feat", "x y uR depth cosStereo sigma2 scale")
Pair = collections.namedtuple("Pair", "x3d status source sweeps cos_rays margins A")


def feature(kf, idx, wrong=None):
    kp = (kf["keys_un"] if wrong == "undistorted_keys" and kf.get("keys_un") is not None else kf["keys"])[idx]
    uR = f32(-1) if kf.get("u_right") is None else f32(kf["u_right"][idx])
    stereo = uR >= 0
    o = int(kf["keys"][idx]["octave"])
    return Feat(f32(kp["x"]), f32(kp["y"]), uR, f32(kf["depth"][idx]) if stereo else f32(-1), f32(kf["cos_stereo"][idx]) if stereo else f32(0),
                f32(kf["level_sigma2"][o]), f32(kf["scale_factors"][o]))


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _unproject(K, f):
    z = f.depth
    if not z > 0:
        return [f32(0), f32(0), f32(0)]
    v = [(f.x - K["cx"]) * z * K["invfx"], (f.y - K["cy"]) * z * K["invfy"], z]
    q = K["Twc_q"]
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    c = [q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]]
    return [((v[i] + q[3] * uv[i]) + c[i]) + K["Twc_t"][i] for i in range(3)]


def _rel(a, b):
    """the distance of a from the bound b, relative to the bound (absolute where it is 0)"""
    a, b = f64(a), f64(b)
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def _reprojects(K, f, mbf, X, z, which, wrong, margins):
    R, t = K["Rcw"], K["tcw"]
    x = _dot(R[0:3], X) + t[0]
    y = _dot(R[3:6], X) + t[1]
    invz = f32(1) / z
    u = K["fx"] * x * invz + K["cx"]
    v = K["fy"] * y * invz + K["cy"]
    eX, eY = u - f.x, v - f.y
    if not f.uR >= 0:
        e2, thr, name = eX * eX + eY * eY, 5.991 * f64(f.sigma2), "chi2_mono%d" % which
    else:
        eR = (u - mbf * invz) - f.uR
        e2, thr, name = eX * eX + eY * eY + eR * eR, 7.8 * f64(f.sigma2), "chi2_stereo%d" % which
    margins[name] = _rel(e2, thr)
    return not (f64(e2) >= thr if wrong == name + "_ge" else f64(e2) > thr)


def _f32s(K, key):
    return [f32(v) for v in np.asarray(K[key], f32).reshape(-1)]


def _kf_scalars(kf):
    K = {k: f32(kf[k]) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mbf")}
    for key in ("Rcw", "tcw", "Ow", "Twc_q", "Twc_t"):
        K[key] = _f32s(kf, key)
    return K


def tri_pair(kf1, kf2, idx1, idx2, ratio_factor, wrong=None):
    with np.errstate(all="ignore"):
        return _tri_pair(_kf_scalars(kf1), _kf_scalars(kf2), feature(kf1, idx1, wrong), feature(kf2, idx2, wrong), f32(ratio_factor), wrong)


def _tri_pair(K1, K2, f1, f2, ratioFactor, wrong):
    margins = {}
    zero = [f32(0)] * 3
    out = lambda X, status, source, sweeps, A=None: Pair(np.array(X, f32), status, source, sweeps, cosRays, margins, A)
    stereo1, stereo2 = bool(f1.uR >= 0), bool(f2.uR >= 0)
    xn1 = [(f1.x - K1["cx"]) * K1["invfx"], (f1.y - K1["cy"]) * K1["invfy"], f32(1)]
    xn2 = [(f2.x - K2["cx"]) * K2["invfx"], (f2.y - K2["cy"]) * K2["invfy"], f32(1)]
    R1, R2 = K1["Rcw"], K2["Rcw"]
    ray1 = [(R1[i] * xn1[0] + R1[3 + i] * xn1[1]) + R1[6 + i] * xn1[2] for i in range(3)]
    ray2 = [(R2[i] * xn2[0] + R2[3 + i] * xn2[1]) + R2[6 + i] * xn2[2] for i in range(3)]
    cosRays = _dot(ray1, ray2) / (np.sqrt(_dot(ray1, ray1)) * np.sqrt(_dot(ray2, ray2)))
    cosStereo = cosRays + f32(1)
    cosStereo1 = cosStereo2 = cosStereo
    if stereo1:
        cosStereo1 = f1.cosStereo
    if stereo2 and (wrong == "elseif_if" or not stereo1):
        cosStereo2 = f2.cosStereo
    if wrong != "min_dropped":
        cosStereo = cosStereo2 if cosStereo2 < cosStereo1 else cosStereo1
    margins["parallax"] = _rel(cosRays, cosStereo)
    margins["cos_positive"] = abs(f64(cosRays))
    mono_gate = not (stereo1 or stereo2) or wrong == "mono_gate_on_stereo"
    if mono_gate:
        margins["cos_9998"] = _rel(cosRays, 0.9998)
    A = None
    sweeps = 0
    if cosRays < cosStereo and cosRays > 0 and ((not mono_gate) or f64(cosRays) < 0.9998):
        T1 = [[R1[3 * r + j] if j < 3 else K1["tcw"][r] for j in range(4)] for r in range(3)]
        T2 = [[R2[3 * r + j] if j < 3 else K2["tcw"][r] for j in range(4)] for r in range(3)]
        A = [[xn1[0] * T1[2][j] - T1[0][j] for j in range(4)], [xn1[1] * T1[2][j] - T1[1][j] for j in range(4)],
             [xn2[0] * T2[2][j] - T2[0][j] for j in range(4)], [xn2[1] * T2[2][j] - T2[1][j] for j in range(4)]]
        svd = jacobi_svd4(A, wrong)
        V, sweeps, source = svd.V, svd.sweeps, FROM_SVD
        if sweeps >= MAX_SWEEPS:
            return out(zero, SWEEP_CAP, source, sweeps, A)
        if V[3][3] == 0 and wrong != "v33_ignored":
            return out(zero, V33_ZERO, source, sweeps, A)
        X = [V[0][3] / V[3][3], V[1][3] / V[3][3], V[2][3] / V[3][3]]
    elif stereo1 and cosStereo1 < cosStereo2:
        margins["stereo_order"] = _rel(cosStereo1, cosStereo2)
        source, X = FROM_KF1, _unproject(K1, f1)
    elif stereo2 and cosStereo2 < cosStereo1:
        margins["stereo_order"] = _rel(cosStereo2, cosStereo1)
        source, X = FROM_KF2, _unproject(K2, f2)
    else:
        return out(zero, LOW_PARALLAX, FROM_NONE, 0)
    z1 = _dot(R1[6:9], X) + K1["tcw"][2]
    margins["z1"] = abs(f64(z1))
    if (z1 < 0) if wrong == "z1_lt" else (z1 <= 0):
        return out(X, Z1, source, sweeps, A)
    z2 = _dot(R2[6:9], X) + K2["tcw"][2]
    margins["z2"] = abs(f64(z2))
    if (z2 < 0) if wrong == "z2_lt" else (z2 <= 0):
        return out(X, Z2, source, sweeps, A)
    if not _reprojects(K1, f1, K1["mbf"], X, z1, 1, wrong, margins):
        return out(X, REPROJ1, source, sweeps, A)
    if not _reprojects(K2, f2, K2["mbf"] if wrong == "kf2_own_mbf" else K1["mbf"], X, z2, 2, wrong, margins):
        return out(X, REPROJ2, source, sweeps, A)
    n1 = [X[i] - K1["Ow"][i] for i in range(3)]
    n2 = [X[i] - K2["Ow"][i] for i in range(3)]
    dist1, dist2 = np.sqrt(_dot(n1, n1)), np.sqrt(_dot(n2, n2))
    margins["dist"] = min(f64(dist1), f64(dist2))
    if dist1 == 0 or dist2 == 0:
        return out(X, ZERO_DIST, source, sweeps, A)
    ratioDist = dist2 / dist1
    ratioOctave = f1.scale / f2.scale
    if wrong == "ratio_abs":
        bad = abs(ratioDist - ratioOctave) > ratioFactor
    else:
        margins["ratio_low"] = _rel(ratioDist * ratioFactor, ratioOctave)
        margins["ratio_high"] = _rel(ratioDist, ratioOctave * ratioFactor)
        bad = ratioDist * ratioFactor < ratioOctave or ratioDist > ratioOctave * ratioFactor
    return out(X, SCALE_RATIO if bad else ACCEPTED, source, sweeps, A)


def status_byte(p):
    return (p.source << 6) | p.status


# ---- keyframes ----------------------------------------------------------------------------------------------------------------------------------------
SCALE = np.array([f32(1.2) ** l for l in range(8)], f32)   # stand-ins for mvScaleFactors / mvLevelSigma2: inputs of the pair, any values do
SIGMA2 = (SCALE * SCALE).astype(f32)


def rot(axis, angle):
    a = np.asarray(axis, f64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def quat_of(R):
    """unit quaternion x y z w of a rotation matrix (float64)"""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:   # a half turn: the axis from the diagonal
        x = np.sqrt(max(0.0, (1 + R[0, 0]) / 2)); y = np.sqrt(max(0.0, (1 + R[1, 1]) / 2)); z = np.sqrt(max(0.0, (1 + R[2, 2]) / 2))
        q = np.array([x, np.copysign(y, R[0, 1]) if x > 0 else y, np.copysign(z, R[0, 2]) if x > 0 else np.copysign(z, R[1, 2]), 0.0])
    return q / np.linalg.norm(q)


def keyframe(R, C, keys_xy, octaves=None, fx=512.0, fy=512.0, cx=256.0, cy=256.0, mb=0.125, mbf=64.0, u_right=None, depth=None, cos_stereo=None,
             keys_un=None, level_sigma2=SIGMA2, scale_factors=SCALE):
    """R = Rcw (world -> camera), C = the camera centre.  The defaults are powers of two: products with them are exact."""
    R, C = np.asarray(R, f64), np.asarray(C, f64)
    n = len(keys_xy)
    keys = np.zeros(n, KP_DTYPE)
    keys["x"], keys["y"] = np.asarray(keys_xy, f32).reshape(n, 2).T
    keys["octave"] = 0 if octaves is None else octaves
    kf = dict(keys=keys, keys_un=None, fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy), mb=f32(mb), mbf=f32(mbf), invfx=f32(1) / f32(fx), invfy=f32(1) / f32(fy),
              u_right=None if u_right is None else np.asarray(u_right, f32), depth=None if depth is None else np.asarray(depth, f32),
              cos_stereo=None if cos_stereo is None else np.asarray(cos_stereo, f32), level_sigma2=np.asarray(level_sigma2, f32),
              scale_factors=np.asarray(scale_factors, f32), Rcw=R.astype(f32).reshape(9), tcw=(-R @ C).astype(f32), Ow=C.astype(f32),
              Twc_q=quat_of(R.T).astype(f32), Twc_t=C.astype(f32))
    if keys_un is not None:
        kf["keys_un"] = keys.copy()
        kf["keys_un"]["x"], kf["keys_un"]["y"] = np.asarray(keys_un, f32).reshape(n, 2).T
    return kf


def project(kf, X):
    """float64 pinhole projection of world points -> (uv n x 2, z n)"""
    R, t = kf["Rcw"].astype(f64).reshape(3, 3), kf["tcw"].astype(f64)
    P = np.asarray(X, f64).reshape(-1, 3) @ R.T + t
    return np.stack([f64(kf["fx"]) * P[:, 0] / P[:, 2] + f64(kf["cx"]), f64(kf["fy"]) * P[:, 1] / P[:, 2] + f64(kf["cy"])], 1), P[:, 2]


def cos_stereo_of(mb, depth):
    """the shell's expression: cosf(2 * atan2f(mb / 2, depth)), here with numpy's float32 functions -- an input of the pair, not part of it"""
    return np.cos(f32(2) * np.arctan2(f32(mb) / f32(2), np.asarray(depth, f32))).astype(f32)


# ---- pair cases ------------------------------------------------------------------------------------------------------------------------------------------
I3 = np.eye(3)
RATIO = 1.5 * 1.2
POW2 = np.array([2.0 ** l for l in range(8)], f32)   # a scale table whose quotients are exact


def _xy(kf):
    return float(kf["keys"]["x"][0]), float(kf["keys"]["y"][0])


def _two_views(X, C2=(0.5, 0.0, 0.0), R2=None, noise1=(0, 0), noise2=(0, 0), oct1=0, oct2=0):
    """KF1 at the origin, KF2 at C2, one key each: the float64 projection of the world point X plus noise"""
    k1 = keyframe(I3, (0, 0, 0), [(0, 0)], [oct1])
    k2 = keyframe(I3 if R2 is None else R2, C2, [(0, 0)], [oct2])
    for kf, nz in ((k1, noise1), (k2, noise2)):
        uv, _ = project(kf, X)
        kf["keys"]["x"], kf["keys"]["y"] = f32(uv[0, 0] + nz[0]), f32(uv[0, 1] + nz[1])
    return k1, k2


def _stereo_kf(R, C, uv, depth, cos, uR=None, **kw):
    d = np.atleast_1d(np.asarray(depth, f32))
    mbf = kw.get("mbf", 64.0)
    return keyframe(R, C, [uv], u_right=[uv[0] - mbf / float(d[0])] if uR is None else [uR], depth=d, cos_stereo=[cos], **kw)


def _mono_accept():
    return _two_views((0.3, -0.2, 4.0)) + (0, 0, RATIO)


_COS_9998 = {}


def _mono_cos_9998(side):
    """Two views whose rays meet at the float next to 0.9998 on the named side.  0.9998 is a double that no float equals, so `cos < 0.9998`
    has no equality: the two floats around it are the gate's two sides.  KF2's key x is bisected over the floats until the decision flips; the
    quotient of two floats just above 1 cannot be every float below 1, so the geometry is varied until the two sides are neighbours."""
    if not _COS_9998:
        z, r = 4.0, np.sqrt((1 - 0.9998) / (1 + 0.9998))   # baseline b, point in the middle: cos = (z^2 - b^2 / 4) / (z^2 + b^2 / 4), r = b / (2 z)
        for s in np.arange(0.0, 0.05, 0.001):   # a common slope of both rays moves |ray1| |ray2|, and with it the floats the quotient can be
            k1, k2 = _two_views((z * r, z * s, z), C2=(2 * z * r, 0.0, 0.0))
            x0 = k2["keys"]["x"][0]
            below = lambda x: f64(_with_x(k1, k2, x).cos_rays) < 0.9998
            lo, hi = f32(x0 - 2), f32(x0 + 2)   # moving the key towards the centre closes the angle: cos rises with x
            assert below(lo) and not below(hi)
            while np.nextafter(lo, hi) != hi:
                mid = f32((f64(lo) + f64(hi)) / 2)
                lo, hi = (mid, hi) if below(mid) else (lo, mid)
            if np.nextafter(_with_x(k1, k2, lo).cos_rays, f32(2)) == _with_x(k1, k2, hi).cos_rays:
                break
        else:
            raise AssertionError("no geometry puts the two floats around 0.9998 next to each other")
        _COS_9998["below"], _COS_9998["above"] = (k1, lo), (k1, hi)
        _COS_9998["k2"] = k2
    k1, x = _COS_9998[side]
    k1, k2 = {k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in k1.items()}, {k: np.copy(v) if isinstance(v, np.ndarray) else v for k, v in _COS_9998["k2"].items()}
    k2["keys"]["x"] = x
    return k1, k2, 0, 0, RATIO


def _with_x(k1, k2, x):
    k2["keys"]["x"] = x
    return tri_pair(k1, k2, 0, 0, RATIO)


def _cos_zero():
    """rays at a right angle, exactly: KF2 turned a quarter about y, both keys at the principal point, so cosParallaxRays == 0 and `> 0` fails"""
    R2 = np.array([[0.0, 0, -1], [0, 1, 0], [1, 0, 0]])   # camera z = world x
    return keyframe(I3, (0, 0, 0), [(256, 256)]), keyframe(R2, (-4, 0, 4), [(256, 256)]), 0, 0, RATIO


def _cos_tiny():
    """_cos_zero with KF1's key one float off the principal point: the cosine is the least it can be above 0, and the pair goes on to the SVD"""
    k1, k2, *_ = _cos_zero()
    k1["keys"]["x"] = np.nextafter(f32(256), f32(1e9))
    return k1, k2, 0, 0, RATIO


def _from_svd_stereo1():
    """stereo on KF1 only, cosRays below its cosine: the SVD"""
    k1, k2 = _two_views((0.3, -0.2, 4.0))
    return _stereo_kf(I3, (0, 0, 0), _xy(k1), 4.0, 0.999), k2, 0, 0, RATIO


def _exact_pair(stereo1, stereo2, src, sigma_zero=None, z_plane=None, z_off=0.0, scale=SCALE, oct1=0, oct2=0, ratio=RATIO):
    """Power-of-two geometry: every product of the unprojection and of the reprojection is exact, so the reprojection errors are exactly 0.
    World point X = (0.25, 0.5, 2); KF1 at the origin, KF2 at (0.5, 0, 0), both unrotated, so dist1 == dist2; fx = fy = 512, c = 256, mbf = 64.
      KF1 sees (320, 384), KF2 sees (192, 384); right-eye coordinates 288 and 160; depth 2 in both.
    The cosine inputs (0.5 on the side of `src`, 0.75 on the other) lose against cosRays = 0.97, so the pair goes to UnprojectStereo of `src`.
    sigma_zero: the keyframe (1 / 2) whose sigma2 table is all 0: its chi-square gate is met with equality, 0 > 0 -- the only equality a float
    sum and a double product with 5.991 or 7.8 have, since such a product is a float for no other finite sigma2 short of a 2^-29 coincidence.
    z_plane: the keyframe (1 / 2) moved along z so that the point lies in its plane z = z_off."""
    C1, C2 = [0.0, 0, 0], [0.5, 0, 0]
    if z_plane == 1:
        C1[2] = 2.0
    if z_plane == 2:
        C2[2] = 2.0
    sg = lambda k: np.zeros(8, f32) if sigma_zero == k else SIGMA2
    mk = lambda k, C, uv, st, cos, o: (_stereo_kf(I3, C, uv, 2.0, cos, level_sigma2=sg(k), scale_factors=scale, octaves=[o]) if st else
                                       keyframe(I3, C, [uv], [o], level_sigma2=sg(k), scale_factors=scale))
    k1 = mk(1, C1, (320.0, 384.0), stereo1, 0.5 if src == 1 else 0.75, oct1)
    k2 = mk(2, C2, (192.0, 384.0), stereo2, 0.5 if src == 2 else 0.75, oct2)
    if z_plane:
        kf = k1 if z_plane == 1 else k2
        kf["tcw"][2] = f32(-2) + f32(z_off)   # z = 2 + tcw[2], exactly
    return k1, k2, 0, 0, ratio


def _exact_pair_off(stereo1, stereo2, src, off):
    """_exact_pair with sigma2 == 0 on keyframe `off` and one float of error there: in the key's y where that side is monocular, in the right-eye
    coordinate where it is stereo (UnprojectStereo reads the key, not the right-eye coordinate)"""
    k1, k2, *_ = _exact_pair(stereo1, stereo2, src, sigma_zero=off)
    kf = k1 if off == 1 else k2
    what = "u_right" if kf["u_right"] is not None else None
    if what:
        kf["u_right"][0] = np.nextafter(kf["u_right"][0], f32(1e9))
    else:
        kf["keys"]["y"] = np.nextafter(kf["keys"]["y"], f32(1e9))
    return k1, k2, 0, 0, RATIO


def _both_stereo(cos1, cos2):
    """both stereo on the geometry of _exact_pair (cosRays = 0.97).  Only cos1 counts: the else-if of :1091"""
    return (_stereo_kf(I3, (0, 0, 0), (320.0, 384.0), 2.0, cos1), _stereo_kf(I3, (0.5, 0, 0), (192.0, 384.0), 2.0, cos2), 0, 0, RATIO)


def _stereo_0_9999():
    """stereo on KF1, rays at cos = 0.9999 > 0.9998: the SVD all the same, 0.9998 being the monocular gate.  The stereo cosine 1.5 is an input
    like any other and keeps the parallax gate far away"""
    z, r = 4.0, np.sqrt((1 - 0.9999) / (1 + 0.9999))
    k1, k2 = _two_views((z * r, 0.0, z), C2=(2 * z * r, 0.0, 0.0))
    return _stereo_kf(I3, (0, 0, 0), _xy(k1), 4.0, 1.5), k2, 0, 0, RATIO


def _kf2_mbf():
    """both stereo, the SVD's point; KF2's mbf is twice KF1's and its right-eye key is consistent with KF1's mbf, as :1168 reads it"""
    X = (0.3, -0.2, 4.0)
    k1, k2 = _two_views(X)
    a = _stereo_kf(I3, (0, 0, 0), _xy(k1), 4.0, 0.999, mbf=64.0)
    z2 = project(k2, X)[1][0]
    u2 = _xy(k2)[0]
    return a, _stereo_kf(I3, (0.5, 0, 0), _xy(k2), z2, 0.999, uR=u2 - 64.0 / z2, mbf=128.0), 0, 0, RATIO


def _behind(which):
    if which == 1:   # the two keys of a point in front, exchanged: the disparity changes sign and the lines meet behind both cameras
        k1, k2 = _two_views((0.3, -0.2, 4.0))
        a, b = _xy(k1), _xy(k2)
        k1["keys"]["x"], k1["keys"]["y"], k2["keys"]["x"], k2["keys"]["y"] = f32(b[0]), f32(b[1]), f32(a[0]), f32(a[1])
        return k1, k2, 0, 0, RATIO
    # KF2 four units ahead of KF1 on its axis, the point between them: in front of KF1, behind KF2, on the line KF2's key names
    return _two_views((1.0, -0.5, 4.0), C2=(0.0, 0.0, 6.0)) + (0, 0, RATIO)


def _reproj(which, stereo):
    """the SVD's point with the named view's key 9 pixels off in y: the SVD splits the inconsistency between the views, the shifted view at
    octave 0 fails its gate and the other view at octave 7 (sigma2 = 12.8) would pass its own"""
    kw = dict(noise1=(0, 9.0), oct1=0, oct2=7) if which == 1 else dict(noise2=(0, 9.0), oct1=7, oct2=0)
    k1, k2 = _two_views((0.3, -0.2, 4.0), **kw)
    if stereo and which == 1:
        k1 = _stereo_kf(I3, (0, 0, 0), _xy(k1), 4.0, 0.999)
    if stereo and which == 2:
        k2 = _stereo_kf(I3, (0.5, 0, 0), _xy(k2), 4.0, 0.999)
    return k1, k2, 0, 0, 100.0   # the octave ratio 1.2^7 is not this case's business


def _zero_dist(which, tiny=False):
    """UnprojectStereo of a feature with depth <= 0 is (0 0 0) (src/KeyFrame.cc:827).  Rcw, tcw and Ow are separate inputs of the pair: with
    tcw = (0 0 1) in both views the origin has z = 1 in both, with all sigma2 = 1e12 it passes both gates, and with the OTHER keyframe's Ow at the
    origin its distance is exactly 0.  tiny: that Ow at (2^-60, 0, 0) instead: the distance is not 0 and the pair goes on to the ratio test."""
    k1, k2, *_ = _exact_pair(which == 1, which == 2, which)
    src, oth = (k1, k2) if which == 1 else (k2, k1)
    src["depth"][:] = -1.0
    src["level_sigma2"] = oth["level_sigma2"] = np.full(8, 1e12, f32)
    k1["tcw"] = np.array([0, 0, 1], f32)
    k2["tcw"] = np.array([0, 0, 1], f32)
    oth["Ow"] = np.array([2.0 ** -60 if tiny else 0, 0, 0], f32)
    src["Ow"] = np.array([0, 0, -1], f32)
    return k1, k2, 0, 0, RATIO


def _ratio(kind):
    """accepted geometry (dist2 / dist1 about 1) and octaves that put the ratio test on either side"""
    o1, o2 = dict(low=(7, 0), high=(0, 7), product_form=(4, 0))[kind]   # 1.2^7 = 3.58; 1.2^4 = 2.07 > 1.8 while |1 - 2.07| < 1.8
    return _two_views((0.3, -0.2, 4.0), oct1=o1, oct2=o2) + (0, 0, RATIO)


def _ratio_exact(side, outside):
    """dist2 / dist1 == 1 exactly, scale factors 2^level, ratioFactor 2: ratioDist * 2 < 2 and ratioDist > 0.5 * 2 are both met with equality;
    outside: ratioFactor one float below 2"""
    o1, o2 = (1, 0) if side == "low" else (0, 1)
    return _exact_pair(True, False, 1, scale=POW2, oct1=o1, oct2=o2, ratio=np.nextafter(f32(2), f32(0)) if outside else f32(2))


def _undistorted():
    """keys_un 12 pixels away from the distorted keys in one view: reading them is another point and a failed gate"""
    k1, k2 = _two_views((0.3, -0.2, 4.0))
    for kf in (k1, k2):
        kf["keys_un"] = kf["keys"].copy()
    k2["keys_un"]["y"] += f32(12)
    return k1, k2, 0, 0, RATIO


def _v33_zero():
    """both keys at the principal point, both cameras unrotated, KF2 displaced along x: the rays are parallel (cos = 1, which passes with a stereo
    cosine above 1 -- an input), A's third column is exactly 0 and the null vector is (0 0 1 0): a point at infinity, V(3,3) == 0 exactly"""
    return _stereo_kf(I3, (0, 0, 0), (256.0, 256.0), 2.0, 2.0), keyframe(I3, (0.5, 0, 0), [(256.0, 256.0)]), 0, 0, RATIO


# name, maker -> (kf1, kf2, idx1, idx2, ratio_factor), status, source, the gates met exactly (left out of the margin), the wrong forms that move it
Spec = collections.namedtuple("Spec", "name make status source exact moved_by")
SVD_FORMS = ("sort_ascending", "threshold_no_maxdiag")   # every pair that takes x3D from a full-rank SVD: another column / other last bits
PAIR_SPECS = [
    Spec("mono_accept", _mono_accept, ACCEPTED, FROM_SVD, (), SVD_FORMS),
    Spec("mono_cos_below_9998", lambda: _mono_cos_9998("below"), ACCEPTED, FROM_SVD, ("cos_9998",), SVD_FORMS),
    Spec("mono_cos_above_9998", lambda: _mono_cos_9998("above"), LOW_PARALLAX, FROM_NONE, ("cos_9998",), ()),
    Spec("cos_zero", _cos_zero, LOW_PARALLAX, FROM_NONE, ("cos_positive",), ()),
    Spec("cos_one_float_above_zero", _cos_tiny, ACCEPTED, FROM_SVD, ("cos_positive",), SVD_FORMS),
    Spec("from_svd_stereo1", _from_svd_stereo1, ACCEPTED, FROM_SVD, (), SVD_FORMS),
    Spec("from_kf1", lambda: _exact_pair(True, False, 1), ACCEPTED, FROM_KF1, (), ("min_dropped",)),
    Spec("from_kf2", lambda: _exact_pair(False, True, 2), ACCEPTED, FROM_KF2, (), ("min_dropped",)),
    Spec("stereo_both_first_lower", lambda: _both_stereo(0.5, 0.75), ACCEPTED, FROM_KF1, (), ("min_dropped",)),
    Spec("stereo_both_second_lower", lambda: _both_stereo(0.999, 0.5), ACCEPTED, FROM_SVD, (), ("elseif_if",) + SVD_FORMS),
    Spec("stereo_above_9998", _stereo_0_9999, ACCEPTED, FROM_SVD, (), ("mono_gate_on_stereo",) + SVD_FORMS),
    Spec("chi2_mono1_equal", lambda: _exact_pair(False, True, 2, sigma_zero=1), ACCEPTED, FROM_KF2, ("chi2_mono1",), ("chi2_mono1_ge", "min_dropped")),
    Spec("chi2_mono1_outside", lambda: _exact_pair_off(False, True, 2, 1), REPROJ1, FROM_KF2, ("chi2_mono1",), ("min_dropped",)),
    Spec("chi2_stereo1_equal", lambda: _exact_pair(True, False, 1, sigma_zero=1), ACCEPTED, FROM_KF1, ("chi2_stereo1",), ("chi2_stereo1_ge", "min_dropped")),
    Spec("chi2_stereo1_outside", lambda: _exact_pair_off(True, False, 1, 1), REPROJ1, FROM_KF1, ("chi2_stereo1",), ("min_dropped",)),
    Spec("chi2_mono2_equal", lambda: _exact_pair(True, False, 1, sigma_zero=2), ACCEPTED, FROM_KF1, ("chi2_mono2",), ("chi2_mono2_ge", "min_dropped")),
    Spec("chi2_mono2_outside", lambda: _exact_pair_off(True, False, 1, 2), REPROJ2, FROM_KF1, ("chi2_mono2",), ("min_dropped",)),
    Spec("chi2_stereo2_equal", lambda: _exact_pair(False, True, 2, sigma_zero=2), ACCEPTED, FROM_KF2, ("chi2_stereo2",), ("chi2_stereo2_ge", "min_dropped")),
    Spec("chi2_stereo2_outside", lambda: _exact_pair_off(False, True, 2, 2), REPROJ2, FROM_KF2, ("chi2_stereo2",), ("min_dropped",)),
    Spec("z1_zero", lambda: _exact_pair(False, True, 2, z_plane=1), Z1, FROM_KF2, ("z1",), ("z1_lt", "min_dropped")),
    Spec("z1_one_float", lambda: _exact_pair(False, True, 2, z_plane=1, z_off=2.0 ** -22), REPROJ1, FROM_KF2, ("z1",), ("min_dropped",)),
    Spec("z2_zero", lambda: _exact_pair(True, False, 1, z_plane=2), Z2, FROM_KF1, ("z2",), ("z2_lt", "min_dropped")),
    Spec("z2_one_float", lambda: _exact_pair(True, False, 1, z_plane=2, z_off=2.0 ** -22), REPROJ2, FROM_KF1, ("z2",), ("min_dropped",)),
    Spec("z1_behind", lambda: _behind(1), Z1, FROM_SVD, (), SVD_FORMS),
    Spec("z2_behind", lambda: _behind(2), Z2, FROM_SVD, (), SVD_FORMS),
    Spec("reproj1_mono", lambda: _reproj(1, False), REPROJ1, FROM_SVD, (), SVD_FORMS),
    Spec("reproj1_stereo", lambda: _reproj(1, True), REPROJ1, FROM_SVD, (), SVD_FORMS),
    Spec("reproj2_mono", lambda: _reproj(2, False), REPROJ2, FROM_SVD, (), SVD_FORMS),
    Spec("reproj2_stereo", lambda: _reproj(2, True), REPROJ2, FROM_SVD, (), SVD_FORMS),
    Spec("kf2_reads_kf1_mbf", _kf2_mbf, ACCEPTED, FROM_SVD, (), ("kf2_own_mbf",) + SVD_FORMS),
    Spec("zero_dist1", lambda: _zero_dist(2), ZERO_DIST, FROM_KF2, ("dist",), ("min_dropped",)),
    Spec("zero_dist2", lambda: _zero_dist(1), ZERO_DIST, FROM_KF1, ("dist",), ("min_dropped",)),
    Spec("zero_dist1_tiny", lambda: _zero_dist(2, True), SCALE_RATIO, FROM_KF2, ("dist",), ("min_dropped",)),
    Spec("ratio_low", lambda: _ratio("low"), SCALE_RATIO, FROM_SVD, (), SVD_FORMS),
    Spec("ratio_high", lambda: _ratio("high"), SCALE_RATIO, FROM_SVD, (), ("ratio_abs",) + SVD_FORMS),
    Spec("ratio_product_form", lambda: _ratio("product_form"), SCALE_RATIO, FROM_SVD, (), ("ratio_abs",) + SVD_FORMS),
    Spec("ratio_low_equal", lambda: _ratio_exact("low", False), ACCEPTED, FROM_KF1, ("ratio_low", "ratio_high"), ("min_dropped",)),
    Spec("ratio_low_outside", lambda: _ratio_exact("low", True), SCALE_RATIO, FROM_KF1, ("ratio_low", "ratio_high"), ("min_dropped", "ratio_abs")),
    Spec("ratio_high_equal", lambda: _ratio_exact("high", False), ACCEPTED, FROM_KF1, ("ratio_low", "ratio_high"), ("min_dropped",)),
    Spec("ratio_high_outside", lambda: _ratio_exact("high", True), SCALE_RATIO, FROM_KF1, ("ratio_low", "ratio_high"), ("min_dropped", "ratio_abs")),
    Spec("distorted_keys", _undistorted, ACCEPTED, FROM_SVD, (), ("undistorted_keys",) + SVD_FORMS),
    Spec("v33_zero", _v33_zero, V33_ZERO, FROM_SVD, ("parallax",), ("v33_ignored", "mono_gate_on_stereo") + SVD_FORMS),
]


Case = collections.namedtuple("Case", "name kf1 kf2 idx1 idx2 ratio spec")
_CASES, _RESULTS = [], {}


def cases():
    if not _CASES:
        for s in PAIR_SPECS:
            _CASES.append(Case(s.name, *s.make(), s))
    return _CASES


def case_by_name(name):
    return next(c for c in cases() if c.name == name)


NAMES = [s.name for s in PAIR_SPECS]


def expected(case, wrong=None):
    key = (case.name, wrong)
    if key not in _RESULTS:
        _RESULTS[key] = tri_pair(case.kf1, case.kf2, case.idx1, case.idx2, case.ratio, wrong)
    return _RESULTS[key]


def same_pair(a, b):
    return a.status == b.status and a.source == b.source and np.array_equal(a.x3d.view(np.uint32), b.x3d.view(np.uint32))


def margin(case):
    """the least distance from the gates the case passed through, the ones it meets exactly left out"""
    m = expected(case).margins
    return min((v for k, v in m.items() if k not in case.spec.exact), default=np.inf)


# ---- svd cases ----------------------------------------------------------------------------------------------------------------------------------------
def _tiny_offdiag():
    A = np.diag([1.0, 0.5, 0.25, 0.125]).astype(f32)
    A[1, 0] = f32(1e-8)   # below 2 eps maxDiag = 2.4e-7, far above FLT_MIN
    return A


SvdSpec = collections.namedtuple("SvdSpec", "name make sweeps moved_by")   # sweeps: the count claimed (None: not claimed)
SVD_SPECS = [
    SvdSpec("diagonal", lambda: np.diag([3.0, -2.0, 1.0, 0.5]).astype(f32), 0, ("sort_ascending",)),
    SvdSpec("diagonal_unsorted", lambda: np.diag([0.5, -2.0, 3.0, 1.0]).astype(f32), 0, ("sort_ascending",)),
    SvdSpec("zero", lambda: np.zeros((4, 4), f32), 0, ()),
    SvdSpec("tiny_offdiagonal", _tiny_offdiag, 0, ("threshold_no_maxdiag", "sort_ascending")),
    SvdSpec("equal_values", lambda: np.eye(4, dtype=f32), 0, ()),
    SvdSpec("rank_one", lambda: np.outer([1, 2, 3, 4], [4, 3, 2, 1]).astype(f32), None, SVD_FORMS),
    SvdSpec("most_sweeps", lambda: most_sweeps_matrix(), None, SVD_FORMS),
]
SVD_NAMES = [s.name for s in SVD_SPECS]


def svd_case(name):
    return next(s for s in SVD_SPECS if s.name == name)


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------------------------------
SCENES = (("mono", 9001, False), ("stereo", 9101, True))   # name, seed, stereo
SCENE_PAIRS = 300
SCENE_NAMES = [s[0] for s in SCENES]
_SCENES = {}


def make_scene(seed, n, stereo, neighbours=1):
    """KF1 and `neighbours` posed pinhole keyframes over one random cloud of n points with pixel noise -> (kf1, [(kf2, idx1, idx2)], ratio):
    feature i of every keyframe sees point i; every tenth pair of a neighbour is a mismatch.  Neighbour j stands 0.6 + 0.15 j to the side."""
    rs = np.random.RandomState(seed)
    X = np.stack([rs.uniform(-3, 3, n), rs.uniform(-2, 2, n), rs.uniform(2, 12, n)], 1)
    poses = [(rot([0.1, 1.0, 0.05], 0.03), np.array([0.0, 0.0, 0.0]))]
    poses += [(rot([0.2, -1.0, 0.1], 0.08 - 0.01 * j), np.array([(0.6 + 0.15 * j) * (-1) ** j, 0.05 * (j + 1), -0.1])) for j in range(neighbours)]
    cam = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, mb=0.11, mbf=0.11 * 458.654)
    kfs = []
    for k, (R, C) in enumerate(poses):
        kf = keyframe(R, C, np.zeros((n, 2)), rs.randint(0, 8, n), **cam)
        uv, z = project(kf, X)
        und = uv + rs.normal(0, 0.7, uv.shape)
        r2 = ((und - [cam["cx"], cam["cy"]]) / [cam["fx"], cam["fy"]]) ** 2
        dist = und + (und - [cam["cx"], cam["cy"]]) * (-0.28 * r2.sum(1, keepdims=True))   # a radial term: the distorted keys the pair reads
        kf["keys"]["x"], kf["keys"]["y"] = (dist if k % 2 == 1 else und).astype(f32).T
        kf["keys_un"] = kf["keys"].copy()
        kf["keys_un"]["x"], kf["keys_un"]["y"] = und.astype(f32).T
        if stereo:
            has = rs.uniform(size=n) < 0.6
            d = (z + rs.normal(0, 0.02, n)).astype(f32)
            kf["depth"] = np.where(has, d, f32(-1)).astype(f32)
            kf["u_right"] = np.where(has, kf["keys"]["x"] - kf["mbf"] / d, f32(-1)).astype(f32)
            kf["cos_stereo"] = cos_stereo_of(kf["mb"], np.where(has, d, f32(1)))
        kfs.append(kf)
    problems = []
    for j in range(neighbours):
        idx1 = rs.permutation(n).astype(np.int32)
        idx2 = idx1.copy()
        bad = np.arange(0, n, 10)
        idx2[bad] = idx2[(bad + 7) % n]
        problems.append((kfs[1 + j], idx1, idx2))
    return kfs[0], problems, f32(1.5) * f32(1.2)


def scene(name):
    """a seeded scene of the suite -> (kf1, kf2, idx1, idx2, ratio)"""
    if name not in _SCENES:
        _, seed, stereo = next(s for s in SCENES if s[0] == name)
        k1, problems, ratio = make_scene(seed, SCENE_PAIRS, stereo)
        _SCENES[name] = (k1,) + problems[0] + (ratio,)
    return _SCENES[name]


_SCENE_RESULTS = {}


def scene_expected(name, wrong=None):
    if (name, wrong) not in _SCENE_RESULTS:
        k1, k2, i1, i2, ratio = scene(name)
        _SCENE_RESULTS[(name, wrong)] = [tri_pair(k1, k2, int(a), int(b), ratio, wrong) for a, b in zip(i1, i2)]
    return _SCENE_RESULTS[(name, wrong)]


def most_sweeps_matrix():
    """the A of the pair, over the constructed cases and the scenes, whose SVD takes the most sweeps (the first of equals)"""
    best = None
    for p in [expected(c) for c in cases()] + [p for s in SCENE_NAMES for p in scene_expected(s)]:
        if p.A is not None and (best is None or p.sweeps > best.sweeps):
            best = p
    return np.array(best.A, f32)


def max_sweeps_met():
    """the largest sweep count of the restatement over every constructed case, svd case and seeded scene"""
    counts = [expected(c).sweeps for c in cases()] + [p.sweeps for s in SCENE_NAMES for p in scene_expected(s)]
    counts += [jacobi_svd4(s.make()).sweeps for s in SVD_SPECS]
    return max(counts)


# ---- the cases as files, for the host program (tests/cpp/tri_host.cc) -----------------------------------------------------------------------------------
def _write_kf(f, kf):
    """int32 n nlevels stereo | float fx fy cx cy invfx invfy mbf Rcw[9] tcw[3] Ow[3] q[4] t[3] | keys n x 28 bytes | float sigma2[nlevels]
    scale[nlevels] | stereo: float uRight[n] depth[n] cosStereo[n]"""
    n, nl, st = len(kf["keys"]), len(kf["scale_factors"]), kf.get("u_right") is not None
    np.array([n, nl, int(st)], np.int32).tofile(f)
    np.array([kf[k] for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mbf")], f32).tofile(f)
    for key in ("Rcw", "tcw", "Ow", "Twc_q", "Twc_t"):
        np.ascontiguousarray(kf[key], f32).tofile(f)
    np.ascontiguousarray(kf["keys"], KP_DTYPE).tofile(f)
    np.ascontiguousarray(kf["level_sigma2"], f32).tofile(f)
    np.ascontiguousarray(kf["scale_factors"], f32).tofile(f)
    if st:
        for key in ("u_right", "depth", "cos_stereo"):
            np.ascontiguousarray(kf[key], f32).tofile(f)


def write_pairs(path, kf1, kf2, idx1, idx2, ratio):
    """float ratio | int32 nPairs | kf1 | kf2 | int32 idx1[nPairs] idx2[nPairs]"""
    i1, i2 = np.atleast_1d(np.asarray(idx1, np.int32)), np.atleast_1d(np.asarray(idx2, np.int32))
    with open(path, "wb") as f:
        np.array([ratio], f32).tofile(f)
        np.array([len(i1)], np.int32).tofile(f)
        _write_kf(f, kf1)
        _write_kf(f, kf2)
        i1.tofile(f)
        i2.tofile(f)


def read_pairs(path, n):
    """what the host program writes back: float x3d[3n] | uint8 status[n] | int32 sweeps[n]"""
    with open(path, "rb") as f:
        return np.fromfile(f, f32, 3 * n).reshape(n, 3), np.fromfile(f, np.uint8, n), np.fromfile(f, np.int32, n)


def as_arrays(pairs):
    """a list of Pair -> (x3d n x 3 float32, status bytes, sweeps)"""
    return (np.array([p.x3d for p in pairs], f32).reshape(-1, 3), np.array([status_byte(p) for p in pairs], np.uint8),
            np.array([p.sweeps for p in pairs], np.int32))


# ---- the matrices of the suite, for tools/make_golden_triangulate_eigen.cc and tests/test_tri_eigen_golden.py ------------------------------------------
def svd_inputs():
    """every 4 x 4 matrix of the suite in a fixed order: the svd cases, the A of every constructed pair case that reaches the SVD, the A of
    every scene pair that does -> (n, 4, 4) float32"""
    out = [np.array(s.make(), f32) for s in SVD_SPECS]
    out += [np.array(expected(c).A, f32) for c in cases() if expected(c).A is not None]
    for sc in SCENE_NAMES:
        out += [np.array(p.A, f32) for p in scene_expected(sc) if p.A is not None]
    return np.stack(out)


def write_svd_inputs(path):
    """int32 n | float A[n][16] row-major"""
    A = svd_inputs()
    with open(path, "wb") as f:
        np.array([len(A)], np.int32).tofile(f)
        np.ascontiguousarray(A, f32).tofile(f)
