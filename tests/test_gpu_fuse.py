"""GPU tests of ORBmatcher::Fuse(KeyFrame*, const vector<MapPoint*>&, th) on the device: the candidate search of ygzf_fuse_candidates against a
numpy restatement of src/ORBmatcher.cc:764-868 built on the oracle's GetFeaturesInArea / PredictScale / Hamming distance, bit for bit; the
K-keyframe batch against one-keyframe calls; the host shell (ygz::FuseBatch, ORBmatcher::Fuse over host/FuseApply.h) end to end against the
sequential restatement; the context's batch state across a call; argument errors."""
import os
import subprocess

import numpy as np
import pytest

from orb_ygz_slam_amd.capi import EUROC, KP_DTYPE, Extractor, YgzfError, make_camera
from orb_ygz_slam_amd.fuse_scene import _rot, edge_point, make_kf, make_points
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

f32 = np.float32


def ref_candidates(oracle, kf, world, normal, maxinv, mininv, mf, desc, th, skip_row=None, mutation=None):
    """Numpy restatement of src/ORBmatcher.cc:764-868 for one keyframe: float32 scalars in the reference's order, double where it promotes.
    mutation (tests only: the wrong forms the constructed cases must tell apart): "proj_order" = isInFrustum's u = (fx*PcX)*invz + cx,
    "gate_float" = the 7.8 / 5.99 gates compared in float, "view_div" = the viewing test as dot/dist3D < 0.5 in float."""
    P = len(world)
    bi = np.full(P, -1, np.int32)
    bd = np.full(P, 256, np.int32)
    R, t, Ow = kf["Rcw"], kf["tcw"], kf["Ow"]
    cam = kf["cam"]
    fx, fy, cx, cy, bf = f32(cam.fx), f32(cam.fy), f32(cam.cx), f32(cam.cy), f32(cam.mbf)
    minX, minY, maxX, maxY = f32(cam.min_x), f32(cam.min_y), f32(cam.max_x), f32(cam.max_y)
    keys, kdesc, sf, ig = kf["keys"], kf["desc"], kf["scale_factors"], kf["inv_level_sigma2"]
    ur_kf = kf["u_right"]
    for i in range(P):
        if skip_row is not None and skip_row[i]:
            continue
        p = world[i]
        pc = [((R[r, 0] * p[0] + R[r, 1] * p[1]) + R[r, 2] * p[2]) + t[r] for r in range(3)]
        if pc[2] < f32(0):
            continue
        invz = f32(1) / pc[2]
        x, y = pc[0] * invz, pc[1] * invz
        u, v = fx * x + cx, fy * y + cy
        if mutation == "proj_order":
            u, v = (fx * pc[0]) * invz + cx, (fy * pc[1]) * invz + cy
        if not (u >= minX and u < maxX and v >= minY and v < maxY):
            continue
        ur = u - bf * invz
        PO = [p[0] - Ow[0], p[1] - Ow[1], p[2] - Ow[2]]
        dist3D = np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2])
        if dist3D < mininv[i] or dist3D > maxinv[i]:
            continue
        Pn = normal[i]
        dot = (PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2]
        if (dot / dist3D < f32(0.5)) if mutation == "view_div" else (float(dot) < 0.5 * float(dist3D)):
            continue
        ratio = mf[i] / dist3D
        pred = int(oracle.predict_scale(np.array([ratio], f32), float(kf["log_scale_factor"]), kf["nlevels"])[0])
        radius = f32(th) * sf[pred]
        idx = oracle.features_in_area(keys, sf, kf["w"], kf["h"], float(u), float(v), float(radius))
        best, bidx = 256, -1
        for j in idx:
            kp = keys[j]
            lvl = int(kp["octave"])
            if lvl < pred - 1 or lvl > pred:
                continue
            ex, ey = u - kp["x"], v - kp["y"]
            if ur_kf is not None and ur_kf[j] >= 0:
                er = ur - ur_kf[j]
                e2 = (ex * ex + ey * ey) + er * er
                if (e2 * ig[lvl] > f32(7.8)) if mutation == "gate_float" else (float(e2 * ig[lvl]) > 7.8):
                    continue
            else:
                e2 = ex * ex + ey * ey
                if (e2 * ig[lvl] > f32(5.99)) if mutation == "gate_float" else (float(e2 * ig[lvl]) > 5.99):
                    continue
            d = oracle.hamming(desc[i], kdesc[j])
            if d < best:
                best, bidx = d, int(j)
        bi[i], bd[i] = bidx, best
    return bi, bd


# ---- constructed cases at the bounds where Fuse's arithmetic differs from isInFrustum ---------------------------------------------------------
# Each point is built so that ONE wrong form of the search changes its result (ref_candidates' `mutation`):
#   proj_in / proj_out: u = fx*(PcX*invz) + cx and isInFrustum's (fx*PcX)*invz + cx fall on opposite sides of max_x  -> "proj_order"
#   gate_7.8:           a stereo key at level 0 whose float e2 is exactly 7.8f (> 7.8): the double compare rejects it -> "gate_float"
#   view_eq / view_below: PO.Pn == 0.5*dist3D exactly (passes) and one float step of the normal below it (fails).  The float form dot/dist3D < 0.5
#                       ("view_div") gives the same answer for every pair of normal floats -- a correctly rounded quotient of x < 0.5*y stays below
#                       0.5 -- so these two pin the bound itself (a `<=`, another constant, an approximate division) rather than that mutation.
def constructed_case(seed=0):
    rng = np.random.default_rng(seed)
    kf = make_kf(rng, 752, 480, 8, 8, 1.2, np.eye(3), [0, 0, 0], mbf=40.0, stereo_frac=0.0, dup_frac=0.0)
    fx, fy, cx, cy, bf = (f32(getattr(kf["cam"], a)) for a in ("fx", "fy", "cx", "cy", "mbf"))
    mx = f32(kf["cam"].max_x)
    keys = np.zeros(0, KP_DTYPE)
    rows = []          # (world, normal, mf, key index, label)
    keylist, ur = [], []

    def add_key(x, y, octave, u_right=-1.0):
        k = np.zeros(1, KP_DTYPE)
        k["x"], k["y"], k["octave"], k["size"] = x, y, octave, 31
        keylist.append(k)
        ur.append(f32(u_right))
        return len(keylist) - 1

    # A: the two projection orders put u on opposite sides of max_x
    found = {}
    for _ in range(200000):
        z = f32(rng.uniform(1.5, 9.0))
        invz = f32(1) / z
        X = f32((float(mx) - float(cx)) / float(fx) * float(z))
        X = np.nextafter(X, f32(np.inf) if rng.random() < 0.5 else f32(-np.inf))
        for _k in range(int(rng.integers(0, 4))):
            X = np.nextafter(X, f32(np.inf))
        u1 = fx * (X * invz) + cx
        u2 = (fx * X) * invz + cx
        if (u1 < mx) != (u2 < mx):
            key = "in" if u1 < mx else "out"
            found.setdefault(key, (X, z))
        if len(found) == 2:
            break
    for lab, (X, z) in sorted(found.items()):
        Y = f32(f32(240.0 - float(cy)) / fy * z)
        ki = add_key(f32(746.0), f32(240.0), 7)
        P = np.array([X, Y, z], f32)
        dist = float(np.linalg.norm(P.astype(np.float64)))
        rows.append((P, (P / np.linalg.norm(P)).astype(f32), f32(dist * 10), ki, "proj_" + lab))
    # B: a stereo key at level 0 whose float e2 is exactly 7.8f
    z = f32(4.0)
    invz = f32(1) / z
    X, Y = f32(-0.3), f32(-0.1)
    u, v = fx * (X * invz) + cx, fy * (Y * invz) + cy
    urr = u - bf * invz
    target = f32(7.8)
    hit = None
    kx = (u - np.linspace(0.2, 2.6, 200001).astype(f32)).astype(f32)
    ex = (u - kx).astype(f32)
    e2x = (ex * ex + f32(0) * f32(0)).astype(f32)
    need = np.sqrt(np.maximum(float(target) - e2x.astype(np.float64), 0)).astype(f32)
    kr0 = (urr - need).astype(f32)
    for step in range(-3, 4):
        kr = kr0
        for _ in range(abs(step)):
            kr = np.nextafter(kr, f32(np.inf) if step > 0 else f32(-np.inf))
        er = (urr - kr).astype(f32)
        e2 = (e2x + er * er).astype(f32)
        ok = np.nonzero(e2 == target)[0]
        if len(ok):
            hit = (kx[ok[0]], kr[ok[0]])
            break
    assert hit is not None
    ki = add_key(hit[0], v, 0, hit[1])
    P = np.array([X, Y, z], f32)
    dist = float(np.linalg.norm(P.astype(np.float64)))
    rows.append((P, (P / np.linalg.norm(P)).astype(f32), f32(dist * 0.9), ki, "gate_7.8"))
    # C: the viewing test at its bound: dot == 0.5*dist3D exactly (passes) and one step of the normal below it (fails)
    P = np.array([f32(0.4), f32(-0.2), f32(3.0)], f32)
    dist = np.sqrt((P[0] * P[0] + P[1] * P[1]) + P[2] * P[2])
    half = f32(0.5) * dist
    d = P.astype(np.float64) / np.linalg.norm(P.astype(np.float64))
    perp = np.cross(d, [1.0, 0.0, 0.0]); perp /= np.linalg.norm(perp)
    n = (0.5 * d + np.sqrt(0.75) * perp).astype(f32)
    dot = lambda n: (P[0] * n[0] + P[1] * n[1]) + P[2] * n[2]
    eq = None
    for _ in range(200):
        dv = dot(n)
        if dv == half:
            eq = n.copy()
            break
        n[2] = np.nextafter(n[2], f32(np.inf) if dv < half else f32(-np.inf))
    assert eq is not None
    below = eq.copy()
    while dot(below) >= half:
        below[2] = np.nextafter(below[2], f32(-np.inf))
    invz = f32(1) / P[2]
    u, v = fx * (P[0] * invz) + cx, fy * (P[1] * invz) + cy
    ki = add_key(u, v, 0)
    rows.append((P, eq, f32(float(dist) * 0.9), ki, "view_eq"))
    ki = add_key(u, v, 0)
    rows.append((P, below, f32(float(dist) * 0.9), ki, "view_below"))
    return kf, keylist, ur, rows, (u, v)


def assemble(seed=0):
    kf, kl, ur, rows, _ = constructed_case(seed)
    rng = np.random.default_rng(seed + 1)
    kf = dict(kf)
    kf["keys"] = np.concatenate(kl)
    kf["u_right"] = np.array(ur, f32)
    kf["desc"] = rng.integers(0, 256, (len(kl), 32), dtype=np.uint8)
    world = np.stack([r[0] for r in rows]).astype(f32)
    normal = np.stack([r[1] for r in rows]).astype(f32)
    mf = np.array([r[2] for r in rows], f32)
    desc = np.stack([kf["desc"][r[3]] for r in rows])
    maxinv = np.full(len(rows), 1000, f32)
    mininv = np.full(len(rows), 0.001, f32)
    return kf, (world, normal, maxinv, mininv, mf, desc), [r[4] for r in rows], [r[3] for r in rows]


def scene(seed, P=240):
    rng = np.random.default_rng(seed)
    kfs = [make_kf(rng, 752, 480, 700, 8, 1.2, np.eye(3), [0, 0, 0], mbf=40.0, stereo_frac=0.5),
           make_kf(rng, 752, 480, 500, 8, 1.2, _rot(0.02, -0.05, 0.01), [0.1, -0.02, 0.05]),
           make_kf(rng, 640, 480, 400, 5, 1.5, _rot(-0.03, 0.04, 0.0), [-0.2, 0.05, 0.1], mbf=30.0, stereo_frac=0.7)]
    world, normal, maxinv, mininv, mf, desc = make_points(rng, kfs, P)
    extra_w, extra = [], []
    for kf in kfs[:2]:                                                     # u exactly at max_x (rejected: IsInImage is half-open) / just below
        for exact in (True, False):
            pc, wpt = edge_point(kf, exact=exact)
            extra_w.append(wpt)
    world = np.concatenate([world, np.array(extra_w, f32)])
    n_extra = len(extra_w)
    normal = np.concatenate([normal, np.tile(np.array([[0, 0, 1]], f32), (n_extra, 1))])
    maxinv = np.concatenate([maxinv, np.full(n_extra, 100, f32)])
    mininv = np.concatenate([mininv, np.full(n_extra, 0.01, f32)])
    mf = np.concatenate([mf, np.full(n_extra, 3.0, f32)])
    desc = np.concatenate([desc, rng.integers(0, 256, (n_extra, 32), dtype=np.uint8)])
    return kfs, (world, normal, maxinv, mininv, mf, desc)


@pytest.fixture(scope="module")
def ex():
    e = Extractor(1000, 1.2, 8, 20, 7, 752, 480)
    yield e
    e.close()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuse_candidates_match_restatement(oracle, ex, seed):
    kfs, pts = scene(seed)
    K, P = len(kfs), len(pts[0])
    rng = np.random.default_rng(100 + seed)
    skip = (rng.random((K, P)) < 0.1).astype(np.uint8)
    for th, sk in ((3.0, None), (5.0, skip)):
        bi, bd = ex.fuse_candidates(kfs, *pts, th=th, skip=sk)
        assert bi.shape == (K, P) and bd.shape == (K, P)
        for k in range(K):
            ri, rd = ref_candidates(oracle, kfs[k], *pts, th, None if sk is None else sk[k])
            assert (bi[k] == ri).all() and (bd[k] == rd).all(), (seed, th, k, np.nonzero((bi[k] != ri) | (bd[k] != rd))[0][:10])
        found = bi >= 0
        assert found.sum() > 20                                        # the scene does produce matches
        assert ((bd <= 50) & found).any() and ((bd > 50) & found).any()
        if sk is not None:
            assert (bi[sk != 0] == -1).all() and (bd[sk != 0] == 256).all()
    # the edge points: u == max_x is outside (half-open IsInImage), the float just below is inside: a key right there matches it
    kf = dict(kfs[0])
    ew = pts[0][-4:-2]
    pc, _ = edge_point(kf, exact=False)
    u_below = f32(kf["cam"].fx) * (f32(pc[0]) * (f32(1) / f32(pc[2]))) + f32(kf["cam"].cx)
    v = f32(kf["cam"].fy) * (f32(pc[1]) * (f32(1) / f32(pc[2]))) + f32(kf["cam"].cy)
    # (a key right of x = 746.125 falls outside the 64 columns of Frame::PosInGrid, so the key sits 6 px left, at the coarsest level:
    # mfMaxDistance = 12 clamps PredictScale to L-1 there, whose radius and sigma admit 6 px)
    kf["keys"] = kf["keys"].copy()
    kf["keys"][100]["x"], kf["keys"][100]["y"], kf["keys"][100]["octave"] = u_below - f32(6), v, kf["nlevels"] - 1
    kf["u_right"] = None
    edesc = np.stack([kf["desc"][100], kf["desc"][100]])
    eargs = (ew, np.tile(np.array([[0, 0, 1]], f32), (2, 1)), np.full(2, 100, f32), np.full(2, 0.01, f32), np.full(2, 12.0, f32), edesc)
    bi, bd = ex.fuse_candidates([kf], *eargs)
    assert bi[0, 0] == -1 and bi[0, 1] == 100 and bd[0, 1] == 0
    ri, rd = ref_candidates(oracle, kf, *eargs, 3.0)
    assert (ri == bi[0]).all() and (rd == bd[0]).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fuse_candidates_constructed_bounds(oracle, ex, seed):
    kf, pts, labels, _ = assemble(seed)
    bi, bd = ex.fuse_candidates([kf], *pts)
    ri, rd = ref_candidates(oracle, kf, *pts, 3.0)
    assert (bi[0] == ri).all() and (bd[0] == rd).all(), (labels, bi[0], ri)
    got = dict(zip(labels, bi[0] >= 0))
    assert got == {"proj_in": True, "proj_out": False, "gate_7.8": False, "view_eq": True, "view_below": False}, got
    # each constructed case is there to catch its mutation: the wrong form gives another answer on exactly those points
    for mutation, flips in (("proj_order", {"proj_in", "proj_out"}), ("gate_float", {"gate_7.8"}), ("view_div", set())):
        mi, _ = ref_candidates(oracle, kf, *pts, 3.0, mutation=mutation)
        assert {lab for lab, a, b in zip(labels, mi >= 0, ri >= 0) if a != b} == flips, mutation


def test_fuse_candidates_empty(ex):
    kfs, pts = scene(4, P=20)
    bi, bd = ex.fuse_candidates([], *pts)
    assert bi.shape == (0, len(pts[0]))
    e = [np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, f32), np.zeros(0, f32), np.zeros(0, f32), np.zeros((0, 32), np.uint8)]
    bi, bd = ex.fuse_candidates(kfs, *e)
    assert bi.shape == (len(kfs), 0)


def test_fuse_batch_equals_single_calls(ex):
    kfs, pts = scene(7, P=600)
    kfs = kfs + [kfs[0], kfs[2]]                                           # duplicated rows
    bi, bd = ex.fuse_candidates(kfs, *pts)
    for k, kf in enumerate(kfs):
        si, sd = ex.fuse_candidates([kf], *pts)
        assert (si[0] == bi[k]).all() and (sd[0] == bd[k]).all(), k
    assert (bi[3] == bi[0]).all() and (bi[4] == bi[2]).all()


def test_fuse_rows_at_slice_edge_and_empty_keyframe(oracle, ex):
    """The row table where it can go wrong: 65 points (one past the 64-point slice), a keyframe without keys between a stereo and a mono one,
    skips at the last point of row 0 and the first of row 2."""
    rng = np.random.default_rng(21)
    stereo = make_kf(rng, 752, 480, 300, 8, 1.2, np.eye(3), [0, 0, 0], mbf=40.0, stereo_frac=0.6)
    empty = dict(make_kf(rng, 752, 480, 16, 8, 1.2, _rot(0.01, 0.02, 0.0), [0.05, 0.0, 0.02]))
    empty["keys"], empty["desc"] = empty["keys"][:0], empty["desc"][:0]
    mono = make_kf(rng, 640, 480, 200, 5, 1.5, _rot(-0.03, 0.04, 0.0), [-0.2, 0.05, 0.1])
    assert stereo["u_right"] is not None and (stereo["u_right"] >= 0).any() and mono["u_right"] is None and len(empty["keys"]) == 0
    kfs = [stereo, empty, mono]
    P = 65
    pts = make_points(rng, [stereo, mono], P)
    # the two skipped entries are points that do find a key when searched, so a skip byte read at the wrong offset shows
    hit = [ref_candidates(oracle, kf, *pts, 3.0)[0] >= 0 for kf in (stereo, mono)]
    a = int(np.nonzero(hit[0])[0][0])
    b = int(np.nonzero(hit[1] & (np.arange(P) != a))[0][0])
    order = [b] + [i for i in range(P) if i not in (a, b)] + [a]
    pts = tuple(x[order] for x in pts)
    skip = np.zeros((3, P), np.uint8)
    skip[0, 64] = skip[2, 0] = 1
    bi, bd = ex.fuse_candidates(kfs, *pts, skip=skip)
    assert bi.shape == (3, P) and bd.shape == (3, P)
    for k, kf in enumerate(kfs):
        ri, rd = ref_candidates(oracle, kf, *pts, 3.0, skip[k])
        assert (bi[k] == ri).all() and (bd[k] == rd).all(), (k, np.nonzero((bi[k] != ri) | (bd[k] != rd))[0][:10])
        si, sd = ex.fuse_candidates([kf], *pts, skip=skip[k:k + 1])
        assert (si[0] == bi[k]).all() and (sd[0] == bd[k]).all(), k
    assert (bi[skip != 0] == -1).all() and (bd[skip != 0] == 256).all()
    assert (bi[1] == -1).all() and (bd[1] == 256).all()
    assert (bi[0, :64] >= 0).any() and (bi[2, 1:] >= 0).any()           # the rows next to the empty one do find keys


def test_fuse_reverse_shape(oracle, ex):
    """1 keyframe x 30 000 points (LocalMapping.cc:1273-1304) equals 1 000-point chunks, and the restatement on a sample."""
    rng = np.random.default_rng(11)
    kf = make_kf(rng, 752, 480, 2000, 8, 1.2, np.eye(3), [0, 0, 0], mbf=40.0, stereo_frac=0.5)
    pts = make_points(rng, [kf], 30000)
    bi, bd = ex.fuse_candidates([kf], *pts)
    assert bi.shape == (1, 30000)
    for s in range(0, 30000, 1000):
        ci, cd = ex.fuse_candidates([kf], *(a[s:s + 1000] for a in pts))
        assert (ci[0] == bi[0, s:s + 1000]).all() and (cd[0] == bd[0, s:s + 1000]).all(), s
    sample = rng.choice(30000, 300, replace=False)
    ri, rd = ref_candidates(oracle, kf, *(a[sample] for a in pts), 3.0)
    assert (ri == bi[0, sample]).all() and (rd == bd[0, sample]).all()
    assert (bi[0] >= 0).sum() > 2000


def test_fuse_keeps_context_batch_state():
    """A fuse_candidates call between extract_batch_* and match_batch_prev leaves the match results unchanged."""
    from orb_ygz_slam_amd.synth import synth_frame
    frames = np.stack([synth_frame(50 + s, 752, 480) for s in range(4)])
    cam = make_camera(752, 480)
    kfs, pts = scene(8, P=200)
    results = []
    for fuse in (False, True):
        e = Extractor(1000, 1.2, 8, 20, 7, 752, 480, max_batch=4)
        try:
            e.extract_batch_host(frames[:2])
            e.match_batch_prev(cam)
            e.extract_batch_host(frames[2:])
            if fuse:
                bi, _ = e.fuse_candidates(kfs, *pts)
                assert (bi >= 0).any()
            e.match_batch_prev(cam)
            results.append([e.match_fetch(p) for p in range(2)] + [e.match_counts().copy()])
        finally:
            e.close()
    a, b = results
    for x, y in zip(a, b):
        if isinstance(x, tuple):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)
        else:
            assert np.array_equal(x, y)


def test_fuse_errors(ex):
    import ctypes as C
    from orb_ygz_slam_amd.capi import FuseKf, FusePoints, _p
    kfs, pts = scene(9, P=50)
    L = ex.L
    bi = np.zeros(len(kfs) * 50, np.int32)
    bd = np.zeros(len(kfs) * 50, np.int32)

    def call(kfs_, pts_):
        return ex.fuse_candidates(kfs_, *pts_)
    bad = dict(kfs[0])
    bad["keys"] = kfs[0]["keys"].copy()
    bad["keys"]["octave"][5] = 8                                              # outside the keyframe's 8-level tables
    with pytest.raises(YgzfError, match="octave"):
        call([kfs[1], bad], pts)
    bad2 = dict(kfs[2])
    bad2["keys"] = kfs[2]["keys"].copy()
    bad2["keys"]["octave"][0] = -1
    with pytest.raises(YgzfError, match="octave"):
        call([bad2], pts)
    big = dict(kfs[0])
    n = 40000
    big["keys"] = np.resize(kfs[0]["keys"], n)
    big["desc"] = np.resize(kfs[0]["desc"], (n, 32))
    big["u_right"] = None
    with pytest.raises(YgzfError, match="keypoints in one grid"):
        call([big], pts)
    # NULL arrays through the C ABI directly
    w = np.ascontiguousarray(pts[0], f32)
    fp = FusePoints(w.ctypes.data, None, None, None, None, None)
    arr = (FuseKf * 1)()
    rc = L.ygzf_fuse_candidates(ex.h, 1, arr, 50, C.byref(fp), None, 3.0, _p(bi), _p(bd))
    assert rc < 0 and b"null" in L.ygzf_last_error(ex.h)
    rc = L.ygzf_fuse_candidates(ex.h, 1, None, 50, C.byref(fp), None, 3.0, _p(bi), _p(bd))
    assert rc < 0 and b"null" in L.ygzf_last_error(ex.h)
    rc = L.ygzf_fuse_candidates(ex.h, -1, arr, 50, C.byref(fp), None, 3.0, _p(bi), _p(bd))
    assert rc < 0
    # the context is still usable
    bi2, bd2 = call(kfs, pts)
    ref_i, ref_d = call(kfs, pts)
    assert (bi2 == ref_i).all() and (bd2 == ref_d).all()
    assert (bi2 >= 0).any()


def _build_shell(tmp):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
    exe = os.path.join(tmp, "fuse_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "fuse_shell.cc")] + [os.path.join(host, f) for f in
                                                                  ("ORBextractor.cc", "ORBmatcher.cc", "ORBmatcherFuse.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_fuse_shell_end_to_end(tmp_path):
    """ygz::FuseBatch (LocalMapping.cc:1259-1269) and per-target ORBmatcher::Fuse give the final graph of the sequential restatement."""
    from orb_ygz_slam_amd import load_library
    load_library()
    exe = _build_shell(str(tmp_path))
    for seed in (1, 2, 3):
        out = subprocess.run([exe, str(seed)], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stdout + out.stderr
        assert "fuse shell ok" in out.stdout, out.stdout
