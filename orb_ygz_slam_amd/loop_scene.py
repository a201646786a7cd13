"""Seeded synthetic scenes for the loop-closing projection searches (ygzf_fuse_sim3_candidates, ygzf_search_by_projection_sim3,
ygzf_search_by_sim3): used by tests/test_gpu_loop_search.py and tests/test_loop_cases.py.  Built on fuse_scene's helpers; pure
numpy, deterministic per generator.  Keyframes carry a Sim3 pose Scw = [s R | t] with s != 1 and its decomposition (Rcw = R, tcw = t / s,
Ow = -R' tcw: what the device contract takes)."""
import numpy as np

from .capi import EUROC
from .fuse_scene import _rot, make_kf, make_points

f32 = np.float32


def decompose_scw(Scw):
    """Scw (4x4 float32) -> Rcw, tcw, Ow as src/ORBmatcher.cc:274-278 writes them, in the scalar form of host/ORBmatcherLoop.h: scw = the float
    of the double root of the double sum of squares of row 0; every entry times the double 1 / scw, rounded to float; Ow = -(Rcw' tcw) as float
    dots left to right."""
    S = np.asarray(Scw, f32)
    r0 = S[0, :3].astype(np.float64)
    scw = f32(np.sqrt((r0[0] * r0[0] + r0[1] * r0[1]) + r0[2] * r0[2]))
    inv = 1.0 / float(scw)
    R = (S[:3, :3].astype(np.float64) * inv).astype(f32)
    t = (S[:3, 3].astype(np.float64) * inv).astype(f32)
    Ow = np.array([-((R[0, c] * t[0] + R[1, c] * t[1]) + R[2, c] * t[2]) for c in range(3)], f32)
    return R, t, Ow


def make_sim3_kf(rng, w, h, n, nlevels, scale, R, t, s, dup_frac=0.05):
    """A monocular keyframe whose corrected pose is the Sim3 Scw = [s R | t]; Rcw / tcw / Ow hold its decomposition."""
    S = np.eye(4, dtype=f32)
    S[:3, :3] = (f32(s) * np.asarray(R, f32)).astype(f32)
    S[:3, 3] = np.asarray(t, f32)
    Rc, tc, Ow = decompose_scw(S)
    kf = make_kf(rng, w, h, n, nlevels, scale, Rc, tc, dup_frac=dup_frac)
    kf["Ow"] = Ow
    kf["Scw"] = S
    return kf


def cluster_points(rng, kf, n_clusters, per):
    """Point clusters that compete for the same keys: `per` points seeded from one key each, a fraction of a pixel apart, descriptors a few bits
    from the key's -- SearchByProjection(pKF, Scw, ..)'s vpMatched[idx] test gives the key to the first and sends the others to their next best."""
    world, normal, mf, desc = [], [], [], []
    R, t, ow = kf["Rcw"].astype(np.float64), kf["tcw"].astype(np.float64), kf["Ow"].astype(np.float64)
    for _ in range(n_clusters):
        j = int(rng.integers(8, len(kf["keys"])))
        k = kf["keys"][j]
        for _p in range(per):
            off = rng.normal(0, 0.4, 2)
            z = rng.uniform(2.0, 8.0)
            pc = np.array([(k["x"] + off[0] - EUROC["cx"]) / EUROC["fx"] * z, (k["y"] + off[1] - EUROC["cy"]) / EUROC["fy"] * z, z])
            wp = (R.T @ (pc - t)).astype(f32)
            d = kf["desc"][j].copy()
            for b in rng.choice(256, int(rng.choice([0, 2, 5, 9])), replace=False):
                d[b // 8] ^= np.uint8(1 << (b % 8))
            v = wp.astype(np.float64) - ow
            dist = np.linalg.norm(v)
            world.append(wp); normal.append((v / dist).astype(f32)); desc.append(d)
            mf.append(f32(dist * 1.2 ** (int(k["octave"]) - rng.uniform(0.1, 0.9))))
    mf = np.array(mf, f32)
    return (np.array(world, f32), np.array(normal, f32), (f32(1.2) * mf).astype(f32), (f32(0.8) * (mf / f32(1.2 ** 7))).astype(f32), mf,
            np.array(desc, np.uint8))


def loop_scene(seed, P=240, K=3, n_keys=(700, 500, 400), clusters=12):
    """K Sim3 keyframes (scales 1.07, 0.93, 1.21, ...) and a loop-point list: fuse_scene.make_points' mixture (accepted and rejected at every
    test) plus clusters competing for keys of keyframe 0."""
    rng = np.random.default_rng(seed)
    kfs = []
    for k in range(K):
        ang = (0.02 * k, -0.05 + 0.03 * k, 0.01 * k)
        kfs.append(make_sim3_kf(rng, 752, 480, n_keys[k % len(n_keys)], 8, 1.2, _rot(*ang), [0.1 * k, -0.02 * k, 0.05 * k],
                                (1.07, 0.93, 1.21, 0.88)[k % 4]))
    pts = make_points(rng, kfs, P)
    cl = cluster_points(rng, kfs[0], clusters, 4)
    pts = tuple(np.concatenate([a, b]) for a, b in zip(pts, cl))
    order = rng.permutation(len(pts[0]))
    return kfs, tuple(a[order] for a in pts)


def _flip(rng, d, n):
    d = d.copy()
    for b in rng.choice(256, n, replace=False):
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def sim3_pair(seed, n_common=300, n_extra=200, s12=1.15):
    """A pair of overlapping keyframes for SearchBySim3: n_common structure points seen by both (key k of KF1 and key k of KF2, each keyframe with
    a MapPoint of its own for it, KF2's in a map drifted by the Sim3 S12), the rest unrelated keys, part of them with MapPoints.  Returns
    kf1, kf2 (fuse_scene keyframe dicts with their rigid poses), pts1, pts2 (world, max_dist_inv, min_dist_inv, mf_max_distance, desc per key),
    has1, has2 (a MapPoint in the slot) and the transforms dict of capi.Extractor.search_by_sim3."""
    rng = np.random.default_rng(seed)
    w, h, L = 752, 480, 8
    n = n_common + n_extra
    R1, t1 = _rot(0.01, 0.02, -0.01), np.array([0.05, -0.02, 0.01], f32)
    R2, t2 = _rot(-0.02, 0.01, 0.02), np.array([-0.1, 0.03, 0.02], f32)
    kf1 = make_kf(rng, w, h, n, L, 1.2, R1, t1, dup_frac=0.0)
    kf2 = make_kf(rng, w, h, n, L, 1.2, R2, t2, dup_frac=0.0)
    R12 = _rot(0.03, -0.04, 0.02).astype(np.float64)
    t12 = np.array([0.15, -0.05, 0.1])
    sR12 = (f32(s12) * R12.astype(f32)).astype(f32)                                   # s12 * R12
    sR21 = (f32(1.0 / f32(s12)) * R12.astype(f32).T).astype(f32)                      # (1 / s12) * R12'
    t12f = t12.astype(f32)
    t21 = np.array([-((sR21[r, 0] * t12f[0] + sR21[r, 1] * t12f[1]) + sR21[r, 2] * t12f[2]) for r in range(3)], f32)
    fx, fy, cx, cy = EUROC["fx"], EUROC["fy"], EUROC["cx"], EUROC["cy"]

    def side(kf):
        N = len(kf["keys"])
        return dict(world=np.zeros((N, 3), f32), mf=np.ones(N, f32), desc=rng.integers(0, 256, (N, 32), dtype=np.uint8), has=np.zeros(N, np.uint8))
    a, b = side(kf1), side(kf2)
    for k in range(8, 8 + n_common):
        z1 = rng.uniform(2.0, 9.0)
        c1 = np.array([(rng.uniform(40, w - 40) - cx) / fx * z1, (rng.uniform(40, h - 40) - cy) / fy * z1, z1])
        c2 = (1.0 / s12) * (R12.T @ (c1 - t12))
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        octv = int(rng.integers(0, L))
        for kf, c, sd, T in ((kf1, c1, a, (R1, t1)), (kf2, c2, b, (R2, t2))):
            noise = rng.normal(0, 1.0, 2) * 1.2 ** octv * rng.choice([0.2, 1.0, 3.0])
            kf["keys"]["x"][k] = f32(fx * c[0] / c[2] + cx + noise[0])
            kf["keys"]["y"][k] = f32(fy * c[1] / c[2] + cy + noise[1])
            kf["keys"]["octave"][k] = octv
            kf["desc"][k] = _flip(rng, base, int(rng.choice([0, 5, 20])))
            sd["world"][k] = (T[0].astype(np.float64).T @ (c - T[1].astype(np.float64))).astype(f32)
            sd["desc"][k] = _flip(rng, base, int(rng.choice([0, 10, 40, 75, 95, 110, 140])))
            sd["has"][k] = rng.random() < 0.9
        # PredictScale sees the distance in the OTHER camera's frame
        lv = octv - rng.uniform(0.1, 0.9) + int(rng.choice([0, 0, 0, 0, 1, -2]))
        a["mf"][k] = f32(np.linalg.norm(c2) * 1.2 ** lv)
        b["mf"][k] = f32(np.linalg.norm(c1) * 1.2 ** lv)
    for kf, sd in ((kf1, a), (kf2, b)):                                              # unrelated MapPoints on some of the other keys
        R, t = kf["Rcw"].astype(np.float64), kf["tcw"].astype(np.float64)
        for k in list(range(8)) + list(range(8 + n_common, n)):
            z = rng.uniform(1.5, 12.0) * (-1 if rng.random() < 0.05 else 1)
            c = np.array([(kf["keys"]["x"][k] - cx) / fx * z, (kf["keys"]["y"][k] - cy) / fy * z, z])
            sd["world"][k] = (R.T @ (c - t)).astype(f32)
            sd["mf"][k] = f32(abs(z) * 1.2 ** rng.uniform(0, 7))
            sd["has"][k] = rng.random() < 0.5

    def pts(sd):
        mf = sd["mf"]
        mx, mn = (f32(1.2) * mf).astype(f32), (f32(0.8) * (mf / f32(1.2 ** 7))).astype(f32)
        far = rng.random(len(mf)) < 0.04
        mx[far] = f32(0.5)
        return sd["world"], mx, mn, mf, sd["desc"]
    T = dict(R1w=kf1["Rcw"], t1w=kf1["tcw"], R2w=kf2["Rcw"], t2w=kf2["tcw"], sR12=sR12, t12=t12f, sR21=sR21, t21=t21, s12=f32(s12),
             R12=R12.astype(f32))
    return kf1, kf2, pts(a), pts(b), a["has"], b["has"], T
