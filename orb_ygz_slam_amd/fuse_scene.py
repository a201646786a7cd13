"""Seeded synthetic keyframes and MapPoints for ORBmatcher::Fuse (ygzf_fuse_candidates): used by tests/test_gpu_fuse.py and tools/fuse_rate.py.
Pure numpy, deterministic per generator."""
import numpy as np

from .capi import EUROC, KP_DTYPE, make_camera

f32 = np.float32


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)


def make_kf(rng, w, h, n, nlevels, scale, R, t, mbf=0.0, stereo_frac=0.0, dup_frac=0.05):
    """A keyframe: random keys (a few duplicated with their descriptor: equal distances), mvuRight for a fraction when mbf > 0."""
    keys = np.zeros(n, KP_DTYPE)
    keys["x"] = rng.uniform(0, w, n).astype(f32)
    keys["y"] = rng.uniform(0, h, n).astype(f32)
    keys["x"][:8] = np.array([0, w - 0.01, 0.2, w - 0.3, 1.0, w - 1.0, 0.5, w - 0.5], f32)   # keys on the borders of the grid
    keys["y"][:8] = np.array([0, h - 0.01, h - 0.2, 0.3, 1.0, h - 1.0, h - 0.5, 0.5], f32)
    keys["octave"] = rng.integers(0, nlevels, n)
    keys["size"] = 31
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    nd = int(n * dup_frac)
    src = rng.integers(8, n, nd)
    dst = rng.integers(8, n, nd)
    keys[dst] = keys[src]
    desc[dst] = desc[src]
    sf = (scale ** np.arange(nlevels)).astype(f32)
    for l in range(1, nlevels):
        sf[l] = f32(sf[l - 1] * f32(scale))
    ur = None
    if mbf > 0:
        ur = np.full(n, -1, f32)
        st = rng.random(n) < stereo_frac
        ur[st] = (keys["x"][st] - rng.uniform(2, 40, st.sum())).astype(f32)
    R = np.asarray(R, f32)
    t = np.asarray(t, f32)
    Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(f32)
    cam = make_camera(w, h, mbf=mbf)
    inv_sigma2 = (f32(1) / (sf * sf)).astype(f32)
    return dict(keys=keys, desc=desc, u_right=ur, scale_factors=sf, inv_level_sigma2=inv_sigma2, cam=cam, Rcw=R, tcw=t, Ow=Ow,
                log_scale_factor=f32(np.log(f32(scale))), w=w, h=h, nlevels=nlevels)


def make_points(rng, kfs, P):
    """MapPoints seeded from keys of the keyframes (projection near the key, descriptor = the key's with a few flipped bits), plus points behind
    the camera, outside the image, beyond the distance limits, at grazing view angles and at u == max_x exactly."""
    world = np.zeros((P, 3), f32)
    normal = np.zeros((P, 3), f32)
    mf = np.zeros(P, f32)
    desc = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    for i in range(P):
        kf = kfs[int(rng.integers(0, len(kfs)))]
        j = int(rng.integers(0, len(kf["keys"])))
        k = kf["keys"][j]
        sig = np.sqrt(1.0 / kf["inv_level_sigma2"][k["octave"]])
        off = rng.normal(0, 1.0, 2) * sig * rng.choice([0.3, 1.0, 2.4, 2.9])   # around the 5.99 / 7.8 gates
        z = rng.uniform(1.5, 12.0)
        xc = (k["x"] + off[0] - EUROC["cx"]) / EUROC["fx"] * z
        yc = (k["y"] + off[1] - EUROC["cy"]) / EUROC["fy"] * z
        pc = np.array([xc, yc, z])
        if rng.random() < 0.04:
            pc[2] = -pc[2]                                               # behind the camera
        R, t = kf["Rcw"].astype(np.float64), kf["tcw"].astype(np.float64)
        world[i] = (R.T @ (pc - t)).astype(f32)
        d = kf["desc"][j].copy()
        nflip = int(rng.choice([0, 3, 10, 25, 45, 49, 50, 51, 60, 120]))
        for b in rng.choice(256, nflip, replace=False):
            d[b // 8] ^= np.uint8(1 << (b % 8))
        desc[i] = d
        ow = kf["Ow"].astype(np.float64)
        v = world[i].astype(np.float64) - ow
        dist = np.linalg.norm(v)
        nv = v / dist
        if rng.random() < 0.08:                                          # near the 60 degree limit (cos 0.5) or beyond
            perp = np.cross(nv, [0.0, 0.0, 1.0])
            perp /= np.linalg.norm(perp)
            ang = np.deg2rad(rng.choice([59.99, 60.0, 60.01, 75.0]))
            nv = np.cos(ang) * nv + np.sin(ang) * perp
        normal[i] = nv.astype(f32)
        lvl = int(k["octave"]) + int(rng.choice([0, 0, 0, 0, 1, -1]))   # mostly the key's level; 0 / L-1 clamp from below / above
        if rng.random() < 0.1:
            lvl = int(rng.choice([-3, kf["nlevels"] + 2]))
        mf[i] = f32(dist * float(kf["scale_factors"][0]) * (1.2 ** lvl) * rng.uniform(0.9, 1.1))
    maxinv = (f32(1.2) * mf).astype(f32)
    mininv = (f32(0.8) * (mf / f32(1.2 ** 7))).astype(f32)
    far = rng.random(P) < 0.05
    maxinv[far] = f32(0.5)                                                # beyond the distance limits
    near = rng.random(P) < 0.05
    mininv[near] = f32(1e6)
    return world, normal, maxinv, mininv, mf, desc


def edge_point(kf, depth=2.0, exact=True):
    """A point of camera depth `depth` whose projection u is exactly max_x (exact) or the float just below it."""
    fx, cx, mx = f32(kf["cam"].fx), f32(kf["cam"].cx), f32(kf["cam"].max_x)
    z = f32(depth)
    invz = f32(1) / z
    X = f32((mx - cx) / fx * z)
    target = mx if exact else np.nextafter(mx, f32(0))
    for _ in range(4000):
        u = fx * (X * invz) + cx
        if u == target:
            break
        X = np.nextafter(X, f32(np.inf) if u < target else f32(-np.inf))
    pc = np.array([X, f32(kf["h"] / 2 - EUROC["cy"]) / f32(EUROC["fy"]) * z, z], np.float64)
    R, t = kf["Rcw"].astype(np.float64), kf["tcw"].astype(np.float64)
    return pc, (R.T @ (pc - t)).astype(f32)
