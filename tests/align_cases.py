"""Constructed inputs for SparseImgAlign (k_sia_precompute / k_sia_run, orb_ygz_slam_amd/csrc/align_kernels.hip; the oracle: oracle/oracle_align.cpp).
No GPU and no extractor: every image is a closed formula (a sum of sinusoids rounded to 8 bits), every keypoint is placed by hand.

Base geometry: level 0 is 96 x 72, four levels of round(w * inv[l]) with inv[l] the float products of 1 / 1.2; fx = fy = 80, cx = 48, cy = 36; the
current frame is the formula shifted by (0.6, -0.4) px (scaled per level); 63 features on a grid of steps 9.5 x 8.25 from (10, 10); world points
are the keypoints' back-projections at depths in [2, 2.5]; identity poses.  ygzf_sia_run takes each level's size and image separately, so a case
may hand in any pyramid: that is how a level is cropped (a patch that is visible at a coarser level and leaves a finer one's border -- the
"stale" patch: the reference keeps the coarser patch under a zeroed Jacobian) or made 7 or 8 columns wide.

A case is a dict: name, family, keys, world, ref_T, cur_T, ref_pyr, cur_pyr, inv, cam, max_level, min_level, mp_valid, outlier (or None),
expect_ret (or None), twin (name of the case whose answer must differ from this one's, or None), stale ({level: indices} the case claims) and
reach(case, answers) -> None or a message.  `answers` is what run_oracle returns.

Gate cases (family ref_gate / cur_gate / unstaged) hand in the SAME image for both frames, so residuals are zero up to rounding, the first
iteration converges, and `ret` is exactly the number of features that pass both gates: expect_ret comes from gates_pass, a float32 model of the
two border tests written from the reference (src/SparseImageAlign.cc:73-77, :160-166), and a gate that is off by one changes an integer.
  ref_gate  the decisive keypoint sits on u_i = 3 | 2 | w - 4 | w - 3 (or v) of the reference level: 3.0, 2.99, w - 4 + 0.99 and w - 3.0 at level 0,
            the closest float on either side at level 2; its depth is one at which the back-projection projects back onto the same side
  cur_gate  the current level is the reference level without its outer 5 columns and 4 rows, the current pose is the translation that
            accounts for it (all points at depth 2), and the decisive keypoint projects to the closest float on either side of the gate
Each is a single-level run (level 0 and level 2) so that no gate case is a stale case too.

The other families: stale (a level cropped in both frames; each case has a twin without its stale features), count (stale_a repeated under a
jitter to 1024 / 1025 / 1755 / 1756 / 1800 features), negative_depth, narrow (level 3 handed in 7 and 8 columns wide), unstaged (one level of
509 x 331, gate case), rollback.  Their builders say what each is made of.

Limits every case's reach asserts (common_limits): projected coordinates below 2^20 in magnitude, |z| >= 0.05 in the current camera, final H
with an fp64 condition number of at most 1e4.  Rank-deficient systems and coordinates near the int range are out of scope here."""
import functools

import numpy as np

from orb_ygz_slam_amd.capi import KP_DTYPE

F32 = np.float32
W0, H0, NLEVELS = 96, 72, 4
CAM = dict(fx=80.0, fy=80.0, cx=48.0, cy=36.0)
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], F32)
N_ITER = 10
BORDER = 3


def inv_scale(n=NLEVELS):
    inv = np.ones(n, F32)
    for l in range(1, n):
        inv[l] = inv[l - 1] * F32(1.0 / 1.2)
    return inv


INV = inv_scale()
SIZES = [(int(round(W0 * float(INV[l]))), int(round(H0 * float(INV[l])))) for l in range(NLEVELS)]   # (96, 72) (80, 60) (67, 50) (56, 42)


def formula(X, Y):
    """the scene, over level-0 coordinates (float64 arrays) -> uint8"""
    v = 128.0 + 42.0 * np.sin(0.23 * X + 0.4) + 36.0 * np.sin(0.19 * Y + 1.1) + 24.0 * np.sin(0.11 * X + 0.14 * Y + 2.0) + 16.0 * np.sin(0.31 * X - 0.27 * Y)
    return np.clip(np.floor(v + 0.5), 0, 255).astype(np.uint8)


def level_image(level, w=None, h=None, shift=(0.0, 0.0), x0=0, y0=0, inv=INV):
    """level `level` of the scene shifted by `shift` level-0 pixels: columns x0 .. x0 + w - 1, rows y0 .. y0 + h - 1 of it"""
    w = SIZES[level][0] if w is None else w
    h = SIZES[level][1] if h is None else h
    x, y = np.meshgrid(np.arange(x0, x0 + w, dtype=np.float64), np.arange(y0, y0 + h, dtype=np.float64))
    return np.ascontiguousarray(formula(x / float(inv[level]) + shift[0], y / float(inv[level]) + shift[1]))


SHIFT = (0.6, -0.4)


def pyramid(shift=(0.0, 0.0), widths=None):
    """widths: {level: columns} crops a level on the right"""
    return [level_image(l, w=(widths or {}).get(l), shift=shift) for l in range(NLEVELS)]


def make_keys(xy):
    xy = np.asarray(xy, F32).reshape(-1, 2)
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["angle"], k["class_id"] = 31.0, -1.0, -1
    return k


def backproject(xy, depth, cam=CAM):
    xy = np.asarray(xy, F32).reshape(-1, 2)
    z = np.asarray(depth, F32)
    return np.stack([(xy[:, 0] - F32(cam["cx"])) / F32(cam["fx"]) * z, (xy[:, 1] - F32(cam["cy"])) / F32(cam["fy"]) * z, z * np.ones(len(xy), F32)], -1).astype(F32)


def grid_xy():
    return np.array([(10 + 9.5 * i, 10 + 8.25 * j) for j in range(7) for i in range(9)], F32)   # 63 features


def grid_depth(n):
    return (2.0 + 0.5 * ((np.arange(n) * 37) % 64) / 63.0).astype(F32)


# ---- the float32 model of the two gates -----------------------------------------------------------------------------------------------------------
def ref_coords(keys, scale):
    return (keys["x"].astype(F32) * F32(scale)).astype(F32), (keys["y"].astype(F32) * F32(scale)).astype(F32)


def gate(u, v, w, h):
    """both border tests on float32 coordinates (floor, then the integer comparisons)"""
    ui, vi = np.floor(u.astype(np.float64)), np.floor(v.astype(np.float64))
    return (ui - BORDER >= 0) & (vi - BORDER >= 0) & (ui + BORDER < w) & (vi + BORDER < h)


def ref_pass(case, level):
    u, v = ref_coords(case["keys"], case["inv"][level])
    ok = gate(u, v, case["ref_pyr"][level].shape[1], case["ref_pyr"][level].shape[0])
    if case["mp_valid"] is not None:
        ok &= case["mp_valid"] != 0
    if case["outlier"] is not None:
        ok &= case["outlier"] == 0
    return ok


def quat_rotate(q, v):
    """Eigen's _transformVector in float32, as the oracle and the kernel write it"""
    q = np.asarray(q, F32)
    uv = np.stack([q[1] * v[:, 2] - q[2] * v[:, 1], q[2] * v[:, 0] - q[0] * v[:, 2], q[0] * v[:, 1] - q[1] * v[:, 0]], -1).astype(F32)
    uv = (uv + uv).astype(F32)
    c = np.stack([q[1] * uv[:, 2] - q[2] * uv[:, 1], q[2] * uv[:, 0] - q[0] * uv[:, 2], q[0] * uv[:, 1] - q[1] * uv[:, 0]], -1).astype(F32)
    return ((v + q[3] * uv).astype(F32) + c).astype(F32)


def project(case, level, T7):
    """current-level coordinates of every feature under T_cur_from_ref = T7 (the reference pose of every case is the identity), float32 in the kernel's
    expression order: fx * x / z + cx, then * scale.  -> u, v, z"""
    assert np.array_equal(case["ref_T"], IDENT)
    T7 = np.asarray(T7, F32)
    xc = (quat_rotate(T7[:4], case["world"].astype(F32)) + T7[4:]).astype(F32)
    cam = case["cam"]
    with np.errstate(all="ignore"):
        ucx = ((F32(cam["fx"]) * xc[:, 0]).astype(F32) / xc[:, 2]).astype(F32) + F32(cam["cx"])
        ucy = ((F32(cam["fy"]) * xc[:, 1]).astype(F32) / xc[:, 2]).astype(F32) + F32(cam["cy"])
        s = F32(case["inv"][level])
        return (ucx.astype(F32) * s).astype(F32), (ucy.astype(F32) * s).astype(F32), xc[:, 2]


def cur_pass(case, level, T7):
    u, v, _ = project(case, level, T7)
    return gate(u, v, case["cur_pyr"][level].shape[1], case["cur_pyr"][level].shape[0])


def gates_pass(case, level, T7):
    return ref_pass(case, level) & cur_pass(case, level, T7)


def stale_sets(case):
    """{level: indices visible at a coarser level of the run that fail this level's reference gate}"""
    seen = np.zeros(len(case["keys"]), bool)
    out = {}
    for level in range(case["max_level"], case["min_level"] - 1, -1):
        ok = ref_pass(case, level)
        st = np.nonzero(seen & ~ok)[0]
        if len(st):
            out[level] = [int(i) for i in st]
        seen |= ok
    return out


# ---- running a case ---------------------------------------------------------------------------------------------------------------------------------
def oracle_args(case):
    return (case["keys"], case["world"], case["ref_T"], case["ref_pyr"], case["cur_T"], case["cur_pyr"], case["inv"], case["cam"], case["max_level"], case["min_level"], N_ITER)


def run_oracle(oracle, case, device_order=False, n_iter=None, levels=None):
    a = list(oracle_args(case))
    if n_iter is not None:
        a[10] = n_iter
    if levels is not None:
        a[8], a[9] = levels
    return oracle.sparse_img_align(*a, mp_valid=case["mp_valid"], outlier=case["outlier"], device_order=device_order)


def run_device(ex, case):
    from orb_ygz_slam_amd import make_camera
    cam = make_camera(W0, H0, case["cam"]["fx"], case["cam"]["fy"], case["cam"]["cx"], case["cam"]["cy"])
    return ex.sia_run(cam, case["keys"], case["world"], case["ref_T"], case["ref_pyr"], case["cur_T"], case["cur_pyr"], case["inv"], case["max_level"], case["min_level"], N_ITER,
                      mp_valid=case["mp_valid"], outlier=case["outlier"])


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).reshape(-1).view(np.uint32)


def same_bits(a, b):
    """ret, SE3, info and H bit for bit"""
    return a[0] == b[0] and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a[1:], b[1:]))


def T_start(case):
    """T_cur_from_ref of the first iteration (the reference pose is the identity)"""
    return np.asarray(case["cur_T"], F32)


def common_limits(case, ans):
    """the limits of every case, at the first and at the final pose: None or a message"""
    ret, T, info, H = ans
    for T7 in (T_start(case), T):
        for level in range(case["min_level"], case["max_level"] + 1):
            u, v, z = project(case, level, T7)
            if not (np.abs(u).max() < 2 ** 20 and np.abs(v).max() < 2 ** 20):
                return "a projected coordinate reaches 2^20"
            if not np.abs(z).min() >= 0.05:
                return "|z| below 0.05 in the current camera"
    cond = np.linalg.cond(np.asarray(H, np.float64))
    if not cond <= 1e4:
        return "cond(H) = %.3g" % cond
    if case["expect_ret"] is not None and not np.all(np.isfinite(T)):
        return "SE3 not finite"
    return None


def _case(name, family, xy, depth, ref_pyr, cur_pyr, levels, cur_T=IDENT, mp_valid=None, outlier=None, expect_ret=None, twin=None, reach=None, world=None, decisive=(), cam=CAM):
    keys = make_keys(xy)
    c = dict(name=name, family=family, keys=keys, world=backproject(xy, depth, cam) if world is None else np.ascontiguousarray(world, F32), ref_T=IDENT.copy(),
             cur_T=np.asarray(cur_T, F32).copy(), ref_pyr=ref_pyr, cur_pyr=cur_pyr, inv=INV.copy(), cam=dict(cam), max_level=levels[0], min_level=levels[1],
             mp_valid=None if mp_valid is None else np.asarray(mp_valid, np.uint8), outlier=None if outlier is None else np.asarray(outlier, np.uint8),
             expect_ret=expect_ret, twin=twin, decisive=list(decisive))
    c["stale"] = stale_sets(c)
    c["reach"] = reach or (lambda case, ans: None)
    return c


# ---- gate cases ---------------------------------------------------------------------------------------------------------------------------------------
POSITIONS = ["u3", "u2", "uw4", "uw3", "v3", "v2", "vh4", "vh3"]      # u_i = 3, u_i = 2, u_i = w - 4, u_i = w - 3 and the same for v
PASSES = {"u3": True, "u2": False, "uw4": True, "uw3": False, "v3": True, "v2": False, "vh4": True, "vh3": False}


def _neighbours(f, target, lo, hi):
    """f: monotone float32 -> float32.  The smallest float32 x in [lo, hi] with f(x) >= target, and the float before it."""
    lo, hi = F32(lo), F32(hi)
    assert f(lo) < target <= f(hi)
    while np.nextafter(lo, F32(np.inf)) < hi:
        mid = F32((np.float64(lo) + np.float64(hi)) / 2)
        if mid <= lo or mid >= hi:
            break
        if f(mid) >= target:
            hi = mid
        else:
            lo = mid
    return hi, lo


def _gate_coord(pos, f, w, h, level):
    """the level-0 keypoint coordinate whose image under f (the coordinate the gate floors) is the closest float on the stated side of the gate.
    (Level 0 on the reference side does not come here: its scale is 1 and the cases use 3.0, 2.99, n - 4 + 0.99 and n - 3.0.)"""
    n = w if pos[0] == "u" else h
    kind = pos[1:]
    if kind in ("3", "2"):
        at, below = _neighbours(f, 3.0, 0.0, 40.0)
        return at if kind == "3" else below
    at, below = _neighbours(f, float(n - 3), 0.0, 200.0)
    return below if kind in ("w4", "h4") else at


def _gate_reach(level):
    def reach(case, ans):
        T0 = T_start(case)
        rp, cp = ref_pass(case, level), cur_pass(case, level, T0)
        u, v = ref_coords(case["keys"], case["inv"][level]) if case["family"] != "cur_gate" else project(case, level, T0)[:2]
        wl, hl = (case["ref_pyr"] if case["family"] != "cur_gate" else case["cur_pyr"])[level].shape[::-1]
        for i, pos in case["decisive"]:
            c, n = (u[i], wl) if pos[0] == "u" else (v[i], hl)
            want = {"3": 3, "2": 2, "w4": n - 4, "h4": n - 4, "w3": n - 3, "h3": n - 3}[pos[1:]]
            if int(np.floor(c)) != want:
                return "feature %d (%s): floor(%r) is not %d" % (i, pos, c, want)
            # only the gate the case is about decides: the other frame's gate passes, and so does the other axis
            if case["family"] == "cur_gate" and not rp[i]:
                return "feature %d (%s) fails the reference gate" % (i, pos)
            if (rp[i] and cp[i]) != PASSES[pos]:
                return "feature %d (%s): passes = %s" % (i, pos, rp[i] and cp[i])
        if int(ans[2][0]) != 1:
            return "%d iterations: the identical images did not converge at once" % int(ans[2][0])
        return common_limits(case, ans)
    return reach


def _ref_gate_cases():
    out = []
    for level in (0, 2):
        w, h = SIZES[level]
        img = level_image(level)
        pyr = [img if l == level else level_image(l) for l in range(NLEVELS)]
        s = INV[level]
        f = lambda x: F32(F32(x) * s)
        gxy, gz = grid_xy(), grid_depth(63)

        def build(name, positions, twin):
            xy, z, dec = list(gxy), list(gz), []
            for pos in positions:
                if level == 0:
                    n = w if pos[0] == "u" else h
                    cgate = {"3": 3.0, "2": 2.99, "w4": n - 4 + 0.99, "h4": n - 4 + 0.99, "w3": n - 3.0, "h3": n - 3.0}[pos[1:]]
                else:
                    cgate = _gate_coord(pos, f, w, h, level)
                other = F32(30.5 + 2.0 * POSITIONS.index(pos))
                p = (cgate, other) if pos[0] == "u" else (other, cgate)
                # a depth at which the back-projection projects back onto the same side (the current gate must not decide)
                for d in (2.0, 2.25, 2.5, 2.125, 2.375):
                    probe = _case("probe", "ref_gate", [p], [d], pyr, pyr, (level, level))
                    if not PASSES[pos] or gates_pass(probe, level, IDENT)[0]:
                        break
                dec.append((len(xy), pos))
                xy.append(p)
                z.append(d)
            c = _case(name, "ref_gate", xy, z, pyr, pyr, (level, level), twin=twin, reach=_gate_reach(level), decisive=dec)
            c["expect_ret"] = int(gates_pass(c, level, IDENT).sum())
            return c
        out.append(build("ref_gate_L%d_base" % level, [], None))
        for pos in POSITIONS:
            sibling = POSITIONS[POSITIONS.index(pos) - 1]
            out.append(build("ref_gate_L%d_%s" % (level, pos), [pos], "ref_gate_L%d_base" % level if PASSES[pos] else "ref_gate_L%d_%s" % (level, sibling)))
        out.append(build("ref_gate_L%d_all" % level, POSITIONS, "ref_gate_L%d_base" % level))
    return out


def _cur_gate_cases():
    out = []
    DX, DY, Z = 5, 4, 2.0
    for level in (0, 2):
        w, h = SIZES[level]
        wc, hc = w - 2 * DX, h - 2 * DY
        ref = level_image(level)
        cur = np.ascontiguousarray(ref[DY:DY + hc, DX:DX + wc])
        rp = [ref if l == level else level_image(l) for l in range(NLEVELS)]
        cp = [cur if l == level else level_image(l) for l in range(NLEVELS)]
        s = float(INV[level])
        T = IDENT.copy()
        T[4], T[5] = F32(-DX * Z / (CAM["fx"] * s)), F32(-DY * Z / (CAM["fy"] * s))
        gxy = grid_xy()

        def proj(axis):
            def f(x):
                p = (F32(x), F32(40.0)) if axis == "u" else (F32(40.0), F32(x))
                probe = _case("probe", "cur_gate", [p], [Z], rp, cp, (level, level), cur_T=T)
                return project(probe, level, T)[0 if axis == "u" else 1][0]
            return f

        def build(name, positions, twin):
            xy, dec = list(gxy), []
            for pos in positions:
                cgate = _gate_coord(pos, proj(pos[0]), wc, hc, level)
                other = F32(36.5 + 1.5 * POSITIONS.index(pos))
                p = (cgate, other) if pos[0] == "u" else (other, cgate)
                dec.append((len(xy), pos))
                xy.append(p)
            c = _case(name, "cur_gate", xy, np.full(len(xy), Z, F32), rp, cp, (level, level), cur_T=T, twin=twin, reach=_gate_reach(level), decisive=dec)
            c["expect_ret"] = int(gates_pass(c, level, T).sum())
            return c
        out.append(build("cur_gate_L%d_base" % level, [], None))
        for pos in POSITIONS:
            sibling = POSITIONS[POSITIONS.index(pos) - 1]
            out.append(build("cur_gate_L%d_%s" % (level, pos), [pos], "cur_gate_L%d_base" % level if PASSES[pos] else "cur_gate_L%d_%s" % (level, sibling)))
        out.append(build("cur_gate_L%d_all" % level, POSITIONS, "cur_gate_L%d_base" % level))
    return out


# ---- stale patches --------------------------------------------------------------------------------------------------------------------------------------
def _stale_reach(want_levels):
    def reach(case, ans):
        st = case["stale"]
        if sorted(st) != sorted(want_levels):
            return "stale at levels %s, not %s" % (sorted(st), sorted(want_levels))
        if any(len(v) == 0 for v in st.values()):
            return "a level without a stale feature"
        live = [i for i in set().union(*st.values()) if (case["mp_valid"] is None or case["mp_valid"][i]) and (case["outlier"] is None or not case["outlier"][i])]
        if not live:
            return "every stale feature is excluded"
        return common_limits(case, ans)
    return reach


def _without(case, drop, name):
    keep = np.setdiff1d(np.arange(len(case["keys"])), np.asarray(sorted(drop), int))
    c = dict(case, name=name, keys=case["keys"][keep].copy(), world=case["world"][keep].copy(), twin=None, decisive=[],
             mp_valid=None if case["mp_valid"] is None else case["mp_valid"][keep].copy(), outlier=None if case["outlier"] is None else case["outlier"][keep].copy())
    c["stale"] = stale_sets(c)
    c["reach"] = lambda cs, ans: ("the twin still has stale features" if cs["stale"] else common_limits(cs, ans))
    return c


def _stale_cases():
    out = []
    gxy = grid_xy()

    def add(name, xy, widths, levels, want, **kw):
        z = grid_depth(len(xy))
        c = _case(name, "stale", xy, z, pyramid(widths=widths), pyramid(SHIFT, widths=widths), levels, twin=name + "_twin", reach=_stale_reach(want), **kw)
        out.append(c)
        out.append(_without(c, set().union(*c["stale"].values()), name + "_twin"))
        return c
    # (a) level 0 of both frames has 60 columns: the column x = 57.5 (u_i + 3 = 60) is stale there, and its content lies at 56.9 in the current frame
    a = add("stale_a", gxy, {0: 60}, (2, 0), [0])
    # (b) only level 1 is cropped (50 columns): visible at level 2, stale at level 1, rebuilt at level 0.  x = 56.7: 47.25 at level 1 (47 + 3 = 50), 46.75 in the current frame
    xb = np.concatenate([gxy, np.array([(56.7, 14.0), (56.6, 31.5), (56.8, 52.0)], F32)])
    add("stale_b", xb, {1: 50}, (2, 0), [1])
    # (c) visible at level 3, stale at levels 2 (43 columns) and 1 (51 columns): x = 57.7 is 40.07 / 48.08 there and 39.65 / 47.58 in the current frame
    xc = np.concatenate([gxy, np.array([(57.7, 12.5), (57.75, 33.0), (57.65, 50.5)], F32)])
    add("stale_c", xc, {2: 43, 1: 51}, (3, 1), [1, 2])
    # (d) = (a) with exclusion flags on some stale and some live features
    st = a["stale"][0]
    valid, outl = np.ones(len(gxy), np.uint8), np.zeros(len(gxy), np.uint8)
    valid[[st[0], 3, 20]] = 0
    outl[[st[1], 11, 40]] = 1
    add("stale_d", gxy, {0: 60}, (2, 0), [0], mp_valid=valid, outlier=outl)
    return out


N_CLASSES = [1024, 1025, 1755, 1756, 1800]


def _count_cases():
    """stale case (a) with its features repeated under a sub-pixel jitter: the register form up to 1024 features and the cache form beyond,
    Jacobian terms in LDS up to 1755 and rebuilt beyond"""
    out = []
    gxy = grid_xy()
    for n in N_CLASSES:
        rng = np.random.default_rng(n)
        xy = np.concatenate([gxy] * (-(-n // len(gxy))))[:n].copy()
        xy += (rng.uniform(-0.2, 0.2, xy.shape) * (np.arange(n) >= len(gxy))[:, None]).astype(F32)
        z = (2.0 + 0.5 * rng.uniform(size=n)).astype(F32)
        out.append(_case("count_%d" % n, "count", xy, z, pyramid(widths={0: 60}), pyramid(SHIFT, widths={0: 60}), (2, 0), reach=_stale_reach([0])))
    return out


# ---- the rest ---------------------------------------------------------------------------------------------------------------------------------------------
def _negative_depth_cases():
    gxy, gz = grid_xy(), grid_depth(63)
    xy = np.concatenate([gxy, np.array([(33.0, 27.0), (61.0, 44.0)], F32)])
    z = np.concatenate([gz, np.array([-2.2, -2.4], F32)])

    def reach(case, ans):
        zc = project(case, 0, ans[1])[2]
        if not ((zc[63:] < 0).all() and gates_pass(case, 0, ans[1])[63:].all()):
            return "the two points behind the camera do not pass the gates"
        return common_limits(case, ans)
    c = _case("negative_depth", "negative_depth", xy, z, pyramid(), pyramid(SHIFT), (2, 0), expect_ret=65, twin="negative_depth_twin", reach=reach)
    t = _case("negative_depth_twin", "negative_depth", gxy, gz, pyramid(), pyramid(SHIFT), (2, 0), expect_ret=63, reach=common_limits)
    return [c, t]


NARROW_SHIFT = (0.25, -0.4)


def _narrow_cases():
    """level 3 handed in 7 (8) columns wide and 42 rows tall, a run on that level alone: u_i can only be 3 (3 or 4)"""
    out = []
    s3 = float(INV[3])
    for w, us in ((7, [3.45, 3.6, 3.5, 3.7]), (8, [3.45, 4.55, 3.6, 4.4])):
        n = 14
        xy = np.array([(us[i % 4] / s3, (5.0 + 2.4 * i) / s3) for i in range(n)], F32)
        z = (2.0 + 2.0 * ((np.arange(n) * 5) % n) / (n - 1.0)).astype(F32)
        rp = [level_image(l) if l != 3 else level_image(3, w=w) for l in range(NLEVELS)]
        cp = [level_image(l, shift=NARROW_SHIFT) if l != 3 else level_image(3, w=w, shift=NARROW_SHIFT) for l in range(NLEVELS)]

        def reach(case, ans, w=w):
            ok = gates_pass(case, 3, T_start(case)) & gates_pass(case, 3, ans[1])
            if ok.sum() < 12 or len(set(case["world"][ok, 2].tolist())) < 12:
                return "%d features pass both gates" % ok.sum()
            ui = np.floor(ref_coords(case["keys"], case["inv"][3])[0][ok])
            if sorted(set(ui.tolist())) != ([3.0] if w == 7 else [3.0, 4.0]):
                return "u_i = %s" % sorted(set(ui.tolist()))
            return common_limits(case, ans)
        out.append(_case("width_%d" % w, "narrow", xy, z, rp, cp, (3, 3), reach=reach))
    return out


UNSTAGED_W, UNSTAGED_H = 509, 331
UNSTAGED_CAM = dict(fx=400.0, fy=400.0, cx=254.5, cy=165.5)      # (the base camera would look at this level from far off its axis)


def _unstaged_case():
    """one level of 509 x 331 = 168 479 bytes, more than a CU's LDS (never staged), at a pitch of 1 mod 4; both frames the same image"""
    w, h = UNSTAGED_W, UNSTAGED_H
    img = level_image(0, w=w, h=h)
    pyr = [img] + [level_image(l) for l in range(1, NLEVELS)]
    xy = [(20 + 52.5 * i, 18 + 37.25 * j) for j in range(9) for i in range(8)]     # 72 on a grid
    dec = []
    for pos in POSITIONS:
        n = w if pos[0] == "u" else h
        cgate = {"3": 3.0, "2": 2.99, "w4": n - 4 + 0.99, "h4": n - 4 + 0.99, "w3": n - 3.0, "h3": n - 3.0}[pos[1:]]
        other = F32(101.5 + 23.0 * POSITIONS.index(pos))
        dec.append((len(xy), pos))
        xy.append((cgate, other) if pos[0] == "u" else (other, cgate))
    z = grid_depth(len(xy)).copy()
    for i, pos in dec:          # a depth at which the back-projection projects back onto the same side
        for d in (2.0, 2.25, 2.5, 2.125, 2.375, 2.0625):
            z[i] = d
            probe = _case("probe", "unstaged", [xy[i]], [d], pyr, pyr, (0, 0), cam=UNSTAGED_CAM)
            if not PASSES[pos] or gates_pass(probe, 0, IDENT)[0]:
                break
    c = _case("unstaged_509x331", "unstaged", xy, z, pyr, pyr, (0, 0), reach=_gate_reach(0), decisive=dec, cam=UNSTAGED_CAM)
    c["expect_ret"] = int(gates_pass(c, 0, IDENT).sum())
    return [c]


def _rollback_cases():
    """A level that takes a step back.  On these smooth images Gauss-Newton from a wrong start undershoots and never raises chi2, so the rise is built:
    three MapPoints that belong elsewhere (their keypoints' patches do not match where they project) lie at v = 2.8 of the current level 2 at the
    start, outside the border; the first step moves every projection down by a quarter pixel, they enter, and the mean residual multiplies.  The
    second linearisation is refused and the level ends on its starting pose.  One run on level 2 alone (answer: the starting pose, two
    linearisations) and one that goes on to level 0."""
    s2 = float(INV[2])
    gxy, gz = grid_xy(), grid_depth(63)
    keys_xy = np.array([(30.0, 30.0), (50.0, 41.0), (70.0, 25.0)], F32)
    target = np.array([(20.0 / s2, 2.8 / s2), (33.0 / s2, 2.8 / s2), (45.0 / s2, 2.8 / s2)], F32)
    world = np.concatenate([backproject(gxy, gz), backproject(target, np.array([2.2, 2.3, 2.1], F32))])

    def reach(case, ans):
        levels = case["max_level"] - case["min_level"] + 1
        if not int(ans[2][0]) < N_ITER * levels:
            return "%d iterations" % int(ans[2][0])
        if cur_pass(case, 2, T_start(case))[63:].any():
            return "the misplaced points pass the current gate at the start"
        if case["min_level"] == 2 and not (np.array_equal(bits(ans[1]), bits(T_start(case))) and int(ans[2][0]) == 2 and ans[0] == 66):
            return "level 2 alone does not end on its starting pose after two linearisations"
        return common_limits(case, ans)
    return [_case("rollback" if lv[1] == 0 else "rollback_level2", "rollback", np.concatenate([gxy, keys_xy]), None, pyramid(), pyramid(SHIFT), lv, world=world, reach=reach)
            for lv in ((2, 0), (2, 2))]


def rolled_back(oracle, case):
    """(level, k) of the first rollback -- iteration k of a level took back iteration k - 1's step because chi2 rose by more than a fifth -- or None.
    Seen from outside: with n_iter = k on that level alone the run returns the pose that n_iter = k - 2 returns (NLSSolver_impl.hpp:52-59 puts
    old_model back, the pose from before the last accepted step), having counted k linearisations."""
    c = dict(case)
    for level in range(case["max_level"], case["min_level"] - 1, -1):
        poses = [np.asarray(c["cur_T"], F32)]
        for k in range(1, N_ITER + 1):
            ret, T, info, H = run_oracle(oracle, c, n_iter=k, levels=(level, level))
            if int(info[0]) < k:
                break                       # converged
            if k >= 2 and np.array_equal(bits(T), bits(poses[k - 2])) and not np.array_equal(bits(T), bits(poses[k - 1])):
                return level, k
            poses.append(T.copy())
        c["cur_T"] = run_oracle(oracle, c, levels=(level, level))[1].copy()     # (the reference pose is the identity: T_cur_from_ref is the current pose)
    return None


@functools.lru_cache(maxsize=None)
def cases():
    out = _ref_gate_cases() + _cur_gate_cases() + _stale_cases() + _count_cases() + _negative_depth_cases() + _narrow_cases() + _unstaged_case() + _rollback_cases()
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    assert all(c["twin"] is None or c["twin"] in names for c in out)
    return out


def by_name():
    return {c["name"]: c for c in cases()}
