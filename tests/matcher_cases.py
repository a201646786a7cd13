"""Constructed inputs for the matcher (no GPU, no extractor): crowding, ties, thresholds and boundaries that keypoints out of the extractor
never produce.  cases() returns named cases as plain arrays for search_by_projection_last ("last", mode 0 of k_match_last),
search_by_projection_mappoints ("mappoints", mode 1), search_by_projection_kf ("kf", mode 2), search_for_initialization ("init", mode 3) and
search_by_bow ("bow"), and one for search_for_triangulation ("tri").  Descriptors are built to exact Hamming distances (chosen bits of a base are flipped), from a fixed seed.

The frame is 512 x 384 (grid cells of exactly 8 x 8 px: x * (64 / 512) is exact in float) and the camera fx = fy = 256, cx = 256, cy = 192, so
that with identity poses the unit-depth back-projection of (u, v) projects onto (u, v) exactly for coordinates that are multiples of 1/64:
a test can put a keypoint exactly on a window's edge.

Every case carries `reach`: a predicate over the inputs and the ORACLE's answer, evaluated on the CPU (tests/test_matcher_cases.py), that
proves the case is what its family claims; and `expect`: what ygzf_match_path_stats must report for it on the device (tests/test_gpu_match_cases.py).

run_oracle(O, case) / run_device(ex, case, oracle_result) call either side with the case's arrays; same(a, b, case) compares two answers."""
import numpy as np

from orb_ygz_slam_amd.capi import KP_DTYPE

W, H = 512, 384
CAM = dict(fx=256.0, fy=256.0, cx=256.0, cy=192.0)
NLEVELS = 8
TH_HIGH, TH_LOW = 100, 50


def scale_table():
    """ORBextractor's mvScaleFactor (float products; tests/test_matcher_cases.py checks it against the oracle's table)"""
    s = np.ones(NLEVELS, np.float32)
    for i in range(1, NLEVELS):
        s[i] = s[i - 1] * np.float32(1.2)
    return s


SF = scale_table()
I3, Z3 = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)


# ---- descriptors ---------------------------------------------------------------------------------------------------------------------------
def flip(d, bits):
    out = np.array(d, np.uint8).copy()
    for b in bits:
        out[int(b) >> 3] ^= np.uint8(1 << (int(b) & 7))
    return out


def ham(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def ham_matrix(A, B):
    """|A| x |B| Hamming distances"""
    A = np.ascontiguousarray(A, np.uint8).reshape(-1, 32)
    B = np.ascontiguousarray(B, np.uint8).reshape(-1, 32)
    if len(A) == 0 or len(B) == 0:
        return np.zeros((len(A), len(B)), np.int32)
    return np.unpackbits(A[:, None, :] ^ B[None, :, :], axis=2).sum(axis=2).astype(np.int32)


def make_keys(xy, octave=0, angle=0.0):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["octave"] = octave
    k["angle"] = angle
    k["size"] = 31.0
    k["response"] = 1.0
    k["class_id"] = -1
    return k


# ---- a scene of candidates (the current frame) and queries (Last keypoints / MapPoints / KeyFrame points) ------------------------------------------
class Scene:
    def __init__(self):
        self.c = dict(xy=[], oct=[], desc=[], ang=[], owner=[], ur=[])
        self.q = dict(xy=[], oct=[], desc=[], ang=[], obs=[], valid=[])

    def cand(self, xy, desc, octave=0, angle=0.0, owner=0, u_right=-1.0):
        self.c["xy"].append(xy); self.c["oct"].append(octave); self.c["desc"].append(desc); self.c["ang"].append(angle)
        self.c["owner"].append(owner); self.c["ur"].append(u_right)
        return len(self.c["xy"]) - 1

    def query(self, xy, desc, octave=0, angle=0.0, obs=1, valid=1):
        self.q["xy"].append(xy); self.q["oct"].append(octave); self.q["desc"].append(desc); self.q["ang"].append(angle)
        self.q["obs"].append(obs); self.q["valid"].append(valid)
        return len(self.q["xy"]) - 1

    def arrays(self):
        c, q = self.c, self.q
        ck = make_keys(np.array(c["xy"], np.float32).reshape(-1, 2), np.array(c["oct"], np.int32), np.array(c["ang"], np.float32))
        qk = make_keys(np.array(q["xy"], np.float32).reshape(-1, 2), np.array(q["oct"], np.int32), np.array(q["ang"], np.float32))
        return dict(cur_keys=ck, cur_desc=np.array(c["desc"], np.uint8).reshape(-1, 32), owner=np.array(c["owner"], np.uint8),
                    u_right=np.array(c["ur"], np.float32), q_keys=qk, q_desc=np.array(q["desc"], np.uint8).reshape(-1, 32),
                    obs=np.array(q["obs"], np.uint8), valid=np.array(q["valid"], np.uint8))


class Case:
    def __init__(self, name, family, fn, a, reach, expect=None, limit=False, none=False, ref_valid=None):
        self.name, self.family, self.fn, self.a, self.reach, self.limit, self.none = name, family, fn, a, reach, limit, none
        self.ref_valid = ref_valid             # queries the reference's own code may be given (None: all); see for_reference()
        self.expect = dict(expect or {})       # counter -> 0 | ">0"

    def __repr__(self):
        return "%s:%s" % (self.fn, self.name)


def for_reference(c):
    """The case as the reference's own code can take it.  SearchByProjection(Cur, KeyFrame) with ORBdist >= 256 writes mvpMapPoints[-1] for a
    query whose window holds keypoints but no acceptable one (src/ORBmatcher.cc:1431, undefined); the oracle and the device define "no match"
    there, so the answer for the remaining queries is the same and those queries are marked unusable for the reference alone."""
    if c.ref_valid is None:
        return c
    a = dict(c.a, valid=(c.a["valid"] & np.asarray(c.ref_valid, np.uint8)).astype(np.uint8))
    return Case(c.name, c.family, c.fn, a, c.reach, c.expect, c.limit, c.none)


def projected_case(name, family, fn, scene, radius, reach, expect=None, limit=False, none=False, check_level=False, check_ori=True, nnratio=0.8,
                   orb_dist=100, mono=True, tz=0.0, mb=0.0, mbf=0.0, stereo=False, ref_valid=None):
    """The same scene as the arguments of one of the three projection searches.  `radius`: the search radius of a level-0 query in pixels
    (last / kf: th = radius; mappoints: viewing cosine 1 -> RadiusByViewingCos 2.5, th = radius / 2.5)."""
    s = scene.arrays()
    a = dict(s, radius=float(radius), check_level=check_level, check_ori=check_ori, nnratio=nnratio, orb_dist=orb_dist, mono=mono, mb=mb, mbf=mbf,
             tcw=np.array([0, 0, tz], np.float32), stereo=stereo)
    qk = s["q_keys"]
    a["world"] = np.stack([(qk["x"] - np.float32(CAM["cx"])) / np.float32(CAM["fx"]), (qk["y"] - np.float32(CAM["cy"])) / np.float32(CAM["fy"]),
                           np.ones(len(qk), np.float32)], -1).astype(np.float32).reshape(-1, 3)
    a["th"] = float(radius) / 2.5 if fn == "mappoints" else float(radius)
    return Case(name, family, fn, a, reach, expect, limit, none, ref_valid)


def _cam(a):
    return dict(CAM, mb=a.get("mb", 0.0), mbf=a.get("mbf", 0.0))


def run_oracle(O, c):
    """-> the oracle's answer (or, inside `with O.reference_matcher():`, the reference's own code's) as a tuple"""
    a = c.a
    if c.fn == "last":
        return O.search_by_projection_last(a["cur_keys"], a["cur_desc"], SF, W, H, _cam(a), a["q_keys"], a["world"], a["q_desc"], I3, a["tcw"], I3, Z3,
                                           a["th"], a["mono"], a["check_level"], a["check_ori"], mp_valid=a["valid"], mp_has_obs=a["obs"],
                                           u_right=a["u_right"] if a["stereo"] else None, cur_owner=a["owner"])
    if c.fn == "mappoints":
        qk = a["q_keys"]
        kw = dict(mp_has_obs=a["obs"], owner=a["owner"])
        if a["stereo"]:
            kw.update(proj_xr=(qk["x"] - np.float32(a["mbf"])).astype(np.float32), u_right=a["u_right"])
        return O.search_by_projection_mappoints(a["cur_keys"], a["cur_desc"], SF, W, H, _cam(a), a["valid"], qk["x"], qk["y"], np.ones(len(qk), np.float32),
                                                qk["octave"], a["q_desc"], a["th"], a["check_level"], a["nnratio"], **kw)
    if c.fn == "kf":
        qk = a["q_keys"]
        dist = np.sqrt((a["world"].astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)).astype(np.float32)
        mf_max = (dist * SF[qk["octave"]]).astype(np.float32)      # PredictScale: the level the query was built with
        return O.search_by_projection_kf(a["cur_keys"], a["cur_desc"], SF, W, H, _cam(a), a["valid"], a["world"], (np.float32(1.2) * mf_max).astype(np.float32),
                                         (np.float32(0.8) * mf_max / SF[NLEVELS - 1]).astype(np.float32), mf_max, qk["angle"], a["q_desc"], I3, a["tcw"],
                                         np.log(np.float32(1.2)), a["th"], a["orb_dist"], a["check_ori"], owner=(a["owner"] != 0).astype(np.uint8))
    if c.fn == "init":
        return O.search_for_initialization(a["keys1"], a["desc1"], a["keys2"], a["desc2"], SF, W, H, CAM, a["prev"], a["window"], a["nnratio"], a["check_ori"])
    if c.fn == "bow":
        return O.search_by_bow(a["kf_off"], a["kf_idx"], a["f_off"], a["f_idx"], a["kf_valid"], a["kf_keys"], a["kf_desc"], a["f_keys"], a["f_desc"],
                               a["nnratio"], a["check_ori"])
    if c.fn == "tri":
        return O.search_for_triangulation(scale_factors2=SF, level_sigma2_2=(SF * SF).astype(np.float32), **a)
    raise KeyError(c.fn)


def run_device(ex, c, oracle_result=None):
    """-> the device's answer through orb_ygz_slam_amd.Extractor `ex` (kf: the host prologue's (valid, u, v, level) come from the oracle)"""
    from orb_ygz_slam_amd import make_camera
    a = c.a
    cam = make_camera(W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], a.get("mb", 0.0), a.get("mbf", 0.0))
    if c.fn == "last":
        return ex.search_by_projection_last(cam, a["cur_keys"], a["cur_desc"], a["q_keys"], a["world"], a["q_desc"], I3, a["tcw"], I3, Z3, a["th"], a["mono"],
                                            a["check_level"], a["check_ori"], mp_valid=a["valid"], mp_has_obs=a["obs"],
                                            u_right=a["u_right"] if a["stereo"] else None, cur_owner=a["owner"], scale_factors=SF)
    if c.fn == "mappoints":
        qk = a["q_keys"]
        kw = dict(mp_has_obs=a["obs"], owner=a["owner"])
        if a["stereo"]:
            kw.update(proj_xr=(qk["x"] - np.float32(a["mbf"])).astype(np.float32), u_right=a["u_right"])
        return ex.search_by_projection_mappoints(cam, a["cur_keys"], a["cur_desc"], a["valid"], qk["x"], qk["y"], np.ones(len(qk), np.float32), qk["octave"],
                                                 a["q_desc"], a["th"], a["check_level"], a["nnratio"], scale_factors=SF, **kw)
    if c.fn == "kf":
        valid, u, v, lvl = oracle_result[3]
        return ex.search_by_projection_kf(cam, a["cur_keys"], a["cur_desc"], valid, u, v, lvl, a["q_keys"]["angle"], a["q_desc"], a["th"], a["orb_dist"],
                                          a["check_ori"], owner=(a["owner"] != 0).astype(np.uint8), scale_factors=SF)
    if c.fn == "init":
        return ex.search_for_initialization(cam, a["keys1"], a["desc1"], a["keys2"], a["desc2"], a["prev"], a["window"], a["nnratio"], a["check_ori"],
                                            scale_factors=SF)
    if c.fn == "bow":
        return ex.search_by_bow(a["kf_off"], a["kf_idx"], a["f_off"], a["f_idx"], a["kf_valid"], a["kf_keys"], a["kf_desc"], a["f_keys"], a["f_desc"],
                                a["nnratio"], a["check_ori"])
    if c.fn == "tri":
        return ex.search_for_triangulation(scale_factors2=SF, level_sigma2_2=(SF * SF).astype(np.float32), **a)
    raise KeyError(c.fn)


def same(got, exp, c, culled_as_null=False):
    """count, every assignment, ownership (projection searches) / updated prev_matched (init).  culled_as_null: `got` is the reference's own
    code, where a slot matched and then culled by the rotation check reads -1 (the oracle and the device leave -2 there)."""
    if int(got[0]) != int(exp[0]):
        return "count %d, expected %d" % (got[0], exp[0])
    em = np.where(exp[1] == -2, -1, exp[1]) if culled_as_null else exp[1]
    if not (np.asarray(got[1]) == em).all():
        bad = np.nonzero(np.asarray(got[1]) != em)[0]
        return "assignment differs at %s: %s, expected %s" % (bad[:8], np.asarray(got[1])[bad[:8]], em[bad[:8]])
    if c.fn in ("last", "mappoints") and not (got[2] == exp[2]).all():
        return "ownership differs"
    if c.fn == "kf" and not ((got[2] != 0) == (exp[2] != 0)).all():      # (the reference's Cur-vs-KeyFrame search only knows "slot taken")
        return "ownership differs"
    if c.fn == "init" and not (np.asarray(got[2]).view(np.uint32) == np.asarray(exp[2]).view(np.uint32)).all():
        return "updated prev_matched differs"
    return None


# ---- what a query sees: GetFeaturesInArea restated on the constructed frame (cells of 8 px, roundf = half away from zero) ------------------------
def _cell(v):
    return np.floor(np.asarray(v, np.float32) * np.float32(0.125) + np.float32(0.5)).astype(np.int64)     # coordinates are >= 0 here


def window(cur_keys, u, v, r, min_level=-1, max_level=-1):
    """indices of the keypoints GetFeaturesInArea(u, v, r, min_level, max_level) returns, in its visiting order (column, row, index)"""
    u, v, r = np.float32(u), np.float32(v), np.float32(r)
    px, py = _cell(cur_keys["x"]), _cell(cur_keys["y"])
    x0, x1 = max(0, int(np.floor((u - r) * np.float32(0.125)))), min(63, int(np.ceil((u + r) * np.float32(0.125))))
    y0, y1 = max(0, int(np.floor((v - r) * np.float32(0.125)))), min(47, int(np.ceil((v + r) * np.float32(0.125))))
    ok = (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1) & (px < 64) & (py < 48)
    ok &= (np.abs(cur_keys["x"] - u) < r) & (np.abs(cur_keys["y"] - v) < r)
    if min_level > 0 or max_level >= 0:
        ok &= cur_keys["octave"] >= min_level
        if max_level >= 0:
            ok &= cur_keys["octave"] <= max_level
    idx = np.nonzero(ok)[0]
    return idx[np.lexsort((idx, py[idx], px[idx]))]


def query_radius(c, i):
    a = c.a
    return np.float32(a["radius"]) * SF[int(a["q_keys"]["octave"][i])]


def pick_stats(c, res):
    """For every query of a projection-search case that holds a keypoint in the oracle's answer `res`: (query, window size, rank of the
    pick in the query's (distance, visiting order) list, the pick's position in the visiting order)."""
    a = c.a
    match = np.asarray(res[1])
    out = []
    for j in np.nonzero(match >= 0)[0]:
        i = int(match[j])
        k = a["q_keys"][i]
        idx = window(a["cur_keys"], k["x"], k["y"], query_radius(c, i))
        idx = idx[a["owner"][idx] != 2] if c.fn != "kf" else idx[a["owner"][idx] == 0]
        d = ham_matrix(a["q_desc"][i], a["cur_desc"][idx])[0]
        pos = int(np.nonzero(idx == j)[0][0])
        rank = int(((d < d[pos]) | ((d == d[pos]) & (np.arange(len(idx)) < pos))).sum())
        out.append((i, len(idx), rank, pos))
    return out


def list_depth(fn):
    return 8 if fn == "mappoints" else 4      # the speculative list; two extensions of eight follow


def extensions_needed(c, res):
    """list extensions the fixpoint needs for the oracle's answer: a query whose pick (mappoints: whose runner-up, the entry after the pick)
    lies at list position p needs ceil((p + 1 - depth) / 8) blocks; more than two = the list is exhausted"""
    depth, extra = list_depth(c.fn), (1 if c.fn == "mappoints" else 0)
    return [max(0, -(-(rank + extra + 1 - depth) // 8)) for _, _, rank, _ in pick_stats(c, res)]


# ---- builders --------------------------------------------------------------------------------------------------------------------------------
def lattice(step, margin=24):
    return [(float(x), float(y)) for y in range(margin, H - margin, step) for x in range(margin, W - margin, step)]


def crowd(scene, rng, centre, n_q, n_c, dist_of, spread=3.0, obs=lambda i: 1, cand_oct=lambda j: 0, q_oct=0, q_jitter=1.0):
    """n_q queries with ONE descriptor around `centre`, n_c candidates within `spread` px of it, candidate j at Hamming distance dist_of(j):
    every query sees the same (distance, order) list, so blocking queries take its entries one after the other"""
    Q = rng.integers(0, 256, 32, dtype=np.uint8)
    perm = rng.permutation(256)
    for j in range(n_c):
        xy = (centre[0] + float(rng.integers(-int(spread * 4), int(spread * 4) + 1)) / 4, centre[1] + float(rng.integers(-int(spread * 4), int(spread * 4) + 1)) / 4)
        scene.cand(xy, flip(Q, perm[:dist_of(j)]), cand_oct(j))
    for i in range(n_q):
        xy = (centre[0] + float(rng.integers(-int(q_jitter * 4), int(q_jitter * 4) + 1)) / 4, centre[1] + float(rng.integers(-int(q_jitter * 4), int(q_jitter * 4) + 1)) / 4)
        scene.query(xy, Q, q_oct, obs=obs(i))


def _alt(j):
    return j & 1      # neighbouring list entries on different levels: the MapPoint search's ratio test (same level only) stays out of the way


PROJ = ("last", "mappoints", "kf")
NO_HANDOVER = dict(fallbacks=0, round_cap=0, ext_room=0)


def crowd_cases(rng):
    out = []
    for fn in PROJ:
        depth = list_depth(fn)
        # family 1: picks beyond the speculative list, within its two extensions, 64 slots suffice
        s = Scene()
        cs = lattice(40)
        for k in range(4 if fn != "mappoints" else 6):
            crowd(s, rng, cs[k], 12, 15, lambda j: 2 + j, cand_oct=_alt, obs=lambda i: 1)
        # ... and one crowd whose last query needs the LAST entry of its second extension; that block's entries sit exactly on TH_HIGH
        crowd(s, rng, cs[8], 20 if fn != "mappoints" else 23, 24 if fn != "mappoints" else 27, lambda j, depth=depth: 2 + j if j < depth + 8 else TH_HIGH, cand_oct=_alt)

        def reach1(c, res, depth=depth):
            need = extensions_needed(c, res)
            assert max(need) == 2 and sum(need) <= 64 and sum(1 for n in need if n) >= 20, need
            assert max(rank for _, _, rank, _ in pick_stats(c, res)) + (c.fn == "mappoints") == depth + 15
            d = ham_matrix(c.a["q_desc"][-1:], c.a["cur_desc"])[0]
            assert (d == TH_HIGH).sum() >= 8
        out.append(projected_case("extensions", 1, fn, s, 8.0, reach1, dict(NO_HANDOVER, ext_blocks=">0")))
        # family 2: some query's pick lies beyond list + two extensions
        s = Scene()
        crowd(s, rng, cs[0], 40, 44, lambda j: 2 + j if j < 24 else TH_HIGH, cand_oct=_alt)     # the deep entries sit exactly on TH_HIGH
        crowd(s, rng, cs[3], 3, 5, lambda j: 4 + 3 * j, cand_oct=_alt)

        def reach2(c, res):
            need = extensions_needed(c, res)
            assert max(need) > 2 and sum(1 for _, _, rank, _ in pick_stats(c, res) if rank >= 20) >= 5, need
        out.append(projected_case("list_exhausted", 2, fn, s, 8.0, reach2, dict(fallbacks=">0", ext_room=">0", round_cap=0), limit=True))
        # family 3: more than 64 extension blocks in one launch, no query needs a third
        s = Scene()
        for k in range(30):
            crowd(s, rng, cs[k], 12, 15, lambda j, depth=depth: 2 + j if j < depth + 4 else TH_HIGH, cand_oct=_alt)

        def reach3(c, res):
            need = extensions_needed(c, res)
            assert max(need) <= 2 and sum(need) > 64, (max(need), sum(need))
        out.append(projected_case("slots_exhausted", 3, fn, s, 8.0, reach3, dict(fallbacks=">0", ext_room=">0", round_cap=0), limit=True))
    return out


def chain_cases(rng):
    """family 4: query i prefers candidate i, then i + 1; query 0 prefers candidate 1: every round of the fixpoint moves one query"""
    out = []
    for fn, n in (("last", 60), ("last", 96), ("last", 97), ("last", 150), ("kf", 60), ("kf", 96), ("kf", 97), ("kf", 150)):
        s = Scene()
        B = rng.integers(0, 256, 32, dtype=np.uint8)
        perm = rng.permutation(256)
        P, Zb = perm[:10], perm[10:20]
        for j in range(n + 1):
            s.cand((16.0 + 3 * j, 100.0), flip(B, P) if j & 1 else B)
        for i in range(n):
            near_is_odd = (i & 1) if i else 1          # query 0: candidate 1 at distance 10, candidate 0 at 20
            s.query((16.0 + 3 * i + 1.5, 100.0), flip(flip(B, P), Zb) if near_is_odd else flip(B, Zb))

        def reach(c, res, n=n):
            st = sorted(pick_stats(c, res))
            assert len(st) == n and all(w == 2 for _, w, _, _ in st)
            assert st[0][2] == 0 and all(rank == 1 for _, _, rank, _ in st[1:])       # everybody but query 0 was pushed to his second choice
            # query k + 1 moves in round k, so round n - 1 is the first without a move: 96 queries converge in round 95, the last one permitted;
            # with 97 a pick still moves in that round and the pair is handed over
            assert (n > 96) == c.limit
        exp = dict(fallbacks=">0", round_cap=">0", ext_room=0) if n > 96 else dict(NO_HANDOVER, ext_blocks=0)
        out.append(projected_case("chain_%d" % n, 4, fn, s, 2.0, reach, exp, limit=n > 96))
    # the same chain with links that do not block (no observations): query 20 is pushed to candidate 21 but does not push query 21, which takes
    # 21 as well and replaces it; the chain starts again at query 30 (prefers 31).  Claims by non-blocking queries would push 21 .. 29 along.
    for fn in ("last",):      # (the Cur-vs-KeyFrame search knows no such points: every query blocks)
        s = Scene()
        B = rng.integers(0, 256, 32, dtype=np.uint8)
        perm = rng.permutation(256)
        P, Zb = perm[:10], perm[10:20]
        n = 60
        for j in range(n + 1):
            s.cand((16.0 + 3 * j, 100.0), flip(B, P) if j & 1 else B)
        for i in range(n):
            near = i + 1 if i in (0, 30) else i
            s.query((16.0 + 3 * i + 1.5, 100.0), flip(flip(B, P), Zb) if near & 1 else flip(B, Zb), obs=0 if i in (20, 50) else 1)

        def reach_links(c, res, n=n):
            m = np.asarray(res[1])
            want = np.array([-1] + list(range(20)) + list(range(21, 30)) + [-1] + list(range(30, 50)) + list(range(51, 60)) + [-1])
            assert res[0] == n and (m == want).all(), list(m)      # 60 picks, 58 holders: queries 20 and 50 were replaced
        out.append(projected_case("chain_nonblocking_links", 4, fn, s, 2.0, reach_links, dict(NO_HANDOVER, ext_blocks=0)))
    return out


def wide_cases(rng):
    """family 5: more than 256 candidates in one window / one grid cell, the wanted ones visited after the 256th"""
    out = []
    for fn in PROJ:
        for name, n_q, n_fill, one_cell in (("wide_cell", 12, 300, True), ("wide_cell_exhausted", 24, 300, True), ("wide_window", 20, 600, False)):
            s = Scene()
            Q = rng.integers(0, 256, 32, dtype=np.uint8)
            perm = rng.permutation(256)
            F = flip(Q, perm[:90])                     # the crowd: identical descriptors, all at distance 90 (acceptable, and tied)
            if one_cell:
                centre, radius = (64.0, 64.0), 8.0     # cell (8, 8) = [60, 68) x [60, 68)
                for j in range(n_fill):
                    s.cand((61.0 + float(rng.integers(0, 25)) / 4, 61.0 + float(rng.integers(0, 25)) / 4), F, j & 1)
                for i in range(n_q + 2):               # the wanted candidates come last in the cell's index order
                    s.cand((62.0 + (i % 5), 66.0), flip(Q, perm[:1 + i]), i & 1)
            else:
                centre, radius = (100.0, 100.0), 30.0
                for j in range(n_fill):
                    s.cand((80.0 + float(rng.integers(0, 120)) / 4, 80.0 + float(rng.integers(0, 161)) / 4), F, j & 1)
                for i in range(n_q + 2):               # ... and here in the last grid columns of the window
                    # (the seventh-best is the first keypoint of its grid column: where a walk over the column ranges starts a range)
                    s.cand((116.0 + (i % 4), 90.0 + (i - 6) % (n_q + 2)), flip(Q, perm[:1 + i]), i & 1)
            for i in range(n_q):
                s.query(centre, Q)

            def reach(c, res, n_q=n_q, one_cell=one_cell):
                st = pick_stats(c, res)
                assert len(st) == n_q and all(w > 256 for _, w, _, _ in st)
                assert sum(1 for _, _, _, pos in st if pos >= 256) >= n_q - 2
                if one_cell:
                    k = c.a["cur_keys"]
                    assert ((_cell(k["x"]) == 8) & (_cell(k["y"]) == 8)).sum() > 256
                need = extensions_needed(c, res)
                assert (max(need) > 2) == c.limit and max(need) >= 1
            lim = name.endswith("exhausted")
            exp = dict(fallbacks=">0", ext_room=">0", rescans=">0") if lim else dict(NO_HANDOVER, ext_blocks=">0")
            out.append(projected_case(name, 5, fn, s, radius, reach, exp, limit=lim))
    # SearchForInitialization: six F1 keypoints with one descriptor, F2 with 300 keypoints in one cell; the fourth query's list ends before it
    # has a runner-up and the later ones find all four entries held at smaller distances: full rescans over more than 256 candidates
    Q = rng.integers(0, 256, 32, dtype=np.uint8)
    perm = rng.permutation(256)
    xy2 = [(61.0 + float(rng.integers(0, 25)) / 4, 61.0 + float(rng.integers(0, 25)) / 4) for _ in range(300)] + [(62.0 + i, 66.0) for i in range(6)]
    d2 = [flip(Q, perm[:40])] * 300 + [flip(Q, perm[:2 + 2 * i]) for i in range(6)]
    a = dict(keys1=make_keys([(64.0, 64.0)] * 6), desc1=np.array([Q] * 6), keys2=make_keys(xy2), desc2=np.array(d2), prev=np.array([(64.0, 64.0)] * 6, np.float32),
             window=8, nnratio=0.9, check_ori=True)

    def reach_init(c, res):
        assert res[0] == 6 and (res[1] == 300 + np.arange(6)).all()
        assert len(window(c.a["keys2"], 64.0, 64.0, 8.0)) > 256
    out.append(Case("wide_cell_rescan", 5, "init", a, reach_init, dict(rescans=">0")))
    return out


def tie_cases(rng):
    """family 6: identical candidate descriptors -- the first in visiting order wins; best equal to runner-up"""
    out = []
    for fn in PROJ:
        for name, obs in (("ties_blocking", lambda i: 1), ("ties_alternating_obs", lambda i: i & 1)):
            s = Scene()
            cs = lattice(48)
            crowd(s, rng, cs[0], 10, 14, lambda j: 5, spread=7.0, cand_oct=_alt, obs=obs)       # candidates over several cells
            crowd(s, rng, cs[1], 10, 14, lambda j: 5, spread=0.5, cand_oct=_alt, obs=obs)       # ... and within one
            crowd(s, rng, cs[2], 6, 8, lambda j: 5 + (j >> 1), spread=7.0, cand_oct=lambda j: (j >> 1) & 1, obs=obs)   # pairs of equals

            def reach(c, res, fn=fn):
                a = c.a
                st = pick_stats(c, res)
                assert res[0] >= 10 and len(st) >= 5      # (a holder without observations is overwritten: fewer holders than matches)
                k = a["cur_keys"][:14]
                assert len(set(zip(_cell(k["x"]), _cell(k["y"])))) >= 4 and len(set(zip(_cell(a["cur_keys"][14:28]["x"]), _cell(a["cur_keys"][14:28]["y"])))) <= 2
                d = ham_matrix(a["q_desc"][:1], a["cur_desc"][:14])[0]
                assert (d == 5).all()
                if fn != "mappoints":      # the pick is the first of the equals nobody before it took: its rank counts exactly those
                    assert max(rank for _, _, rank, _ in st) >= 4
            out.append(projected_case(name, 6, fn, s, 9.0, reach, NO_HANDOVER))
    # MapPoint search: best == runner-up on ONE level is rejected by the ratio test (100 > 0.8 * 100), on different levels accepted
    s = Scene()
    cs = lattice(48)
    for k, (lv, d) in enumerate(((0, 40), (1, 40), (0, 100), (1, 100), (0, 0), (1, 0))):
        Q = rng.integers(0, 256, 32, dtype=np.uint8)
        perm = rng.permutation(256)
        s.cand((cs[k][0] - 2, cs[k][1]), flip(Q, perm[:d]), 0)
        s.cand((cs[k][0] + 2, cs[k][1] + 1), flip(Q, perm[100:100 + d]), lv)
        s.query(cs[k], Q)

    def reach_mp(c, res):
        m = res[1]
        assert res[0] == 4 and m[2] == 1 and m[6] == 3 and m[0] == -1 and m[4] == -1       # zero distances: 0 > 0.8 * 0 is false -> accepted
    out.append(projected_case("ties_best_equals_second", 6, "mappoints", s, 8.0, reach_mp, NO_HANDOVER))
    return out


RATIO_PAIRS = {0.6: ((6, 10), (12, 20), (30, 50), (60, 100)), 0.7: ((7, 10), (14, 20), (35, 50), (70, 100)), 0.75: ((3, 4), (15, 20), (75, 100)),
               0.8: ((8, 10), (16, 20), (40, 50), (80, 100)), 0.9: ((9, 10), (18, 20), (45, 50), (90, 100))}


def threshold_cases(rng):
    """family 7: distances exactly at and one above the accept thresholds; ratio tests exactly on bestDist == ratio * bestDist2"""
    out = []
    cs = lattice(32)

    def singles(dists):
        s = Scene()
        for k, d in enumerate(dists):
            Q = rng.integers(0, 256, 32, dtype=np.uint8)
            s.cand(cs[k], flip(Q, rng.permutation(256)[:d]))
            s.query(cs[k], Q)
        return s
    for fn, th, kw in (("last", TH_HIGH, {}), ("mappoints", TH_HIGH, {}), ("kf", 100, dict(orb_dist=100)), ("kf", 64, dict(orb_dist=64)), ("kf", 0, dict(orb_dist=0))):
        dists = [max(th - 1, 0), th, th + 1, th + 2, th, th + 1]

        def reach(c, res, dists=dists, th=th):
            d = np.array([ham(c.a["q_desc"][k], c.a["cur_desc"][k]) for k in range(len(dists))])
            assert (d == np.array(dists)).all()
            assert (np.asarray(res[1]) == np.where(d <= th, np.arange(len(d)), -1)).all()
        out.append(projected_case("accept_at_%d" % th, 7, fn, singles(dists), 4.0, reach, NO_HANDOVER, **kw))
    # ORBdist = 256 (mode 2): the keys keep distances above 255 for "nothing", so the accept threshold is clamped to 255 at the ABI.  254 and 255
    # are accepted; a complemented descriptor (256) is never picked; an empty window and a window whose only keypoint is taken give no match
    s = Scene()
    for k, d in enumerate((254, 255, 256)):
        Q = rng.integers(0, 256, 32, dtype=np.uint8)
        s.cand(cs[k], flip(Q, rng.permutation(256)[:d]))
        s.query(cs[k], Q)
    Q = rng.integers(0, 256, 32, dtype=np.uint8)
    s.query(cs[3], Q)                                   # nothing within reach
    s.cand(cs[4], flip(Q, [5, 77, 200]), owner=1)       # the slot already carries a MapPoint
    s.query(cs[4], Q)

    def reach256(c, res):
        a = c.a
        assert [ham(a["q_desc"][k], a["cur_desc"][k]) for k in range(3)] == [254, 255, 256] and ham(a["q_desc"][4], a["cur_desc"][3]) == 3
        assert len(window(a["cur_keys"], cs[3][0], cs[3][1], 4.0)) == 0 and list(window(a["cur_keys"], cs[4][0], cs[4][1], 4.0)) == [3]
        assert res[0] == 2 and list(np.asarray(res[1])) == [0, 1, -1, -1]
    out.append(projected_case("accept_at_256", 7, "kf", s, 4.0, reach256, NO_HANDOVER, orb_dist=256, ref_valid=[1, 1, 0, 1, 0]))
    # the MapPoint search's ratio rule: rejected iff same level and (float) best > nnratio * (float) second
    for ratio, pairs in RATIO_PAIRS.items():
        s = Scene()
        expect = []
        k = 0
        for b, d2 in pairs:
            for bb, lv in ((b, 0), (b + 1, 0), (b + 1, 1)):      # on the edge; one above; one above with the runner-up on another level
                Q = rng.integers(0, 256, 32, dtype=np.uint8)
                perm = rng.permutation(256)
                s.cand((cs[k][0] - 2, cs[k][1]), flip(Q, perm[:bb]), 0)
                s.cand((cs[k][0] + 2, cs[k][1]), flip(Q, perm[128:128 + d2]), lv)
                s.query(cs[k], Q)
                rejected = lv == 0 and bool(np.float32(bb) > np.float32(ratio) * np.float32(d2)) and bb <= TH_HIGH
                expect.append(-1 if (rejected or bb > TH_HIGH) else k)
                k += 1

        def reach(c, res, expect=expect, ratio=ratio, pairs=pairs):
            assert list(np.asarray(res[1])[0::2]) == expect, (list(np.asarray(res[1])[0::2]), expect)
            if ratio in (0.7, 0.9):      # float arithmetic accepts these pairs, the same test in double would not
                assert all(float(b) > float(np.float32(ratio)) * float(d2) and not np.float32(b) > np.float32(ratio) * np.float32(d2) for b, d2 in pairs)
        out.append(projected_case("ratio_%g" % ratio, 7, "mappoints", s, 4.0, reach, NO_HANDOVER, nnratio=ratio))
    return out


def histogram_cases(rng):
    """family 8: rotation-consistency votes on the 10 % rule, equal bins, bin edges.  The reference bins with factor = 1 / HISTO_LENGTH = 1 / 30
    (a quirk: 30 degrees per bin, not 12), so rot < 360 only reaches bins 0 .. 12 and its `bin == HISTO_LENGTH -> 0` wrap cannot be reached;
    `359.99` and `-0.5` are the largest differences there are and land in bin 12."""
    out = []
    cs = lattice(24)
    sets = {"ten_percent_1_of_10": [0.0] * 10 + [150.0] * 1 + [270.0] * 0, "ten_percent_2_of_20": [0.0] * 20 + [150.0] * 2 + [270.0] * 1,
            "ten_percent_3_of_30": [0.0] * 30 + [150.0] * 3 + [270.0] * 2, "ten_percent_below": [0.0] * 20 + [150.0] * 1 + [270.0] * 1,
            "equal_bins": [30.0, 90.0, 150.0, 210.0] * 5,
            "bin_edges": [15.0] * 5 + [45.0] * 4 + [345.0] * 3 + [359.99] * 3 + [0.0] * 3 + [14.999] * 2 + [-340.0] * 3 + [-0.5] * 2 + [75.0] * 1}
    for fn in ("last", "kf"):
        for name, rots in sets.items():
            s = Scene()
            order = rng.permutation(len(rots))
            for k, o in enumerate(order):
                rot = rots[o]
                ca = float(rng.integers(0, 8)) * 40.0 if rot >= 0 else 350.0
                qa = np.float32(ca) + np.float32(rot) if rot >= 0 else np.float32(350.0 + rot)     # negative: rot = qa - ca < 0 -> + 360
                if qa >= 360.0:                                                                    # (wrapped: the difference is negative too)
                    qa = np.float32(qa - np.float32(360.0))
                Q = rng.integers(0, 256, 32, dtype=np.uint8)
                s.cand(cs[k], Q, angle=ca)
                s.query(cs[k], Q, angle=float(qa))

            def reach(c, res, name=name, n=len(rots)):
                m = np.asarray(res[1])
                culled = int((m == -2).sum())
                assert res[0] + culled == n and res[0] > 0
                want = {"ten_percent_1_of_10": 0, "ten_percent_2_of_20": 1, "ten_percent_3_of_30": 2, "ten_percent_below": 2, "equal_bins": 5}.get(name)
                if want is not None:
                    assert culled == want, (name, culled)
                if name == "bin_edges":
                    a = c.a
                    rot = (a["q_keys"]["angle"] - a["cur_keys"]["angle"]).astype(np.float32)
                    rot = np.where(rot < 0, rot + np.float32(360.0), rot).astype(np.float32)
                    assert {15.0, 45.0, 75.0, 345.0, 0.0} <= set(rot.tolist())      # rot / 30 = 0.5, 1.5, 2.5, 11.5: on a bin edge; exactly 0
                    assert rot.max() > 359.9 and (a["q_keys"]["angle"] < a["cur_keys"]["angle"]).sum() >= 5      # just below 360; negative differences
                    bins = np.floor(rot * (np.float32(1.0) / np.float32(30)) + np.float32(0.5)).astype(int)      # roundf, in float as the kernel
                    assert list(np.bincount(bins, minlength=13)) == [5, 8, 4, 1, 0, 0, 0, 0, 0, 0, 0, 0, 8]      # edges round up; 14.999 stays in bin 0
                    assert culled == 5                                              # bins 1, 12 (equal: the first is max1) and 0 stay, 2 and 3 go
            out.append(projected_case(name, 8, fn, s, 4.0, reach, NO_HANDOVER, check_ori=True))
    return out


def geometry_cases(rng):
    """family 9: image bounds, cell-rounding edges, window edges, the stereo gate, level orders and ranges"""
    out = []
    Q = rng.integers(0, 256, 32, dtype=np.uint8)
    # keypoints and projections exactly on the bounds: x = max_x rounds into column 64 and is dropped from the grid; u = max_x is kept
    s = Scene()
    pts = [(0.0, 100.0), (512.0, 100.0), (100.0, 0.0), (100.0, 384.0), (511.75, 200.0), (200.0, 383.75), (0.0, 0.0), (512.0, 384.0), (507.75, 300.0), (508.0, 310.0)]
    for p in pts:
        s.cand(p, Q)
    for p in pts:
        s.query(p, Q)
    # projections exactly on max_x / max_y are kept (level 3: radius 6.9, so that a keypoint of column 63 is in reach), one ulp outside dropped
    # by SearchByProjection(Cur, Last); the MapPoint search leaves that test to Frame::isInFrustum
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(1e9)))
    for cxy, qxy in (((506.0, 100.0), (512.0, 100.0)), ((506.0, 200.0), (up(512.0), 200.0)), ((300.0, 378.0), (300.0, 384.0)), ((340.0, 378.0), (340.0, up(384.0)))):
        Qk = rng.integers(0, 256, 32, dtype=np.uint8)
        s.cand(cxy, Qk)
        s.query(qxy, Qk, 3)

    def reach_bounds(c, res):
        m = np.asarray(res[1])
        # column 64 / row 48 are never in the grid: 508 * 0.125 = 63.5 and 511.75 * 0.125 = 63.97 round to 64
        assert m[1] == -1 and m[3] == -1 and m[7] == -1 and m[9] == -1 and m[4] == -1 and m[5] == -1
        assert m[0] == 0 and m[2] == 2 and m[6] == 6 and m[8] == 8
        assert m[10] == 10 and m[12] == 12
        assert (m[11], m[13]) == ((-1, -1) if c.fn == "last" else (11, 13))
    out.append(projected_case("bounds", 9, "last", s, 4.0, reach_bounds, NO_HANDOVER))
    out.append(projected_case("bounds", 9, "mappoints", s, 4.0, reach_bounds, NO_HANDOVER))
    # two identical candidates either side of a cell-rounding edge: x = 12 is column 2 (1.5 rounds away from zero), x = 11.5 column 1, so the
    # LATER keypoint is visited first; rows likewise
    s = Scene()
    for k, (pa, pb) in enumerate((((12.0, 20.0), (11.5, 20.0)), ((100.0, 44.0), (100.0, 43.5)), ((204.0, 60.0), (203.75, 61.0)), ((301.0, 100.0), (300.5, 100.0)))):
        Qk = rng.integers(0, 256, 32, dtype=np.uint8)
        s.cand(pa, Qk); s.cand(pb, Qk)
        s.query(((pa[0] + pb[0]) / 2, (pa[1] + pb[1]) / 2), Qk)

    def reach_round(c, res):
        m = np.asarray(res[1])
        assert list(m[:8]) == [-1, 0, -1, 1, -1, 2, 3, -1], list(m[:8])       # the last pair shares a cell: index order
    out.append(projected_case("cell_rounding_edge", 9, "last", s, 5.0, reach_round, NO_HANDOVER))
    out.append(projected_case("cell_rounding_edge", 9, "kf", s, 5.0, reach_round, NO_HANDOVER))
    # a candidate at exactly |dx| == radius is outside (strict <); a quarter pixel nearer it is inside
    s = Scene()
    for k, off in enumerate(((6.0, 0.0), (5.75, 0.0), (-6.0, 0.0), (0.0, 6.0), (0.0, -5.75), (5.75, 5.75), (6.0, 5.75))):
        c0 = (100.0 + 40 * k, 200.0)
        s.cand((c0[0] + off[0], c0[1] + off[1]), Q)
        s.query(c0, Q)

    def reach_edge(c, res):
        assert list(np.asarray(res[1])) == [-1, 1, -1, -1, 4, 5, -1]
    for fn in PROJ:
        out.append(projected_case("window_edge", 9, fn, s, 6.0, reach_edge, NO_HANDOVER))
    # the stereo gate |ur - uRight| > radius excludes; equality passes.  mbf = 32: ur = u - 32
    s = Scene()
    for k, dr in enumerate((6.0, 6.25, -6.0, -6.25, 0.0)):
        c0 = (100.0 + 40 * k, 250.0)
        s.cand(c0, Q, u_right=c0[0] - 32.0 + dr)
        s.query(c0, Q)
    s.cand((340.0, 250.0), Q, u_right=-1.0)       # monocular keypoint: no gate
    s.query((340.0, 250.0), Q)

    def reach_stereo(c, res):
        assert list(np.asarray(res[1])) == [0, -1, 2, -1, 4, 5]
    out.append(projected_case("stereo_gate", 9, "last", s, 6.0, reach_stereo, NO_HANDOVER, mono=False, mb=0.125, mbf=32.0, stereo=True))
    out.append(projected_case("stereo_gate", 9, "mappoints", s, 6.0, reach_stereo, NO_HANDOVER, mb=0.125, mbf=32.0, stereo=True))
    # levels: shuffled instead of sorted, all on one level, the coarsest only; the forward / backward level ranges of SearchByProjection(Cur, Last)
    for name, levels in (("levels_shuffled", None), ("levels_all_two", 2), ("levels_coarsest", 7)):
        s = Scene()
        n = 160
        xy = np.stack([rng.integers(30 * 4, 480 * 4, n) / 4.0, rng.integers(30 * 4, 350 * 4, n) / 4.0], -1)
        for i in range(n):
            Qi = rng.integers(0, 256, 32, dtype=np.uint8)
            lv = int(rng.integers(0, 8)) if levels is None else levels
            dl = int(rng.integers(-2, 3))
            s.cand((xy[i, 0] + float(rng.integers(-8, 9)) / 4, xy[i, 1] + float(rng.integers(-8, 9)) / 4), flip(Qi, rng.permutation(256)[:int(rng.integers(0, 60))]),
                   min(max(lv + dl, 0), 7), angle=float(rng.integers(0, 360)))
            s.query(tuple(xy[i]), Qi, lv, angle=float(rng.integers(0, 360)), obs=int(rng.integers(0, 2)))

        def reach_lv(c, res, levels=levels):
            o = c.a["q_keys"]["octave"]
            assert res[0] > 20
            if c.fn == "last":       # the level range the variant claims was the one applied, and it shows in the answer
                m = np.asarray(res[1])
                j = np.nonzero(m >= 0)[0]
                diff = c.a["cur_keys"]["octave"][j] - o[m[j]]
                co = c.a["cur_keys"]["octave"]
                if c.name.endswith("_forward"):          # nCurOctave >= nLastOctave
                    assert (diff >= 0).all() and ((diff >= 2).any() or ((co == o - 1) & (m == -1)).any())
                elif c.name.endswith("_backward"):       # nCurOctave <= nLastOctave
                    assert (diff <= 0).all() and (diff <= -2).any()
                else:
                    assert (np.abs(diff) <= 1).all() and ((np.abs(co - o) >= 2) & (m == -1)).any()
            if levels is None:
                assert (np.diff(o) < 0).sum() > 40 and len(set(o)) == 8
            else:
                assert (o == levels).all()
        for fn, kw in (("last", dict(check_level=True)), ("last", dict(check_level=True, mono=False, mb=0.001, tz=0.002)),
                       ("last", dict(check_level=True, mono=False, mb=0.001, tz=-0.002)), ("mappoints", dict(check_level=True)), ("kf", {})):
            tag = name + ("_backward" if kw.get("tz", 0) > 0 else "_forward" if kw.get("tz", 0) < 0 else "")      # tlc = -tcw: forward is tz < 0
            out.append(projected_case(tag, 9, fn, s, 5.0, reach_lv, dict(fallbacks=0), check_ori=False, **kw))
    return out


def size_cases(rng):
    """family 10: 0, 1, 127, 128, 129, 131 queries (from 128 on the library spreads a pair over several workgroups; 129 and 131 are no multiple of
    three: match_split=3.  Which plan ran does not show in the answer: these cases assert equality with the oracle only); 0 and 1 candidates"""
    out = []
    cs = lattice(20)
    for fn in PROJ:
        for nq, nc in ((0, 5), (1, 1), (1, 0), (5, 0), (5, 1), (127, 127), (128, 128), (129, 129), (131, 140)):
            s = Scene()
            for k in range(max(nq, nc)):
                Qk = rng.integers(0, 256, 32, dtype=np.uint8)
                if k < nc:
                    s.cand(cs[k], flip(Qk, rng.permutation(256)[:k % 40]), angle=0.0)
                if k < nq:
                    s.query(cs[k], Qk)

            def reach(c, res, nq=nq, nc=nc):
                assert len(c.a["q_keys"]) == nq and len(c.a["cur_keys"]) == nc and res[0] == min(nq, nc)
            out.append(projected_case("sizes_%dq_%dc" % (nq, nc), 10, fn, s, 4.0, reach, NO_HANDOVER, none=min(nq, nc) == 0))
    return out


def bow_cases(rng):
    """families 7, 8, 11 for SearchByBoW: node sizes around the 64-lane rounds and the 4096 limit, KeyFrame features of one node that prefer the
    same Frame feature, invalid ones in between, TH_LOW and the ratio on their edges, votes from several nodes"""
    out = []
    kd, kv, ka, fd, fa = [], [], [], [], []
    ko, ki, fo, fi = [0], [], [0], []
    sizes = (1, 63, 64, 65, 4095, 4096, 2, 130)
    for nF in sizes:
        B = rng.integers(0, 256, 32, dtype=np.uint8)
        perm = rng.permutation(256)
        f0 = len(fd)
        for j in range(nF):                                  # the node's crowd: 60 .. 90 bits from the base
            fd.append(flip(B, rng.permutation(256)[:int(rng.integers(60, 91))])); fa.append(0.0)
        fd[f0 + nF - 1] = flip(B, perm[:3])                  # the wanted Frame features come LAST in the node (round 63 / lane 63 of the mask)
        if nF >= 2:
            fd[f0 + nF - 2] = flip(B, perm[3:9])
        fi.extend(range(f0, f0 + nF)); fo.append(len(fi))
        for k, (bits, valid) in enumerate(((perm[9:10], 1), (perm[10:12], 0), (perm[12:13], 1), (perm[13:14], 1), (perm[14:16], 1))):
            kd.append(flip(B, bits)); kv.append(valid); ka.append(30.0 * (len(ko) % 3))
            ki.append(len(kd) - 1)
        ko.append(len(ki))
    a = dict(kf_off=np.array(ko, np.int32), kf_idx=np.array(ki, np.int32), f_off=np.array(fo, np.int32), f_idx=np.array(fi, np.int32), kf_valid=np.array(kv, np.uint8),
             kf_keys=make_keys(np.zeros((len(kd), 2)), 0, np.array(ka, np.float32)), kf_desc=np.array(kd), f_keys=make_keys(np.zeros((len(fd), 2)), 0, np.array(fa, np.float32)),
             f_desc=np.array(fd), nnratio=0.7, check_ori=True)

    def reach_nodes(c, res, sizes=sizes):
        m = np.asarray(res[1])
        ends = np.cumsum(sizes) - 1
        assert (m[ends] != -1).all() and sum(1 for e, n in zip(ends, sizes) if n >= 2 and m[e - 1] != -1) == len(sizes) - 1
        assert res[0] + int((m == -2).sum()) == 2 * len(sizes) - 1 and int((m == -2).sum()) == 0      # three bins with 5 / 6 / 4 votes: all kept
    out.append(Case("node_sizes", 11, "bow", a, reach_nodes))
    # thresholds, ratios and the histogram: one KeyFrame feature and two Frame features per node
    for ratio, pairs in RATIO_PAIRS.items():
        kd, ka, fd, fa, expect = [], [], [], [], []
        rots = [0.0] * 20 + [150.0] * 2 + [270.0]
        for k, (b, d2) in enumerate([(b, d2) for b, d2 in pairs for _ in (0, 1)] + [(50, 200), (51, 200), (49, 200), (0, 0), (20, 20), (0, 1)] + [(1, 100)] * len(rots)):
            if k < 2 * len(pairs) and k & 1:
                b -= 1                                       # one below the edge: accepted
            B = rng.integers(0, 256, 32, dtype=np.uint8)
            perm = rng.permutation(256)
            kd.append(B); fd.append(flip(B, perm[:b])); fd.append(flip(B, perm[56:56 + d2]))
            r = k - (2 * len(pairs) + 6)
            ka.append(rots[r] if r >= 0 else 60.0); fa.extend([0.0, 0.0])     # the edge nodes vote for a bin of their own
            expect.append(b <= TH_LOW and bool(np.float32(b) < np.float32(ratio) * np.float32(d2)))
        n = len(kd)
        a = dict(kf_off=np.arange(n + 1, dtype=np.int32), kf_idx=np.arange(n, dtype=np.int32), f_off=2 * np.arange(n + 1, dtype=np.int32), f_idx=np.arange(2 * n, dtype=np.int32),
                 kf_valid=np.ones(n, np.uint8), kf_keys=make_keys(np.zeros((n, 2)), 0, np.array(ka, np.float32)), kf_desc=np.array(kd),
                 f_keys=make_keys(np.zeros((2 * n, 2)), 0, np.array(fa, np.float32)), f_desc=np.array(fd), nnratio=ratio, check_ori=True)

        def reach(c, res, expect=expect, n=n):
            m = np.asarray(res[1])
            assert list(m[0::2] != -1) == expect and (m[1::2] == -1).all()
            assert int((m == -2).sum()) == 1 and m[2 * n - 2] == -2      # bins of 20, a few and 2 votes stay (2 < 0.1f * 20 is false), the fourth goes
        out.append(Case("edges_ratio_%g" % ratio, 7, "bow", a, reach))
    return out


def init_cases(rng):
    """families 6, 7, 8, 10, 12 for SearchForInitialization (resolved in one wave, no fixpoint)"""
    out = []
    cs = lattice(40)

    def case(name, family, k1, d1, k2, d2, reach, expect=None, window=10, nnratio=0.9, check_ori=True, prev=None, none=False):
        k1 = k1 if isinstance(k1, np.ndarray) else make_keys(k1)
        k2 = k2 if isinstance(k2, np.ndarray) else make_keys(k2)
        prev = np.stack([k1["x"], k1["y"]], -1).astype(np.float32) if prev is None else np.asarray(prev, np.float32)
        a = dict(keys1=k1, desc1=np.array(d1, np.uint8).reshape(-1, 32), keys2=k2, desc2=np.array(d2, np.uint8).reshape(-1, 32), prev=prev, window=window,
                 nnratio=nnratio, check_ori=check_ori)
        return Case(name, family, "init", a, reach, expect, none=none)
    # family 12a: thirty F1 keypoints converge on three F2 keypoints with strictly decreasing distances: each takes the keypoint over
    T = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(3)]
    k1, d1 = [], []
    for i in range(30):
        t = i % 3
        k1.append((cs[t][0] + (i % 5) - 2, cs[t][1])); d1.append(flip(T[t], rng.permutation(256)[:40 - i]))

    def reach_take(c, res):
        m = np.asarray(res[1])
        assert res[0] == 3 and list(np.nonzero(m >= 0)[0]) == [27, 28, 29]
    out.append(case("takeover_decreasing", 12, k1, d1, [cs[0], cs[1], cs[2]], T, reach_take, dict(rescans=0), check_ori=False))
    # 12b: the same with a rotation check that later culls the final holders (their angle differs): the votes of the losers stay
    ang = np.zeros(30, np.float32); ang[29] = 90.0

    def reach_culled(c, res):
        # 29 votes in bin 0 -- 27 of them from queries that lost their keypoint again -- and one in bin 3: the last holder is culled
        assert res[0] == 2 and list(np.nonzero(np.asarray(res[1]) >= 0)[0]) == [27, 28]
    out.append(case("takeover_loser_culled", 12, make_keys(k1, 0, ang), d1, [cs[0], cs[1], cs[2]], T, reach_culled, dict(rescans=0)))
    # 12c: increasing distances: six F2 keypoints C_k = B + a private block; F1 first matches four of them exactly, then queries at the base
    # find all four entries of their list held at distance 0 and rescan: the fifth is free (20 against 40: accepted), then nothing is
    B = rng.integers(0, 256, 32, dtype=np.uint8)
    perm = rng.permutation(256)
    C = [flip(B, perm[20 * k:20 * k + 20]) for k in range(5)] + [flip(B, perm[100:140])]
    k2 = [(cs[5][0] + 2 * k - 5, cs[5][1]) for k in range(6)]
    d1 = C[:4] + [B, B, flip(B, perm[200:201])]
    k1 = [cs[5]] * 7

    def reach_inc(c, res):
        m = np.asarray(res[1])
        assert list(m) == [0, 1, 2, 3, 4, 5, -1], list(m)       # (the sixth query rescans too: the fifth keypoint is held at its own 20, the last is free)
        assert (ham_matrix(c.a["desc1"][4:5], c.a["desc2"])[0] == [20, 20, 20, 20, 20, 40]).all()
    out.append(case("increasing_rescan", 12, k1, d1, k2, C, reach_inc, dict(rescans=">0")))
    # 12d: a candidate held at exactly the query's distance is excluded (<=)
    Tq = rng.integers(0, 256, 32, dtype=np.uint8)
    p = rng.permutation(256)
    d1 = [flip(Tq, p[:10]), flip(Tq, p[10:20]), flip(Tq, p[20:29])]

    def reach_eq(c, res):
        assert list(np.asarray(res[1])) == [-1, -1, 0]       # the second (equal) does not take it over, the third (one nearer) does
    out.append(case("held_at_equal_distance", 12, [cs[6]] * 3, d1, [cs[6]], [Tq], reach_eq, dict(rescans=0)))
    # family 7: TH_LOW and the ratio test bestDist < bestDist2 * ratio on its edge (equality rejects)
    for ratio, pairs in RATIO_PAIRS.items():
        k1, d1, k2, d2, expect = [], [], [], [], []
        lat = lattice(32)
        allp = [(b - e, d2_) for b, d2_ in pairs for e in (0, 1)] + [(50, 200), (51, 200), (49, 200), (20, 20), (0, 0)]
        for k, (b, s2) in enumerate(allp):
            Qk = rng.integers(0, 256, 32, dtype=np.uint8)
            perm = rng.permutation(256)
            k1.append(lat[k]); d1.append(Qk)
            k2.extend([(lat[k][0] - 2, lat[k][1]), (lat[k][0] + 2, lat[k][1])]); d2.extend([flip(Qk, perm[:b]), flip(Qk, perm[56:56 + s2])])
            expect.append(2 * k if (b <= TH_LOW and bool(np.float32(b) < np.float32(s2) * np.float32(ratio))) else -1)

        def reach(c, res, expect=expect):
            assert list(np.asarray(res[1])) == expect, (list(np.asarray(res[1])), expect)
        out.append(case("edges_ratio_%g" % ratio, 7, k1, d1, k2, d2, reach, dict(rescans=0), nnratio=ratio, check_ori=False))
    # family 10 / 9: sizes, higher-level F1 keypoints (skipped), window clipped at the image corner
    for n1, n2 in ((1, 1), (127, 127), (128, 128), (129, 129), (64, 1)):
        lat = lattice(20)
        Qs = [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(max(n1, n2))]
        k1 = make_keys(lat[:n1], np.array([1 if i % 7 == 3 else 0 for i in range(n1)], np.int32))

        def reach(c, res, n1=n1, n2=n2):
            lv0 = c.a["keys1"]["octave"][:n2] == 0
            assert res[0] == int(lv0.sum()) and res[0] > 0
        out.append(case("sizes_%d_%d" % (n1, n2), 10, k1, Qs[:n1], lat[:n2], Qs[:n2], reach, dict(rescans=0)))
    return out


def triangulation_cases(rng):
    """families 6 and 8 for SearchForTriangulation: of equal distances the LAST candidate of the node wins (the reference's scan replaces the
    holder on `dist <= bestDist`); rotation votes from twelve nodes, 10 + 1 + 1: one vote is exactly 10 % of ten and stays"""
    from tests.tri_cases import geometry
    F12, Cw1, R2w, t2w, cam2 = geometry(0.002)          # lateral motion: the epipolar line of (x, y) runs through (x + 3 s, y - 2 s)
    k1, d1, a1, k2, d2 = [], [], [], [], []
    o1, o2 = [0], [0]
    rots = [0.0] * 10 + [150.0, 270.0]
    for n, rot in enumerate(rots):
        Q = rng.integers(0, 256, 32, dtype=np.uint8)
        perm = rng.permutation(256)
        x, y = 60.0 + 50 * n, 150.0 + 10 * (n % 3)
        k1.append((x, y)); d1.append(Q); a1.append(rot)
        for s_ in range(1, 5):                           # four equals ...
            k2.append((x + 3.0 * s_, y - 2.0 * s_)); d2.append(flip(Q, perm[:7]))
        k2.append((x + 15.0, y - 10.0)); d2.append(flip(Q, perm[:9]))      # ... and a worse one after them
        o1.append(len(k1)); o2.append(len(k2))
    a = dict(off1=np.array(o1, np.int32), idx1=np.arange(len(k1), dtype=np.int32), off2=np.array(o2, np.int32), idx2=np.arange(len(k2), dtype=np.int32),
             kf1=dict(keys=make_keys(k1, 0, np.array(a1, np.float32)), desc=np.array(d1), has_mp=np.zeros(len(k1), np.uint8), u_right=None),
             kf2=dict(keys=make_keys(k2), desc=np.array(d2), has_mp=np.zeros(len(k2), np.uint8), u_right=None), F12=F12, Cw1=Cw1, R2w=R2w, t2w=t2w, cam2=cam2,
             only_stereo=False, check_ori=True)

    def reach(c, res):
        assert res[0] == 12 and (np.asarray(res[1]) == 5 * np.arange(12) + 3).all(), res
    return [Case("last_of_equals_and_votes", 6, "tri", a, reach)]


_CACHE = []


def cases():
    if not _CACHE:
        rng = np.random.default_rng(20240611)
        for f in (crowd_cases, chain_cases, wide_cases, tie_cases, threshold_cases, histogram_cases, geometry_cases, size_cases, bow_cases, init_cases, triangulation_cases):
            _CACHE.extend(f(rng))
        names = [repr(c) for c in _CACHE]
        assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return _CACHE


def case_ids():
    return [repr(c) for c in cases()]
