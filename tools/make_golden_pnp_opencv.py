"""Records tests/golden/pnp_opencv.npz on a machine that has cv2: what OpenCV's own cv2.SVDecomp, cv2.solve(.., DECOMP_SVD),
cv2.invert(.., DECOMP_SVD) and cv2.mulTransposed return on the matrices that EPnP hands them in the cases of tests/pnp_cases.py (the sample
set of the first four budget hypotheses of every constructed case and seeded scene).  The project fixes these four routines as one text
(csrc/pnp_math.h, restated in tests/pnp_cases.py) and until this fixture exists that text is pinned to nothing but its restatement
(DESIGN.md); tests/test_pnp_opencv_golden.py skips.

A one-sided Jacobi SVD built with another hypot, another summation order or FMA contraction differs from the fixed text in the last bits, and
on the rank-8 MtM of four correspondences in the whole basis of the null space.  So the comparison is not bit for bit: the tool measures the
largest deviation of the fixed text from cv2 over the WELL-CONDITIONED matrices (condition number below 1e8) and stores it in the fixture's
metadata; the test's bound is a small multiple of that.  Null-space vectors are compared as subspaces.

  python tools/make_golden_pnp_opencv.py [--out tests/golden/pnp_opencv.npz]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pnp_cases as PC  # noqa: E402

WELL = 1e8                                   # the condition number below which a matrix counts as well-conditioned
APPROX_COLUMNS = ((0, 1, 3, 6), (0, 1, 2), (0, 1, 2, 3, 4))


def subsets():
    """(case name, hypothesis, subset) of every budget hypothesis whose matrices are finite"""
    for name in PC.NAMES + PC.SCENE_NAMES:
        P = PC.case_by_name(name).problem
        if len(P.P3D) < P.min_set:
            continue
        for h in range(min(len(P.samples), P.max_its, 4)):   # (four per case keep the fixture small)
            sub = tuple(int(i) for i in P.samples[h])
            m = PC.matrices(P, sub)
            if all(np.isfinite(v).all() for v in m.values()):
                yield name, h, P, sub, m


def ours(m):
    """the fixed text on the matrices m -> dict of results in cv2's layout"""
    lists = lambda a: [list(map(float, r)) for r in a]
    out = {}
    At, W, _ = PC.jacobi_svd(lists(m["mtm"].T), want_v=False)
    out["mtm_w"], out["mtm_null"] = np.array(W), np.array(At[8:])
    At, W, _ = PC.jacobi_svd(lists(m["pw0tpw0"].T))
    out["pw0_w"] = np.array(W)
    out["cc_inv"] = np.array(PC.invert_svd(lists(m["cc"])))
    out["mtm"] = np.array(PC.mul_transposed(lists(m["M"])))
    out["betas"] = [np.array(PC.solve_svd(lists(m["l"][:, cols]), list(map(float, m["rho"])))) for cols in APPROX_COLUMNS]
    rot = []
    for abt in m["abt"]:
        At, _, Vt = PC.jacobi_svd(lists(abt.T))
        rot.append(np.array(At).T @ np.array(Vt))   # U V'
    out["rot"] = np.array(rot)
    return out


def opencv(m):
    import cv2
    out = {}
    w, u, _ = cv2.SVDecomp(m["mtm"].copy(), flags=cv2.SVD_MODIFY_A)
    out["mtm_w"], out["mtm_null"] = w.reshape(-1), u.T[8:].copy()
    out["pw0_w"] = cv2.SVDecomp(m["pw0tpw0"].copy())[0].reshape(-1)
    out["cc_inv"] = cv2.invert(m["cc"], flags=cv2.DECOMP_SVD)[1]
    out["mtm"] = cv2.mulTransposed(m["M"], True)
    out["betas"] = [cv2.solve(np.ascontiguousarray(m["l"][:, cols]), m["rho"].reshape(6, 1), flags=cv2.DECOMP_SVD)[1].reshape(-1) for cols in APPROX_COLUMNS]
    rot = []
    for abt in m["abt"]:
        _, u, vt = cv2.SVDecomp(abt.copy())
        rot.append(u @ vt)
    out["rot"] = np.array(rot)
    return out


def cond(a):
    w = np.linalg.svd(a, compute_uv=False)
    return np.inf if w[-1] == 0 else w[0] / w[-1]


def subspace_gap(A, B):
    """the sine of the largest principal angle between the row spaces of A and B (rows need not be orthonormal)"""
    qa, qb = np.linalg.qr(A.T)[0], np.linalg.qr(B.T)[0]
    return float(np.linalg.norm(qa - qb @ (qb.T @ qa), 2))


def deviations(m, a, b):
    """kind -> relative deviation of the fixed text `a` from OpenCV `b`, for the quantities whose matrix is well-conditioned"""
    rel = lambda x, y: float(np.abs(x - y).max() / max(np.abs(y).max(), 1e-300))
    d = {"mul_transposed": rel(a["mtm"], b["mtm"]), "mtm_w": rel(a["mtm_w"][:8], b["mtm_w"][:8])}
    if a["mtm_w"][7] > 1e-8 * a["mtm_w"][0]:   # eight singular values stand clear of the null space: the null space is determined
        d["mtm_null"] = subspace_gap(a["mtm_null"], b["mtm_null"])
    if cond(m["pw0tpw0"]) < WELL:
        d["pw0_w"] = rel(a["pw0_w"], b["pw0_w"])
    if cond(m["cc"]) < WELL:
        d["invert"] = rel(a["cc_inv"], b["cc_inv"])
    for k, cols in enumerate(APPROX_COLUMNS):
        if cond(m["l"][:, cols]) < WELL:
            d["solve"] = max(d.get("solve", 0.0), rel(a["betas"][k], b["betas"][k]))
    for k, abt in enumerate(m["abt"]):
        if cond(abt) < WELL:
            d["rot"] = max(d.get("rot", 0.0), rel(a["rot"][k], b["rot"][k]))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pnp_opencv.npz"))
    a = ap.parse_args()
    import cv2
    rec, worst = {}, {}
    for name, h, P, sub, m in subsets():
        b = opencv(m)
        key = "%s/%d" % (name, h)
        for k in ("mtm_w", "mtm_null", "pw0_w", "cc_inv", "rot"):
            rec[key + "/" + k] = np.asarray(b[k], np.float64)
        rec[key + "/mtm_diag"] = np.diag(b["mtm"]).copy()
        for j, x in enumerate(b["betas"]):
            rec[key + "/betas%d" % j] = x
        for k, v in deviations(m, ours(m), b).items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, key)
    kinds = sorted(worst)
    print("largest deviation of the fixed text from cv2 %s over the well-conditioned matrices:" % cv2.__version__)
    for k in kinds:
        print("  %-16s %.3e  (%s)" % (k, worst[k][0], worst[k][1]))
    np.savez_compressed(a.out, opencv_version=np.array(cv2.__version__), kinds=np.array(kinds), max_deviation=np.array([worst[k][0] for k in kinds]), **rec)
    print("wrote %s, %d bytes" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
