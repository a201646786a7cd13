"""Records tests/golden/pnp_ref.npz: what the REFERENCE's own src/PnPsolver.cc returns from every iterate / find call of every constructed
case and seeded scene of tests/pnp_cases.py -- whether a matrix came back, the matrix, nInliers, bNoMore, vbInliers, and mnIterations /
mnBestInliers after the call.

The reference file is compiled where it lies in the reference checkout, into a build directory outside the repository, against the stand-in
Frame.h / MapPoint.h / Converter.h of tools/pnp_ref_shim/, a scripted Thirdparty/DBoW2/DUtils/Random.h earlier on the include path (it hands
out the case's sample sets), and a slice of the OpenCV C API (tools/pnp_ref_shim/cv_slice.h) whose cvSVD / cvSolve / cvInvert /
cvMulTransposed are THIS PROJECT's fixed text (csrc/pnp_math.h), not OpenCV's.  So the record pins the reference's EPnP and RANSAC logic and
roundings over the fixed linear algebra; the linear algebra itself is pinned to nothing but its restatement (tests/pnp_cases.py), and to a
compiled OpenCV only through tools/make_golden_pnp_opencv.py on a machine that has one.  Nothing but the .npz is written into the repository.

  python tools/make_golden_pnp_ref.py --reference <checkout> [--build-dir <dir>]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import pnp_cases as PC  # noqa: E402


def build(ref, out):
    shim = os.path.join(ROOT, "tools", "pnp_ref_shim")
    exe = os.path.join(out, "pnp_ref")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-w", "-ffp-contract=off", "-I", shim, "-I", os.path.join(ROOT, "orb_ygz_slam_amd", "csrc"),
                           "-I", os.path.join(ref, "include"), "-I", ref, "-include", os.path.join(shim, "MapPoint.h"), "-include", os.path.join(shim, "Frame.h"),
                           "-include", os.path.join(shim, "Converter.h"), os.path.join(ref, "src", "PnPsolver.cc"),
                           os.path.join(shim, "pnp_ref_main.cpp"), "-o", exe])
    return exe


def read_calls(P, path):
    buf = open(path, "rb").read()
    pos, meta, Ts, inl = 0, [], [], []
    for _ in P.calls:
        v = np.frombuffer(buf, "<i4", 6, pos)
        pos += 24
        Ts.append(np.frombuffer(buf, "<f4", 16, pos))
        pos += 64
        inl.append(np.frombuffer(buf, "u1", int(v[3]), pos))
        pos += int(v[3])
        meta.append(v)
    assert pos == len(buf)
    return np.array(meta, np.int32).reshape(-1, 6), np.array(Ts, np.float32).reshape(-1, 16), (np.concatenate(inl) if inl else np.zeros(0, np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "pnp_ref.npz"))
    a = ap.parse_args()
    out = a.build_dir or tempfile.mkdtemp(prefix="pnp_ref_")
    assert not os.path.abspath(out).startswith(ROOT + os.sep), "the build directory must lie outside the repository"
    os.makedirs(out, exist_ok=True)
    exe = build(os.path.abspath(a.reference), out)
    rec = {}
    for name in PC.NAMES + PC.SCENE_NAMES:
        P = PC.case_by_name(name).problem
        cin, cout = os.path.join(out, name + ".in"), os.path.join(out, name + ".out")
        PC.write_case(P, cin)
        r = subprocess.run([exe, cin, cout], capture_output=True, text=True)
        assert r.returncode == 0, (name, r.stdout, r.stderr[-2000:])
        meta, T, inl = read_calls(P, cout)
        rec[name + "/meta"], rec[name + "/T"], rec[name + "/inliers"] = meta, T, np.packbits(inl)
        rec[name + "/sizes"] = meta[:, 3].copy()
        print("%-24s %s" % (name, [tuple(int(x) for x in m) for m in meta]))
    np.savez_compressed(a.out, names=np.array(PC.NAMES + PC.SCENE_NAMES), **rec)
    print("wrote %s, %d bytes" % (a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
