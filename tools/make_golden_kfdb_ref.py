"""Records tests/golden/kfdb_ref.npz: what the REFERENCE's own src/KeyFrameDatabase.cc and DBoW2 (ScoringObject.cpp, BowVector.cpp, the
vocabulary's score()) return on every constructed case and seeded scene of tests/kfdb_cases.py -- minimum scores, candidate lists, every
keyframe's six query fields after every query and the double score() of the query against every stored keyframe.

The reference files are compiled where they lie in the reference checkout, into a build directory outside the repository, against the stand-in
KeyFrame.h / Frame.h / Common.h of tools/kfdb_ref_shim/ and oracle/ref_shim for the OpenCV slice DBoW2 includes.  The vocabulary is generated
text (a million words straight under the root, so that size() covers every word id of the cases), read by the reference's loadFromTextFile.
Nothing but the .npz is written into the repository.

  python tools/make_golden_kfdb_ref.py --reference <checkout> [--build-dir <dir>]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import kfdb_cases as K  # noqa: E402

N_WORDS = 1000000


def build(ref, out):
    d2, du = os.path.join(ref, "Thirdparty", "DBoW2", "DBoW2"), os.path.join(ref, "Thirdparty", "DBoW2", "DUtils")
    shim, oshim = os.path.join(ROOT, "tools", "kfdb_ref_shim"), os.path.join(ROOT, "oracle", "ref_shim")
    exe = os.path.join(out, "kfdb_ref")
    srcs = [os.path.join(d2, f) for f in ("FORB.cpp", "BowVector.cpp", "FeatureVector.cpp", "ScoringObject.cpp")]
    srcs += [os.path.join(du, f) for f in ("Random.cpp", "Timestamp.cpp")]
    srcs += [os.path.join(ref, "src", "KeyFrameDatabase.cc"), os.path.join(oshim, "mini_cv.cpp"), os.path.join(ROOT, "oracle", "oracle_cvprims.cpp"),
             os.path.join(shim, "kfdb_ref_main.cpp")]
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-msse4.2", "-w", "-ffp-contract=off", "-DYGZ_REAL_DBOW2", "-I", shim, "-I", oshim,
                           "-I", os.path.join(ROOT, "oracle"), "-I", ref, "-I", os.path.join(ref, "include"),
                           "-include", os.path.join(oshim, "dbow2_stubs.h"), "-include", os.path.join(shim, "Common.h")] + srcs + ["-o", exe, "-lpthread"])
    return exe


def write_vocabulary(path):
    """"k L scoring weighting" (L1 norm, tf-idf), then one line per node: parent isLeaf 32 descriptor bytes weight; no trailing newline"""
    line = "0 1 " + "0 " * 32 + "1"
    with open(path, "w") as f:
        f.write("10 6 0 0\n" + "\n".join([line] * N_WORDS))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--build-dir", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "kfdb_ref.npz"))
    a = ap.parse_args()
    out = a.build_dir or tempfile.mkdtemp(prefix="kfdb_ref_")
    assert not os.path.abspath(out).startswith(ROOT + os.sep), "the build directory must lie outside the repository"
    os.makedirs(out, exist_ok=True)
    exe = build(os.path.abspath(a.reference), out)
    voc = os.path.join(out, "voc.txt")
    write_vocabulary(voc)
    worlds = K.worlds()
    paths = []
    for i, (name, w) in enumerate(worlds.items()):
        paths.append(os.path.join(out, "world_%03d.bin" % i))
        with open(paths[-1], "wb") as f:
            f.write(K.world_bytes(w))
    text = subprocess.run([exe, voc] + paths, check=True, capture_output=True, text=True).stdout
    parts = text.split("world ")[1:]
    assert len(parts) == len(worlds)
    arrays = {}
    for (name, w), part in zip(worlds.items(), parts):
        answers = K.parse_answers(part.split("\n", 1)[1], len(w.kfs))
        assert len(answers) == sum(1 for op in w.ops if op[0] >= K.LOOP), name
        arrays.update(K.golden_arrays(name, w, answers))
    np.savez_compressed(a.out, **arrays)
    print("%s: %d worlds, %d bytes" % (a.out, len(worlds), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
