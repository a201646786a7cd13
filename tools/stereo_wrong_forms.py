"""The "old" column of DESIGN.md section 2's stereo table, on the CPU: every wrong form of tests/stereo_cases.py switched on in the numpy
restatement and run on the three rendered pairs of tests/test_gpu_stereo.py (oracle keypoints) -> the number of left keypoints whose answer
moves, per pair.  A form that moves none is one those tests cannot see.      python tools/stereo_wrong_forms.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle_py as O                       # noqa: E402
from orb_ygz_slam_amd.scene import stereo_scene         # noqa: E402
from tests import stereo_cases as SC                    # noqa: E402

MB, MBF = 0.11, 47.9
moved = {m: [] for m in SC.MUTATIONS + SC.EQUIVALENT}
for w, h, nfeat, seed in ((752, 480, 1200, 3), (640, 480, 1000, 4), (1280, 720, 2500, 5)):
    left, right, _, _ = stereo_scene(seed, w, h)
    ex = O.Extractor(nfeat, 1.2, 8, 20, 7)
    (kl, dl), (kr, dr) = ex.extract(left), ex.extract(right)
    pl, pr = ex.pyramid(left), ex.pyramid(right)
    s, inv = SC.scale_tables(8)
    run = lambda m: SC.ref_stereo(pl, pr, kl, dl, kr, dr, s, inv, MB, MBF, m)
    base = run(None)
    assert SC.same(base, ex.compute_stereo_matches(left, right, kl, dl, kr, dr, MB, MBF)), "the restatement differs from the oracle"
    for m in moved:
        r = run(m)
        moved[m].append(int(((r[0].view(np.uint32) != base[0].view(np.uint32)) | (r[1].view(np.uint32) != base[1].view(np.uint32))).sum()))
for m, v in moved.items():
    print("%-20s %s" % (m, " / ".join(map(str, v))))
