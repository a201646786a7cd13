#!/usr/bin/env python3
"""tools/plan_sweep.py OUT -- which launch plans the library takes, for comparing two builds (YGZF_LIBRARY selects the other one, tools/ab_libs.sh):
one context per (pin set, geometry) with YGZF_DEBUG=oct, batches of 1, 3, 16 and 17 noise frames each (16 / 17: the small octree plan's limit
at 8 levels), and to OUT per extraction the octree plan lines of the library's report and the FAST kernel ygzf_profile_read names.
YGZF_FORCE stays set for the context's whole life, so a build that reads the pins at every geometry and one that reads them once agree."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

GEOS = [(752, 480, 8, 1000, 1.2), (640, 480, 8, 1000, 1.2), (333, 517, 8, 1500, 1.2), (1280, 360, 6, 1200, 1.2), (1241, 376, 8, 500, 1.2),
        (320, 240, 4, 3000, 1.2), (320, 240, 2, 5000, 1.2), (200, 150, 3, 150, 1.2), (130, 110, 8, 200, 1.2), (1920, 1080, 8, 4000, 1.2),
        (752, 480, 12, 1000, 1.1), (640, 480, 4, 500, 2.0)]
LEVEL1 = [31, 32, 33, 64, 95, 128, 129, 160, 223, 224, 225, 255, 256, 257, 266, 288, 320, 383, 448, 479, 512, 522, 544, 767, 1000]
for sf in (1.1, 1.2, 1.27):                                  # tests/test_gpu_extract.py, test_pyramid_tiles_of_every_fold
    GEOS += [(int(round(w1 * sf)) + 1, [64, 97, 130, 301][i % 4], 3, 200, sf) for i, w1 in enumerate(LEVEL1)]
PINS = [{}, {"oct_plan": "hist"}, {"oct_plan": "sort"}, {"oct_hist_bins": 16}, {"oct_hist_bins": 512}, {"oct_groups": 1}, {"oct_block": 256},
        {"oct_lds_kb": 8}, {"fast_persist": 0}, {"fast_persist": 1}]
KEEP = re.compile(r"\[ygzf octree (small plan|histogram plan|sort plan|single launch)")
FAST = ("k_fast_tab", "k_fast_tab_persist", "k_fast_quads")


def main():
    out = sys.argv[1]
    raw = out + ".stderr"
    fd = os.open(raw, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    os.dup2(fd, 2)                                           # the library reports on stderr
    from orb_ygz_slam_amd import Extractor
    from orb_ygz_slam_amd.capi import force_env
    os.environ["YGZF_DEBUG"] = "oct"
    for pins in PINS:
        os.environ["YGZF_FORCE"] = force_env(base="", **pins)
        for (w, h, nl, nf, sf) in GEOS:
            imgs = np.random.default_rng(w * 7 + h).integers(0, 256, (17, h, w), dtype=np.uint8)
            ex = Extractor(nf, sf, nl, 20, 7, max_width=w, max_height=h, max_batch=17)
            ex.profile_enable(True)
            for n in (1, 3, 16, 17):
                ex.profile_reset()
                os.write(2, ("CASE pins %s geometry %dx%d/%d/%d/%.2f frames %d\n" % (force_env(base="", **pins) or "-", w, h, nl, nf, sf, n)).encode())
                ex.extract_batch_host(imgs[:n])
                prof = ex.profile_read()
                os.write(2, ("FAST %s\n" % ",".join(k for k in FAST if prof.get(k, (0, 0))[1] > 0)).encode())
            ex.close()
    with open(raw) as f, open(out, "w") as o:
        for line in f:
            if line.startswith(("CASE ", "FAST ")) or KEEP.match(line):
                o.write(line)
    os.remove(raw)
    print("plan sweep: %d pin sets x %d geometries -> %s" % (len(PINS), len(GEOS), out))


if __name__ == "__main__":
    main()
