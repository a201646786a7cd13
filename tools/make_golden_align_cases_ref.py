#!/usr/bin/env python3
"""tools/make_golden_align_cases_ref.py -- what THE REFERENCE'S OWN SparseImgAlign (src/SparseImageAlign.cc + include/NLSSolver_impl.hpp in
oracle/_ref/libref_orbmatcher.so) returns on the constructed cases of tests/align_cases.py (border gates met with equality, stale patches, a level
7 columns wide, points behind the camera, a rollback, ...) -> tests/golden/align_cases_ref.npz: per case the return value, the SE3, the number of
linearisations with the final chi2, and the Hessian.  n_iter = 10, the reference's own table.  Run where the reference checkout is; the replaying
tests need neither the checkout nor the library."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle_py as O  # noqa: E402
from tests import align_cases as AC  # noqa: E402


def main(path=None):
    if O.ref_matcher_lib() is None:
        sys.exit("oracle/_ref/libref_orbmatcher.so is missing: build it from the reference checkout first (make -C oracle ref_matcher)")
    out = {}
    for c in AC.cases():
        with O.reference_matcher():
            ret, T, info, Hm = AC.run_oracle(O, c)
        n = c["name"]
        out["ret_" + n], out["T_" + n], out["info_" + n], out["H_" + n] = np.int64(ret), np.asarray(T, np.float32), np.asarray(info, np.float32), np.asarray(Hm, np.float32)
        print(n, "ret", ret, "T", np.asarray(T), "info", np.asarray(info))
    path = path or os.path.join(ROOT, "tests", "golden", "align_cases_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path)


if __name__ == "__main__":
    main()
