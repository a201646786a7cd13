"""CPU tier of the constructed stereo cases (tests/stereo_cases.py): the numpy restatement of Frame::ComputeStereoMatches equals the oracle bit
for bit on every case; every case reaches the step it claims (the restatement's trace); every trace code is reached; every wrong form in
MUTATIONS changes the answer of exactly the labelled keypoints declared for it and of no other keypoint of its family's cases, and the forms in
EQUIVALENT change nothing; and the oracle equals the reference's own src/Frame.cc (libref_frame.so, as tests/test_ref_frame.py calls it) on
every case the reference defines.  A model of two of the kernels' shortcuts (the bin scan and the histogram select) says of every case that
its inputs stay inside what those shortcuts assume: a check of the cases, not of the kernels, which only the GPU tier runs."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle_py as O
from tests import stereo_cases as SC

CASES = SC.cases()
IDS = [repr(c) for c in CASES]


@pytest.fixture(scope="module")
def answers(oracle):
    """case -> (the restatement's answer, its trace, the oracle's answer), computed once"""
    out = {}
    for c in CASES:
        trace = []
        r = SC.run_restatement(oracle, c, trace=trace)
        out[repr(c)] = (r, trace, SC.run_oracle(oracle, c))
    return out


def test_scale_tables_are_the_extractors(oracle):
    for n in (8, 12):
        t = oracle.Extractor(1000, 1.2, n, 20, 7).tables()
        s, inv = SC.scale_tables(n)
        assert np.array_equal(s.view(np.uint32), t["scale"].view(np.uint32)) and np.array_equal(inv.view(np.uint32), t["inv_scale"].view(np.uint32))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_oracle(answers, case):
    r, trace, o = answers[repr(case)]
    assert len(trace) == len(case.keys_l) == len(o[0])
    assert SC.same(r, o), [(i, t["code"], r[0][i], o[0][i]) for i, t in enumerate(trace) if r[0][i] != o[0][i] or r[1][i] != o[1][i]][:5]
    for i, t in enumerate(trace):                     # the trace tells the answer: a match exactly where it says ACCEPT
        assert (t["code"] in ("ACCEPT", "ACCEPT_ZERO_DISP")) == (o[0][i] >= 0) == (o[1][i] > 0)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_reaches_what_it_claims(answers, case):
    _, trace, _ = answers[repr(case)]
    assert case.expect and set(case.expect) == set(case.labels)
    assert case.reach(trace) is None, case.reach(trace)
    assert case.undefined is None or case.undefined in SC.UNDEFINED


def test_every_trace_code_is_reached(answers):
    seen = {t["code"] for _, trace, _ in answers.values() for t in trace}
    assert seen == set(SC.CODES)
    claimed = {w["code"] for c in CASES for w in c.expect.values() if "code" in w}
    assert claimed == set(SC.CODES)


def test_sizes_the_families_promise():
    by = {c.name: c for c in CASES}
    assert len(by["n_right_65535"].keys_r) == 65535
    assert sorted(len(by["n_left_%d" % n].keys_l) for n in (1, 3, 4, 5)) == [1, 3, 4, 5]
    assert [len(by["list_%d" % n].keys_l) for n in (1, 2, 3, 4, 1024, 1025, 2500)] == [1, 2, 3, 4, 1024, 1025, 2500]
    assert {c.cfg for c in CASES} == set(SC.CONFIGS)


def _moved(case, a, b):
    ch = np.nonzero((a[0].view(np.uint32) != b[0].view(np.uint32)) | (a[1].view(np.uint32) != b[1].view(np.uint32)))[0]
    spot = lambda i: case.keys_l[i].tobytes() + case.desc_l[i].tobytes()
    return {spot(i) for i in ch}, spot


@pytest.mark.parametrize("mutation", SC.MUTATIONS + SC.EQUIVALENT)
def test_mutation_moves_the_declared_keypoints(oracle, answers, mutation):
    """(a repeated left keypoint counts as the labelled one it repeats)"""
    family = SC.MUTATION_FAMILY[mutation]
    declared = {} if mutation in SC.EQUIVALENT else SC.MOVES[mutation]
    assert mutation in SC.EQUIVALENT or sum(len(v.split()) for v in declared.values()) >= 1
    mine = [c for c in CASES if c.family == family]
    assert set(declared) <= {c.name for c in mine}
    for c in mine:
        got, spot = _moved(c, SC.run_restatement(oracle, c, mutation=mutation), answers[repr(c)][0])
        want = {spot(c.labels[l]) for l in declared.get(c.name, "").split()}
        names = sorted(l for l, i in c.labels.items() if spot(i) in got)
        assert got == want, (c, names, declared.get(c.name))


def test_equivalent_form_argument():
    """thdist_double: SAD < 1.5f * 1.4f * median in float and 10 * SAD < 21 * median in integers agree for every median and the integers around
    the threshold, over the whole range of the SAD"""
    m = np.arange(0, 61201, dtype=np.int64)
    th = (np.float32(1.5) * np.float32(1.4) * m.astype(np.float32)).astype(np.float32)
    for d in (-1, 0, 1, 2):
        s = (21 * m) // 10 + d
        assert np.array_equal(s.astype(np.float32) < th, 10 * s < 21 * m)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_shortcuts_hold_on_the_case(answers, case):
    """a check of the case, not of the kernel (the model is Python written from a reading of the kernels and cannot fail when they change): under
    the model the bins a left keypoint reads hold every right keypoint whose band covers its row, and the two-pass histogram select gives
    element n / 2 of the sorted SADs, so a device answer that differs on the case is not owed to an input outside the shortcuts' assumptions"""
    _, trace, _ = answers[repr(case)]
    s, _ = SC.scale_tables(case.nlevels)
    h = case.left.shape[0]
    for v in {float(k["y"]) for k in case.keys_l}:
        if 0 <= v < h:
            read, covering = SC.model_bin_scan(case.keys_r, s, h, int(v))
            assert read == covering, v
    sads = sorted(t["sad"] for t in trace if t["code"] in ("ACCEPT", "ACCEPT_ZERO_DISP", "CUT"))
    if sads:
        assert SC.model_histogram_median(sads) == sads[len(sads) // 2]


def test_oracle_equals_reference_where_the_reference_is_defined(answers):
    L = O.ref_frame_lib()
    if L is None:
        pytest.skip("oracle/_ref/libref_frame.so not built (reference checkout absent)")
    L.yr_stereo_config.argtypes = [C.c_int, C.c_float]
    L.yo_compute_stereo_matches.restype = None
    L.yo_compute_stereo_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                            C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    excluded = set()
    for c in CASES:
        _, trace, o = answers[repr(c)]
        if not c.ref_defined:
            excluded.add(c.undefined)
            continue
        # a case given to the reference stays inside what it defines: every left row in the table, no clipped band, every patch and window inside
        # its level, at least one accepted match
        h = c.left.shape[0]
        assert all(t["code"] not in ("ROW_OUT", "PATCH_OUT") for t in trace) and any(t["code"] in ("ACCEPT", "ACCEPT_ZERO_DISP", "CUT") for t in trace)
        s, _ = SC.scale_tables(c.nlevels)
        r = np.float32(2) * s[c.keys_r["octave"]]
        assert (np.floor(c.keys_r["y"] - r) >= 0).all() and (np.ceil(c.keys_r["y"] + r) <= h - 1).all()
        L.yr_stereo_config(c.nlevels, 1.2)
        il, ir = np.ascontiguousarray(c.left), np.ascontiguousarray(c.right)
        ur, dp = np.zeros(len(c.keys_l), np.float32), np.zeros(len(c.keys_l), np.float32)
        L.yo_compute_stereo_matches(None, p(il), p(ir), il.shape[1], il.shape[0], len(c.keys_l), p(c.keys_l), p(c.desc_l), len(c.keys_r), p(c.keys_r),
                                    p(c.desc_r), c.mb, c.mbf, p(ur), p(dp))
        assert SC.same((ur, dp), o), c
    assert excluded == set(SC.UNDEFINED)
    assert sorted(c.name for c in CASES if not c.ref_defined) == ["band_clipped", "band_empty", "left_row_outside", "nothing_accepted",
                                                                  "right_window_off_the_left_edge"]
