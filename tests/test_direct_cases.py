"""CPU tier of the constructed direct-projection and frustum cases (tests/direct_cases.py): the numpy restatement of FindDirectProjection (from
A_cur_ref onward, plus GetWarpAffineMatrix for identity rotations) and of isInFrustum + PredictScale equals the oracle bit for bit on every
case it covers (NaN for NaN in the singular family), and only the three rotation cases are left out of it; every case is what it claims (the
expectation of every label, the first-principles patches, A == s * I, the reach predicate); every wrong form in the mutation lists changes the
answer of exactly the labels declared for it in MOVES and of no other label of its family, and the form in EQUIVALENT changes nothing; and the
oracle equals the reference's own src/ORBmatcher.cc + src/Align.cc and src/Frame.cc on every case, the rotation family included.  No
comparison here carries a tolerance."""
import numpy as np
import pytest

from oracle import oracle_py as O
from tests import direct_cases as DC

f32 = np.float32
CASES = DC.direct_cases()
IDS = [repr(c) for c in CASES]
FCASES = DC.frustum_cases(O)
FIDS = [repr(c) for c in FCASES]


@pytest.fixture(scope="module")
def answers(oracle):
    """case -> (the restatement's answer or None, its trace, the oracle's answer), computed once"""
    out = {}
    for c in CASES:
        trace = []
        r = DC.run_restatement(oracle, c, trace=trace) if c.restated else None
        out[repr(c)] = (r, trace, DC.run_oracle(oracle, c))
    return out


@pytest.fixture(scope="module")
def fanswers(oracle):
    return {repr(c): (DC.ref_frustum(c), DC.run_frustum_oracle(oracle, c)) for c in FCASES}


def test_ids_are_unique():
    assert len(set(IDS)) == len(IDS) and len(set(FIDS)) == len(FIDS)


def test_scale_tables_are_the_extractors(oracle):
    for sf, n, _, _ in DC.CONFIGS.values():
        t = oracle.Extractor(1000, sf, n, 20, 7).tables()
        mine = DC.scale_tables(sf, n)
        for k in ("scale", "inv_scale", "sigma2", "inv_sigma2"):
            assert np.array_equal(mine[k].view(np.uint32), t[k].view(np.uint32)), (sf, n, k)


def test_every_level_used_holds_patch_and_window(oracle):
    """at most 192 x 144, and every pyramid level holds the 10 x 10 patch plus the 8 x 8 window"""
    for cfg, (sf, n, w, h) in DC.CONFIGS.items():
        assert w <= 192 and h <= 144
        lw, lh = oracle.Extractor(1000, sf, n, 20, 7).level_size(w, h, n - 1)
        assert lw >= 18 and lh >= 18, cfg


# ---- the direct path ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_equals_oracle(answers, case):
    r, trace, o = answers[repr(case)]
    if not case.restated:
        assert case.family == "rotation"
        return
    assert len(trace) == len(case.ref_kp) == len(o[1])
    assert DC.same_direct(r, o) and DC.same_direct(o, r), DC.moved_labels(case, r, o)
    if case.family == "singular":
        assert np.isnan(o[0]).all() and not o[2].any()


def test_only_the_rotation_family_is_left_out():
    out = [c for c in CASES if not c.restated]
    assert len(out) <= 3 and all(c.family == "rotation" for c in out)
    assert {c.family for c in CASES} == {"warp_border", "align_border", "align_values", "singular", "search_level", "rotation", "batch"}
    assert {c.cfg for c in CASES} == {"L8", "P4", "L2", "L1"}


def _count(want, got):
    return got >= int(want[2:]) if isinstance(want, str) else got == want


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_what_it_claims(oracle, answers, case):
    r, trace, o = answers[repr(case)]
    px, sl, ok, pt = o
    assert case.expect and set(case.expect) == set(case.labels)
    assert case.reach() is None, case.reach()
    assert case.undefined is None
    sf, nl, _, _ = DC.CONFIGS[case.cfg]
    tabs = DC.scale_tables(sf, nl)
    groups = {}
    for label, e in case.expect.items():
        i = case.labels[label]
        t = trace[i] if case.restated else {}
        known = {"A", "D", "sl", "code", "updates", "ok", "px", "crop", "zeros", "H", "det_H", "mean_diff", "first_n2", "D_end_gt_3", "D_above_3",
                 "threshold_k", "same", "A_entries_nonzero", "det_negative"}
        assert set(e) <= known, set(e) - known
        if "A" in e:
            assert t["A"] == [e["A"], 0.0, 0.0, e["A"]], (label, t["A"])
        if "D" in e:
            assert t["D"] == e["D"], (label, t["D"])
        if "D_above_3" in e:
            assert t["D"] > 3.0
        if "D_end_gt_3" in e:                                        # the cap, not the threshold, ended the climb
            assert t["D_end"] > 3.0 and t["sl"] == nl - 1
        if "sl" in e:
            assert sl[i] == e["sl"], (label, sl[i])
        if "code" in e:
            assert t["code"] == e["code"], (label, t["code"], t["updates"])
        if "updates" in e:
            assert _count(e["updates"], t["updates"]), (label, t["updates"])
        if "ok" in e:
            assert ok[i] == e["ok"], label
        if "zeros" in e:
            assert int((pt[i] == 0).sum()) == e["zeros"]
        if "H" in e:
            assert (t["H"][0], t["H"][4]) == e["H"] and t["H"][8] == 64.0
        if "det_H" in e:
            H = [f32(v) for v in t["H"]]                              # Matrix3f::inverse()'s determinant, from the first column
            c00, c10, c20 = H[4] * H[8] - H[5] * H[7], H[5] * H[6] - H[3] * H[8], H[3] * H[7] - H[4] * H[6]
            assert (c00 * H[0] + c10 * H[3]) + c20 * H[6] == e["det_H"], label
        if "mean_diff" in e:                                         # the first update's third component takes the whole offset, exactly
            assert t["first_update"][2] == e["mean_diff"], (label, t["first_update"])
        if "first_n2" in e:
            assert float(t["first_n2"]) == e["first_n2"] and t["first_n2"] == f32(0.03 * 0.03), (label, t["first_n2"])
        if e.get("px") == "unchanged":
            assert np.array_equal(px[i].view(np.uint32), case.px0[i].view(np.uint32)), (label, px[i])
        if e.get("px") == "start":
            start = (case.px0[i] * tabs["inv_scale"][sl[i]]) * tabs["scale"][sl[i]]
            assert np.array_equal(px[i].view(np.uint32), start.astype(f32).view(np.uint32)), (label, px[i])
        if e.get("px") == "nan":
            assert np.isnan(px[i]).all() and ok[i] == 0, label
        if "crop" in e:                                              # the warped patch from first principles
            slot, octave, x0, y0 = e["crop"]
            level = oracle.Extractor(1000, sf, nl, 20, 7).pyramid(case.images[slot])[octave] if octave else case.images[slot]
            assert np.array_equal(pt[i], DC.crop_with_zeros(level, x0, y0)), label
        if "threshold_k" in e:
            D = DC.threshold_search()
            below, above = max((v, k) for k, v in D.items() if v < 3.0), min((v, k) for k, v in D.items() if v > 3.0)
            assert (below[1], above[1]) == DC.THRESHOLD_K and 3.0 not in D.values() and e["threshold_k"] in DC.THRESHOLD_K
            assert t["D"] == D[e["threshold_k"]]
        if "A_entries_nonzero" in e:
            A = DC.warp_matrix_f64(case, i)
            assert all(a != 0 for a in A), (label, A)                    # (a claim about the case in double, not a comparison of answers)
        if "det_negative" in e:
            A = DC.warp_matrix_f64(case, i)
            assert A[0] * A[3] - A[1] * A[2] < 0
        if "same" in e:
            groups.setdefault(e["same"], []).append(i)
    for g in groups.values():                                        # copies of one candidate return the same bits wherever they sit
        for i in g[1:]:
            assert DC.same_direct(tuple(x[i:i + 1] for x in o), tuple(x[g[0]:g[0] + 1] for x in o))


def test_sizes_the_families_promise(answers):
    by = {c.name: c for c in CASES if c.family == "batch"}
    assert [len(by["n_%d" % n].ref_kp) for n in (1, 3, 4, 5, 8, 9)] == [1, 3, 4, 5, 8, 9]
    even, odd = by["copies_even"], by["copies_odd"]
    pos = sorted([i for l, i in even.labels.items() if l.startswith("X")] + [i for l, i in odd.labels.items() if l.startswith("X")])
    assert pos == list(range(9))                                       # the copied candidate sits at every position of a 9-batch
    a, b = answers[repr(even)][2], answers[repr(odd)][2]
    i, j = even.labels["X0"], odd.labels["X1"]
    assert DC.same_direct(tuple(x[i:i + 1] for x in a), tuple(x[j:j + 1] for x in b))
    assert len(set(by["two_ref_slots"].ref_slot.tolist())) == 2 and by["cur_is_ref_slot"].cur_slot == by["cur_is_ref_slot"].ref_slot[0]
    codes = {t["code"] for _, trace, _ in answers.values() for t in trace}
    assert codes == {"GATE", "CONVERGED", "EXHAUSTED"}
    assert {s for c in CASES for s in answers[repr(c)][2][1].tolist()} >= {0, 1, 2, 3}


@pytest.mark.parametrize("mutation", DC.DIRECT_MUTATIONS)
def test_direct_mutation_moves_the_declared_labels(oracle, answers, mutation):
    family = DC.MUTATION_FAMILY[mutation]
    declared = DC.MOVES[mutation]
    assert sum(len(v.split()) for v in declared.values()) >= 1
    mine = [c for c in CASES if c.family == family and c.restated]
    assert set(declared) <= {c.name for c in mine}
    for c in mine:
        got = DC.moved_labels(c, DC.run_restatement(oracle, c, mutation=mutation), answers[repr(c)][0])
        assert got == sorted(declared.get(c.name, "").split()), (c, got, declared.get(c.name))


def test_every_listed_mutation_has_a_family():
    assert set(DC.DIRECT_MUTATIONS + DC.FRUSTUM_MUTATIONS + DC.EQUIVALENT) == set(DC.MUTATION_FAMILY)
    assert set(DC.MOVES) == set(DC.DIRECT_MUTATIONS + DC.FRUSTUM_MUTATIONS)
    want = {"warp_lt_w", "warp_le_0", "warp_gt", "align_lo_3", "align_lo_5", "align_hi_open", "level_ge", "level_uncapped", "level_sigma_octave",
            "no_mean_diff", "iters_9", "stop_le", "patch_scale_octave", "hessian_unit_missing", "z_le", "u_open", "v_open", "dist_open", "cos_le",
            "level_floor", "level_unclamped_low", "level_unclamped_high", "xr_plus"}
    assert set(DC.MUTATION_FAMILY) == want


def test_oracle_equals_reference_direct(answers):
    if O.ref_matcher_lib() is None:
        pytest.skip("oracle/_ref/libref_orbmatcher.so not built (reference checkout absent)")
    from tests.test_ref_matcher import _ref_find_direct_projection_batch
    for c in CASES:
        o = answers[repr(c)][2]
        g = DC.run_oracle(O, c, fn=_ref_find_direct_projection_batch)
        assert DC.same_direct(g, o) and DC.same_direct(o, g), (c, DC.moved_labels(c, g, o))


# ---- the frustum ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FCASES, ids=FIDS)
def test_frustum_restatement_equals_oracle(fanswers, case):
    r, o = fanswers[repr(case)]
    assert DC.same_frustum(r, o) and DC.same_frustum(o, r), DC.moved_frustum_labels(case, r, o)


@pytest.mark.parametrize("case", FCASES, ids=FIDS)
def test_frustum_case_is_what_it_claims(fanswers, case):
    _, (iv, px, py, pxr, lv, vc) = fanswers[repr(case)]
    assert case.reach() is None, case.reach()
    assert case.undefined is None
    for label, e in case.expect.items():
        i = case.labels[label]
        assert set(e) <= {"in_view", "u", "v", "level", "cos"}
        if "in_view" in e:
            assert iv[i] == e["in_view"], label
        if "u" in e:
            assert px[i] == f32(e["u"]), (label, px[i])
        if "v" in e:
            assert py[i] == f32(e["v"]), (label, py[i])
        if "level" in e:
            assert lv[i] == e["level"], (label, lv[i])
        if "cos" in e:
            assert vc[i] == f32(e["cos"]) and f32(e["cos"]) == f32(case.limit), (label, vc[i])


def test_frustum_sizes_and_steps(oracle, fanswers):
    by = {c.name: c for c in FCASES}
    assert [len(by["n_%d" % n].a["world"]) for n in (1, 255, 256, 257)] == [1, 255, 256, 257]
    assert {c.family for c in FCASES} == {"depth", "image", "distance", "angle", "level", "mask", "batch"}
    for cfg in ("L8", "L12", "P4", "L1"):
        c = by["steps_%s" % cfg]
        assert sorted(c.steps) == list(range(1, c.nlevels))
        for k, s in c.steps.items():                                 # a step is where the oracle's level changes, and nowhere else below it
            below = np.nextafter(s, f32(0))
            assert list(oracle.predict_scale(np.array([below, s], f32), float(c.lsf), c.nlevels)) == [k - 1, k]
        assert set(fanswers[repr(c)][1][4].tolist()) == set(range(c.nlevels))
    r, o = fanswers[repr(by["posed_257"])]
    assert 50 < int(o[0].sum()) < 257 and not np.array_equal(o[1], o[3])          # projXR differs from projX: mbf is in play
    # one float above each image bound is what the `above` labels project to (the restatement without the gates tells)
    assert f32(256) * f32(0.375 + 2.0 ** -24) + f32(96) == np.nextafter(f32(192), f32(np.inf))
    assert f32(256) * f32(0.28125 + 2.0 ** -24) + f32(72) == np.nextafter(f32(144), f32(np.inf))


@pytest.mark.parametrize("mutation", DC.FRUSTUM_MUTATIONS + DC.EQUIVALENT)
def test_frustum_mutation_moves_the_declared_labels(fanswers, mutation):
    family = DC.MUTATION_FAMILY[mutation]
    declared = {} if mutation in DC.EQUIVALENT else DC.MOVES[mutation]
    assert mutation in DC.EQUIVALENT or sum(len(v.split()) for v in declared.values()) >= 1
    mine = [c for c in FCASES if c.family == family]
    assert mine and set(declared) <= {c.name for c in mine}
    free = DC.MAY_MOVE.get(mutation)
    for c in mine:
        got = DC.moved_frustum_labels(c, DC.ref_frustum(c, mutation=mutation), fanswers[repr(c)][0])
        if free:
            got = [l for l in got if not l.startswith(free)]
        assert got == sorted(declared.get(c.name, "").split()), (c, got, declared.get(c.name))


def test_oracle_equals_reference_frustum(fanswers):
    if O.ref_frame_lib() is None:
        pytest.skip("oracle/_ref/libref_frame.so not built (reference checkout absent)")
    for c in FCASES:
        with O.reference_frame():
            g = DC.run_frustum_oracle(O, c)
        o = fanswers[repr(c)][1]
        assert DC.same_frustum(g, o) and DC.same_frustum(o, g), c


def test_fused_case_matches_on_the_edges(oracle):
    f = DC.fused_case()
    c = f["case"]
    w, h = c.frame
    iv, px, py, pxr, lv, vc = DC.run_frustum_oracle(oracle, c)
    assert iv.all() and px.tolist() == [192.0, 96.0, 192.0, 96.0] and py.tolist() == [72.0, 144.0, 144.0, 72.0]      # exactly on maxX / maxY
    n, match, owner = oracle.search_by_projection_mappoints(f["keys"], f["desc"], c.scale, w, h, c.cam, iv, px, py, vc, lv, f["mp_desc"], f["th"], False, 0.8)
    assert n == 4 and {i: int(m) for i, m in enumerate(match)} == f["expect_match"]
