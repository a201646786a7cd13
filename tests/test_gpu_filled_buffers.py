"""The small suites again, on device memory that starts out hostile: YGZF_DEBUG=fill (csrc/ygzf_internal.h) fills every allocation of a context
with 0xFF and fills the per-call scratch -- dPack, tmp.a/b/c -- again before every use, so a word that a call reads without having written
it is a NaN / -1 / 255 and not the zero of a fresh page or the same case's own earlier answer.  The flag changes no result: every test
selected below must pass under it exactly as without it.

One child pytest per group, one after the other (one GPU process at a time; a child that dies stops its own test only), after the precedent
of test_solver_blocks_beyond_packed_max_bypass_the_staging in tests/test_gpu_pnp.py.  A child must pass at least the number of tests its
selection had without the flag (the selected files are those of the commit before this one; a renamed test fails the group, it does not
shrink it), skip nothing, and
show ygzf_destroy's `[ygzf] fill:` line with allocations -- and, where the group makes packed transfers, scratch refills -- above zero.

Then, in this process, the buffers that legitimately persist between calls (st.*, dir.*, f10.*, grid.*, bow.*): the largest constructed case
and then the smallest on one filled context, against the case module's expected answer and a fresh context's."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

REMAP_TIMEOUT = 50
FILL_LINE = re.compile(r"\[ygzf\] fill: (\d+) allocations, (\d+) scratch refills, (\d+) bytes")


def T(name, *tests):
    """node ids of a file of tests/ (all of it, or the named tests with every parameter)"""
    path = os.path.join("tests", "test_gpu_%s.py" % name)
    return ["%s::%s" % (path, t) for t in tests] or [path]


# group -> (node ids, -k expression or None, tests that pass without the flag, seconds the child took without the flag, packed transfers?)
GROUPS = {
    # n = 0, 1, 2, 3, 63, 64, 65, problems without hypotheses, PnP without masks (its device-only tail), every case twice around another size
    "solvers": (T("pose_opt") + T("sim3") + T("sim3_opt") + T("pnp") + T("tri"),
                "(test_batches or test_mixed_batches or test_without_inlier_bits or test_case_single_call_twice or test_pair_counts_as_one_problem)"
                " and not beyond_packed_max", 205, 3.7, True),
    "matcher": (T("match_cases") + T("stereo_cases") + T("direct_cases") + T("align_cases") + T("bow_cases") + T("distinctive_cases") + T("frustum") +
                T("grid"), None, 947, 3.8, True),
    # (trimmed for time alone: the class shells, and test_constructed_points and test_fuse_reverse_shape, whose host-side expected answers
    # took 7.0 and 1.4 of the whole selection's 12.7 s)
    "stores": (T("kfdb") + T("kf_store") + T("bow_kf") + T("loop_search") + T("fuse"),
               "not shell and not test_constructed_points and not test_fuse_reverse_shape", 143, 4.3, True),
    "detectors": (T("fast_arcs") + T("fast_ring_score") + T("grid_detectors", "test_fast_keypoint_degenerate_images", "test_dso_multilevel_retry_passes") +
                  T("fast10") + T("describe_layout"), None, 58, 5.7, False),
    # (without test_mgpu_tail_chunks_on_one_slot: 3.0 of 6.9 s, and the multi-GPU handle's buffers are not filled)
    "extractor": (T("extract", "test_extract_batch_and_degenerate", "test_carry_previous_switch") + T("context_reuse"),
                  "not test_mgpu_tail_chunks_on_one_slot", 22, 3.8, False),
}


def child_command(group):
    ids, k = GROUPS[group][:2]
    return [sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", "-p", "no:cacheprovider"] + ids + (["-k", k] if k else [])


def fill_env():
    flags = [f for f in os.environ.get("YGZF_DEBUG", "").split(",") if f and f != "fill"]
    return dict(os.environ, YGZF_DEBUG=",".join(flags + ["fill"]))


@pytest.mark.parametrize("group", sorted(GROUPS))
def test_group_passes_on_filled_buffers(group):
    """Without the flag the children took 5.7 and 4.8 s (detectors), 3.8 (extractor), 3.8 and 3.8 (matcher), 3.7 and 3.7 (solvers) and 4.3 s
    (stores) on an MI355X, interpreter start included, and with it 5.0, 3.9, 3.6, 3.6 and 4.2 s (GROUPS holds the larger figure and the
    number of tests that passed).  tests/test_gpu_remap.py is not among them: test_remap_program_on_filled_buffers below.
    The timeout is ten times the figure, a backstop against a hang and no speed assertion."""
    _, _, minimum, seconds, packed = GROUPS[group]
    out = subprocess.run(child_command(group), cwd=ROOT, env=fill_env(), capture_output=True, text=True, timeout=10 * seconds)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    summary = [l for l in out.stdout.splitlines() if re.search(r"\d+ passed", l)]   # (-s: the tests' own prints are in stdout too)
    assert summary and "skipped" not in summary[-1] and "failed" not in summary[-1] and "error" not in summary[-1], out.stdout[-1000:]
    passed = int(re.search(r"(\d+) passed", summary[-1]).group(1))
    lines = [tuple(map(int, l)) for l in FILL_LINE.findall(out.stderr)]
    print("%s: %s; %d contexts: %s allocations, refills, bytes" % (group, summary[-1], len(lines), [sum(x) for x in zip(*lines)]))
    assert passed >= minimum, "%d passed, the selection had %d" % (passed, minimum)
    assert lines and sum(a for a, _, _ in lines) > 0, "no context of the child reported a filled allocation: " + out.stderr[-1000:]
    assert not packed or sum(r for _, r, _ in lines) > 0, "no scratch refill in a group that makes packed transfers"


def test_remap_program_on_filled_buffers(tmp_path):
    """tests/test_gpu_remap.py runs all of its device work in one program of its own (child_main) and keeps that program's stderr, so it cannot
    be a pytest child above: the program itself runs here under the flag -- every case under every path, frame count and pitch class, the
    host form, the remapped pyramid, the extraction behind it, the error returns -- and must leave a record without failures for every check.
    It took 3.8 s without the flag (the setup of tests/test_gpu_remap.py's fixture) and 5.1 s with it on an MI355X; the timeout is ten times that."""
    import json
    import time
    from tests import test_gpu_remap as TR
    out = str(tmp_path / "records.json")
    code = ("import torch\n"
            "torch.cuda.init()\n"
            "import sys\n"
            "sys.path.insert(0, %r)\n"
            "from tests.test_gpu_remap import child_main\n"
            "child_main(%r)\n") % (ROOT, out)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=fill_env(), capture_output=True, text=True, timeout=REMAP_TIMEOUT)
    print("the remap program took %.1f s" % (time.perf_counter() - t0))
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    rec = json.load(open(out))
    assert set(rec) - {"_timing"} == set(TR.CASE_IDS + TR.OTHER_IDS)
    for name in TR.CASE_IDS + TR.OTHER_IDS:
        assert not rec[name]["failures"], "\n".join([name] + rec[name]["failures"][:40])
    lines = [tuple(map(int, l)) for l in FILL_LINE.findall(r.stderr)]
    print("%d contexts: %s allocations, refills, bytes" % (len(lines), [sum(x) for x in zip(*lines)]))
    assert lines and sum(a for a, _, _ in lines) > 0, r.stderr[-1000:]


# ---- large, then small, on one filled context: the buffers that persist between calls ---------------------------------------------------------
# (the matcher's own buffers: test_limit_natural_limit_on_one_context in tests/test_gpu_match_cases.py, the aligner's:
# test_stale_case_then_its_twin_on_one_context in tests/test_gpu_align_cases.py -- both run in the matcher group above)

class Contexts:
    """Extractors of one test: filled() is created under YGZF_DEBUG=fill, fresh() without it; done() closes them and returns the summed
    figures of the fill lines that ygzf_destroy wrote"""

    def __init__(self, capfd):
        self.capfd, self.made = capfd, []

    def _make(self, debug, a, k):
        from orb_ygz_slam_amd import Extractor
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("YGZF_DEBUG", debug)
            self.made.append(Extractor(*a, **k))
        return self.made[-1]

    def filled(self, *a, **k):
        return self._make(fill_env()["YGZF_DEBUG"], a, k)

    def fresh(self, *a, **k):
        return self._make(",".join(f for f in os.environ.get("YGZF_DEBUG", "").split(",") if f and f != "fill"), a, k)

    def done(self):
        self.capfd.readouterr()
        for ex in self.made:
            ex.close()
        lines = FILL_LINE.findall(self.capfd.readouterr().err)
        assert len(lines) == 1 and int(lines[0][0]) > 0, lines
        return tuple(map(int, lines[0]))


@pytest.fixture
def contexts(capfd):
    c = Contexts(capfd)
    yield c
    for ex in c.made:
        ex.close()


def test_stereo_smallest_case_after_the_largest(oracle, contexts):
    """ComputeStereoMatches (st.*): the case with the most right keypoints, the one with the most left keypoints, then the one with a single
    keypoint on either side"""
    from tests import stereo_cases as SC
    cases = [c for c in SC.cases() if c.cfg == "L8"]
    bigs = [max(cases, key=lambda c: len(c.keys_r)), max(cases, key=lambda c: len(c.keys_l))]
    small = min(cases, key=lambda c: (len(c.keys_l), len(c.keys_r)))
    assert len(small.keys_l) == 1 and len(bigs[0].keys_r) == 65535 and len(bigs[1].keys_l) >= 2500, (small, bigs)
    nl, w, h = SC.CONFIGS["L8"]
    ex, fresh = (make(1000, 1.2, nl, 20, 7, max_width=w, max_height=h, max_batch=2) for make in (contexts.filled, contexts.fresh))
    for big in bigs:
        assert SC.same(SC.run_device(ex, big), SC.run_oracle(oracle, big)), big
    got = SC.run_device(ex, small)
    assert SC.same(got, SC.run_oracle(oracle, small)) and SC.same(got, SC.run_device(fresh, small)), (small, got)
    print(bigs, small, contexts.done())


def test_direct_projection_one_candidate_after_the_largest_batch(oracle, contexts):
    """FindDirectProjection (dir.*): the L8 case with the most candidates, with patches, then a one-candidate case"""
    from tests import direct_cases as DC
    cases = [c for c in DC.direct_cases() if c.cfg == "L8"]
    big = max(cases, key=lambda c: len(c.px0))
    small = next(c for c in cases if c.name == "n_1")
    assert len(small.px0) == 1 and len(big.px0) >= 9
    sf, nl, w, h = DC.CONFIGS["L8"]
    ex, fresh = (make(1000, sf, nl, 20, 7, max_width=w, max_height=h, max_batch=1) for make in (contexts.filled, contexts.fresh))
    for e in (ex, fresh):
        e.image_cache_reserve(max(len(big.images), len(small.images)), w, h)
    e_big, e_small = DC.run_oracle(oracle, big), DC.run_oracle(oracle, small)
    g = DC.run_device(ex, big)
    assert DC.same_direct(g, e_big) and DC.same_direct(e_big, g), big
    for want_patches in (True, False):
        g, f = DC.run_device(ex, small, want_patches), DC.run_device(fresh, small, want_patches)
        assert DC.same_direct(g, e_small) and DC.same_direct(e_small, g) and DC.same_direct(g, f) and DC.same_direct(f, g), (small, want_patches, g)
    print(big, small, contexts.done())


def test_bow_one_key_after_the_longest_list_and_the_largest_tree(oracle, contexts):
    """ygzf_bow_transform (bow.*, voc.*): the 16 771-node tree, the 257-key list, then one key"""
    from tests import bow_cases as BC
    by = {c.name: c for c in BC.cases()}
    ex, fresh = (make(max_width=64, max_height=64) for make in (contexts.filled, contexts.fresh))
    assert len(by["branch_129"].voc["parent"]) == 16771 and len(by["batch_257"].desc) == 257 and len(by["batch_1"].desc) == 1
    for name in ("branch_129", "batch_257", "batch_1"):
        c = by[name]
        ex.vocabulary_set(c.voc["parent"], c.voc["desc"], c.voc["L"])
        leaf, nid = ex.bow_transform(c.desc, c.levelsup)
        e_leaf, e_nid = BC.restate(c.voc, c.desc, c.levelsup)
        assert np.array_equal(leaf, e_leaf) and np.array_equal(nid, e_nid), c
    c = by["batch_1"]
    fresh.vocabulary_set(c.voc["parent"], c.voc["desc"], c.voc["L"])
    f_leaf, f_nid = fresh.bow_transform(c.desc, c.levelsup)
    assert np.array_equal(leaf, f_leaf) and np.array_equal(nid, f_nid)
    print(contexts.done())


def test_features_in_area_one_key_after_five_thousand(oracle, contexts):
    """ygzf_features_in_area: 5000 keypoints crowded into few cells with a query that returns most of them, then one keypoint and one query
    (the inputs of test_features_in_area_edges in tests/test_gpu_grid.py)"""
    from orb_ygz_slam_amd import make_camera, KP_DTYPE
    w, h = 752, 480
    ex, fresh = (make(1000, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=1) for make in (contexts.filled, contexts.fresh))
    cam, sf = make_camera(w, h), ex.tables()["scale"]
    rng = np.random.default_rng(9)
    k = np.zeros(5000, KP_DTYPE)
    k["x"] = np.concatenate([rng.uniform(100, 130, 3000), rng.choice([0.0, 11.75, 23.5, 751.0, 5.875], 2000)]).astype(np.float32)
    k["y"] = np.concatenate([rng.uniform(200, 215, 3000), rng.choice([0.0, 10.0, 20.0, 479.0, 5.0], 2000)]).astype(np.float32)
    k["octave"] = rng.integers(0, 8, 5000)
    xyr = np.array([[115, 207, 30], [400, 240, 2000], [0, 0, 12], [115, 207, 0]], np.float32)
    lv = np.array([[-1, -1], [-1, -1], [0, -1], [2, 5]], np.int32)

    def expected(keys, q):
        return oracle.features_in_area(keys, sf, w, h, float(xyr[q, 0]), float(xyr[q, 1]), float(xyr[q, 2]), int(lv[q, 0]), int(lv[q, 1]))
    got, cnt = ex.features_in_area(cam, k, xyr, lv)
    for q in range(len(xyr)):
        assert cnt[q] == len(expected(k, q)) and np.array_equal(got[q], expected(k, q)), q
    assert cnt[1] > 4000
    one = k[100:101]
    for q in (0, 2, 3):            # the key lies inside the first query's circle alone
        got, cnt = ex.features_in_area(cam, one, xyr[q:q + 1], lv[q:q + 1])
        f_got, f_cnt = fresh.features_in_area(cam, one, xyr[q:q + 1], lv[q:q + 1])
        assert cnt[0] == len(expected(one, q)) == f_cnt[0] and np.array_equal(got[0], expected(one, q)) and np.array_equal(got[0], f_got[0]), q
    assert len(expected(one, 0)) == 1
    print(contexts.done())


def _noise_and_flat():
    return np.random.default_rng(3).integers(0, 256, (240, 320), dtype=np.uint8), np.full((82, 82), 77, np.uint8)


def test_fast10_small_images_after_320x240_noise(oracle, contexts):
    """the Thirdparty/fast replacement (f10.*): 320 x 240 noise at a low barrier, then an 82 x 82 flat image and 30 x 22 noise"""
    noise, flat = _noise_and_flat()
    ex, fresh = (make(max_width=64, max_height=64) for make in (contexts.filled, contexts.fresh))
    tiny = np.random.default_rng(4).integers(0, 256, (30, 22), dtype=np.uint8)
    for img, thr in ((noise, 5), (flat, 20), (tiny, 20), (noise, 40), (tiny, 5)):
        got, exp = ex.fast10(img, thr), oracle.fast10(img, thr)
        assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got, exp)), (img.shape, thr)
        if img is not noise:
            assert all(a.shape == b.shape and (a == b).all() for a, b in zip(got, fresh.fast10(img, thr))), (img.shape, thr)
    assert len(oracle.fast10(noise, 5)[0]) > 1000 and len(oracle.fast10(flat, 20)[0]) == 0 and len(oracle.fast10(tiny, 5)[0]) > 0
    print(contexts.done())


def _same_keys(k, d, ok, od, what):
    assert len(k) == len(ok), (what, len(k), len(ok))
    for f in ("x", "y", "size", "angle", "response", "octave", "class_id"):
        assert np.array_equal(k[f], ok[f]), (what, f)
    assert np.array_equal(d, od), what


@pytest.mark.parametrize("detector", ["fast_keypoint", "dso_multilevel", "dso"])
def test_grid_detector_82x82_flat_after_320x240_noise(oracle, contexts, detector):
    """the DSO / FAST_KEYPOINT detectors (grid.*, f10.*): 320 x 240 noise, then an 82 x 82 flat image, then the noise again"""
    noise, flat = _noise_and_flat()
    ex, fresh = (make(500, 1.2, 4, 20, 7, max_width=320, max_height=240, max_batch=1) for make in (contexts.filled, contexts.fresh))

    def device(e, img):
        return {"fast_keypoint": e.extract_fast_keypoint, "dso_multilevel": e.extract_dso_multilevel, "dso": e.extract_dso}[detector](img)

    def expected(img):
        oex = oracle.Extractor(500, 1.2, 4, 20, 7)
        return {"fast_keypoint": oex.extract_fast, "dso_multilevel": oex.extract_dso_multilevel, "dso": oex.extract_dso}[detector](img)
    for img in (noise, flat, noise):
        g, e = device(ex, img), expected(img)
        _same_keys(g[0], g[1], e[0], e[1], (detector, img.shape))
        assert g[2:] == e[2:], (detector, img.shape, g[2:], e[2:])            # mnGridSize
        if img is flat:
            f = device(fresh, img)
            _same_keys(g[0], g[1], f[0], f[1], (detector, "fresh"))
            assert g[2:] == f[2:]
    assert len(expected(noise)[0]) > 100
    print(contexts.done())


def test_describe_one_key_after_all_keys_of_320x240_noise(oracle, contexts):
    """ygzf_describe_keys (grid.list, grid.angles): every key of the extracted noise image, then one key, with and without IC_Angle"""
    noise, _ = _noise_and_flat()
    ex, fresh = (make(500, 1.2, 4, 20, 7, max_width=320, max_height=240, max_batch=1) for make in (contexts.filled, contexts.fresh))
    oex = oracle.Extractor(500, 1.2, 4, 20, 7)
    keys, desc = oex.extract(noise)
    assert len(keys) > 300
    for e in (ex, fresh):
        e.extract_batch_host(noise[None])
    for recompute in (False, True):
        ang, d = ex.describe_keys(keys, frame=0, recompute_angle=recompute)
        ok, od = oex.describe_keys(noise, keys, recompute)
        assert np.array_equal(d, od) and (not recompute or np.array_equal(ang, ok["angle"])), recompute
        assert recompute or np.array_equal(d, desc)
        one = keys[len(keys) // 2:len(keys) // 2 + 1]
        ang, d = ex.describe_keys(one, frame=0, recompute_angle=recompute)
        ok, od = oex.describe_keys(noise, one, recompute)
        f_ang, f_d = fresh.describe_keys(one, frame=0, recompute_angle=recompute)
        assert np.array_equal(d, od) and np.array_equal(d, f_d) and (not recompute or (np.array_equal(ang, ok["angle"]) and np.array_equal(ang, f_ang))), recompute
    print(contexts.done())
