"""GPU tests of the keyframe database on the device -- ygzf_kfdb_add / _erase / _clear / _size / _query, k_kfdb_query / k_kfdb_repack -- against the
restatement of tests/kfdb_cases.py (which tests/test_kfdb_cases.py pins to the reference's own code on the CPU), exactly: ints, and the fp64
scores by their bits.  Every constructed case and seeded scene with one and with three query vectors per call; slot reuse; growth of the arena
across its initial capacity with repacking; clear; an extraction batch between two passes; the error returns; and the host shell
(csrc/host/KeyFrameDatabase.cc: both Detect members and ygz::DetectLoopWithMinScore) end to end through tests/cpp/kfdb_shell.cc."""
import os
import subprocess

import numpy as np
import pytest

from orb_ygz_slam_amd.capi import KFDB_INITIAL_ENTRIES, KFDB_MAX_QUERY_WORDS, Extractor, YgzfError, make_camera
from tests import kfdb_cases as K
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

WORLDS = K.worlds()
_refs = {}


@pytest.fixture(scope="module")
def ex():
    e = Extractor(1000, 1.2, 8, 20, 7, 752, 480)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got[:2], want[:2])) and np.array_equal(bits(got[2]), bits(want[2]))


def play(ex, w, batch, ref=None):
    """Plays the world's script on the device store beside the restatement's database; at every query operation the store answers the query
    vector (and, batch 3, two more vectors in the same call).  -> per query operation the per-vector (common, first, score) of the device.
    ref: the restatement's answers from an earlier pass (built when None) -> (device, restatement)."""
    ex.kfdb_clear()
    db = K.DB()
    got, want = [], []
    for code, a, _ in w.ops:
        if code == K.ADD:
            db.add(w, a)
            assert ex.kfdb_add(a, w.kfs[a].ids, w.kfs[a].vals) == db.slot_of[a]         # the lowest free slot
        elif code == K.ERASE:
            db.erase(w, a)
            ex.kfdb_erase(a)
        elif code == K.CLEAR:
            db.clear()
            ex.kfdb_clear()
        else:
            q = w.frames[a] if code == K.RELOC else w.kfs[a]
            vecs = [q, w.kfs[len(w.kfs) // 2], K.KF(0, [], [])][:batch]
            assert ex.kfdb_size() == (len(db.slot_of), len(db.slots))
            c, f, s = ex.kfdb_query([(v.ids, v.vals) for v in vecs])
            got.append([(c[i], f[i], s[i]) for i in range(len(vecs))])
            if ref is None:
                want.append([K.store_arrays(w, db, v) for v in vecs])
    return got, (want if ref is None else ref)


def reference(ex, name):
    """(device answers with three vectors per call, the restatement's) of a world: computed once, shared, left unchanged"""
    if name not in _refs:
        _refs[name] = play(ex, WORLDS[name], 3)
    return _refs[name]


@pytest.mark.parametrize("name", list(WORLDS))
def test_query_matches_restatement_three_vectors(ex, name):
    got, want = reference(ex, name)
    assert len(got) == sum(1 for op in WORLDS[name].ops if op[0] >= K.LOOP) > 0
    for i, (g, r) in enumerate(zip(got, want)):
        for v in range(3):
            assert same(g[v], r[v]), (name, i, v, [np.flatnonzero(x != y)[:5] for x, y in zip(g[v][:2], r[v][:2])], np.flatnonzero(bits(g[v][2]) != bits(r[v][2]))[:5])


@pytest.mark.parametrize("name", list(WORLDS))
def test_query_matches_restatement_one_vector_and_the_batch(ex, name):
    got3, want = reference(ex, name)
    got1, _ = play(ex, WORLDS[name], 1, ref=want)
    for g1, g3, r in zip(got1, got3, want):
        assert same(g1[0], r[0]) and same(g1[0], g3[0])


def rows(n, words, seed, universe=20000):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        ids = np.sort(rng.choice(universe, words, replace=False)).astype(np.uint32)
        v = rng.random(words) + 0.02
        out.append((ids, v / v.sum()))
    return out


def expect(q, stored):
    """stored: per slot (ids, vals) or None"""
    c, f, s = np.zeros(len(stored), np.int32), np.full(len(stored), -1, np.int32), np.zeros(len(stored))
    for i, r in enumerate(stored):
        if r is not None:
            s[i], c[i], f[i] = K.l1_score(q[0], q[1], r[0], r[1])
    return c, f, s


def test_add_erase_add_again_reuses_the_lowest_slot(ex):
    ex.kfdb_clear()
    r = rows(6, 50, 1, 400)
    assert [ex.kfdb_add(100 + i, *r[i]) for i in range(5)] == [0, 1, 2, 3, 4]
    ex.kfdb_erase(103)
    ex.kfdb_erase(101)
    ex.kfdb_erase(999)                                                                   # unknown key: nothing happens
    assert ex.kfdb_size() == (3, 5)
    q = r[5]
    assert same(ex.kfdb_query([q]), [x[None] for x in expect(q, [r[0], None, r[2], None, r[4]])])
    assert ex.kfdb_add(101, *r[3]) == 1 and ex.kfdb_add(200, ids=np.zeros(0, np.uint32), vals=np.zeros(0)) == 3 and ex.kfdb_add(201, *r[1]) == 5
    assert ex.kfdb_size() == (6, 6)
    got = ex.kfdb_query([q])
    assert same(got, [x[None] for x in expect(q, [r[0], r[3], r[2], (r[0][0][:0], r[0][1][:0]), r[4], r[1]])])
    assert got[0][0, 3] == 0 and got[1][0, 3] == -1 and bits(got[2][0, 3]) == bits(-0.0)   # an empty stored vector scores -0.0 as the reference's score() does


def test_growth_across_the_initial_capacity_repacks(ex):
    """70 rows of 1 000 words pass the initial 65 536 entries at the 66th; two erased rows leave holes that the repacking closes"""
    ex.kfdb_clear()
    words = 1000
    n_before = KFDB_INITIAL_ENTRIES // words
    r = rows(n_before + 5, words, 2)
    q = rows(2, 800, 3)
    for i in range(n_before):
        assert ex.kfdb_add(i, *r[i]) == i
    ex.kfdb_erase(3)
    ex.kfdb_erase(10)
    assert ex.kfdb_capacity() == (KFDB_INITIAL_ENTRIES, n_before * words)
    before = ex.kfdb_query(q)
    stored = [None if i in (3, 10) else r[i] for i in range(n_before)]
    for v in range(2):
        assert same([x[v] for x in before], expect(q[v], stored))
    assert ex.kfdb_add(1000, *r[n_before]) == 3                                          # does not fit at the top: the arena doubles
    assert ex.kfdb_capacity() == (2 * KFDB_INITIAL_ENTRIES, (n_before - 1) * words)     # ... and the holes are gone
    for i in range(n_before + 1, n_before + 5):
        ex.kfdb_add(1000 + i, *r[i])
    after = ex.kfdb_query(q)
    keep = [i for i in range(n_before) if i not in (3, 10)]
    assert same([x[:, keep] for x in after], [x[:, keep] for x in before])
    stored = [r[n_before] if i == 3 else r[n_before + 1] if i == 10 else r[i] for i in range(n_before)] + r[n_before + 2:]
    for v in range(2):
        assert same([x[v] for x in after], expect(q[v], stored))
    assert ex.kfdb_size() == (n_before + 3, n_before + 3)


@pytest.fixture()
def fresh():
    e = Extractor(1000, 1.2, 8, 20, 7, 64, 64)          # (an arena of the initial size whatever the tests before did)
    yield e
    e.close()


def test_full_arena_with_mostly_holes_repacks_at_the_same_size(fresh):
    """60 rows of 1 000 words, 40 of them erased: the rows that no longer fit behind the last one find room after a repack into an arena of the
    same size (live entries + the new row <= half of it), and every answer stays what it was"""
    ex = fresh
    words = 1000
    r = rows(70, words, 7)
    q = rows(2, 800, 8)
    for i in range(60):
        ex.kfdb_add(i, *r[i])
    for i in range(40):
        ex.kfdb_erase(i)
    cap = ex.kfdb_capacity()[0]
    assert cap == KFDB_INITIAL_ENTRIES
    for i in range(60, 60 + (cap - 60 * words) // words):                               # fill up to the last row that fits
        assert ex.kfdb_add(i, *r[60 + i % 5]) == i - 60
    filled = ex.kfdb_size()[0] - 20
    assert ex.kfdb_capacity()[1] + words > cap and (20 + filled + 1) * words <= cap // 2
    before = ex.kfdb_query(q)
    assert ex.kfdb_add(5000, *r[69]) == filled
    assert ex.kfdb_capacity() == (cap, (20 + filled + 1) * words)                        # same size, no holes
    after = ex.kfdb_query(q)
    keep = [s for s in range(60) if s != filled]
    assert same([x[:, keep] for x in after], [x[:, keep] for x in before])
    stored = [r[60 + (60 + s) % 5] if s < filled else r[69] if s == filled else None if s < 40 else r[s] for s in range(60)]
    for v in range(2):
        assert same([x[v] for x in after], expect(q[v], stored))


def test_clear_empties_the_store(ex):
    r = rows(3, 40, 4, 300)
    ex.kfdb_add(7777, *r[0])
    ex.kfdb_clear()
    assert ex.kfdb_size() == (0, 0)
    c, f, s = ex.kfdb_query([r[2]])
    assert c.shape == f.shape == s.shape == (1, 0)
    assert ex.kfdb_add(7777, *r[0]) == 0 and ex.kfdb_add(5, *r[1]) == 1                 # the key is free again
    assert same(ex.kfdb_query([r[2]]), [x[None] for x in expect(r[2], r[:2])])
    c, f, s = ex.kfdb_query([])
    assert c.shape == (0, 2)


def test_two_passes_with_an_extraction_batch_between():
    """The store keeps its answers across an extraction batch, and a store call between extract_batch_host and match_batch_prev leaves the
    match results unchanged."""
    from orb_ygz_slam_amd.synth import synth_frame
    frames = np.stack([synth_frame(60 + s, 752, 480) for s in range(4)])
    cam = make_camera(752, 480)
    r = rows(12, 300, 5, 3000)
    results, answers = [], []
    for between in (False, True):
        e = Extractor(1000, 1.2, 8, 20, 7, 752, 480, max_batch=4)
        try:
            for i in range(10):
                e.kfdb_add(i, *r[i])
            answers.append(e.kfdb_query(r[10:]))
            e.extract_batch_host(frames[:2])
            e.match_batch_prev(cam)
            e.extract_batch_host(frames[2:])
            if between:
                e.kfdb_erase(4)
                e.kfdb_add(44, *r[4])
                answers.append(e.kfdb_query(r[10:]))
            e.match_batch_prev(cam)
            results.append([e.match_fetch(p) for p in range(2)] + [e.match_counts().copy()])
            answers.append(e.kfdb_query(r[10:]))
        finally:
            e.close()
    for a in answers[1:]:
        assert same(a, answers[0])
    for v in range(2):
        assert same([x[v] for x in answers[0]], expect(r[10 + v], r[:10]))
    for x, y in zip(*results):
        if isinstance(x, tuple):
            for u, v in zip(x, y):
                assert np.array_equal(u, v)
        else:
            assert np.array_equal(x, y)


def test_error_returns_leave_the_store_usable(ex):
    ex.kfdb_clear()
    r = rows(4, 30, 6, 200)
    ex.kfdb_add(1, *r[0])
    ex.kfdb_add(2, *r[1])
    ids, vals = r[2]
    swapped, repeated = ids.copy(), ids.copy()
    swapped[[4, 5]] = swapped[[5, 4]]
    repeated[7] = repeated[6]
    bad_add = [((1, ids, vals), "-5", "already"), ((3, swapped, vals), "-1", "ascending"), ((3, repeated, vals), "-1", "ascending"),
               ((3, np.append(ids[:-1], np.uint32(2 ** 31)), vals), "-1", "2^31"),
               ((3, None, vals, 30), "-1", "null"), ((3, ids, None, 30), "-1", "null"), ((3, ids, vals, -1), "-1", "negative")]
    for args, code, word in bad_add:
        with pytest.raises(YgzfError) as e:
            ex.kfdb_add(*args)
        assert "error " + code in str(e.value) and word in str(e.value), str(e.value)
    assert ex.kfdb_size() == (2, 2)
    long_ids = np.arange(KFDB_MAX_QUERY_WORDS + 1, dtype=np.uint32)
    long_vals = np.full(len(long_ids), 1.0 / len(long_ids))
    bad_query = [([(ids, vals), (long_ids, long_vals)], "-4", "8192"), ([(swapped, vals)], "-1", "ascending"), ([(repeated, vals)], "-1", "ascending"),
                 ([(np.append(ids[:-1], np.uint32(2 ** 31)), vals)], "-1", "2^31"),
                 ([(None, vals)], "-1", "null"), ([(ids, None)], "-1", "null")]
    for qs, code, word in bad_query:
        with pytest.raises(YgzfError) as e:
            ex.kfdb_query(qs)
        assert "error " + code in str(e.value) and word in str(e.value), str(e.value)
        c, f, s = e.value.outputs                                                        # preset before the error return
        assert (c == 0).all() and (f == -1).all() and (bits(s) == 0).all() and c.shape == (len(qs), 2)
    assert same(ex.kfdb_query([(long_ids[:-1], long_vals[:-1])]), [x[None] for x in expect((long_ids[:-1], long_vals[:-1]), r[:2])])   # the limit itself is accepted
    top = (np.append(ids[:-1], np.uint32(2 ** 31 - 1)), vals)                            # the largest id the store takes, as the smallest common word
    assert ex.kfdb_add(3, *top) == 2
    assert same(ex.kfdb_query([top, r[3]]), [np.stack(x) for x in zip(expect(top, r[:2] + [top]), expect(r[3], r[:2] + [top]))])
    ex.kfdb_erase(3)
    assert same(ex.kfdb_query([r[3]]), [x[None] for x in expect(r[3], r[:2] + [None])])


def _build_shell(tmp):
    host = os.path.join(ROOT, "orb_ygz_slam_amd", "csrc", "host")
    lib = os.path.join(ROOT, "orb_ygz_slam_amd", "lib")
    exe = os.path.join(tmp, "kfdb_shell")
    srcs = [os.path.join(ROOT, "tests", "cpp", "kfdb_shell.cc")] + [os.path.join(host, f) for f in ("KeyFrameDatabase.cc", "ORBextractor.cc", "ygzf_pool.cc")]
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-pthread", "-I", host, "-I", os.path.join(host, "standalone"),
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp")] + srcs + ["-L", lib, "-lygzf", "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_kfdb_shell_end_to_end(tmp_path):
    """ygz::KeyFrameDatabase over the device -- add / erase, DetectLoopCandidates, ygz::DetectLoopWithMinScore, DetectRelocalizationCandidates --
    on KeyFrames with BowVectors, covisibility lists and connected sets returns the candidates and the minimum scores of the restatement and
    leaves all six fields of every keyframe as it does, after every query of every world."""
    from orb_ygz_slam_amd import load_library
    load_library()
    exe = _build_shell(str(tmp_path))
    paths = []
    for i, w in enumerate(WORLDS.values()):
        paths.append(os.path.join(str(tmp_path), "world_%03d.bin" % i))
        with open(paths[-1], "wb") as f:
            f.write(K.world_bytes(w))
    out = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.count("kfdb shell ok") == len(WORLDS), out.stdout[-2000:] + out.stderr[-2000:]
    parts = out.stdout.split("world ")[1:]
    assert len(parts) == len(WORLDS)
    for (name, w), part in zip(WORLDS.items(), parts):
        got = K.parse_answers(part.split("\n", 1)[1], len(w.kfs))
        want = K.run(w)
        assert len(got) == len(want) > 0, name
        for g, r in zip(got, want):
            assert g.op == r.op and g.cands == r.cands, (name, g.op, g.cands, r.cands)
            assert g.min_score.view(np.uint32) == r.min_score.view(np.uint32), (name, g.op, g.min_score, r.min_score)
            assert np.array_equal(g.fields, r.fields), (name, g.op, np.argwhere(g.fields != r.fields)[:5])
