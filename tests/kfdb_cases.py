"""Inputs and a numpy / Python restatement for KeyFrameDatabase (reference src/KeyFrameDatabase.cc:36-284), DBoW2's L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) and the minimum-score loop of LoopClosing::DetectLoop (src/LoopClosing.cc:125-136).  No GPU.

A World is plain records: keyframes (mnId, BowVector as ascending ids + values, the ordered covisibility list, the connected set, isBad and the
six query fields), frames (mnId, BowVector) and a script of operations -- add / erase / clear, DetectLoopCandidates with a given minScore,
DetectLoop's pair (minimum score, then DetectLoopCandidates), DetectRelocalizationCandidates.  run(world) plays the script and returns one
Answer per query: minScore, the candidate list, every keyframe's six fields after it, and the double score() gives against every stored keyframe.

run(world, mutation) plays a wrong form (MUTATIONS).  run(world, form="arrays") plays the form the device path takes: per stored keyframe the
number of common words, the smallest common word and the score (store_arrays -- what ygzf_kfdb_query returns per slot), the list built by sorting
on (smallest common word, order of add), everything else as the reference has it.  Both forms must agree everywhere.

cases() are constructed worlds: each has a label, a predicate `reach` over the answers that proves the case is what its label says, and `wrong`,
the wrong forms that change its answers (every other one must leave them alone).  scene(seed) is a seeded world.  tests/test_kfdb_cases.py checks
all of that and pins the restatement to tests/golden/kfdb_ref.npz, which tools/make_golden_kfdb_ref.py records from the reference's own code."""
import numpy as np

MUTATIONS = ("ge_word_gate", "gt_min_score", "ge_retain", "slot_order", "keep_connected", "loop_rule_for_reloc", "acc_f64", "last_duplicate",
             "pairwise_l1", "compare_before_cast")
SCENE_SEEDS = (27, 23, 11, 29)      # scene(seed): 3, 13, 42 and 281 stored keyframes (tests/test_kfdb_cases.py chose them: sizes, every gate bites, pairwise summation shows)
ADD, ERASE, CLEAR, LOOP, LOOP_MIN, RELOC = range(6)
F32 = np.float32


class KF:
    def __init__(self, mnid, ids, vals, cov=(), conn=None, bad=False):
        self.id = int(mnid)
        self.ids = np.ascontiguousarray(ids, np.uint32)
        self.vals = np.ascontiguousarray(vals, np.float64)
        assert len(self.ids) == len(self.vals) and (np.diff(self.ids.astype(np.int64)) > 0).all()
        self.cov = [int(c) for c in cov]                      # mvpOrderedConnectedKeyFrames, as keyframe indices
        self.conn = set(self.cov) if conn is None else set(int(c) for c in conn)   # keys of mConnectedKeyFrameWeights
        self.bad = bool(bad)


class World:
    def __init__(self):
        self.kfs, self.frames, self.ops = [], [], []

    def kf(self, mnid, words, cov=(), conn=None, bad=False):
        """words: dict id -> value, or (ids, vals) -> the keyframe's index"""
        ids, vals = (sorted(words), [words[k] for k in sorted(words)]) if isinstance(words, dict) else words
        self.kfs.append(KF(mnid, ids, vals, cov, conn, bad))
        return len(self.kfs) - 1

    def frame(self, mnid, words):
        ids, vals = (sorted(words), [words[k] for k in sorted(words)]) if isinstance(words, dict) else words
        self.frames.append(KF(mnid, ids, vals))
        return len(self.frames) - 1

    def op(self, code, a=0, b=0.0):
        self.ops.append((int(code), int(a), float(F32(b))))
        return self


def world_bytes(w):
    """The world as tests/cpp/kfdb_shell.cc and the golden tool read it (little endian, int32 unless said otherwise)"""
    out = [np.array([len(w.kfs), len(w.frames), len(w.ops)], np.int32).tobytes()]
    for k in w.kfs:
        cov, conn = np.array(k.cov, np.int32), np.array(sorted(k.conn), np.int32)
        out += [np.array([k.id, int(k.bad), len(k.ids)], np.int32).tobytes(), k.ids.tobytes(), k.vals.tobytes(),
                np.int32(len(cov)).tobytes(), cov.tobytes(), np.int32(len(conn)).tobytes(), conn.tobytes()]
    for f in w.frames:
        out += [np.array([f.id, len(f.ids)], np.int32).tobytes(), f.ids.tobytes(), f.vals.tobytes()]
    for code, a, b in w.ops:
        out += [np.array([code, a], np.int32).tobytes(), F32(b).tobytes()]
    return b"".join(out)


# ---- L1Scoring::score --------------------------------------------------------------------------------------------------------------------------
def _pairwise(t):
    return float(t[0]) if len(t) == 1 else _pairwise(t[:len(t) // 2]) + _pairwise(t[len(t) // 2:])


def l1_score(ids1, vals1, ids2, vals2, pairwise=False):
    """ScoringObject.cpp:23-68 -> (score as the double it returns, common words, smallest common word or -1).  The merge meets the common words
    ascending and adds each term to a double that starts at 0 (:32, :41); np.cumsum adds in that order."""
    _, i1, i2 = np.intersect1d(ids1, ids2, assume_unique=True, return_indices=True)
    vi, wi = vals1[i1], vals2[i2]
    terms = np.abs(vi - wi) - np.abs(vi) - np.abs(wi)                                   # :41
    if pairwise:
        s = 0.0 + _pairwise(terms) if len(terms) else 0.0
    else:
        s = float(np.cumsum(np.concatenate([[0.0], terms]))[-1])
    return np.float64(-s / 2.0), len(i1), int(ids1[i1[0]]) if len(i1) else -1           # :65


# ---- the database ------------------------------------------------------------------------------------------------------------------------------
class DB:
    """mvInvertedFile (word -> keyframe indices in insertion order) and, beside it, what the device store keeps: the slot of every stored
    keyframe (the lowest free one at its add) and its add-sequence number."""

    def __init__(self):
        self.clear()

    def clear(self):                                                                    # :61-64
        self.inv, self.slots, self.slot_of, self.seq, self.n_added = {}, [], {}, {}, 0

    def add(self, w, k):                                                                # :36-41
        assert k not in self.slot_of, "a second add of a stored keyframe is an error of the device path"
        for word in w.kfs[k].ids:
            self.inv.setdefault(int(word), []).append(k)
        free = [s for s, x in enumerate(self.slots) if x is None]
        if free:
            self.slots[free[0]] = k
        else:
            self.slots.append(k)
        self.slot_of[k] = self.slots.index(k)
        self.seq[k] = self.n_added
        self.n_added += 1

    def erase(self, w, k):                                                              # :43-59
        for word in w.kfs[k].ids:
            l = self.inv.get(int(word), [])
            if k in l:
                l.remove(k)
        if k in self.slot_of:
            self.slots[self.slot_of.pop(k)] = None
            del self.seq[k]


def store_arrays(w, db, q, pairwise=False):
    """What ygzf_kfdb_query returns for the query vector q (a KF record) per slot: (common int32, first int32, score float64);
    free slots 0 / -1 / 0.0"""
    S = len(db.slots)
    common, first, score = np.zeros(S, np.int32), np.full(S, -1, np.int32), np.zeros(S, np.float64)
    for s, k in enumerate(db.slots):
        if k is not None:
            score[s], common[s], first[s] = l1_score(q.ids, q.vals, w.kfs[k].ids, w.kfs[k].vals, pairwise)
    return common, first, score


def _encounters(w, db, q, mutation, form):
    """The walk of :76-91 / :187-200 as (keyframe, times met) in the order of first encounter"""
    if form == "arrays" or mutation == "slot_order":
        common, first, _ = store_arrays(w, db, q)
        live = [s for s in range(len(db.slots)) if common[s] > 0]
        if mutation != "slot_order":
            live.sort(key=lambda s: (first[s], db.seq[db.slots[s]]))
        return [(db.slots[s], int(common[s])) for s in live]
    met = {}
    for word in q.ids:
        for k in db.inv.get(int(word), []):
            met[k] = met.get(k, 0) + 1                                                  # (dicts keep the order of first insertion)
    return list(met.items())


def _retain(acc, best_acc, mutation):
    """:158-177 / :266-283"""
    th = 0.75 * best_acc if mutation == "acc_f64" else F32(0.75) * best_acc
    keep = [k for a, k in acc if (a >= th if mutation == "ge_retain" else a > th)]
    if mutation == "last_duplicate":
        return [k for i, k in enumerate(keep) if k not in keep[i + 1:]], th
    return [k for i, k in enumerate(keep) if k not in keep[:i]], th


def detect_loop(w, db, state, qi, min_score, mutation=None, form="reference"):
    """:67-178 -> (candidates, trace).  state: per keyframe [mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore]"""
    q = w.kfs[qi]
    min_score = F32(min_score)
    connected = set() if mutation == "keep_connected" else q.conn                        # :68
    sharing = []
    for k, times in _encounters(w, db, q, mutation, form):
        st = state[k]
        for _ in range(1 if form == "arrays" else times):
            n = times if form == "arrays" else 1
            if st[0] != q.id:                                                           # :82
                st[1] = 0
                if k not in connected:                                                  # :84
                    st[0] = q.id
                    sharing.append(k)
                elif form == "arrays":
                    n = 1                                                               # (every meeting resets a connected keyframe: it ends at 1)
            st[1] += n                                                                  # :89
    trace = dict(sharing=list(sharing), scored=[], acc=[])
    if not sharing:
        return [], trace
    max_common = max(state[k][1] for k in sharing)                                      # :100-105
    min_common = int(F32(max_common) * F32(0.8))                                        # :107
    trace.update(max_common=max_common, min_common=min_common)

    def gate(words):
        return words >= min_common if mutation == "ge_word_gate" else words > min_common
    score_and_match = []
    for k in sharing:
        if gate(state[k][1]):                                                           # :116
            d = l1_score(q.ids, q.vals, w.kfs[k].ids, w.kfs[k].vals, mutation == "pairwise_l1")[0]
            si = F32(d)                                                                 # :119
            state[k][2] = si
            trace["scored"].append(k)
            ok = d >= np.float64(min_score) if mutation == "compare_before_cast" else (si > min_score if mutation == "gt_min_score" else si >= min_score)
            if ok:                                                                      # :122
                score_and_match.append((si, k))
    if not score_and_match:
        return [], trace
    wide = np.float64 if mutation == "acc_f64" else F32
    acc, best_acc = [], wide(min_score)                                                 # :131
    for si, k in score_and_match:
        best, a, best_k = si, wide(si), k
        for k2 in w.kfs[k].cov[:10]:                                                    # :137
            s2 = state[k2]
            if s2[0] == q.id and gate(s2[1]):                                           # :144
                a = wide(a + wide(s2[2]))
                if s2[2] > best:
                    best_k, best = k2, s2[2]
        acc.append((a, best_k))
        if a > best_acc:
            best_acc = a
    trace["acc"] = acc
    out, trace["retain"] = _retain(acc, best_acc, mutation)
    return out, trace


def detect_reloc(w, db, state, fi, mutation=None, form="reference"):
    """:180-284 -> (candidates, trace)"""
    q = w.frames[fi]
    sharing = []
    for k, times in _encounters(w, db, q, mutation, form):
        st = state[k]
        if st[3] != q.id:                                                               # :193
            st[4] = 0
            st[3] = q.id
            sharing.append(k)
        st[4] += times                                                                  # :198
    trace = dict(sharing=list(sharing), scored=[], acc=[])
    if not sharing:
        return [], trace
    max_common = max(state[k][4] for k in sharing)
    min_common = int(F32(max_common) * F32(0.5))                                        # :215
    trace.update(max_common=max_common, min_common=min_common)

    def gate(words):
        return words >= min_common if mutation == "ge_word_gate" else words > min_common
    score_and_match = []
    for k in sharing:
        if gate(state[k][4]):                                                           # :226
            si = F32(l1_score(q.ids, q.vals, w.kfs[k].ids, w.kfs[k].vals, mutation == "pairwise_l1")[0])
            state[k][5] = si
            trace["scored"].append(k)
            score_and_match.append((si, k))
    if not score_and_match:
        return [], trace
    wide = np.float64 if mutation == "acc_f64" else F32
    acc, best_acc = [], wide(0)                                                         # :238
    for si, k in score_and_match:
        best, a, best_k = si, wide(si), k
        for k2 in w.kfs[k].cov[:10]:
            s2 = state[k2]
            if s2[3] != q.id:                                                           # :251
                continue
            if mutation == "loop_rule_for_reloc" and not gate(s2[4]):
                continue
            a = wide(a + wide(s2[5]))                                                   # :254 (a neighbour met but not scored adds its stale score)
            if s2[5] > best:
                best_k, best = k2, s2[5]
        acc.append((a, best_k))
        if a > best_acc:
            best_acc = a
    trace["acc"] = acc
    out, trace["retain"] = _retain(acc, best_acc, mutation)
    return out, trace


def min_score_of(w, qi, pairwise=False):
    """src/LoopClosing.cc:125-136"""
    q = w.kfs[qi]
    m = F32(1)
    for k in q.cov:                                                                     # GetVectorCovisibleKeyFrames
        if w.kfs[k].bad:
            continue
        s = F32(l1_score(q.ids, q.vals, w.kfs[k].ids, w.kfs[k].vals, pairwise)[0])
        if s < m:
            m = s
    return m


class Answer:
    def __init__(self, op, min_score, cands, fields, raw, trace):
        self.op, self.min_score, self.cands, self.fields, self.raw, self.trace = op, F32(min_score), list(cands), fields, raw, trace

    def same(self, o):
        return (self.op == o.op and self.min_score.view(np.uint32) == o.min_score.view(np.uint32) and self.cands == o.cands and
                np.array_equal(self.fields, o.fields) and np.array_equal(np.isnan(self.raw), np.isnan(o.raw)) and
                np.array_equal(np.nan_to_num(self.raw).view(np.uint64), np.nan_to_num(o.raw).view(np.uint64)))


def fields_of(state):
    """-> int64 [keyframes, 6]; the two scores as the bits of their floats"""
    return np.array([[s[0], s[1], int(F32(s[2]).view(np.uint32)), s[3], s[4], int(F32(s[5]).view(np.uint32))] for s in state], np.int64).reshape(-1, 6)


def run(w, mutation=None, form="reference", on_query=None):
    """Plays the script -> [Answer per query operation].  on_query(op index, db, query record) is called before each query (the GPU test
    mirrors the store there)."""
    db = DB()
    state = [[0, 0, F32(0), 0, 0, F32(0)] for _ in w.kfs]
    answers = []
    for i, (code, a, b) in enumerate(w.ops):
        if code == ADD:
            db.add(w, a)
        elif code == ERASE:
            db.erase(w, a)
        elif code == CLEAR:
            db.clear()
        else:
            q = w.frames[a] if code == RELOC else w.kfs[a]
            if on_query:
                on_query(i, db, q)
            raw = np.full(len(w.kfs), np.nan)
            for k in db.slot_of:
                raw[k] = l1_score(q.ids, q.vals, w.kfs[k].ids, w.kfs[k].vals, mutation == "pairwise_l1")[0]
            if code == RELOC:
                m = F32(0)
                c, t = detect_reloc(w, db, state, a, mutation, form)
            else:
                m = min_score_of(w, a, mutation == "pairwise_l1") if code == LOOP_MIN else F32(b)
                c, t = detect_loop(w, db, state, a, m, mutation, form)
            answers.append(Answer(i, m, c, fields_of(state), raw, t))
    return answers


def parse_answers(text, n_kfs):
    """The lines tests/cpp/kfdb_shell.cc and the golden tool's driver print -> [Answer] (raw: NaN everywhere when no `raw` line came)
      raw <op> <score bits per keyframe, hex; NaN: not stored>      q <op> <minScore bits, hex> <n> <candidates>
      f <op> <keyframe> <mnLoopQuery> <mnLoopWords> <mLoopScore bits, hex> <mnRelocQuery> <mnRelocWords> <mRelocScore bits, hex>"""
    raws, out, cur = {}, [], None
    for l in text.splitlines():
        t = l.split()
        if not t:
            continue
        if t[0] == "raw":
            r = np.array([int(x, 16) for x in t[2:]], np.uint64).view(np.float64)
            raws[int(t[1])] = np.where(np.isnan(r), np.nan, r)
        elif t[0] == "q":
            op, n = int(t[1]), int(t[3])
            cur = Answer(op, np.array([int(t[2], 16)], np.uint32).view(F32)[0], [int(x) for x in t[4:4 + n]], np.zeros((n_kfs, 6), np.int64),
                         raws.get(op, np.full(n_kfs, np.nan)), None)
            out.append(cur)
        elif t[0] == "f":
            assert cur is not None and int(t[1]) == cur.op
            cur.fields[int(t[2])] = [int(t[3]), int(t[4]), int(t[5], 16), int(t[6]), int(t[7]), int(t[8], 16)]
    return out


def golden_arrays(name, w, answers):
    """What tests/golden/kfdb_ref.npz holds of one world"""
    import hashlib
    off = np.cumsum([0] + [len(a.cands) for a in answers]).astype(np.int32)
    return {name + "/sha": np.frombuffer(hashlib.sha256(world_bytes(w)).digest(), np.uint8),
            name + "/op": np.array([a.op for a in answers], np.int32),
            name + "/min": np.array([a.min_score for a in answers], F32).view(np.uint32),
            name + "/cand": np.array([c for a in answers for c in a.cands], np.int32), name + "/cand_off": off,
            name + "/fields": np.array([a.fields for a in answers], np.int64).reshape(len(answers), len(w.kfs), 6),
            name + "/raw": np.array([a.raw for a in answers], np.float64).reshape(len(answers), len(w.kfs)).view(np.uint64)}


def worlds():
    """Every world of the tests by name"""
    out = {"case/" + c.label: c.world for c in cases()}
    out.update({"scene/%d" % s: scene(s) for s in SCENE_SEEDS})
    return out


# ---- constructed cases -------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, label, world, reach, wrong=()):
        self.label, self.world, self.reach, self.wrong = label, world, reach, tuple(wrong)


Q8 = {i: 1.0 for i in range(1, 9)}       # the usual query: words 1 .. 8 valued 1, so a stored row of values <= 1 scores the sum of its values


def row(*vals):
    """stored words 1 .. len(vals)"""
    return {i + 1: v for i, v in enumerate(vals)}


def cases():
    out = []

    # maxCommonWords 10 -> minCommonWords int(10 * 0.8f) = 8: eight common words are not scored, nine are
    def build():
        w = World()
        q = w.kf(50, {i: 1.0 for i in range(1, 11)})
        ten, eight, nine = w.kf(1, row(*[0.0625] * 10)), w.kf(2, row(*[0.0625] * 8)), w.kf(3, row(*[0.0625] * 9))
        for k in (ten, eight, nine):
            w.op(ADD, k)
        w.op(LOOP, q, 0.01)
        return (Case("words_at_gate_and_one_above", w, lambda a: a[0].trace["min_common"] == 8 and a[0].fields[eight, 1] == 8 and a[0].fields[nine, 1] == 9 and
                        a[0].trace["scored"] == [ten, nine] and a[0].fields[eight, 2] == 0 and a[0].cands == [ten, nine], ("ge_word_gate",)))
    out.append(build())

    # si == minScore passes `si >= minScore`
    def build():
        w = World()
        q = w.kf(50, Q8)
        hit = w.kf(1, row(0.25, 0, 0, 0, 0, 0, 0, 0))
        w.op(ADD, hit).op(LOOP, q, 0.25)
        return (Case("score_equals_min_score", w, lambda a: F32(a[0].raw[hit]) == a[0].min_score == F32(0.25) and a[0].cands == [hit], ("gt_min_score",)))
    out.append(build())

    # the double is below minScore, the float it becomes is not: the comparison is on the float
    def build():
        w = World()
        q = w.kf(50, Q8)
        hit = w.kf(1, row(0.25 - 2.0 ** -40, 0, 0, 0, 0, 0, 0, 0))
        w.op(ADD, hit).op(LOOP, q, 0.25)
        return (Case("score_rounds_up_to_min_score", w, lambda a: a[0].raw[hit] < 0.25 and F32(a[0].raw[hit]) == F32(0.25) and a[0].cands == [hit],
                        ("compare_before_cast", "gt_min_score")))
    out.append(build())

    # accumulated 0.375 == 0.75f * 0.5: not retained
    def build():
        w = World()
        q = w.kf(50, Q8)
        best, edge = w.kf(1, row(0.125, 0.125, 0.125, 0.125, 0, 0, 0, 0)), w.kf(2, row(0.125, 0.125, 0.125, 0, 0, 0, 0, 0))
        w.op(ADD, best).op(ADD, edge).op(LOOP, q, 0.1)
        return (Case("accumulated_equals_retain_threshold", w, lambda a: a[0].trace["retain"] == F32(0.375) and a[0].trace["acc"][1][0] == F32(0.375) and
                        a[0].cands == [best], ("ge_retain",)))
    out.append(build())

    # 0.25f + (0.125 + 2^-26)f is a tie in float and rounds to 0.375 == the threshold; in double it exceeds it
    def build():
        w = World()
        q = w.kf(50, Q8)
        best = w.kf(1, row(0.5, 0, 0, 0, 0, 0, 0, 0))
        nb = w.kf(2, row(0.125 + 2.0 ** -26, 0, 0, 0, 0, 0, 0, 0))
        a_ = w.kf(3, row(0.25, 0, 0, 0, 0, 0, 0, 0), cov=[nb], conn=[])
        for k in (best, nb, a_):
            w.op(ADD, k)
        w.op(LOOP, q, 0.1)
        return (Case("accumulation_rounds_in_float", w, lambda a: a[0].trace["acc"][2][0] == F32(0.375) and a[0].trace["retain"] == F32(0.375) and
                        a[0].cands == [best], ("acc_f64", "ge_retain")))
    out.append(build())

    # two candidates whose best neighbour is the same keyframe: it is returned once, at its first place
    def build():
        w = World()
        q = w.kf(50, Q8)
        n_ = 4
        a_, x_, b_ = w.kf(1, row(0.25, 0, 0, 0, 0, 0, 0, 0), cov=[n_], conn=[]), w.kf(2, row(0.75, 0, 0, 0, 0, 0, 0, 0)), w.kf(4, row(0.25, 0, 0, 0, 0, 0, 0, 0), cov=[n_], conn=[])
        assert w.kf(7, row(0.5, 0, 0, 0, 0, 0, 0, 0)) == n_
        for k in (a_, x_, b_, n_):
            w.op(ADD, k)
        w.op(LOOP, q, 0.1)
        return (Case("two_candidates_one_best_neighbour", w, lambda a: [k for _, k in a[0].trace["acc"]] == [n_, x_, n_, n_] and a[0].cands == [n_, x_],
                        ("last_duplicate",)))
    out.append(build())

    # added in the order of ids 5, 2, 9, all holding the query's first word: the list is in the order of add
    def build():
        w = World()
        q = w.kf(50, Q8)
        ks = [w.kf(i, row(v, 0, 0, 0, 0, 0, 0, 0)) for i, v in ((5, 0.5), (2, 0.5625), (9, 0.625))]
        for k in ks:
            w.op(ADD, k)
        w.op(LOOP, q, 0.1)
        return (Case("added_out_of_id_order", w, lambda a: a[0].trace["sharing"] == ks and a[0].cands == ks))
    out.append(build())

    # the keyframe added first holds only a late word of the query: it is met after the one added second
    def build():
        w = World()
        q = w.kf(50, Q8)
        late, early = w.kf(1, {5: 0.5, 6: 0.0, 7: 0.0, 8: 0.0}), w.kf(2, {1: 0.5, 2: 0.0, 3: 0.0, 4: 0.0})
        w.op(ADD, late).op(ADD, early).op(LOOP, q, 0.1)
        return (Case("first_encounter_is_not_add_order", w, lambda a: a[0].trace["sharing"] == [early, late] and a[0].cands == [early, late], ("slot_order",)))
    out.append(build())

    # erased and added again: the lowest slot again, but the back of every list
    def build():
        w = World()
        q = w.kf(50, Q8)
        ks = [w.kf(i + 1, row(0.5 + i / 16, 0, 0, 0, 0, 0, 0, 0)) for i in range(3)]
        for k in ks:
            w.op(ADD, k)
        w.op(ERASE, ks[0]).op(ADD, ks[0]).op(LOOP, q, 0.1)
        return (Case("erased_and_added_again_moves_back", w, lambda a: a[0].trace["sharing"] == [ks[1], ks[2], ks[0]] and a[0].cands == [ks[1], ks[2], ks[0]],
                        ("slot_order",)))
    out.append(build())

    # the same query twice: nothing is listed the second time and the word counts double; the connected keyframe ends at 1 both times
    def build():
        w = World()
        c_ = 1
        q = w.kf(50, Q8, cov=[c_])
        assert w.kf(1, row(0.5, 0.25, 0, 0, 0, 0, 0, 0)) == c_
        o_ = w.kf(2, row(0.5, 0.375, 0, 0, 0, 0, 0, 0))
        w.op(ADD, c_).op(ADD, o_).op(LOOP_MIN, q).op(LOOP_MIN, q)
        return (Case("same_query_twice", w, lambda a: a[0].cands == [o_] and a[1].cands == [] and a[0].fields[o_, 1] == 8 and a[1].fields[o_, 1] == 16 and
                        a[0].fields[c_, 1] == 1 and a[1].fields[c_, 1] == 1 and a[0].fields[c_, 0] == 0 and a[0].min_score == F32(0.75), ("keep_connected",)))
    out.append(build())

    # a query keyframe with mnId 0 equals every fresh mnLoopQuery: nothing is reset or listed, the counts add up from 0
    def build():
        w = World()
        q = w.kf(0, Q8)
        o_ = w.kf(2, row(0.5, 0, 0, 0, 0, 0, 0, 0))
        w.op(ADD, o_).op(LOOP, q, 0.1)
        return (Case("query_id_equals_fresh_fields", w, lambda a: a[0].cands == [] and a[0].fields[o_, 1] == 8 and a[0].fields[o_, 2] == 0 and a[0].trace["sharing"] == []))
    out.append(build())

    # an empty BowVector in the store and as the query
    def build():
        w = World()
        q, e_ = w.kf(50, Q8), w.kf(51, {})
        o_, empty = w.kf(2, row(0.5, 0, 0, 0, 0, 0, 0, 0)), w.kf(3, {})
        f_ = w.frame(9, {})
        w.op(ADD, empty).op(ADD, o_).op(LOOP, q, 0.1).op(LOOP, e_, 0.1).op(RELOC, f_)
        return (Case("empty_bow_vectors", w, lambda a: a[0].cands == [o_] and a[1].cands == [] and a[2].cands == [] and (a[2].fields[empty] == 0).all() and
                        a[1].raw[o_] == 0 and np.signbit(a[1].raw[o_]) and np.array_equal(a[0].fields, a[2].fields)))
    out.append(build())

    # no common word
    def build():
        w = World()
        q = w.kf(50, Q8)
        o_ = w.kf(2, {9: 0.5, 100: 0.5})
        f_ = w.frame(9, {10: 1.0})
        w.op(ADD, o_).op(LOOP, q, 0.0).op(RELOC, f_)
        return (Case("no_common_word", w, lambda a: a[0].cands == [] and a[1].cands == [] and (a[1].fields == 0).all() and np.signbit(a[0].raw[o_])))
    out.append(build())

    # a neighbour the query met but did not score: DetectLoopCandidates leaves its stale score out ...
    def stale(loop):
        w = World()
        first_q = {i: 1.0 for i in range(11, 19)}
        nb_words = dict([(1, 0.0625)] + [(i, 0.125) for i in range(11, 19)])               # one word of the second query, all eight of the first
        nb = 0
        if loop:
            q1, q2 = w.kf(60, first_q), w.kf(61, Q8)
            assert w.kf(1, nb_words) == nb + 2
            nb = 2
        else:
            assert w.kf(1, nb_words) == nb
            q1, q2 = w.frame(60, first_q), w.frame(61, Q8)
        a_ = w.kf(2, row(0.25, 0, 0, 0, 0, 0, 0, 0), cov=[nb], conn=[])
        w.op(ADD, nb).op(ADD, a_).op(LOOP if loop else RELOC, q1, 0.1).op(LOOP if loop else RELOC, q2, 0.1)
        return w, nb, a_
    w, nb, a_ = stale(True)
    out.append(Case("loop_neighbour_met_but_not_scored", w, lambda a, nb=nb, a_=a_: a[0].cands == [nb] and a[1].fields[nb, 2] == int(F32(1.0).view(np.uint32)) and
                    a[1].fields[nb, 0] == 61 and a[1].fields[nb, 1] == 1 and a[1].trace["scored"] == [a_] and a[1].trace["acc"] == [(F32(0.25), a_)] and
                    a[1].cands == [a_]))
    # ... DetectRelocalizationCandidates adds it, and the neighbour wins
    w, nb, a_ = stale(False)
    out.append(Case("reloc_neighbour_met_but_not_scored", w, lambda a, nb=nb, a_=a_: a[0].cands == [nb] and a[1].fields[nb, 5] == int(F32(1.0).view(np.uint32)) and
                    a[1].fields[nb, 3] == 61 and a[1].fields[nb, 4] == 1 and a[1].trace["scored"] == [a_] and a[1].trace["acc"] == [(F32(1.25), nb)] and
                    a[1].cands == [nb], ("loop_rule_for_reloc",)))

    # a connected keyframe is never a candidate however well it scores
    def build():
        w = World()
        c_ = 1
        q = w.kf(50, Q8, cov=[], conn=[c_])
        assert w.kf(1, row(0.5, 0.5, 0, 0, 0, 0, 0, 0)) == c_
        o_ = w.kf(2, row(0.25, 0, 0, 0, 0, 0, 0, 0))
        w.op(ADD, c_).op(ADD, o_).op(LOOP, q, 0.1)
        return (Case("connected_keyframe_excluded", w, lambda a: a[0].cands == [o_] and a[0].fields[c_, 1] == 1 and a[0].fields[c_, 0] == 0 and a[0].fields[c_, 2] == 0,
                        ("keep_connected",)))
    out.append(build())

    # word ids near 1 000 000
    def build():
        w = World()
        top = list(range(999990, 1000000))
        q = w.kf(50, {i: 0.1 for i in top})
        o_ = w.kf(2, {i: 0.07 + 0.001 * (i % 7) for i in top[2:]})
        f_ = w.frame(9, {i: 0.3 for i in top[5:]})
        w.op(ADD, o_).op(LOOP, q, 0.1).op(RELOC, f_)
        return (Case("word_ids_near_a_million", w, lambda a: a[0].cands == [o_] and a[1].cands == [o_] and a[0].fields[o_, 1] == 8 and a[1].fields[o_, 4] == 5,
                        ("pairwise_l1",)))
    out.append(build())

    # 8 192 words against 8 192 words (the longest query the device takes), 6 144 of them common
    def build():
        w = World()
        rng = np.random.default_rng(8192)
        ids = np.arange(8192, dtype=np.uint32) * 3 + 1
        unit = lambda v: v / v.sum()
        q = w.kf(50, (ids, unit(rng.random(8192) + 0.05)))
        o_ = w.kf(2, (np.sort(np.concatenate([ids[:6144], ids[6144:] + 1])), unit(rng.random(8192) + 0.05)))
        w.op(ADD, o_).op(LOOP, q, 0.05)
        return (Case("longest_query_against_longest_row", w, lambda a: len(w.kfs[q].ids) == len(w.kfs[o_].ids) == 8192 and a[0].fields[o_, 1] == 6144 and
                        a[0].cands == [o_] and 0.2 < a[0].raw[o_] < 0.8, ("pairwise_l1",)))
    out.append(build())
    return out


# ---- seeded scenes -----------------------------------------------------------------------------------------------------------------------------
def scene(seed):
    """3 to 300 keyframes of 1 to 400 words around a few places, random covisibility, a script of adds in shuffled order, erasures and
    re-adds, loop queries (one of them repeated) and relocalisation queries"""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(3, 301))
    places = max(1, n // 25)
    pools = [rng.choice(3000, 500, replace=False) for _ in range(places)]

    def bow(place):
        k = int(rng.integers(1, 401))
        pool = pools[place]
        ids = np.unique(np.concatenate([rng.choice(pool, min(k, len(pool)), replace=False)[: max(1, (k * 4) // 5)], rng.integers(0, 3000, k // 5 + 1)]))[:k]
        v = rng.random(len(ids)) + 0.02
        return ids.astype(np.uint32), v / v.sum()
    w = World()
    place = rng.integers(0, places, n + 3)                       # (the last three keyframes are the loop queries: never stored)
    for i in range(n + 3):
        same = [j for j in np.flatnonzero(place[:n] == place[i]) if j != i]
        cov = list(rng.permutation(same)[: int(rng.integers(0, 14))]) + list(rng.choice(n, int(rng.integers(0, 3))))
        cov = [int(c) for c in dict.fromkeys(cov) if c != i]
        extra = [int(c) for c in rng.choice(n, int(rng.integers(0, 3))) if c != i]
        w.kf(i + 1, bow(place[i]), cov, conn=cov + extra, bad=rng.random() < 0.1)
    frames = [w.frame(1000 + j, bow(int(rng.integers(0, places)))) for j in range(3)]
    order = rng.permutation(n)
    queries = [n, n + 1, n + 2]
    for k in order[: max(2, (2 * n) // 3)]:
        w.op(ADD, k)
    w.op(LOOP_MIN, queries[0]).op(RELOC, frames[0])
    for k in order[: max(1, n // 6)]:
        w.op(ERASE, k)
    for k in order[max(2, (2 * n) // 3):]:
        w.op(ADD, k)
    w.op(LOOP_MIN, queries[1]).op(RELOC, frames[1])
    for k in order[: max(1, n // 6)][::-1]:
        w.op(ADD, k)
    w.op(LOOP, queries[2], 0.02).op(LOOP, queries[2], 0.02).op(RELOC, frames[2]).op(RELOC, frames[0])
    return w
