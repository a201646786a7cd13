// KeyFrameDatabase.cc -- ygz::KeyFrameDatabase over libygzf (product code, host side).  Replaces the reference's src/KeyFrameDatabase.cc: it
// defines the members of the reference's own class (include/KeyFrameDatabase.h is unchanged; stand-alone: standalone/KeyFrameDatabase.h):
//   KeyFrameDatabase(voc), add, erase, clear               src/KeyFrameDatabase.cc:30-64     ygzf_kfdb_add / _erase / _clear
//   DetectLoopCandidates, DetectRelocalizationCandidates   src/KeyFrameDatabase.cc:67-284    ygzf_kfdb_query
// and ygz::DetectLoopWithMinScore (KeyFrameDatabaseDevice.h), which takes the minimum-score loop of LoopClosing::DetectLoop
// (src/LoopClosing.cc:125-136) from the same launch.
//
// What runs where.  The reference walks an inverted file (per query word, the list of keyframes holding it) to count common words, then calls
// mpVoc->score() per keyframe with enough of them.  Here every added BowVector lives in the device store of a context; one query returns, per
// stored keyframe, the number of common words, the smallest common word and the score.  Everything else -- the mn*Query / mn*Words / m*Score
// fields, the connected-keyframe exclusion, both gates, the covisibility accumulation in float, the retain threshold, the de-duplication -- is
// the reference's code on the real KeyFrame fields, in its order.
//
// The order of lKFsSharingWords.  The reference lists a keyframe when the walk first meets it: query words ascending, each word's list in the
// order of add (erase keeps the relative order of a list).  A keyframe is first met at the smallest word it shares with the query, so that
// order is the keyframes with a common word sorted by (smallest common word, order of add).
//
// Side state.  The class has no member to keep a context in and its header cannot change, so the context, the KeyFrame <-> slot maps and
// the add-sequence numbers live beside the object, keyed by its address.  The constructor resets whatever an earlier object left under the
// same address.  mMutex is taken where the reference takes it (add, erase, the walk of both Detect members -- with the device query in front
// of the walk, nothing of KeyFrame's own accessors under it) and, beyond the reference, in clear(): the device store has one stream.
#include "ORBextractor.h"   // first: inside the reference tree this is the replacement header (same include guard); ORBextractor::sDevice
#include "KeyFrameDatabase.h"
#include "ygz_compat.h"

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <set>
#include <unordered_map>
#include <vector>

#include "../../../include/ygzf.h"
#include "KeyFrameDatabaseDevice.h"
#include "ygzf_pool.h"

namespace ygz {
namespace {

struct Side {
    ygzf_ctx *ctx = nullptr;
    const ORBVocabulary *voc = nullptr;
    std::mutex *mu = nullptr;                              // the object's mMutex
    std::unordered_map<KeyFrame *, int> slotOf;
    std::vector<KeyFrame *> kfOf;                          // per slot; nullptr: free
    std::vector<unsigned long long> seqOf;                 // per slot: order of add
    unsigned long long nextSeq = 0;
};

std::mutex g_mu;
std::unordered_map<const KeyFrameDatabase *, Side *> &sides() {
    static std::unordered_map<const KeyFrameDatabase *, Side *> *m = new std::unordered_map<const KeyFrameDatabase *, Side *>();   // (never destroyed: see ygzf_pool.h)
    return *m;
}

Side *side_of(const KeyFrameDatabase *db) {
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = sides().find(db);
    return it == sides().end() ? nullptr : it->second;
}

bool ensure_ctx(Side &S, const char *who) {
    if (S.ctx) return true;
    // Only the context's stream, staging area and keyframe store are used.  ygzf_create has no lighter form: the context also allocates the
    // extractor's buffers for one 64 x 64 frame (what ygzf_pool's contexts cost as well), once per database.
    ygzf_extractor_cfg cfg = {1000, 1.2f, 8, 20, 7, 0};
    if (ygzf_create(ORBextractor::sDevice, &cfg, 64, 64, 1, &S.ctx) != YGZF_OK) {
        ygzf_host::report_failure(who, ygzf_last_error(nullptr));
        S.ctx = nullptr;
        return false;
    }
    return true;
}

void flatten(const DBoW2::BowVector &v, std::vector<uint32_t> &ids, std::vector<double> &vals) {
    ids.clear();
    vals.clear();
    ids.reserve(v.size());
    vals.reserve(v.size());
    for (DBoW2::BowVector::const_iterator vit = v.begin(), vend = v.end(); vit != vend; vit++) {
        ids.push_back((uint32_t) vit->first);
        vals.push_back((double) vit->second);
    }
}

// One query vector against the store: per slot common words, smallest common word, score.  Called with the object's mutex held.
struct Answer {
    int nSlots = 0;
    std::vector<int> common, first;
    std::vector<double> score;
};
bool query(Side &S, const DBoW2::BowVector &v, Answer &A, const char *who) {
    A.nSlots = 0;
    A.common.clear();
    A.first.clear();
    A.score.clear();
    if (S.kfOf.empty()) return true;
    if (!ensure_ctx(S, who)) return false;
    int nSlots = 0;                                        // the store writes one cell per slot of ITS table: the arrays are sized from it
    if (ygzf_kfdb_size(S.ctx, nullptr, &nSlots) != YGZF_OK || nSlots != (int) S.kfOf.size()) {
        ygzf_host::report_failure(who, "the device store and the host's slot maps disagree about the number of slots");
        return false;
    }
    A.nSlots = nSlots;
    A.common.assign(nSlots, 0);
    A.first.assign(nSlots, -1);
    A.score.assign(nSlots, 0.0);
    std::vector<uint32_t> ids;
    std::vector<double> vals;
    flatten(v, ids, vals);
    ygzf_kfdb_query_vec q = {(int) ids.size(), ids.data(), vals.data()};
    if (ygzf_kfdb_query(S.ctx, 1, &q, A.common.data(), A.first.data(), A.score.data()) != YGZF_OK) {
        ygzf_host::report_failure(who, ygzf_last_error(S.ctx));
        return false;
    }
    return true;
}

// The stored keyframes that share a word with the query, in the order the reference's walk first meets them
std::vector<int> slots_in_walk_order(const Side &S, const Answer &A) {
    std::vector<int> order;
    for (int s = 0; s < A.nSlots; s++)
        if (S.kfOf[s] && A.common[s] > 0) order.push_back(s);
    std::sort(order.begin(), order.end(), [&](int a, int b) {
        if (A.first[a] != A.first[b]) return A.first[a] < A.first[b];
        return S.seqOf[a] < S.seqOf[b];
    });
    return order;
}

// The two Detect members are one procedure over different fields of KeyFrame with three rules of their own (src/KeyFrameDatabase.cc):
//                                   loop (:67-178)                                   relocalisation (:180-284)
//   fields                          mnLoopQuery / mnLoopWords / mLoopScore           mnRelocQuery / mnRelocWords / mRelocScore
//   word gate                       words > int(most * 0.8f)  (:107, :116)           words > int(most * 0.5f)  (:215, :226)
//   score floor                     listed only with score >= minScore, and the      none: every scored keyframe is listed, the best
//                                   best group sum starts at minScore (:122, :131)   group sum starts at 0 (:230, :238)
//   a neighbour joins a group       when this query marked it AND it passed the      when this query marked it, scored now or not: a
//                                   word gate (:144)                                 stale mRelocScore is added (:251-254)
struct Rules {
    long unsigned int KeyFrame::*query;
    int KeyFrame::*words;
    float KeyFrame::*score;
    float gateFactor;
    bool loop;
};
const Rules kLoopRules = {&KeyFrame::mnLoopQuery, &KeyFrame::mnLoopWords, &KeyFrame::mLoopScore, 0.8f, true};
const Rules kRelocRules = {&KeyFrame::mnRelocQuery, &KeyFrame::mnRelocWords, &KeyFrame::mRelocScore, 0.5f, false};

struct Met {
    KeyFrame *kf;
    int slot;                                              // its score is A.score[slot]
};

// The walk over the inverted file (:76-91, :187-200), from the per-slot counts: marks and counts every stored keyframe that shares a word with
// query `id` and returns the ones the reference appends to its list, in its order.  The reference meets a keyframe once per common word; what
// the first meeting decides and what every meeting adds is applied here in one step per keyframe:
//   - already marked with this id (an earlier query with the same id, or a fresh keyframe and id 0): not reset, not listed, the words add on;
//   - in `excluded` (the loop query's connected keyframes): zeroed and counted at every meeting, never marked, so it ends at 1;
//   - otherwise: marked, listed, its count is the common words.
// Called with the object's mutex held.
std::vector<Met> mark_and_list(const Rules &R, const Side &S, const Answer &A, long unsigned int id, const std::set<KeyFrame *> *excluded) {
    std::vector<Met> listed;
    for (int s : slots_in_walk_order(S, A)) {
        KeyFrame *kf = S.kfOf[s];
        if (kf->*R.query == id) {
            kf->*R.words += A.common[s];
        } else if (excluded && excluded->count(kf)) {
            kf->*R.words = 1;
        } else {
            kf->*R.query = id;
            kf->*R.words = A.common[s];
            listed.push_back(Met{kf, s});
        }
    }
    return listed;
}

// From the list to the candidates (:94-177, :202-283).  All sums and comparisons are in float, as the reference's `float` locals are.
std::vector<KeyFrame *> pick_candidates(const Rules &R, long unsigned int id, const std::vector<Met> &listed, const Answer &A, float floor) {
    std::vector<KeyFrame *> out;
    if (listed.empty()) return out;
    int most = 0;
    for (const Met &m : listed) most = std::max(most, m.kf->*R.words);
    const int gate = most * R.gateFactor;                  // (float product, truncated)

    struct Entry {
        float value;
        KeyFrame *kf;
    };
    std::vector<Entry> scored;                             // keyframes past the word gate (and the score floor), in list order
    for (const Met &m : listed) {
        if (!(m.kf->*R.words > gate)) continue;
        const float s = (float) A.score[m.slot];           // what `float si = mpVoc->score(query, stored)` holds
        m.kf->*R.score = s;
        if (!R.loop || s >= floor) scored.push_back(Entry{s, m.kf});
    }
    if (scored.empty()) return out;

    // every scored keyframe gathers its ten best covisible neighbours: the group's sum, and its best-scoring member as the group's candidate
    std::vector<Entry> groups;
    float top = R.loop ? floor : 0.f;
    for (const Entry &e : scored) {
        float sum = e.value, best = e.value;
        KeyFrame *lead = e.kf;
        for (KeyFrame *nb : e.kf->GetBestCovisibilityKeyFrames(10)) {
            if (nb->*R.query != id) continue;
            if (R.loop && !(nb->*R.words > gate)) continue;
            const float s = nb->*R.score;
            sum += s;
            if (s > best) {
                best = s;
                lead = nb;
            }
        }
        groups.push_back(Entry{sum, lead});
        if (sum > top) top = sum;
    }

    // groups above three quarters of the best sum; a keyframe that leads several groups is returned where it first appears
    const float keep = 0.75f * top;
    std::set<KeyFrame *> seen;
    for (const Entry &g : groups)
        if (g.value > keep && seen.insert(g.kf).second) out.push_back(g.kf);
    return out;
}

}  // namespace

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary &voc) : mpVoc(&voc) {
    // (mvInvertedFile stays empty: the store on the device takes its place)
    std::lock_guard<std::mutex> lk(g_mu);
    Side *&S = sides()[this];
    if (!S) S = new Side();
    if (S->ctx) ygzf_kfdb_clear(S->ctx);                  // state of an earlier object at this address
    S->slotOf.clear();
    S->kfOf.clear();
    S->seqOf.clear();
    S->nextSeq = 0;
    S->voc = &voc;
    S->mu = &mMutex;
}

void KeyFrameDatabase::add(KeyFrame *pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    static const char *who = "ygz::KeyFrameDatabase::add";
    Side *S = side_of(this);
    if (!S || !ensure_ctx(*S, who)) return;
    if (S->slotOf.count(pKF)) {                            // the reference would list the keyframe twice per word; the store holds it once
        ygzf_host::report_failure(who, "the keyframe is already in the database (erase it first)");
        return;
    }
    std::vector<uint32_t> ids;
    std::vector<double> vals;
    flatten(pKF->mBowVec, ids, vals);
    int slot = -1;
    if (ygzf_kfdb_add(S->ctx, (uint64_t) (uintptr_t) pKF, (int) ids.size(), ids.data(), vals.data(), &slot) != YGZF_OK) {
        ygzf_host::report_failure(who, ygzf_last_error(S->ctx));
        return;
    }
    if ((size_t) slot >= S->kfOf.size()) {
        S->kfOf.resize((size_t) slot + 1, nullptr);
        S->seqOf.resize((size_t) slot + 1, 0);
    }
    S->kfOf[slot] = pKF;
    S->slotOf[pKF] = slot;
    S->seqOf[slot] = S->nextSeq++;
}

void KeyFrameDatabase::erase(KeyFrame *pKF) {
    std::unique_lock<std::mutex> lock(mMutex);
    Side *S = side_of(this);
    if (!S) return;
    auto it = S->slotOf.find(pKF);
    if (it == S->slotOf.end()) return;                     // never added: the reference's walk finds nothing to erase
    if (ygzf_kfdb_erase(S->ctx, (uint64_t) (uintptr_t) pKF) != YGZF_OK) {
        ygzf_host::report_failure("ygz::KeyFrameDatabase::erase", ygzf_last_error(S->ctx));
        return;
    }
    S->kfOf[it->second] = nullptr;
    S->slotOf.erase(it);
}

void KeyFrameDatabase::clear() {
    std::unique_lock<std::mutex> lock(mMutex);
    Side *S = side_of(this);
    if (!S) return;
    if (S->ctx) ygzf_kfdb_clear(S->ctx);
    S->slotOf.clear();
    S->kfOf.clear();
    S->seqOf.clear();
}

std::vector<KeyFrame *> KeyFrameDatabase::DetectLoopCandidates(KeyFrame *pKF, float minScore) {
    const std::set<KeyFrame *> connected = pKF->GetConnectedKeyFrames();   // before the lock, as :68
    Answer A;
    std::vector<Met> listed;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        Side *S = side_of(this);
        if (!S || !query(*S, pKF->mBowVec, A, "ygz::KeyFrameDatabase::DetectLoopCandidates")) return std::vector<KeyFrame *>();
        listed = mark_and_list(kLoopRules, *S, A, pKF->mnId, &connected);
    }
    return pick_candidates(kLoopRules, pKF->mnId, listed, A, minScore);
}

std::vector<KeyFrame *> DetectLoopWithMinScore(KeyFrameDatabase *db, KeyFrame *pKF, const std::vector<KeyFrame *> &vpConnected, float *minScore) {
    static const char *who = "ygz::DetectLoopWithMinScore";
    if (minScore) *minScore = 1;
    Side *S = side_of(db);
    if (!S) {
        ygzf_host::report_failure(who, "no such database");
        return std::vector<KeyFrame *>();
    }
    // KeyFrame's own accessors run before the database's mutex is taken (they take the keyframes' mutexes in the reference tree)
    const std::set<KeyFrame *> connected = pKF->GetConnectedKeyFrames();
    std::vector<KeyFrame *> good;                          // the covisible keyframes whose score bounds the minimum (src/LoopClosing.cc:126-129)
    for (KeyFrame *kf : vpConnected)
        if (!kf->isBad()) good.push_back(kf);
    Answer A;
    std::vector<Met> listed;
    std::vector<KeyFrame *> notStored;
    float lowest = 1;                                      // (:125)
    {
        std::unique_lock<std::mutex> lock(*S->mu);
        if (!query(*S, pKF->mBowVec, A, who)) return std::vector<KeyFrame *>();
        for (KeyFrame *kf : good) {
            auto it = S->slotOf.find(kf);
            if (it == S->slotOf.end()) notStored.push_back(kf);
            else lowest = std::min(lowest, (float) A.score[it->second]);
        }
        listed = mark_and_list(kLoopRules, *S, A, pKF->mnId, &connected);
    }
    for (KeyFrame *kf : notStored) lowest = std::min(lowest, (float) S->voc->score(pKF->mBowVec, kf->mBowVec));   // on the host, outside the lock
    if (minScore) *minScore = lowest;
    return pick_candidates(kLoopRules, pKF->mnId, listed, A, lowest);
}

void ReleaseKeyFrameDatabaseDevice(KeyFrameDatabase *db) {
    Side *S = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = sides().find(db);
        if (it == sides().end()) return;
        S = it->second;
        sides().erase(it);
    }
    if (S->ctx) ygzf_destroy(S->ctx);
    delete S;
}

std::vector<KeyFrame *> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F) {
    Answer A;
    std::vector<Met> listed;
    {
        std::unique_lock<std::mutex> lock(mMutex);
        Side *S = side_of(this);
        if (!S || !query(*S, F->mBowVec, A, "ygz::KeyFrameDatabase::DetectRelocalizationCandidates")) return std::vector<KeyFrame *>();
        listed = mark_and_list(kRelocRules, *S, A, F->mnId, nullptr);
    }
    return pick_candidates(kRelocRules, F->mnId, listed, A, 0.f);
}

}  // namespace ygz
