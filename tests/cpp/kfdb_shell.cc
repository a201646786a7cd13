// kfdb_shell.cc -- GPU test of the KeyFrameDatabase shell (tests/test_gpu_kfdb.py) and the timing behind tools/kfdb_rate.py.
// `kfdb_shell <world file>...`: per file (announced by a `world <file>` line) builds the KeyFrames and Frames of a world the Python test wrote (tests/kfdb_cases.py: world_bytes), plays its
// script on ygz::KeyFrameDatabase over the device -- add / erase / clear, DetectLoopCandidates, ygz::DetectLoopWithMinScore,
// DetectRelocalizationCandidates -- and prints after every query the minimum score, the candidates and every keyframe's six fields in the
// format tests/kfdb_cases.py: parse_answers reads.  Python compares with its restatement.
// `kfdb_shell time <keyframes> <words> <queries> <min repeats> <min seconds>`: a generated store of <keyframes> BowVectors of <words> words out
// of a vocabulary of 100 000, <queries> generated frames.  Three forms, each as the median of its timed repeats with their range:
//   member : DetectRelocalizationCandidates per frame on the device-backed database (one launch per frame + the host bookkeeping)
//   batch  : ygzf_kfdb_query of all frames in one launch on a second context holding the same store (no bookkeeping)
//   host   : the reference's algorithm restated on the host (inverted-file lists, std::map merge score, the same bookkeeping) per frame
// The member form and the host form must return the same candidates.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <list>
#include <random>
#include <string>

#include "KeyFrameDatabase.h"
#include "KeyFrameDatabaseDevice.h"
#include "ORBextractor.h"
#include "ygzf.h"
#include "ygzf_pool.h"

using namespace ygz;

static unsigned bits(float x) { unsigned u; memcpy(&u, &x, 4); return u; }

template <class T> static bool rd(FILE *f, T &v) { return fread(&v, sizeof v, 1, f) == 1; }

static bool read_bow(FILE *f, int n, DBoW2::BowVector &v) {
    if (n < 0) return false;
    std::vector<uint32_t> ids(n);
    std::vector<double> vals(n);
    if (n && (fread(ids.data(), 4, n, f) != (size_t) n || fread(vals.data(), 8, n, f) != (size_t) n)) return false;
    for (int i = 0; i < n; i++) v[ids[i]] = vals[i];
    return true;
}

static int play(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return 2; }
    int nKF = 0, nF = 0, nOps = 0;
    if (!rd(f, nKF) || !rd(f, nF) || !rd(f, nOps) || nKF < 0 || nF < 0 || nOps < 0) return 2;
    std::deque<KeyFrame> kfs(nKF);
    std::deque<Frame> frames(nF);
    for (KeyFrame &k : kfs) {
        int id = 0, bad = 0, n = 0, m = 0, x = 0;
        if (!rd(f, id) || !rd(f, bad) || !rd(f, n) || !read_bow(f, n, k.mBowVec)) return 2;
        k.mnId = (unsigned long) id;
        k.mbBad = bad != 0;
        if (!rd(f, m)) return 2;
        for (; m > 0; m--) { if (!rd(f, x) || x < 0 || x >= nKF) return 2; k.mvpOrderedConnectedKeyFrames.push_back(&kfs[x]); }
        if (!rd(f, m)) return 2;
        for (; m > 0; m--) { if (!rd(f, x) || x < 0 || x >= nKF) return 2; k.mspConnected.insert(&kfs[x]); }
    }
    for (Frame &k : frames) {
        int id = 0, n = 0;
        if (!rd(f, id) || !rd(f, n) || !read_bow(f, n, k.mBowVec)) return 2;
        k.mnId = (unsigned long) id;
    }
    ORBVocabulary voc(1000000);
    KeyFrameDatabase db(voc);
    const unsigned long failuresBefore = ygzf_host::failure_count();
    for (int i = 0; i < nOps; i++) {
        int code = 0, x = 0;
        float b = 0;
        if (!rd(f, code) || !rd(f, x) || !rd(f, b)) return 2;
        if (x < 0 || x >= (code == 5 ? nF : nKF)) return 2;
        if (code == 0) db.add(&kfs[x]);
        else if (code == 1) db.erase(&kfs[x]);
        else if (code == 2) db.clear();
        else {
            float minScore = code == 3 ? b : 0.f;
            std::vector<KeyFrame *> c;
            if (code == 3) c = db.DetectLoopCandidates(&kfs[x], minScore);
            else if (code == 4) c = DetectLoopWithMinScore(&db, &kfs[x], kfs[x].GetVectorCovisibleKeyFrames(), &minScore);
            else c = db.DetectRelocalizationCandidates(&frames[x]);
            printf("q %d %x %zu", i, bits(minScore), c.size());
            for (KeyFrame *k : c) {
                int idx = -1;
                for (int j = 0; j < nKF; j++)
                    if (&kfs[j] == k) idx = j;
                printf(" %d", idx);
            }
            printf("\n");
            for (int k = 0; k < nKF; k++)
                printf("f %d %d %lu %d %x %lu %d %x\n", i, k, kfs[k].mnLoopQuery, kfs[k].mnLoopWords, bits(kfs[k].mLoopScore), kfs[k].mnRelocQuery,
                       kfs[k].mnRelocWords, bits(kfs[k].mRelocScore));
        }
    }
    fclose(f);
    if (ygzf_host::failure_count() != failuresBefore) { printf("failure: %s\n", ygzf_host::last_failure().c_str()); return 1; }
    ReleaseKeyFrameDatabaseDevice(&db);
    printf("kfdb shell ok\n");
    return 0;
}

// ---- the reference's algorithm on the host (src/KeyFrameDatabase.cc:36-41, :180-284), the timing's baseline ------------------------------------
struct HostDb {
    const ORBVocabulary *voc;
    std::vector<std::list<KeyFrame *>> inv;
    HostDb(const ORBVocabulary &v) : voc(&v), inv(v.size()) {}
    void add(KeyFrame *pKF) {
        for (auto &e : pKF->mBowVec) inv[e.first].push_back(pKF);
    }
    std::vector<KeyFrame *> reloc(Frame *F) {
        std::list<KeyFrame *> sharing;
        for (auto &e : F->mBowVec)
            for (KeyFrame *pKFi : inv[e.first]) {
                if (pKFi->mnRelocQuery != F->mnId) {
                    pKFi->mnRelocWords = 0;
                    pKFi->mnRelocQuery = F->mnId;
                    sharing.push_back(pKFi);
                }
                pKFi->mnRelocWords++;
            }
        if (sharing.empty()) return {};
        int maxCommon = 0;
        for (KeyFrame *k : sharing) maxCommon = std::max(maxCommon, k->mnRelocWords);
        const int minCommon = maxCommon * 0.5f;
        std::list<std::pair<float, KeyFrame *>> scored, acc;
        for (KeyFrame *k : sharing)
            if (k->mnRelocWords > minCommon) {
                const float si = voc->score(F->mBowVec, k->mBowVec);
                k->mRelocScore = si;
                scored.push_back({si, k});
            }
        if (scored.empty()) return {};
        float bestAcc = 0;
        for (auto &p : scored) {
            float best = p.first, a = p.first;
            KeyFrame *bestKF = p.second;
            for (KeyFrame *k2 : p.second->GetBestCovisibilityKeyFrames(10)) {
                if (k2->mnRelocQuery != F->mnId) continue;
                a += k2->mRelocScore;
                if (k2->mRelocScore > best) { bestKF = k2; best = k2->mRelocScore; }
            }
            acc.push_back({a, bestKF});
            if (a > bestAcc) bestAcc = a;
        }
        const float retain = 0.75f * bestAcc;
        std::set<KeyFrame *> seen;
        std::vector<KeyFrame *> out;
        for (auto &p : acc)
            if (p.first > retain && !seen.count(p.second)) { out.push_back(p.second); seen.insert(p.second); }
        return out;
    }
};

template <class F> static void timed(const char *name, int minRepeats, double minSeconds, F &&body) {
    std::vector<double> ms;
    body();   // warm-up
    const auto t0 = std::chrono::steady_clock::now();
    while ((int) ms.size() < minRepeats || std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < minSeconds) {
        const auto a = std::chrono::steady_clock::now();
        body();
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count());
        if (ms.size() >= 100000) break;
    }
    std::sort(ms.begin(), ms.end());
    printf("%s median_ms %.4f min_ms %.4f max_ms %.4f repeats %zu\n", name, ms[ms.size() / 2], ms.front(), ms.back(), ms.size());
}

static int time_mode(int nKF, int words, int nQ, int minRepeats, double minSeconds) {
    const unsigned vocWords = 100000;
    std::mt19937 rng(12345);
    auto bow = [&](DBoW2::BowVector &v, unsigned centre) {   // words around a place, so that neighbours in time share many
        std::uniform_int_distribution<unsigned> near(0, 4999), any(0, vocWords - 1);
        std::uniform_real_distribution<double> val(0.02, 1.0);
        double sum = 0;
        while ((int) v.size() < words) {
            const unsigned id = (rng() & 3) ? (centre + near(rng)) % vocWords : any(rng);
            if (v.count(id)) continue;
            const double x = val(rng);
            v[id] = x;
            sum += x;
        }
        for (auto &e : v) e.second /= sum;
    };
    std::deque<KeyFrame> kfs(nKF);
    for (int i = 0; i < nKF; i++) {
        kfs[i].mnId = (unsigned long) i + 1;
        bow(kfs[i].mBowVec, (unsigned) ((long long) i * 37 % vocWords));
        for (int d = 1; d <= 10; d++)
            if (i - d >= 0) kfs[i].mvpOrderedConnectedKeyFrames.push_back(&kfs[i - d]);
    }
    std::deque<Frame> frames(nQ);
    for (int j = 0; j < nQ; j++) bow(frames[j].mBowVec, (unsigned) ((long long) (nKF / (j + 2)) * 37 % vocWords));
    ORBVocabulary voc(vocWords);
    KeyFrameDatabase db(voc);
    HostDb host(voc);
    ygzf_extractor_cfg cfg = {1000, 1.2f, 8, 20, 7, 0};
    ygzf_ctx *ctx = nullptr;
    if (ygzf_create(ORBextractor::sDevice, &cfg, 64, 64, 1, &ctx) != YGZF_OK) { fprintf(stderr, "%s\n", ygzf_last_error(nullptr)); return 1; }
    std::vector<std::vector<uint32_t>> ids(nKF + nQ);
    std::vector<std::vector<double>> vals(nKF + nQ);
    for (int i = 0; i < nKF + nQ; i++)
        for (auto &e : (i < nKF ? kfs[i].mBowVec : frames[i - nKF].mBowVec)) { ids[i].push_back(e.first); vals[i].push_back(e.second); }
    for (int i = 0; i < nKF; i++) {
        db.add(&kfs[i]);
        host.add(&kfs[i]);
        if (ygzf_kfdb_add(ctx, (uint64_t) i, (int) ids[i].size(), ids[i].data(), vals[i].data(), nullptr) != YGZF_OK) { fprintf(stderr, "%s\n", ygzf_last_error(ctx)); return 1; }
    }
    if (ygzf_host::failure_count()) { fprintf(stderr, "%s\n", ygzf_host::last_failure().c_str()); return 1; }
    unsigned long nextId = 1000000;
    std::vector<std::vector<KeyFrame *>> a(nQ), b(nQ);
    char name[128];
    snprintf(name, sizeof name, "keyframes %d words %d queries %d member", nKF, words, nQ);
    timed(name, minRepeats, minSeconds, [&] {
        for (int j = 0; j < nQ; j++) { frames[j].mnId = nextId++; a[j] = db.DetectRelocalizationCandidates(&frames[j]); }
    });
    std::vector<ygzf_kfdb_query_vec> q(nQ);
    for (int j = 0; j < nQ; j++) q[j] = {(int) ids[nKF + j].size(), ids[nKF + j].data(), vals[nKF + j].data()};
    std::vector<int> common((size_t) nQ * nKF), first((size_t) nQ * nKF);
    std::vector<double> score((size_t) nQ * nKF);
    bool ok = true;
    snprintf(name, sizeof name, "keyframes %d words %d queries %d batch", nKF, words, nQ);
    timed(name, minRepeats, minSeconds, [&] { ok = ok && ygzf_kfdb_query(ctx, nQ, q.data(), common.data(), first.data(), score.data()) == YGZF_OK; });
    snprintf(name, sizeof name, "keyframes %d words %d queries %d host", nKF, words, nQ);
    timed(name, minRepeats, minSeconds, [&] {
        for (int j = 0; j < nQ; j++) { frames[j].mnId = nextId++; b[j] = host.reloc(&frames[j]); }
    });
    size_t cands = 0;
    for (int j = 0; j < nQ; j++) { ok = ok && a[j] == b[j]; cands += a[j].size(); }
    printf("candidates %zu same %d failures %lu\n", cands, (int) ok, ygzf_host::failure_count());
    ygzf_destroy(ctx);
    ReleaseKeyFrameDatabaseDevice(&db);
    return ok && !ygzf_host::failure_count() ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc == 7 && !strcmp(argv[1], "time")) return time_mode(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atof(argv[6]));
    if (argc < 2) { fprintf(stderr, "usage: kfdb_shell <world file>... | kfdb_shell time <keyframes> <words> <queries> <min repeats> <min seconds>\n"); return 2; }
    for (int a = 1; a < argc; a++) {
        printf("world %s\n", argv[a]);
        const int rc = play(argv[a]);
        if (rc) return rc;
    }
    return 0;
}
