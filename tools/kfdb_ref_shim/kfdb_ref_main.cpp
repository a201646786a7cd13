// tools/kfdb_ref_shim/kfdb_ref_main.cpp -- TEST INFRASTRUCTURE of tools/make_golden_kfdb_ref.py: plays a world file (tests/kfdb_cases.py:
// world_bytes) on the REFERENCE's own KeyFrameDatabase (src/KeyFrameDatabase.cc, compiled where it lies) with the reference's own DBoW2 behind
// mpVoc->score, and prints the answers in the format tests/kfdb_cases.py: parse_answers reads.  The minimum score of LOOP_MIN is the loop of
// src/LoopClosing.cc:125-136 with the vocabulary's score().
//   usage: kfdb_ref <vocabulary.txt> <world.bin>...
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "Frame.h"
#include "KeyFrame.h"
#include "KeyFrameDatabase.h"

using namespace ygz;

template <class T> static T rd(std::ifstream &f) { T v; f.read((char *) &v, sizeof v); return v; }

static void read_bow(std::ifstream &f, int n, DBoW2::BowVector &v) {
    std::vector<uint32_t> ids(n);
    std::vector<double> vals(n);
    f.read((char *) ids.data(), 4 * (size_t) n);
    f.read((char *) vals.data(), 8 * (size_t) n);
    for (int i = 0; i < n; i++) v.insert(v.end(), std::make_pair(ids[i], vals[i]));
}

static unsigned bits(float x) { unsigned u; memcpy(&u, &x, 4); return u; }
static unsigned long long bits(double x) { unsigned long long u; memcpy(&u, &x, 8); return u; }

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    ORBVocabulary voc;
    if (!voc.loadFromTextFile(argv[1])) return 3;
    for (int a = 2; a < argc; a++) {
        std::ifstream f(argv[a], std::ios::binary);
        if (!f) return 4;
        const int nKF = rd<int>(f), nF = rd<int>(f), nOps = rd<int>(f);
        std::vector<KeyFrame> kfs(nKF);
        std::vector<Frame> frames(nF);
        for (KeyFrame &k : kfs) {
            k.mnId = (long unsigned) rd<int>(f);
            k.bad = rd<int>(f) != 0;
            read_bow(f, rd<int>(f), k.mBowVec);
            for (int n = rd<int>(f); n > 0; n--) k.ordered.push_back(&kfs[rd<int>(f)]);
            for (int n = rd<int>(f); n > 0; n--) k.connected.insert(&kfs[rd<int>(f)]);
            if (!k.mBowVec.empty() && k.mBowVec.rbegin()->first >= voc.size()) return 5;
        }
        for (Frame &k : frames) {
            k.mnId = (long unsigned) rd<int>(f);
            read_bow(f, rd<int>(f), k.mBowVec);
            if (!k.mBowVec.empty() && k.mBowVec.rbegin()->first >= voc.size()) return 5;
        }
        printf("world %s\n", argv[a]);
        KeyFrameDatabase db(voc);
        std::vector<char> stored(nKF, 0);
        for (int i = 0; i < nOps; i++) {
            const int code = rd<int>(f), x = rd<int>(f);
            const float b = rd<float>(f);
            if (code == 0) { db.add(&kfs[x]); stored[x] = 1; }
            else if (code == 1) { db.erase(&kfs[x]); stored[x] = 0; }
            else if (code == 2) { db.clear(); std::fill(stored.begin(), stored.end(), 0); }
            else {
                const DBoW2::BowVector &q = code == 5 ? frames[x].mBowVec : kfs[x].mBowVec;
                printf("raw %d", i);
                for (int k = 0; k < nKF; k++) printf(" %llx", stored[k] ? bits(voc.score(q, kfs[k].mBowVec)) : bits((double) NAN));
                printf("\n");
                float minScore = code == 3 ? b : 0.f;
                std::vector<KeyFrame *> c;
                if (code == 5) c = db.DetectRelocalizationCandidates(&frames[x]);
                else {
                    if (code == 4) {   // the lowest score of the query against its covisible keyframes that are not bad, 1 at most (src/LoopClosing.cc:123-136)
                        minScore = 1;
                        for (KeyFrame *other : kfs[x].ordered)
                            if (!other->bad) minScore = std::min(minScore, (float) voc.score(q, other->mBowVec));
                    }
                    c = db.DetectLoopCandidates(&kfs[x], minScore);
                }
                printf("q %d %x %zu", i, bits(minScore), c.size());
                for (KeyFrame *k : c) printf(" %d", (int) (k - kfs.data()));
                printf("\n");
                for (int k = 0; k < nKF; k++)
                    printf("f %d %d %lu %d %x %lu %d %x\n", i, k, kfs[k].mnLoopQuery, kfs[k].mnLoopWords, bits(kfs[k].mLoopScore), kfs[k].mnRelocQuery,
                           kfs[k].mnRelocWords, bits(kfs[k].mRelocScore));
            }
        }
    }
    return 0;
}
