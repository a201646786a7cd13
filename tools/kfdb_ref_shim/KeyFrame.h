// tools/kfdb_ref_shim/KeyFrame.h -- TEST INFRASTRUCTURE of tools/make_golden_kfdb_ref.py: the members of ygz::KeyFrame that the reference's
// src/KeyFrameDatabase.cc and the minimum-score loop of LoopClosing::DetectLoop touch, as plain data (types and initial values as
// include/KeyFrame.h:276-281 and src/KeyFrame.cc:381-402 have them).
#ifndef YGZ_KEYFRAME_H_
#define YGZ_KEYFRAME_H_
#include "Common.h"
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"

namespace ygz {
class KeyFrame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = 0;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;

    std::set<KeyFrame *> GetConnectedKeyFrames() { return connected; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return ordered; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N) {
        if ((int) ordered.size() < N) return ordered;
        return std::vector<KeyFrame *>(ordered.begin(), ordered.begin() + N);
    }
    bool isBad() { return bad; }

    std::set<KeyFrame *> connected;
    std::vector<KeyFrame *> ordered;
    bool bad = false;
};
}  // namespace ygz
#endif
