// standalone/KeyFrameDatabase.h -- ygz::KeyFrameDatabase's interface (reference include/KeyFrameDatabase.h:33-65) for builds WITHOUT the
// reference tree (this repository's tests: no OpenCV / DBoW2 installed).  Inside the reference tree this file is not used: KeyFrameDatabase.cc is
// compiled against the reference's own, unchanged include/KeyFrameDatabase.h (found first on the include path) and defines its members.
// The ORBVocabulary here is the slice of the reference's (include/ORBVocabulary.h: DBoW2::TemplatedVocabulary) that the database touches: size()
// and score() with the L1 norm the ORB vocabulary is loaded with (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).
#ifndef YGZ_KEYFRAMEDATABASE_H
#define YGZ_KEYFRAMEDATABASE_H
#include <cmath>
#include <list>
#include <mutex>
#include <vector>

#include "ygz_compat.h"

namespace ygz {

class ORBVocabulary {
public:
    explicit ORBVocabulary(unsigned int words = 0) : mWords(words) {}
    unsigned int size() const { return mWords; }
    double score(const DBoW2::BowVector &v1, const DBoW2::BowVector &v2) const {
        DBoW2::BowVector::const_iterator a = v1.begin(), b = v2.begin();
        double score = 0;
        while (a != v1.end() && b != v2.end()) {
            if (a->first == b->first) {
                score += std::fabs(a->second - b->second) - std::fabs(a->second) - std::fabs(b->second);
                ++a;
                ++b;
            } else if (a->first < b->first) a = v1.lower_bound(b->first);
            else b = v2.lower_bound(a->first);
        }
        return -score / 2.0;
    }

private:
    unsigned int mWords;
};

class KeyFrameDatabase {
public:
    KeyFrameDatabase(const ORBVocabulary &voc);

    void add(KeyFrame *pKF);

    void erase(KeyFrame *pKF);

    void clear();

    // Loop Detection
    std::vector<KeyFrame *> DetectLoopCandidates(KeyFrame *pKF, float minScore);

    // Relocalization
    std::vector<KeyFrame *> DetectRelocalizationCandidates(Frame *F);

protected:
    // Associated vocabulary
    const ORBVocabulary *mpVoc;

    // Inverted file (the device form keeps none: the member stays empty)
    std::vector<std::list<KeyFrame *>> mvInvertedFile;

    // Mutex
    std::mutex mMutex;
};

}  // namespace ygz
#endif
