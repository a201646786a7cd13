// tools/kfdb_ref_shim/Frame.h -- TEST INFRASTRUCTURE of tools/make_golden_kfdb_ref.py: the two members of ygz::Frame that
// KeyFrameDatabase::DetectRelocalizationCandidates reads.
#ifndef YGZ_FRAME_H_
#define YGZ_FRAME_H_
#include "Common.h"
#include "Thirdparty/DBoW2/DBoW2/BowVector.h"

namespace ygz {
class Frame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};
}  // namespace ygz
#endif
