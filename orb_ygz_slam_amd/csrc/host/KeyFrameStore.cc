// KeyFrameStore.cc -- ygz::KeyFrameDeviceStore::Put over libygzf's resident keyframes (product code, host side; KeyFrameStore.h holds the rest).
#include "ORBextractor.h"   // first: inside the reference tree this is the replacement header (same include guard)
#include "ORBmatcher.h"
#include "ygz_compat.h"

#include "KeyFrameStore.h"
#include "MatcherPack.h"

namespace ygz {

bool KeyFrameDeviceStore::Put(KeyFrame *pKF) {
    const char *who = "ygz::KeyFrameDeviceStore::Put";
    if (!pKF) return false;
    Guard g(*this);
    return g.resident(pKF, pKF->mnId, pKF->N, [&](ygzf_kf_static &rec, std::vector<uint8_t> &hold) { return pack_keyframe_static(pKF, rec, hold, who); }, who);
}

}  // namespace ygz
