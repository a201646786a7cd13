// KeyFrameDatabaseDevice.h -- what host/KeyFrameDatabase.cc offers beside the members of ygz::KeyFrameDatabase.
//   ygz::DetectLoopWithMinScore: the two steps of LoopClosing::DetectLoop that read the vocabulary -- the minimum score over the connected
//   keyframes (src/LoopClosing.cc:125-136) and mpKeyFrameDB->DetectLoopCandidates(mpCurrentKF, minScore) (:139) -- from ONE device query: the
//   score of the current keyframe against every stored keyframe serves both.  vpConnected = mpCurrentKF->GetVectorCovisibleKeyFrames() (:123);
//   bad keyframes are skipped (:128); a connected keyframe that is not in the database is scored on the host with the vocabulary's score().
//   *minScore receives the minimum (1 when nothing lowers it).  Returns what DetectLoopCandidates returns and leaves every field as it does.
//   ygz::ReleaseKeyFrameDatabaseDevice: frees the device store and the side state of a database that is about to be destroyed (the reference's
//   class has no destructor to do it in; without the call the state lives until the process ends or a database is constructed at the same address).
// A device failure goes through ygzf_host::report_failure: the answer is empty and no field is written.
#ifndef YGZF_KEYFRAMEDATABASE_DEVICE_H
#define YGZF_KEYFRAMEDATABASE_DEVICE_H
#include <vector>

#include "KeyFrameDatabase.h"
#include "ygz_compat.h"

namespace ygz {
std::vector<KeyFrame *> DetectLoopWithMinScore(KeyFrameDatabase *db, KeyFrame *pKF, const std::vector<KeyFrame *> &vpConnected, float *minScore);
void ReleaseKeyFrameDatabaseDevice(KeyFrameDatabase *db);
}  // namespace ygz
#endif
