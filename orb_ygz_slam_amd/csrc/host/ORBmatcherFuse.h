// ORBmatcherFuse.h -- ygz::FuseBatch (host/ORBmatcherFuse.cc): the forward pass of LocalMapping::SearchInNeighbors
// (src/LocalMapping.cc:1259-1269), `for (pKFi : targets) ORBmatcher::Fuse(pKFi, points, th)`, as one device batch with the same result.
// Returns the summed nFused of the targets it applied.  A device failure goes through ygzf_host::report_failure and stops the batch: when the
// first candidate query fails nothing is fused and 0 is returned; when a later query fails (the re-search of Replace survivors before a target
// step) the targets before that step stay fused, exactly as the sequential loop would have left them, and the return value counts them.
#ifndef YGZF_ORBMATCHER_FUSE_H
#define YGZF_ORBMATCHER_FUSE_H
#include <vector>

namespace ygz {
class KeyFrame;
class MapPoint;
int FuseBatch(const std::vector<KeyFrame *> &targets, const std::vector<MapPoint *> &points, float th = 3.0);
}  // namespace ygz
#endif
