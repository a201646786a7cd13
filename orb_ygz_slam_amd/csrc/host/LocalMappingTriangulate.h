// LocalMappingTriangulate.h -- what a user forwards the neighbour loop of LocalMapping::CreateNewMapPoints to (src/LocalMapping.cc:1009-1216;
// host/LocalMappingTriangulate.cc).
//
//   ygz::TriangulatePairsDevice   the per-pair body of :1060-1194 for the pairs of ONE neighbour: x3D (3 floats per pair) and the status byte of
//                                 include/ygzf.h (low four bits 0: accepted).  false: a device failure (ygzf_host::report_failure has it).
//   ygz::CreateNewMapPointsBatch  the whole loop: the per-neighbour searches through ORBmatcher::SearchForTriangulation, every pair of every
//                                 neighbour in ONE ygzf_triangulate_pairs call, then host/TriangulateApply.h, which applies :1197-1214 in the
//                                 reference's order and says why the result is the sequential loop's.  Returns the reference's nnew; after a
//                                 device failure nothing is created and 0 is returned.  computeF12 is LocalMapping::ComputeF12 (a private
//                                 member that inverts K with Eigen: it stays the reference's), checkNewKeyFrames is CheckNewKeyFrames().
//
// Both compute cos(2 * atan2(mb / 2, mvDepth[i])) once per keyframe -- the reference's own expression at the widths LocalMapping.cc gives it,
// float throughout -- and keep it (mb and mvDepth are const members of a KeyFrame); ygz::TriangulateForget drops a keyframe's entry when the
// keyframe is deleted.
//
// Host threshold.  A device call costs about 36 us whatever it holds up to a few hundred pairs; the same text (csrc/tri_math.h) on the calling
// thread costs 0.6 - 0.75 us per pair, and the two meet near 50 pairs (profiles/triangulate_rate.txt).  Calls with fewer than ygzf_host_tri_device_min pairs (default 64,
// environment YGZF_TRI_DEVICE_MIN; 0 = always the device) therefore run that text on the calling thread: the same bits either way.
#ifndef YGZF_LOCAL_MAPPING_TRIANGULATE_H
#define YGZF_LOCAL_MAPPING_TRIANGULATE_H
#include <cstddef>
#include <cstdint>
#include <functional>
#include <list>
#include <utility>
#include <vector>

extern int ygzf_host_tri_device_min;   // read from YGZF_TRI_DEVICE_MIN on first use unless set before; tests set it directly

// Include after the header that declares Matrix3f: the reference's Common.h (inside the reference tree) or ygz_compat.h (stand-alone).
namespace ygz {
class KeyFrame;
class MapPoint;
class Map;
bool TriangulatePairsDevice(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<std::pair<size_t, size_t>> &vMatchedIndices, float ratioFactor,
                            std::vector<float> &x3D, std::vector<uint8_t> &status);
int CreateNewMapPointsBatch(KeyFrame *pCurrentKeyFrame, const std::vector<KeyFrame *> &vpNeighKFs, Map *pMap, std::list<MapPoint *> &lpRecentAddedMapPoints,
                            bool bMonocular, const std::function<Matrix3f(KeyFrame *&, KeyFrame *&)> &computeF12,
                            const std::function<bool()> &checkNewKeyFrames);
void TriangulateForget(KeyFrame *pKF);
}  // namespace ygz
#endif
