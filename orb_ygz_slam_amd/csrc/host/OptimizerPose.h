// OptimizerPose.h -- Optimizer::PoseOptimization(Frame *) (src/Optimizer.cc:1656-1842) on the device, for one frame or a batch of independent
// frames (product code, host side).  Optimizer.cc itself stays the reference's -- bundle adjustment and the IMU overloads live there --; a user
// forwards the one function:  int Optimizer::PoseOptimization(Frame *pFrame) { return PoseOptimizationDevice(pFrame); }
#ifndef YGZF_OPTIMIZER_POSE_H
#define YGZF_OPTIMIZER_POSE_H

#include <vector>

namespace ygz {
class Frame;

// What the reference's function does to the frame: mvbOutlier of every correspondence, SetPose(the optimised pose), the return value
// nInitialCorrespondences - nBad (0, and the pose untouched, with fewer than 3 correspondences).  A device failure is reported through
// ygzf_host::report_failure and returns 0 with the frame as it was.
int PoseOptimizationDevice(Frame *pFrame);

// The same for every frame of the vector in one device call (the first pass over Relocalization's candidates, the frames of a clip): the frames
// are independent problems.  nGood[i] = what PoseOptimizationDevice(vpFrames[i]) returns.
void PoseOptimizationBatch(const std::vector<Frame *> &vpFrames, std::vector<int> &nGood);
}  // namespace ygz
#endif
