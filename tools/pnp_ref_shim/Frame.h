// Frame.h -- what src/PnPsolver.cc reads of a Frame, for tools/make_golden_pnp_ref.py (force-included, under the reference header's include guard)
#ifndef YGZ_FRAME_H_
#define YGZ_FRAME_H_
#include "MapPoint.h"

namespace ygz {
class Frame {
public:
    float fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<cv::KeyPoint> mvKeys;
    std::vector<float> mvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
};
}  // namespace ygz
#endif
