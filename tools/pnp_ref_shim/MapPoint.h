// MapPoint.h -- what src/PnPsolver.cc reads of a MapPoint, for tools/make_golden_pnp_ref.py.  Force-included, under the reference header's own
// include guard: include/PnPsolver.h names "MapPoint.h" in quotes, which finds its neighbour before any include path.
#ifndef YGZ_MAPPOINT_H
#define YGZ_MAPPOINT_H
#include <algorithm>
#include <cmath>
#include <iostream>
#include <vector>

#include "cv_slice.h"

using namespace std;   // (the reference's headers name vector, min and max without their namespace)

namespace ygz {
struct WorldPos { float v[3]; };
class MapPoint {
public:
    WorldPos mWorldPos{};
    bool mbBad = false;
    bool isBad() const { return mbBad; }
    WorldPos GetWorldPos() const { return mWorldPos; }
};
}  // namespace ygz
#endif
