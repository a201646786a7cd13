// Converter.h -- Converter::toCvMat of a world position, for tools/make_golden_pnp_ref.py (force-included, under the reference header's include guard)
#ifndef YGZ_CONVERTER_H_
#define YGZ_CONVERTER_H_
#include "MapPoint.h"

namespace ygz {
struct Converter {
    static cv::Mat toCvMat(const WorldPos &p) {
        cv::Mat m(3, 1, CV_32F);
        for (int i = 0; i < 3; i++) m.at<float>(i) = p.v[i];
        return m;
    }
};
}  // namespace ygz
#endif
