// FrameUndistort.cc -- ygz::Frame::ComputeImagePyramid (src/Frame.cc:773-814) with its undistortion on the device (product code, host side;
// optional).  Compiled inside the reference tree against the reference's own, unchanged include/Frame.h, it is the strong definition of that one
// member: the link drops the reference's body (objcopy --weaken-symbol on Frame.o, the recipe INTEGRATION.md gives) and every other member of
// Frame stays the reference's.  The structure is the reference's: the maps are built once, by the user's own cv::initUndistortRectifyMap on the
// host; the left image goes up raw and is undistorted where the pyramid is built (ORBextractor::ComputePyramidUndistorted: one upload, and
// mImGray is the undistorted level 0 that comes back with the levels); the right eye goes through ygzf_remap_host with the same maps.  The
// 32-bit depth image of RGB-D stays on cv::remap: its float summation order is another primitive.
#include "ORBextractor.h"   // first: inside the reference tree this is the replacement header (same include guard)
#include "ygz_compat.h"

#include "Converter.h"
#include "ygzf_pool.h"

namespace ygz {
void Frame::ComputeImagePyramid() {
    const bool undistort = mbNeedUndistort && (mSensor == Monocular || mSensor == Stereo || mSensor == RGBD);
    if (mbNeedUndistort) {
        if (map1.empty()) {
            // init the undistortion map (:778-783)
            cv::initUndistortRectifyMap(Converter::toCvMat(mK), mDistCoef, Mat(), Converter::toCvMat(mK), cv::Size(mImGray.cols, mImGray.rows), CV_16SC2,
                                        map1, map2);
        }
        // (there is no CPU fallback: maps the extractor refuses are reported there and the frame gets no pyramid)
        if (undistort && !mpORBextractorLeft->SetUndistortMaps(map1, map2)) return;
        if (mSensor == Stereo) {
            cv::Mat img_undistorted;
            if (!mpORBextractorLeft->Undistort(mImRight, img_undistorted)) return;
            mImRight = img_undistorted;
        }
        if (mSensor == RGBD) {
            cv::Mat img_undistorted;
            cv::remap(mImDepth, img_undistorted, map1, map2, cv::INTER_LINEAR);
            mImDepth = img_undistorted;
        }
    }
    if (undistort) mpORBextractorLeft->ComputePyramidUndistorted(mImGray);
    else mpORBextractorLeft->ComputePyramid(mImGray);

    mvImagePyramid.resize(mpORBextractorLeft->GetLevels());
    for (int l = 0; l < mpORBextractorLeft->GetLevels(); l++) {
        mvImagePyramid[l] = mpORBextractorLeft->mvImagePyramid[l].clone();
    }
    // the reference's mImGray = img_undistorted (:789): the undistorted image is level 0 of the pyramid (a header on the frame's own clone)
    if (undistort && !mvImagePyramid.empty() && !mvImagePyramid[0].empty()) mImGray = mvImagePyramid[0];
}
}  // namespace ygz
