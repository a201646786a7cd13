// tri_kernels.hip -- the per-pair body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:1060-1194) for every matched pair of every
// neighbour of a call in one launch.  Pairs are independent of each other: what the reference does with an accepted pair (:1197-1214) and the
// order in which it meets them are replayed on the host from the x3D and status this kernel leaves behind.
//
// One lane per pair, 256 lanes per workgroup; lane g of the launch takes pair g of the call's concatenated list, so the lanes of one wave may
// belong to different problems (ransac::problem_of over the first-pair offsets, per lane here).  KF1's record is a kernel argument, the same
// for every lane; a problem's KF2 record is read through the problem table.  The arithmetic is tri_math.h's, the text the host compiles too.
// Lanes whose pair fails the parallax gate skip the SVD; the sweep loop ends per lane and is bounded by tri::kMaxSweeps.  No LDS, no barrier,
// no atomics; every loop is bounded by an argument (the problem count) or a constant.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "kernels.h"
#include "ransac_device.h"
#include "tri_math.h"

namespace ygzf {

namespace {

constexpr int kTriThreads = 256;

// kernels.h states tri::Kf's layout as TriKfPose
static_assert(sizeof(TriKfPose) == sizeof(tri::Kf) && offsetof(TriKfPose, Rcw) == offsetof(tri::Kf, Rcw) && offsetof(TriKfPose, q) == offsetof(tri::Kf, q) &&
              offsetof(TriKfPose, mbf) == offsetof(tri::Kf, mbf) && offsetof(TriKfPose, t) == offsetof(tri::Kf, t), "TriKfPose is tri::Kf");
__device__ __forceinline__ const tri::Kf &as_kf(const TriKfPose &p) { return reinterpret_cast<const tri::Kf &>(p); }

__device__ __forceinline__ tri::Feat tri_feature(const TriKfDev &K, int idx) {
    const ygzf_kp kp = K.keys[idx];   // octave checked by the host: inside [0, nlevels)
    tri::Feat f;
    f.x = kp.x;
    f.y = kp.y;
    f.uR = K.uRight ? K.uRight[idx] : -1.f;
    const bool stereo = f.uR >= 0.f;   // depth and cosStereo are there where uRight is (checked by the host)
    f.depth = stereo ? K.depth[idx] : -1.f;
    f.cosStereo = stereo ? K.cosStereo[idx] : 0.f;
    f.sigma2 = K.sigma2[kp.octave];
    f.scale = K.scale[kp.octave];
    return f;
}

__global__ __launch_bounds__(kTriThreads) void k_triangulate(TriPairArgs A) {
    const int g = (int) blockIdx.x * kTriThreads + (int) threadIdx.x;
    if (g >= A.totalPairs) return;
    const TriProblemDev &P = ransac::problem_of(A.probs, A.nProblems, g);
    const int i = g - P.firstHyp;
    if (i < 0 || i >= P.nPairs) return;   // (cannot happen with the host's table; a wrong table must not turn into a stray write)
    const tri::Feat f1 = tri_feature(A.kf1, P.idx1[i]), f2 = tri_feature(P.kf2, P.idx2[i]);
    float X[3];
    const uint8_t status = tri::triangulate_pair(as_kf(A.kf1.k), as_kf(P.kf2.k), f1, f2, A.ratioFactor, X, nullptr);
    P.x3d[3 * (size_t) i] = X[0];
    P.x3d[3 * (size_t) i + 1] = X[1];
    P.x3d[3 * (size_t) i + 2] = X[2];
    P.status[i] = status;
}

}  // namespace

void launch_triangulate(hipStream_t st, const TriPairArgs &A) {
    if (A.totalPairs <= 0) return;
    hipLaunchKernelGGL(k_triangulate, dim3((A.totalPairs + kTriThreads - 1) / kTriThreads), dim3(kTriThreads), 0, st, A);
}

}  // namespace ygzf
