// pose_shell.cc -- GPU test of ygz::PoseOptimizationDevice / PoseOptimizationBatch (csrc/host/OptimizerPose.cc) over stub Frames
// (tests/test_gpu_pose_opt.py): mvbOutlier, the return value and the pose SetPose received must be what ygzf_pose_optimization gave the test for the
// same problem -- one frame at a time and all frames in one batch, twice.
//   pose_shell <dir>: <dir>/meta.txt = n; problem_<k>.bin = n | keys | u_right | mp_valid | world | Tcw[7] | outlier_in | inv_sigma2[8] |
//   fx fy cx cy bf | expected Tcw[7] | expected outlier | expected ret
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ORBextractor.h"
#include "OptimizerPose.h"
#include "ygz_compat.h"
#include "ygzf_pool.h"

using namespace ygz;
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

static int bad = 0;
#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); bad++; } \
    } while (0)

struct Problem {
    int n = 0, ret = 0;
    std::vector<cv::KeyPoint> keys;
    std::vector<float> uRight, world, sigma;
    std::vector<uint8_t> valid, outlierIn, outlier;
    float Tcw[7], cam[5], want[7];
    std::vector<MapPoint> mps;
};

template <typename T> static void rd(FILE *f, T *p, size_t n) {
    if (std::fread(p, sizeof(T), n, f) != n) { std::printf("short read\n"); std::exit(2); }
}

static void load(const std::string &path, Problem &P) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { std::printf("cannot read %s\n", path.c_str()); std::exit(2); }
    rd(f, &P.n, 1);
    const size_t n = (size_t) P.n;
    P.keys.resize(n); P.uRight.resize(n); P.valid.resize(n); P.world.resize(3 * n); P.outlierIn.resize(n); P.outlier.resize(n); P.sigma.resize(8);
    rd(f, P.keys.data(), n); rd(f, P.uRight.data(), n); rd(f, P.valid.data(), n); rd(f, P.world.data(), 3 * n); rd(f, P.Tcw, 7);
    rd(f, P.outlierIn.data(), n); rd(f, P.sigma.data(), 8); rd(f, P.cam, 5); rd(f, P.want, 7); rd(f, P.outlier.data(), n); rd(f, &P.ret, 1);
    std::fclose(f);
    P.mps.resize(n);
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < 3; k++) P.mps[i].mWorldPos[k] = P.world[3 * i + k];
}

static void fill(Frame &F, Problem &P) {
    F.N = P.n;
    F.mvKeys = P.keys;
    F.mvuRight = P.uRight;
    F.mvInvLevelSigma2 = P.sigma;
    F.mbf = P.cam[4];
    F.mvpMapPoints.assign(P.n, nullptr);
    F.mvbOutlier.assign(P.n, false);
    for (int i = 0; i < P.n; i++) {
        if (P.valid[i]) F.mvpMapPoints[i] = &P.mps[i];
        F.mvbOutlier[i] = P.outlierIn[i] != 0;
    }
    F.mTcw = ygz_compat::se3_from7(P.Tcw);
}

static void compare(const Frame &F, const Problem &P, int got, const char *how, int k) {
    CHECK(got == P.ret, "%s, problem %d: returned %d, the ABI %d", how, k, got, P.ret);
    float T[7];
    ygz_compat::se3_to7(F.mTcw, T);
    CHECK(std::memcmp(T, P.want, sizeof T) == 0, "%s, problem %d: the pose differs from the ABI's", how, k);
    int diff = 0;
    for (int i = 0; i < P.n; i++) diff += (F.mvbOutlier[i] ? 1 : 0) != (int) P.outlier[i];
    CHECK(diff == 0, "%s, problem %d: %d outlier flags differ", how, k, diff);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    int n = 0;
    FILE *f = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || std::fscanf(f, "%d", &n) != 1) return 2;
    std::fclose(f);
    std::vector<Problem> P(n);
    for (int k = 0; k < n; k++) load(dir + "/problem_" + std::to_string(k) + ".bin", P[k]);
    Frame::fx = P[0].cam[0]; Frame::fy = P[0].cam[1]; Frame::cx = P[0].cam[2]; Frame::cy = P[0].cam[3];
    Frame::mnMinX = 0; Frame::mnMinY = 0; Frame::mnMaxX = 752; Frame::mnMaxY = 480;
    const unsigned long failuresBefore = ygzf_host::failure_count();
    for (int round = 0; round < 2; round++) {
        for (int k = 0; k < n; k++) {
            Frame F;
            fill(F, P[k]);
            compare(F, P[k], PoseOptimizationDevice(&F), "PoseOptimizationDevice", k);
        }
        std::vector<Frame> frames(n);
        std::vector<Frame *> ptrs;
        for (int k = 0; k < n; k++) { fill(frames[k], P[k]); ptrs.push_back(&frames[k]); }
        std::vector<int> nGood;
        PoseOptimizationBatch(ptrs, nGood);
        CHECK((int) nGood.size() == n, "nGood has %d entries", (int) nGood.size());
        for (int k = 0; k < n && k < (int) nGood.size(); k++) compare(frames[k], P[k], nGood[k], "PoseOptimizationBatch", k);
    }
    std::vector<int> none(3, 7);
    PoseOptimizationBatch(std::vector<Frame *>(), none);
    CHECK(none.empty(), "an empty batch leaves nGood empty");
    CHECK(ygzf_host::failure_count() == failuresBefore, "failures were reported on the way");
    if (bad) return 1;
    std::printf("pose shell ok\n");
    return 0;
}
