// sim3_opt_shell.cc -- GPU test of ygz::OptimizeSim3Device / OptimizeSim3Batch (csrc/host/OptimizerSim3.{h,cc}) over stub KeyFrames and a
// stand-in Sim3 type (tests/test_gpu_sim3_opt.py): vpMatches1, g2oS12 and the return value must be what ygzf_optimize_sim3 gave the test for
// the same problem -- one candidate at a time and all candidates of the current keyframe in one batch, with the device forced
// (ygzf_host_sim3_opt_device_min = 0); with the host forced they must be mode "reference" of tests/sim3_opt_cases.py, bit for bit as well; and
// the default threshold must send the single calls below it to the host and the batch above it to the device.
//   sim3_opt_shell <dir>: <dir>/meta.txt = count; problem_<k>.bin = n fix | th2 | K1[4] K2[4] | S12[8] | P1c P2c obs1 obs2 | oct1[n] oct2[n] |
//   inv_sigma2[8] | the ABI's S12[8] removed[n] ret | mode reference's S12[8] removed[n] ret
// KF1 holds every candidate's points one slice after the other; a slice ends with four pairs the filter must drop (no match, no point in
// KF1, a bad point, a point KF2 does not observe), and KF2 observes its points in reverse order, so the index map back is no identity.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ORBextractor.h"
#include "OptimizerSim3.h"
#include "ygz_compat.h"
#include "ygzf_pool.h"

using namespace ygz;
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

static int bad = 0;
#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); bad++; } \
    } while (0)

struct Quat {   // the slice of Eigen::Quaterniond the shell touches
    double c[4];
    double *coeffs() { return c; }
    const double *coeffs() const { return c; }
};
struct Sim3Stub {   // the slice of g2o::Sim3 the shell touches
    Quat r;
    double t[3], s;
    Quat &rotation() { return r; }
    const Quat &rotation() const { return r; }
    double *translation() { return t; }
    const double *translation() const { return t; }
    double &scale() { return s; }
    const double &scale() const { return s; }
};

constexpr int kExtra = 4;

struct Problem {
    int n = 0, fix = 0, ret = 0;
    float th2 = 0, K1[4], K2[4], sigma[8];
    double S12[8], want[8], wantDev[8], wantHost[8];
    std::vector<float> P1c, P2c, obs1, obs2;
    std::vector<int> oct1, oct2;
    std::vector<uint8_t> removed, removedDev, removedHost;
    int retDev = 0, retHost = 0;
    std::vector<MapPoint> mp1, mp2;   // n + kExtra each
    KeyFrame kf2;
    size_t offset = 0;                // the slice's first slot in KF1
};

template <typename T> static void rd(FILE *f, T *p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) { std::printf("short read\n"); std::exit(2); }
}

static void load(const std::string &path, Problem &P) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { std::printf("cannot read %s\n", path.c_str()); std::exit(2); }
    rd(f, &P.n, 1); rd(f, &P.fix, 1); rd(f, &P.th2, 1); rd(f, P.K1, 4); rd(f, P.K2, 4); rd(f, P.S12, 8);
    const size_t n = (size_t) P.n;
    P.P1c.resize(3 * n); P.P2c.resize(3 * n); P.obs1.resize(2 * n); P.obs2.resize(2 * n); P.oct1.resize(n); P.oct2.resize(n); P.removed.resize(n);
    rd(f, P.P1c.data(), 3 * n); rd(f, P.P2c.data(), 3 * n); rd(f, P.obs1.data(), 2 * n); rd(f, P.obs2.data(), 2 * n);
    rd(f, P.oct1.data(), n); rd(f, P.oct2.data(), n); rd(f, P.sigma, 8);
    P.removedDev.resize(n); P.removedHost.resize(n);
    rd(f, P.wantDev, 8); rd(f, P.removedDev.data(), n); rd(f, &P.retDev, 1);
    rd(f, P.wantHost, 8); rd(f, P.removedHost.data(), n); rd(f, &P.retHost, 1);
    std::fclose(f);
}

static void identity(KeyFrame &K, const float cam[4], const float sigma[8]) {
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) K.mRcw(r, c) = r == c ? 1.f : 0.f;
        K.mtcw[r] = 0.f;
    }
    K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3];
    K.mvInvLevelSigma2.assign(sigma, sigma + 8);
}

// the candidate's slice of KF1 and its own KF2; -> vpMatches1 over all of KF1's slots
static std::vector<MapPoint *> fill(KeyFrame &kf1, Problem &P) {
    const int n = P.n, m = n + kExtra;
    P.mp1.assign(m, MapPoint());
    P.mp2.assign(m, MapPoint());
    P.kf2 = KeyFrame();
    identity(P.kf2, P.K2, P.sigma);
    P.kf2.mvKeys.assign(m, cv::KeyPoint());
    std::vector<MapPoint *> matches(kf1.mvKeys.size(), nullptr);
    for (int j = 0; j < m; j++) {
        const size_t slot = P.offset + j;
        const int i2 = m - 1 - j;
        cv::KeyPoint k1 = cv::KeyPoint(), k2 = cv::KeyPoint();
        if (j < n) {
            for (int a = 0; a < 3; a++) { P.mp1[j].mWorldPos[a] = P.P1c[3 * j + a]; P.mp2[j].mWorldPos[a] = P.P2c[3 * j + a]; }
            k1.pt.x = P.obs1[2 * j]; k1.pt.y = P.obs1[2 * j + 1]; k1.octave = P.oct1[j];
            k2.pt.x = P.obs2[2 * j]; k2.pt.y = P.obs2[2 * j + 1]; k2.octave = P.oct2[j];
        } else {
            P.mp1[j].mWorldPos[2] = 5.f; P.mp2[j].mWorldPos[2] = 5.f;
        }
        kf1.mvKeys[slot] = k1;
        P.kf2.mvKeys[i2] = k2;
        kf1.mvpMapPoints[slot] = &P.mp1[j];
        matches[slot] = &P.mp2[j];
        P.mp2[j].mObservations[&P.kf2] = (size_t) i2;
        const int extra = j - n;
        if (extra == 0) matches[slot] = nullptr;                  // no match
        if (extra == 1) kf1.mvpMapPoints[slot] = nullptr;         // no point in KF1
        if (extra == 2) P.mp2[j].mbBad = true;                    // a bad point
        if (extra == 3) P.mp2[j].mObservations.clear();           // KF2 does not observe it
    }
    return matches;
}

static Sim3Stub sim3_of(const double S[8]) {
    Sim3Stub s;
    std::memcpy(s.r.c, S, 4 * sizeof(double));
    std::memcpy(s.t, S + 4, 3 * sizeof(double));
    s.s = S[7];
    return s;
}

static void compare(const Problem &P, const std::vector<MapPoint *> &before, const std::vector<MapPoint *> &after, const Sim3Stub &S, int got, const char *how, int k) {
    CHECK(got == P.ret, "%s, candidate %d: returned %d, the ABI %d", how, k, got, P.ret);
    double o[8];
    OptimizeSim3Read(S, o);
    CHECK(std::memcmp(o, P.want, sizeof o) == 0, "%s, candidate %d: g2oS12 differs from the ABI's", how, k);
    int diff = 0;
    for (size_t slot = 0; slot < before.size(); slot++) {
        const bool inSlice = slot >= P.offset && slot < P.offset + (size_t) P.n;
        MapPoint *want = inSlice && P.removed[slot - P.offset] ? nullptr : before[slot];
        diff += after[slot] != want;
    }
    CHECK(diff == 0, "%s, candidate %d: %d entries of vpMatches1 differ", how, k, diff);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    int n = 0;
    FILE *f = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || std::fscanf(f, "%d", &n) != 1) return 2;
    std::fclose(f);
    std::vector<Problem> P(n);
    size_t slots = 0;
    for (int k = 0; k < n; k++) {
        load(dir + "/problem_" + std::to_string(k) + ".bin", P[k]);
        P[k].offset = slots;
        slots += (size_t) P[k].n + kExtra;
    }
    KeyFrame kf1;
    identity(kf1, P[0].K1, P[0].sigma);
    kf1.mvKeys.assign(slots, cv::KeyPoint());
    kf1.mvpMapPoints.assign(slots, nullptr);
    const unsigned long failuresBefore = ygzf_host::failure_count();
    const int dflt = ygzf_host_sim3_opt_device_min;
    CHECK(dflt == 400, "the default threshold is %d", dflt);
    for (int round = 0; round < 3; round++) {   // the device forced, the host forced, the default threshold
        const bool host = round == 1;
        ygzf_host_sim3_opt_device_min = round == 0 ? 0 : round == 1 ? 1 << 30 : dflt;
        size_t total = 0;
        for (int k = 0; k < n; k++) {
            total += (size_t) P[k].n;
            const bool single = host || (round == 2 && P[k].n < dflt);   // (which form the single call takes)
            std::memcpy(P[k].want, single ? P[k].wantHost : P[k].wantDev, sizeof P[k].want);
            P[k].removed = single ? P[k].removedHost : P[k].removedDev;
            P[k].ret = single ? P[k].retHost : P[k].retDev;
        }
        if (round == 2) CHECK(total >= (size_t) dflt && P[0].n < dflt, "the problems do not straddle the default threshold");
        std::vector<std::vector<MapPoint *>> before(n), matches(n);
        for (int k = 0; k < n; k++) before[k] = fill(kf1, P[k]);
        for (int k = 0; k < n; k++) {
            matches[k] = before[k];
            Sim3Stub S = sim3_of(P[k].S12);
            const int got = OptimizeSim3Device(&kf1, &P[k].kf2, matches[k], S, P[k].th2, P[k].fix != 0);
            compare(P[k], before[k], matches[k], S, got, "OptimizeSim3Device", k);
        }
        for (int k = 0; k < n; k++) {                 // the batch as a whole is above the default threshold
            std::memcpy(P[k].want, host ? P[k].wantHost : P[k].wantDev, sizeof P[k].want);
            P[k].removed = host ? P[k].removedHost : P[k].removedDev;
            P[k].ret = host ? P[k].retHost : P[k].retDev;
        }
        std::vector<KeyFrame *> kf2s;
        std::vector<Sim3Stub> vS;
        for (int k = 0; k < n; k++) { matches[k] = before[k]; kf2s.push_back(&P[k].kf2); vS.push_back(sim3_of(P[k].S12)); }
        std::vector<int> nIn;
        OptimizeSim3Batch(&kf1, kf2s, matches, vS, P[0].th2, P[0].fix != 0, nIn);
        CHECK((int) nIn.size() == n, "nIn has %d entries", (int) nIn.size());
        for (int k = 0; k < n && k < (int) nIn.size(); k++) compare(P[k], before[k], matches[k], vS[k], nIn[k], "OptimizeSim3Batch", k);
    }
    ygzf_host_sim3_opt_device_min = dflt;
    std::vector<int> none(3, 7);
    std::vector<std::vector<MapPoint *>> noMatches;
    std::vector<Sim3Stub> noS;
    OptimizeSim3Batch(&kf1, std::vector<KeyFrame *>(), noMatches, noS, 10.f, true, none);
    CHECK(none.empty(), "an empty batch leaves nIn empty");
    CHECK(ygzf_host::failure_count() == failuresBefore, "failures were reported on the way");
    if (bad) return 1;
    std::printf("sim3 opt shell ok\n");
    return 0;
}
