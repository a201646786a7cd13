// sim3_opt_host.cc -- Optimizer::OptimizeSim3 as a plain host program over host/Sim3OptHost.h and csrc/sim3_opt_math.h, nothing of HIP, Eigen or
// OpenCV: one thread, the sums in the reference's order (e12 then e21 of a correspondence, correspondences ascending).  tests/test_sim3_opt_host_progs.py builds
// it with -fsanitize=address,undefined and holds it against mode "reference" of tests/sim3_opt_cases.py bit for bit; tools/sim3_opt_rate.py
// uses it (-O2, no sanitizer) as the one-thread yardstick.
//   sim3_opt_host case <in> <out>    one problem
//   sim3_opt_host time <in> reps     the problem `reps` times: microseconds per run (median, min, max)
// <in>:  int32 n fix_scale | float th2 | float K1[4] K2[4] | double S12[8] | float P1c[3n] P2c[3n] obs1[2n] obs2[2n] inv_sigma2_1[n] inv_sigma2_2[n]
// <out>: double S12[8] | int32 ret nBad | per round (2): int32 iterations trials stop, double lambda chi2 | uint8 removed[n]
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Sim3OptHost.h"

namespace M = ygzf::sim3opt;

struct Case {
    int n = 0, fix = 0;
    float th2 = 0, K1[4], K2[4];
    double S12[8];
    std::vector<float> P1c, P2c, obs1, obs2, is1, is2;
};
struct Result {
    double S[8];
    int ret = 0, nBad = 0;
    int iters[2] = {0, 0}, trials[2] = {0, 0}, stop[2] = {M::kStopNotRun, M::kStopNotRun};
    double lambda[2] = {0, 0}, chi2[2] = {0, 0};
    std::vector<uint8_t> removed;
};

template <typename T> static void rd(FILE *f, T *p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) { std::printf("short read\n"); std::exit(2); }
}

static Case load(const char *path) {
    Case c;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot read %s\n", path); std::exit(2); }
    int h[2];
    rd(f, h, 2);
    c.n = h[0]; c.fix = h[1];
    rd(f, &c.th2, 1); rd(f, c.K1, 4); rd(f, c.K2, 4); rd(f, c.S12, 8);
    const size_t n = (size_t) c.n;
    c.P1c.resize(3 * n); c.P2c.resize(3 * n); c.obs1.resize(2 * n); c.obs2.resize(2 * n); c.is1.resize(n); c.is2.resize(n);
    rd(f, c.P1c.data(), 3 * n); rd(f, c.P2c.data(), 3 * n); rd(f, c.obs1.data(), 2 * n); rd(f, c.obs2.data(), 2 * n); rd(f, c.is1.data(), n); rd(f, c.is2.data(), n);
    std::fclose(f);
    return c;
}

static void optimize(const Case &c, Result &r) {
    r = Result();
    r.removed.assign((size_t) c.n + 1, 0);
    ygzf_sim3_opt_problem p;
    std::memset(&p, 0, sizeof p);
    p.n = c.n;
    p.P1c = c.P1c.data(); p.P2c = c.P2c.data(); p.obs1 = c.obs1.data(); p.obs2 = c.obs2.data();
    p.inv_sigma2_1 = c.is1.data(); p.inv_sigma2_2 = c.is2.data();
    std::memcpy(p.K1, c.K1, sizeof p.K1); std::memcpy(p.K2, c.K2, sizeof p.K2); std::memcpy(p.S12, c.S12, sizeof p.S12);
    p.th2 = c.th2;
    p.fix_scale = c.fix;
    ygzf_sim3_opt_info info;
    ygz::sim3opt::optimize_host(p, r.S, r.removed.data(), &r.ret, &info);
    r.removed.resize((size_t) c.n);
    r.nBad = info.n_bad;
    for (int k = 0; k < 2; k++) {
        r.iters[k] = info.iterations[k]; r.trials[k] = info.trials[k]; r.stop[k] = info.stop[k];
        r.lambda[k] = info.lambda[k]; r.chi2[k] = info.chi2[k];
    }
}

int main(int argc, char **argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "case")) {
        const Case c = load(argv[2]);
        Result r;
        optimize(c, r);
        FILE *f = std::fopen(argv[3], "wb");
        if (!f) return 2;
        std::fwrite(r.S, sizeof(double), 8, f);
        const int h[2] = {r.ret, r.nBad};
        std::fwrite(h, sizeof(int), 2, f);
        for (int k = 0; k < 2; k++) {
            const int g[3] = {r.iters[k], r.trials[k], r.stop[k]};
            const double d[2] = {r.lambda[k], r.chi2[k]};
            std::fwrite(g, sizeof(int), 3, f);
            std::fwrite(d, sizeof(double), 2, f);
        }
        if (!r.removed.empty()) std::fwrite(r.removed.data(), 1, r.removed.size(), f);
        std::fclose(f);
        return 0;
    }
    if (argc >= 4 && !std::strcmp(argv[1], "time")) {
        const Case c = load(argv[2]);
        const int reps = std::max(1, std::atoi(argv[3]));
        std::vector<double> us;
        Result r;
        long long sink = 0;
        for (int k = 0; k <= reps; k++) {   // the first one untimed
            const auto t0 = std::chrono::steady_clock::now();
            optimize(c, r);
            const auto t1 = std::chrono::steady_clock::now();
            sink += r.ret;
            if (k) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        }
        std::sort(us.begin(), us.end());
        std::printf("%.3f %.3f %.3f %lld\n", us[us.size() / 2], us.front(), us.back(), sink);
        return 0;
    }
    return 2;
}
