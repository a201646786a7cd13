// sim3_host.cc -- a plain host program over host/Sim3Replay.h and csrc/sim3_math.h, nothing of HIP or OpenCV (tests/test_sim3_host_progs.py
// builds it with -fsanitize=address,undefined; tools/sim3_rate.py uses it as the one-thread yardstick).
//   sim3_host case <in> <out>   one solver: evaluates every hypothesis with the kernel's arithmetic on one thread, then replays the calls
//   sim3_host table             stdin: lines "N minInliers probability maxIterations" -> one mRansacMaxIts per line
//   sim3_host draws N count seed   the triples draw_triples gives on the test's scripted RandomInt (an LCG with RAND_MAX = 2^31 - 1)
//   sim3_host time <in> reps    the hypotheses of the case `reps` times: microseconds per evaluation of all of them (median of the reps)
// <in>:  int32 n mN1 H fix minInliers maxIterations nCalls | double probability | float K1[4] K2[4] | int32 calls[nCalls] (-1 = find) |
//        int32 indices1[n] | float X1[3n] X2[3n] maxErr1[n] maxErr2[n] | int32 samples[3H]
// <out>: float hyp[13H] | int32 count[H] | uint64 bits[H words] | per call int32 hyp_index nInliers noMore bestIndex bestInliers iterations, uint8 inliers12[mN1]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "Sim3Replay.h"
#include "sim3_math.h"

struct Case {
    int n = 0, mN1 = 0, H = 0, fix = 0, minInliers = 0, maxIterations = 0, nCalls = 0;
    double probability = 0;
    float K1[4], K2[4];
    std::vector<int> calls, indices1, samples;
    std::vector<float> X1, X2, e1, e2;
};

template <typename T> static void rd(FILE *f, T *p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) { std::printf("short read\n"); std::exit(2); }
}

static Case load(const char *path) {
    Case c;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot read %s\n", path); std::exit(2); }
    int h[7];
    rd(f, h, 7);
    c.n = h[0]; c.mN1 = h[1]; c.H = h[2]; c.fix = h[3]; c.minInliers = h[4]; c.maxIterations = h[5]; c.nCalls = h[6];
    rd(f, &c.probability, 1); rd(f, c.K1, 4); rd(f, c.K2, 4);
    const size_t n = (size_t) c.n;
    c.calls.resize(c.nCalls); c.indices1.resize(n); c.X1.resize(3 * n); c.X2.resize(3 * n); c.e1.resize(n); c.e2.resize(n); c.samples.resize(3 * (size_t) c.H);
    rd(f, c.calls.data(), c.calls.size()); rd(f, c.indices1.data(), n); rd(f, c.X1.data(), 3 * n); rd(f, c.X2.data(), 3 * n);
    rd(f, c.e1.data(), n); rd(f, c.e2.data(), n); rd(f, c.samples.data(), c.samples.size());
    std::fclose(f);
    return c;
}

// what k_sim3_ransac computes, hypothesis after hypothesis on one thread
static void evaluate(const Case &c, std::vector<float> &hyp, std::vector<int> &count, std::vector<uint64_t> &bits) {
    namespace M = ygzf::sim3;
    const int words = (c.n + 63) / 64;
    hyp.assign((size_t) M::kHypFloats * c.H, 0.f);
    count.assign(c.H, 0);
    bits.assign((size_t) words * c.H, 0);
    for (int h = 0; h < c.H; h++) {
        float p1[3][3], p2[3][3];
        for (int k = 0; k < 3; k++)
            for (int a = 0; a < 3; a++) {
                p1[k][a] = c.X1[3 * (size_t) c.samples[3 * h + k] + a];
                p2[k][a] = c.X2[3 * (size_t) c.samples[3 * h + k] + a];
            }
        M::Hyp Hy;
        M::horn(p1, p2, c.fix != 0, Hy);
        for (int i = 0; i < c.n; i++)
            if (M::inlier(Hy, &c.X1[3 * (size_t) i], &c.X2[3 * (size_t) i], c.K1, c.K2, c.e1[i], c.e2[i])) {
                bits[(size_t) h * words + (i >> 6)] |= 1ull << (i & 63);
                count[h]++;
            }
        float *o = &hyp[(size_t) M::kHypFloats * h];
        std::memcpy(o, Hy.R, sizeof Hy.R);
        std::memcpy(o + 9, Hy.t, sizeof Hy.t);
        o[12] = Hy.s;
    }
}

static int run_case(const char *in, const char *out) {
    const Case c = load(in);
    std::vector<float> hyp;
    std::vector<int> count;
    std::vector<uint64_t> bits;
    evaluate(c, hyp, count, bits);
    FILE *f = std::fopen(out, "wb");
    if (!f) return 2;
    std::fwrite(hyp.data(), sizeof(float), hyp.size(), f);
    std::fwrite(count.data(), sizeof(int), count.size(), f);
    std::fwrite(bits.data(), sizeof(uint64_t), bits.size(), f);
    ygz::sim3::Replay R;
    R.N = c.n;
    R.mN1 = c.mN1;
    R.indices1.assign(c.indices1.begin(), c.indices1.end());
    R.set_parameters(c.probability, c.minInliers, c.maxIterations);
    long long need = 0;   // the iterations the calls can reach
    for (int v : c.calls) need += v < 0 ? R.maxIts : v;
    need = std::min<long long>(need, R.maxIts);
    if (R.N >= R.minInliers && need > c.H) { std::printf("the case has %d triples, its calls reach %lld\n", c.H, need); return 2; }
    const int words = (c.n + 63) / 64;
    for (int k = 0; k < c.nCalls; k++) {
        bool noMore = false;
        std::vector<bool> inl;
        int nInliers = 0;
        const int h = R.iterate(c.calls[k] < 0 ? R.maxIts : c.calls[k], count.data(), bits.data(), words, noMore, inl, nInliers);
        const int rec[6] = {h, nInliers, noMore ? 1 : 0, R.bestIndex, R.bestInliers, R.iterations};
        std::fwrite(rec, sizeof(int), 6, f);
        std::vector<uint8_t> bytes(c.mN1);
        for (int i = 0; i < c.mN1; i++) bytes[i] = inl[i] ? 1 : 0;
        std::fwrite(bytes.data(), 1, bytes.size(), f);
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "case")) return run_case(argv[2], argv[3]);
    if (argc >= 2 && !std::strcmp(argv[1], "table")) {
        int N, m, mx;
        double p;
        while (std::scanf("%d %d %lf %d", &N, &m, &p, &mx) == 4) std::printf("%d\n", ygz::sim3::ransac_max_its(N, p, m, mx));
        return 0;
    }
    if (argc >= 5 && !std::strcmp(argv[1], "draws")) {
        unsigned state = (unsigned) std::atol(argv[4]) & 0x7FFFFFFFu;
        auto randomInt = [&state](int lo, int hi) {
            state = (unsigned) (((unsigned long long) state * 1103515245ull + 12345ull) & 0x7FFFFFFFull);
            const int d = hi - lo + 1;
            return int(((double) state / (2147483647.0 + 1.0)) * d) + lo;   // DUtils::Random::RandomInt on this rand()
        };
        std::vector<int> s;
        ygz::sim3::draw_triples(std::atoi(argv[2]), std::atoi(argv[3]), randomInt, s);
        for (size_t i = 0; i + 2 < s.size(); i += 3) std::printf("%d %d %d\n", s[i], s[i + 1], s[i + 2]);
        return 0;
    }
    if (argc >= 4 && !std::strcmp(argv[1], "time")) {
        const Case c = load(argv[2]);
        const int reps = std::max(1, std::atoi(argv[3]));
        std::vector<float> hyp;
        std::vector<int> count;
        std::vector<uint64_t> bits;
        std::vector<double> us;
        long long sink = 0;
        for (int r = 0; r <= reps; r++) {   // the first one untimed
            const auto t0 = std::chrono::steady_clock::now();
            evaluate(c, hyp, count, bits);
            const auto t1 = std::chrono::steady_clock::now();
            for (int v : count) sink += v;
            if (r) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        }
        std::sort(us.begin(), us.end());
        std::printf("%.3f %.3f %.3f %lld\n", us[us.size() / 2], us.front(), us.back(), sink);
        return 0;
    }
    return 2;
}
