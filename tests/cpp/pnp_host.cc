// pnp_host.cc -- a plain host program over host/PnPReplay.h, host/PnPHost.h and csrc/pnp_math.h, nothing of HIP or OpenCV
// (tests/test_pnp_host_progs.py builds it with -fsanitize=address,undefined; tools/pnp_rate.py uses it as the one-thread yardstick).
//   pnp_host case <in> <out>    one solver: evaluates its budget of hypotheses and the Refine of the records with the kernel's arithmetic
//                               on one thread, then replays the calls; iterations beyond the budget are evaluated when reached
//   pnp_host table              stdin: lines "N probability minInliers maxIterations minSet epsilon" -> "minInliers maxIts" per line
//   pnp_host draws N minSet count seed   the sets draw_quads gives on the test's scripted RandomInt (an LCG with RAND_MAX = 2^31 - 1)
//   pnp_host time <in> reps [incremental]   the budget of the case `reps` times: microseconds per evaluation (median, fastest, slowest);
//                               incremental: the reference's schedule instead, iterate(5) until success or bNoMore, evaluating as it goes
// <in>:  int32 n nMatches H minSet minInliers maxIts nCalls | double K[4] | int32 calls[nCalls] (-1 = find) | int32 keyIndices[n] |
//        float P3D[3n] P2D[2n] maxErr[n] | int32 samples[H minSet]
// <out>: int32 Hout | double hyp[12 Hout] | int32 count[Hout] | uint64 bits[Hout words] | int32 refinedN[Hout] | double refinedHyp[12 Hout] |
//        uint64 refinedBits[Hout words] | per call int32 kind index nInliers noMore bestIndex bestInliers iterations size, float T[16], uint8 inliers[size]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "PnPHost.h"

namespace R = ygz::pnp;

struct Case {
    int n = 0, nMatches = 0, H = 0, minSet = 0, minInliers = 0, maxIts = 0, nCalls = 0;
    double K[4];
    std::vector<int> calls, keyIndices, samples;
    std::vector<float> P3D, P2D, maxErr;
    R::HostProblem problem() const {
        R::HostProblem P;
        P.n = n; P.P3D = P3D.data(); P.P2D = P2D.data(); P.maxErr = maxErr.data();
        std::memcpy(P.K, K, sizeof K);
        P.minSet = minSet; P.minInliers = minInliers;
        return P;
    }
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
    c.n = h[0]; c.nMatches = h[1]; c.H = h[2]; c.minSet = h[3]; c.minInliers = h[4]; c.maxIts = h[5]; c.nCalls = h[6];
    rd(f, c.K, 4);
    const size_t n = (size_t) c.n;
    c.calls.resize(c.nCalls); c.keyIndices.resize(n); c.P3D.resize(3 * n); c.P2D.resize(2 * n); c.maxErr.resize(n); c.samples.resize((size_t) c.H * c.minSet);
    rd(f, c.calls.data(), c.calls.size()); rd(f, c.keyIndices.data(), n); rd(f, c.P3D.data(), 3 * n); rd(f, c.P2D.data(), 2 * n);
    rd(f, c.maxErr.data(), n); rd(f, c.samples.data(), c.samples.size());
    std::fclose(f);
    return c;
}

static R::Replay replay_of(const Case &c) {
    R::Replay S;
    S.N = c.n;
    S.nMatches = (size_t) c.nMatches;
    S.keyIndices.assign(c.keyIndices.begin(), c.keyIndices.end());
    S.minInliers = c.minInliers;
    S.maxIts = c.maxIts;
    return S;
}

static int run_case(const char *in, const char *out) {
    const Case c = load(in);
    const R::HostProblem P = c.problem();
    R::Results res;
    const int budget = c.n >= c.minSet ? std::min(c.H, c.maxIts) : 0;
    R::evaluate_all(P, c.samples.data(), budget, res);
    R::Replay S = replay_of(c);
    struct Rec { int v[8]; float T[16]; std::vector<uint8_t> inl; };
    std::vector<Rec> recs;
    for (int k = 0; k < c.nCalls; k++) {
        bool noMore = false;
        std::vector<bool> inl;
        int nInliers = 0, index = -1;
        bool shortOfSets = false;
        const R::Returned kind = S.iterate(c.calls[k] < 0 ? S.maxIts : c.calls[k], res,
            [&](int h) {
                if (h >= c.H) { shortOfSets = true; res.append(); return; }
                R::append_hypothesis(P, &c.samples[(size_t) c.minSet * h], res);
            },
            [&](int h) { R::refine_record(P, res, h); }, noMore, inl, nInliers, index);
        if (shortOfSets) { std::printf("the case has %d sample sets, its calls reach beyond them\n", c.H); return 2; }
        Rec r;
        const int v[8] = {(int) kind, index, nInliers, noMore ? 1 : 0, S.bestIndex, S.bestInliers, S.iterations, (int) inl.size()};
        std::memcpy(r.v, v, sizeof v);
        std::memset(r.T, 0, sizeof r.T);
        if (kind == R::REFINED) ygzf::pnp::pose_to_float(&res.refinedHyp[(size_t) 12 * index], r.T);
        if (kind == R::BEST) ygzf::pnp::pose_to_float(&res.hyp[(size_t) 12 * index], r.T);
        r.inl.resize(inl.size());
        for (size_t i = 0; i < inl.size(); i++) r.inl[i] = inl[i] ? 1 : 0;
        recs.push_back(r);
    }
    FILE *f = std::fopen(out, "wb");
    if (!f) return 2;
    const int Hout = res.size();
    std::fwrite(&Hout, sizeof(int), 1, f);
    std::fwrite(res.hyp.data(), sizeof(double), res.hyp.size(), f);
    std::fwrite(res.count.data(), sizeof(int), res.count.size(), f);
    std::fwrite(res.bits.data(), sizeof(uint64_t), res.bits.size(), f);
    std::fwrite(res.refinedN.data(), sizeof(int), res.refinedN.size(), f);
    std::fwrite(res.refinedHyp.data(), sizeof(double), res.refinedHyp.size(), f);
    std::fwrite(res.refinedBits.data(), sizeof(uint64_t), res.refinedBits.size(), f);
    for (const Rec &r : recs) {
        std::fwrite(r.v, sizeof(int), 8, f);
        std::fwrite(r.T, sizeof(float), 16, f);
        if (!r.inl.empty()) std::fwrite(r.inl.data(), 1, r.inl.size(), f);
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "case")) return run_case(argv[2], argv[3]);
    if (argc >= 2 && !std::strcmp(argv[1], "table")) {
        int N, mi, mx, ms;
        double p, e;
        while (std::scanf("%d %lf %d %d %d %lf", &N, &p, &mi, &mx, &ms, &e) == 6) {
            int a = 0, b = 0;
            R::ransac_parameters(N, p, mi, mx, ms, (float) e, a, b);
            std::printf("%d %d\n", a, b);
        }
        return 0;
    }
    if (argc >= 6 && !std::strcmp(argv[1], "draws")) {
        unsigned state = (unsigned) std::atol(argv[5]) & 0x7FFFFFFFu;
        auto randomInt = [&state](int lo, int hi) {
            state = (unsigned) (((unsigned long long) state * 1103515245ull + 12345ull) & 0x7FFFFFFFull);
            const int d = hi - lo + 1;
            return int(((double) state / (2147483647.0 + 1.0)) * d) + lo;   // DUtils::Random::RandomInt on this rand()
        };
        const int ms = std::atoi(argv[3]);
        std::vector<int> s;
        R::draw_quads(std::atoi(argv[2]), ms, std::atoi(argv[4]), randomInt, s);
        for (size_t i = 0; i < s.size(); i++) std::printf("%d%c", s[i], (i + 1) % ms ? ' ' : '\n');
        return 0;
    }
    if (argc >= 4 && !std::strcmp(argv[1], "time")) {
        const Case c = load(argv[2]);
        const R::HostProblem P = c.problem();
        const int reps = std::max(1, std::atoi(argv[3]));
        const bool incremental = argc >= 5 && !std::strcmp(argv[4], "incremental");
        std::vector<double> us;
        long long sink = 0;
        for (int r = 0; r <= reps; r++) {   // the first one untimed
            R::Results res;
            const auto t0 = std::chrono::steady_clock::now();
            if (!incremental)
                R::evaluate_all(P, c.samples.data(), std::min(c.H, c.maxIts), res);
            else {
                res.resize(c.n, 0);
                R::Replay S = replay_of(c);
                bool noMore = false;
                for (int guard = 0; guard < c.H && !noMore; guard++) {
                    std::vector<bool> inl;
                    int nInliers = 0, index = -1;
                    const R::Returned kind = S.iterate(5, res,
                        [&](int h) { if (h < c.H) R::append_hypothesis(P, &c.samples[(size_t) c.minSet * h], res); else res.append(); },
                        [&](int h) { R::refine_record(P, res, h); }, noMore, inl, nInliers, index);
                    if (kind != R::EMPTY) break;
                }
            }
            const auto t1 = std::chrono::steady_clock::now();
            for (int v : res.count) sink += v;
            if (r) us.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        }
        std::sort(us.begin(), us.end());
        std::printf("%.3f %.3f %.3f %lld\n", us[us.size() / 2], us.front(), us.back(), sink);
        return 0;
    }
    return 2;
}
