// pnp_shell.cc -- GPU test of ygz::PnPsolver / ygz::PnPsolverBatch (csrc/host/PnPsolver.cc) over a stub Frame (tests/test_gpu_pnp.py): the
// solvers of argv[2..] are constructed from stub Frames and MapPoints that hold the case's correspondences, given the case's sample sets
// (SetSamples), evaluated in ONE PnPsolverBatch call -- except the last, which is left to evaluate itself -- and then driven round-robin, call j
// of every solver before call j + 1 of any, as Tracking::Relocalization drives its candidates.  Every call's outcome is written out for the
// test to hold against tests/pnp_cases.py: pnp_iterate.
//   pnp_shell [--min=K] <out> <case>...   <case>: the file of pnp_cases.write_case; --min=K sets ygzf_host_pnp_device_min (0: always the
//                                          device), without it the default stands and a batch this small evaluates on the calling thread
//   <out>: per solver, per call: int32 returned nInliers noMore size | float Tcw[16] (zeros when empty) | uint8 inliers[size]
// The gate of correspondence i travels as mvLevelSigma2[i] with octave i and th2 = 1, so that the solver's float product is the case's gate.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "ORBextractor.h"
#include "PnPsolver.h"
#include "ygz_compat.h"
#include "ygzf_pool.h"

using namespace ygz;
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

template <typename T> static void rd(FILE *f, T *p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) { std::printf("short read\n"); std::exit(2); }
}

struct Scene {
    int n = 0, nMatches = 0, H = 0, minSet = 0, minInliers = 0, maxIts = 0, nCalls = 0;
    double K[4];
    std::vector<int> calls, samples;
    Frame frame;
    std::vector<std::unique_ptr<MapPoint>> mps;
    std::vector<MapPoint *> matches;
    std::unique_ptr<PnPsolver> solver;
};

static void load(const char *path, Scene &S) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot read %s\n", path); std::exit(2); }
    int h[7];
    rd(f, h, 7);
    S.n = h[0]; S.nMatches = h[1]; S.H = h[2]; S.minSet = h[3]; S.minInliers = h[4]; S.maxIts = h[5]; S.nCalls = h[6];
    rd(f, S.K, 4);
    const size_t n = (size_t) S.n;
    std::vector<int> key(n);
    std::vector<float> P3D(3 * n), P2D(2 * n), maxErr(n);
    S.calls.resize(S.nCalls); S.samples.resize((size_t) S.H * S.minSet);
    rd(f, S.calls.data(), S.calls.size()); rd(f, key.data(), n); rd(f, P3D.data(), 3 * n); rd(f, P2D.data(), 2 * n); rd(f, maxErr.data(), n);
    rd(f, S.samples.data(), S.samples.size());
    std::fclose(f);
    S.frame.mvKeys.resize(S.nMatches);
    S.frame.mvLevelSigma2 = maxErr;
    S.frame.mvLevelSigma2.push_back(1.f);   // the octave of the entries the constructor drops
    S.matches.assign(S.nMatches, nullptr);
    for (cv::KeyPoint &kp : S.frame.mvKeys) { kp.pt.x = kp.pt.y = 0.f; kp.octave = (int) n; }
    std::vector<char> used(S.nMatches, 0);
    for (size_t i = 0; i < n; i++) {
        used[key[i]] = 1;
        S.frame.mvKeys[key[i]].pt.x = P2D[2 * i];
        S.frame.mvKeys[key[i]].pt.y = P2D[2 * i + 1];
        S.frame.mvKeys[key[i]].octave = (int) i;
        S.mps.emplace_back(new MapPoint());
        for (int a = 0; a < 3; a++) S.mps.back()->mWorldPos[a] = P3D[3 * i + a];
        S.matches[key[i]] = S.mps.back().get();
    }
    // the entries between them are what the constructor's filter drops (:76-77), one kind after the other: no match, a bad point
    int kind = 0;
    for (int i = 0; i < S.nMatches; i++) {
        if (used[i] || kind++ % 2 == 0) continue;
        S.mps.emplace_back(new MapPoint());
        S.mps.back()->mbBad = true;
        S.matches[i] = S.mps.back().get();
    }
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strncmp(argv[1], "--min=", 6)) {
        ygzf_host_pnp_device_min = std::atoi(argv[1] + 6);
        argv++;
        argc--;
    }
    if (argc < 3) return 2;
    const int B = argc - 2;
    std::vector<std::unique_ptr<Scene>> S;
    const unsigned long failuresBefore = ygzf_host::failure_count();
    std::vector<PnPsolver *> batch;
    for (int k = 0; k < B; k++) {
        S.emplace_back(new Scene());
        load(argv[2 + k], *S[k]);
        Scene &s = *S[k];
        Frame::fx = (float) s.K[0]; Frame::fy = (float) s.K[1]; Frame::cx = (float) s.K[2]; Frame::cy = (float) s.K[3];   // (the same for every case)
        s.solver.reset(new PnPsolver(s.frame, s.matches));
        if (s.solver->Correspondences() != s.n) { std::printf("solver %d kept %d correspondences of %d\n", k, s.solver->Correspondences(), s.n); return 1; }
        // epsilon 0 and a probability close to 1: mRansacMinInliers is minInliers, and mRansacMaxIts is maxIterations unless minInliers == N
        s.solver->SetRansacParameters(0.999999999999, s.minInliers, s.maxIts, s.minSet, 0.f, 1.f);
        if (s.solver->MinInliers() != s.minInliers || s.solver->MaxIterations() != s.maxIts) {
            std::printf("solver %d: parameters %d / %d, the case has %d / %d\n", k, s.solver->MinInliers(), s.solver->MaxIterations(), s.minInliers, s.maxIts);
            return 1;
        }
        s.solver->SetSamples(s.samples);
        if (k + 1 < B || B == 1) batch.push_back(s.solver.get());
    }
    batch.push_back(nullptr);
    PnPsolverBatch(batch);
    PnPsolverBatch(batch);   // nothing is left to evaluate: no second device call, no change
    std::vector<std::vector<uint8_t>> out(B);
    auto put = [](std::vector<uint8_t> &o, const void *p, size_t bytes) { if (bytes) o.insert(o.end(), (const uint8_t *) p, (const uint8_t *) p + bytes); };
    for (int j = 0;; j++) {
        bool any = false;
        for (int k = 0; k < B; k++) {
            Scene &s = *S[k];
            if (j >= s.nCalls) continue;
            any = true;
            bool noMore = false;
            std::vector<bool> inl;
            int nInliers = 0;
            const cv::Mat T = s.calls[j] < 0 ? s.solver->find(inl, nInliers) : s.solver->iterate(s.calls[j], noMore, inl, nInliers);
            if (s.calls[j] < 0) noMore = false;   // (find has no such output)
            const int rec[4] = {T.empty() ? 0 : 1, nInliers, noMore ? 1 : 0, (int) inl.size()};
            put(out[k], rec, sizeof rec);
            float T16[16] = {0};
            if (!T.empty())
                for (int r = 0; r < 4; r++) std::memcpy(T16 + 4 * r, T.ptr<float>(r), 4 * sizeof(float));
            put(out[k], T16, sizeof T16);
            std::vector<uint8_t> bytes(inl.size());
            for (size_t i = 0; i < inl.size(); i++) bytes[i] = inl[i] ? 1 : 0;
            put(out[k], bytes.data(), bytes.size());
        }
        if (!any) break;
    }
    FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    for (int k = 0; k < B; k++)
        if (!out[k].empty()) std::fwrite(out[k].data(), 1, out[k].size(), f);
    std::fclose(f);
    if (ygzf_host::failure_count() != failuresBefore) { std::printf("failures were reported on the way\n"); return 1; }
    std::printf("pnp shell ok\n");
    return 0;
}
