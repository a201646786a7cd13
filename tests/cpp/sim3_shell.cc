// sim3_shell.cc -- GPU test of ygz::Sim3Solver / ygz::Sim3SolverBatch (csrc/host/Sim3Solver.cc) over stub KeyFrames (tests/test_gpu_sim3.py):
// the solvers of argv[2..] are constructed from stub KeyFrames and MapPoints whose camera coordinates are the case's, given the case's triples
// (SetSamples), evaluated in ONE Sim3SolverBatch call -- except the last, which is left to evaluate itself -- and then driven round-robin, call j
// of every solver before call j + 1 of any, as LoopClosing::ComputeSim3 drives its candidates.  Every call's outcome is written out for the test
// to hold against tests/sim3_cases.py: sim3_iterate.
//   sim3_shell <out> <case>...   <case>: the file of sim3_cases.write_case followed by int32 octave1[n] octave2[n] | float sigma2[8]
//   <out>: per solver, per call: int32 returned nInliers noMore | float T12[16] (zeros when empty) | uint8 inliers12[mN1];
//          then per solver: int32 haveBest | float R[9] t[3] s
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "ORBextractor.h"
#include "Sim3Solver.h"
#include "ygz_compat.h"
#include "ygzf_pool.h"

using namespace ygz;
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

template <typename T> static void rd(FILE *f, T *p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) { std::printf("short read\n"); std::exit(2); }
}

struct Scene {
    int n = 0, mN1 = 0, H = 0, fix = 0, minInliers = 0, maxIterations = 0, nCalls = 0;
    double probability = 0;
    std::vector<int> calls, samples;
    KeyFrame kf1, kf2;
    std::vector<std::unique_ptr<MapPoint>> mps;
    std::vector<MapPoint *> matched12;
    std::unique_ptr<Sim3Solver> solver;
};

static MapPoint *point(Scene &S, const float *X, KeyFrame *kf, size_t idx) {
    S.mps.emplace_back(new MapPoint());
    MapPoint *mp = S.mps.back().get();
    for (int a = 0; a < 3; a++) mp->mWorldPos[a] = X[a];
    mp->mObservations[kf] = idx;
    return mp;
}

static void load(const char *path, Scene &S) {
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot read %s\n", path); std::exit(2); }
    int h[7];
    rd(f, h, 7);
    S.n = h[0]; S.mN1 = h[1]; S.H = h[2]; S.fix = h[3]; S.minInliers = h[4]; S.maxIterations = h[5]; S.nCalls = h[6];
    float K1[4], K2[4];
    rd(f, &S.probability, 1); rd(f, K1, 4); rd(f, K2, 4);
    const size_t n = (size_t) S.n;
    std::vector<int> idx1(n), o1(n), o2(n);
    std::vector<float> X1(3 * n), X2(3 * n), e1(n), e2(n), sigma2(8);
    S.calls.resize(S.nCalls); S.samples.resize(3 * (size_t) S.H);
    rd(f, S.calls.data(), S.calls.size()); rd(f, idx1.data(), n); rd(f, X1.data(), 3 * n); rd(f, X2.data(), 3 * n); rd(f, e1.data(), n); rd(f, e2.data(), n);
    rd(f, S.samples.data(), S.samples.size()); rd(f, o1.data(), n); rd(f, o2.data(), n); rd(f, sigma2.data(), 8);
    std::fclose(f);
    // both keyframes at the identity pose: the constructor's Rcw X + tcw returns the world position bit for bit
    for (KeyFrame *kf : {&S.kf1, &S.kf2}) {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) kf->mRcw(r, c) = r == c ? 1.f : 0.f;
        kf->mvLevelSigma2 = sigma2;
    }
    S.kf1.fx = K1[0]; S.kf1.fy = K1[1]; S.kf1.cx = K1[2]; S.kf1.cy = K1[3];
    S.kf2.fx = K2[0]; S.kf2.fy = K2[1]; S.kf2.cx = K2[2]; S.kf2.cy = K2[3];
    S.kf1.mvpMapPoints.assign(S.mN1, nullptr);
    S.matched12.assign(S.mN1, nullptr);
    S.kf1.mvKeys.resize(S.mN1);
    S.kf2.mvKeys.resize(S.mN1);
    const float origin[3] = {0.5f, 0.5f, 4.f};
    std::vector<char> used(S.mN1, 0);
    for (size_t i = 0; i < n; i++) {
        const int i1 = idx1[i];
        used[i1] = 1;
        S.kf1.mvKeys[i1].octave = o1[i];
        S.kf2.mvKeys[i1].octave = o2[i];
        S.kf1.mvpMapPoints[i1] = point(S, &X1[3 * i], &S.kf1, (size_t) i1);
        S.matched12[i1] = point(S, &X2[3 * i], &S.kf2, (size_t) i1);
    }
    // the entries between them are what the constructor's filter drops (:58-72), one kind after the other
    int kind = 0;
    for (int i1 = 0; i1 < S.mN1; i1++) {
        if (used[i1]) continue;
        switch (kind++ % 5) {
        case 0: break;                                                                     // no match
        case 1: S.matched12[i1] = point(S, origin, &S.kf2, (size_t) i1); break;            // matched, but the keyframe has no point there
        case 2: S.kf1.mvpMapPoints[i1] = point(S, origin, &S.kf1, (size_t) i1);            // a bad point on side 2
                S.matched12[i1] = point(S, origin, &S.kf2, (size_t) i1); S.matched12[i1]->mbBad = true; break;
        case 3: S.kf1.mvpMapPoints[i1] = point(S, origin, &S.kf1, (size_t) i1); S.kf1.mvpMapPoints[i1]->mbBad = true;   // a bad point on side 1
                S.matched12[i1] = point(S, origin, &S.kf2, (size_t) i1); break;
        default: S.kf1.mvpMapPoints[i1] = point(S, origin, &S.kf1, (size_t) i1);           // a point that is not observed in keyframe 2
                S.matched12[i1] = point(S, origin, &S.kf2, (size_t) i1); S.matched12[i1]->mObservations.clear(); break;
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const int B = argc - 2;
    std::vector<std::unique_ptr<Scene>> S;
    const unsigned long failuresBefore = ygzf_host::failure_count();
    std::vector<Sim3Solver *> batch;
    for (int k = 0; k < B; k++) {
        S.emplace_back(new Scene());
        load(argv[2 + k], *S[k]);
        Scene &s = *S[k];
        s.solver.reset(new Sim3Solver(&s.kf1, &s.kf2, s.matched12, s.fix != 0));
        if (s.solver->Correspondences() != s.n) { std::printf("solver %d kept %d correspondences of %d\n", k, s.solver->Correspondences(), s.n); return 1; }
        s.solver->SetRansacParameters(s.probability, s.minInliers, s.maxIterations);
        s.solver->SetSamples(s.samples);
        if (k + 1 < B || B == 1) batch.push_back(s.solver.get());
    }
    batch.push_back(nullptr);
    Sim3SolverBatch(batch);
    Sim3SolverBatch(batch);   // nothing is left to evaluate: no second device call, no change
    std::vector<std::vector<uint8_t>> out(B);
    auto put = [](std::vector<uint8_t> &o, const void *p, size_t bytes) { o.insert(o.end(), (const uint8_t *) p, (const uint8_t *) p + bytes); };
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
            const int rec[3] = {T.empty() ? 0 : 1, nInliers, noMore ? 1 : 0};
            put(out[k], rec, sizeof rec);
            float T16[16] = {0};
            if (!T.empty())
                for (int r = 0; r < 4; r++) std::memcpy(T16 + 4 * r, T.ptr<float>(r), 4 * sizeof(float));
            put(out[k], T16, sizeof T16);
            if ((int) inl.size() != s.mN1) { std::printf("solver %d: vbInliers has %d entries\n", k, (int) inl.size()); return 1; }
            std::vector<uint8_t> bytes(s.mN1);
            for (int i = 0; i < s.mN1; i++) bytes[i] = inl[i] ? 1 : 0;
            put(out[k], bytes.data(), bytes.size());
        }
        if (!any) break;
    }
    FILE *f = std::fopen(argv[1], "wb");
    if (!f) return 2;
    for (int k = 0; k < B; k++) std::fwrite(out[k].data(), 1, out[k].size(), f);
    for (int k = 0; k < B; k++) {
        const cv::Mat R = S[k]->solver->GetEstimatedRotation(), t = S[k]->solver->GetEstimatedTranslation();
        const int have = R.empty() ? 0 : 1;
        float v[13] = {0};
        if (have) {
            for (int r = 0; r < 3; r++) {
                std::memcpy(v + 3 * r, R.ptr<float>(r), 3 * sizeof(float));
                v[9 + r] = t.ptr<float>(r)[0];
            }
            v[12] = S[k]->solver->GetEstimatedScale();
        }
        std::fwrite(&have, sizeof have, 1, f);
        std::fwrite(v, sizeof(float), 13, f);
    }
    std::fclose(f);
    if (ygzf_host::failure_count() != failuresBefore) { std::printf("failures were reported on the way\n"); return 1; }
    std::printf("sim3 shell ok\n");
    return 0;
}
