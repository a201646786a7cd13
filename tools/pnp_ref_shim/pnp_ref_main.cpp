// pnp_ref_main.cpp -- drives the REFERENCE's ygz::PnPsolver (its src/PnPsolver.cc, compiled where it lies) through the calls of one case of
// tests/pnp_cases.py and writes every return (tools/make_golden_pnp_ref.py).
//   pnp_ref <case> <out>    <case>: the file of pnp_cases.write_case
//   <out>: per call int32 returned nInliers noMore size iterations bestInliers | float Tcw[16] (zeros when empty) | uint8 inliers[size]
// The gate of correspondence i travels as mvLevelSigma2[i] with octave i and th2 = 1; mRansacMinInliers and mRansacMaxIts are set to the
// case's after SetRansacParameters (the cases state them directly).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#define private public
#include "PnPsolver.h"
#undef private
#include "Thirdparty/DBoW2/DUtils/Random.h"

using namespace ygz;

template <typename T> static void rd(FILE *f, T *p, size_t n) {
    if (n && std::fread(p, sizeof(T), n, f) != n) { std::printf("short read\n"); std::exit(2); }
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int h[7];
    rd(f, h, 7);
    const int n = h[0], nMatches = h[1], H = h[2], minSet = h[3], minInliers = h[4], maxIts = h[5], nCalls = h[6];
    double K[4];
    rd(f, K, 4);
    std::vector<int> calls(nCalls), key(n), samples((size_t) H * minSet);
    std::vector<float> P3D(3 * (size_t) n), P2D(2 * (size_t) n), maxErr(n);
    rd(f, calls.data(), calls.size()); rd(f, key.data(), key.size()); rd(f, P3D.data(), P3D.size()); rd(f, P2D.data(), P2D.size());
    rd(f, maxErr.data(), maxErr.size()); rd(f, samples.data(), samples.size());
    std::fclose(f);
    Frame F;
    F.fx = (float) K[0]; F.fy = (float) K[1]; F.cx = (float) K[2]; F.cy = (float) K[3];
    F.mvKeys.resize(nMatches);
    F.mvLevelSigma2 = maxErr;
    F.mvLevelSigma2.push_back(1.f);
    F.mvpMapPoints.assign(nMatches, nullptr);
    std::vector<std::unique_ptr<MapPoint>> mps;
    std::vector<MapPoint *> matches(nMatches, nullptr);
    for (cv::KeyPoint &kp : F.mvKeys) kp.octave = n;
    std::vector<char> used(nMatches, 0);
    for (int i = 0; i < n; i++) {
        used[key[i]] = 1;
        F.mvKeys[key[i]].pt.x = P2D[2 * i];
        F.mvKeys[key[i]].pt.y = P2D[2 * i + 1];
        F.mvKeys[key[i]].octave = i;
        mps.emplace_back(new MapPoint());
        for (int a = 0; a < 3; a++) mps.back()->mWorldPos.v[a] = P3D[3 * i + a];
        matches[key[i]] = mps.back().get();
    }
    int kind = 0;
    for (int i = 0; i < nMatches; i++) {   // what the constructor drops: no match, a bad point, in turn
        if (used[i] || kind++ % 2 == 0) continue;
        mps.emplace_back(new MapPoint());
        mps.back()->mbBad = true;
        matches[i] = mps.back().get();
    }
    PnPsolver solver(F, matches);
    if (solver.N != n) { std::printf("the solver kept %d correspondences of %d\n", solver.N, n); return 1; }
    solver.SetRansacParameters(0.99, minInliers, maxIts, minSet, 0.f, 1.f);
    solver.mRansacMinInliers = minInliers;
    solver.mRansacMaxIts = maxIts;
    DUtils::Random::Load(samples, n, minSet);
    FILE *o = std::fopen(argv[2], "wb");
    if (!o) return 2;
    for (int j = 0; j < nCalls; j++) {
        bool noMore = false;
        std::vector<bool> inl;
        int nInliers = 0;
        const cv::Mat T = calls[j] < 0 ? solver.find(inl, nInliers) : solver.iterate(calls[j], noMore, inl, nInliers);
        if (calls[j] < 0) noMore = false;
        const int rec[6] = {T.empty() ? 0 : 1, nInliers, noMore ? 1 : 0, (int) inl.size(), solver.mnIterations, solver.mnBestInliers};
        std::fwrite(rec, sizeof(int), 6, o);
        float T16[16] = {0};
        if (!T.empty())
            for (int r = 0; r < 4; r++)
                for (int c = 0; c < 4; c++) T16[4 * r + c] = T.at<float>(r, c);
        std::fwrite(T16, sizeof(float), 16, o);
        for (size_t i = 0; i < inl.size(); i++) { const unsigned char b = inl[i] ? 1 : 0; std::fwrite(&b, 1, 1, o); }
    }
    std::fclose(o);
    return 0;
}
