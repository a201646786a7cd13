// tri_shell.cc -- host/LocalMappingTriangulate.cc over the stand-alone classes, for tests/test_gpu_tri.py.  The inputs are the pair files of
// tests/triangulate_cases.py (one per neighbour, all with the same KF1; tests/cpp/tri_host.cc states the layout).
//   tri_shell pairs min mb1 mb2 in.bin out.bin    ygz::TriangulatePairsDevice on the file's pairs -> float x3d[3 n] | uint8 status[n].  min: the host
//                                                 threshold (0: the device always; a large number: the host always; -1: the default)
//   tri_shell batch min mono stop out.bin mb in.bin ..
//       the files' keyframes as a map: feature i of every keyframe carries descriptor D(i) and vocabulary node i / 4, so SearchForTriangulation
//       finds the true partners that pass the epipolar gate, and every neighbour matches the same KF1 features; every seventh slot of a
//       keyframe holds a MapPoint already.  Runs (a) the neighbour loop as the reference runs it -- live search, ygz::TriangulatePairsDevice
//       per neighbour, :1197-1214 -- on one copy and (b) ygz::CreateNewMapPointsBatch on another, compares the created points (neighbour, idx1,
//       idx2, x3D as bits), every slot and the points' normals and distances, and writes (a)'s points: int32 count | per point int32 neighbour
//       idx1 idx2, float x3D[3].  stop: the neighbour before which CheckNewKeyFrames() turns true (-1: never).  mono: the monocular gate.
//   tri_shell time reps mb in.bin ..              tools/triangulate_rate.py: the whole neighbour loop, searches included, on a map built anew (untimed)
//       for every call -> three lines "median fastest slowest" in us over 9 windows of `reps` calls, one untimed window first:
//       CreateNewMapPointsBatch at the default threshold; the loop neighbour by neighbour (search, one triangulation call, map updates) at the
//       default threshold; CreateNewMapPointsBatch with the triangulation forced onto the host thread; then "created n"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <list>
#include <vector>

#include "ORBextractor.h"
#include "ORBmatcher.h"
#include "ygz_compat.h"
#include "LocalMappingTriangulate.h"

using namespace ygz;

float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::invfx, Frame::invfy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;   // (ORBmatcher.cc reads them)

namespace {

template <typename T> void get(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
}

void read_kf(FILE *f, KeyFrame &K, float mb) {
    int head[3];
    get(f, head, 3);
    const int n = head[0], nl = head[1], st = head[2];
    float s[7], R[9], t[3], O[3], q[4], tw[3];
    get(f, s, 7); get(f, R, 9); get(f, t, 3); get(f, O, 3); get(f, q, 4); get(f, tw, 3);
    K.N = n;
    K.fx = s[0]; K.fy = s[1]; K.cx = s[2]; K.cy = s[3]; K.invfx = s[4]; K.invfy = s[5]; K.mbf = s[6]; K.mb = mb;
    for (int i = 0; i < 9; i++) K.mRcw.m[i] = R[i];
    for (int i = 0; i < 3; i++) { K.mtcw[i] = t[i]; K.mOw[i] = O[i]; K.Twc.t[i] = tw[i]; }
    for (int i = 0; i < 4; i++) K.Twc.q[i] = q[i];
    K.mvKeys.resize(n);
    static_assert(sizeof(cv::KeyPoint) == 28, "cv::KeyPoint layout");
    get(f, K.mvKeys.data(), n);
    K.mvLevelSigma2.resize(nl); get(f, K.mvLevelSigma2.data(), nl);
    K.mvScaleFactors.resize(nl); get(f, K.mvScaleFactors.data(), nl);
    K.mnScaleLevels = nl;
    K.mfScaleFactor = nl > 1 ? K.mvScaleFactors[1] : 1.f;
    if (st) {
        K.mvuRight.resize(n); get(f, K.mvuRight.data(), n);
        K.mvDepth.resize(n); get(f, K.mvDepth.data(), n);
        std::vector<float> cosStereo(n); get(f, cosStereo.data(), n);   // the shell computes its own
    } else {
        K.mvuRight.assign(n, -1.f);
        K.mvDepth.assign(n, -1.f);
    }
    K.mvpMapPoints.assign(n, nullptr);
}

struct Problem {
    float ratio = 0;
    std::vector<std::pair<size_t, size_t>> pairs;
};
void read_problem(const char *path, KeyFrame &K1, KeyFrame &K2, Problem &P, float mb1, float mb2) {
    FILE *in = fopen(path, "rb");
    if (!in) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    int32_t n;
    get(in, &P.ratio, 1); get(in, &n, 1);
    read_kf(in, K1, mb1); read_kf(in, K2, mb2);
    std::vector<int32_t> a(n), b(n);
    get(in, a.data(), n); get(in, b.data(), n);
    for (int i = 0; i < n; i++) P.pairs.push_back({(size_t) a[i], (size_t) b[i]});
    fclose(in);
}

int pairs_mode(int argc, char **argv) {
    if (argc != 7) return 2;
    const int mn = atoi(argv[2]);
    if (mn >= 0) ygzf_host_tri_device_min = mn;
    KeyFrame K1, K2;
    Problem P;
    read_problem(argv[5], K1, K2, P, (float) atof(argv[3]), (float) atof(argv[4]));
    std::vector<float> x3d;
    std::vector<uint8_t> status;
    if (!TriangulatePairsDevice(&K1, &K2, P.pairs, P.ratio, x3d, status)) { fprintf(stderr, "TriangulatePairsDevice failed\n"); return 1; }
    FILE *out = fopen(argv[6], "wb");
    if (!out) return 2;
    fwrite(x3d.data(), sizeof(float), x3d.size(), out);
    fwrite(status.data(), 1, status.size(), out);
    return fclose(out) ? 2 : 0;
}

// ---- the batch ------------------------------------------------------------------------------------------------------------------------
struct World {
    KeyFrame cur;
    std::vector<KeyFrame> neigh;
    Map map;
    std::list<MapPoint *> recent;
    std::vector<MapPoint *> owned;
    ~World() { for (MapPoint *p : owned) delete p; for (MapPoint *p : recent) delete p; }
};

void descriptor(int i, unsigned char *d) {
    unsigned s = 2654435761u * (unsigned) (i + 1);
    for (int b = 0; b < 32; b++) { s = s * 1664525u + 1013904223u; d[b] = (unsigned char) (s >> 24); }
}
void dress(World &w, KeyFrame &K, int id) {
    K.mnId = id;
    K.mDescriptors.create(K.N, 32, CV_8U);
    for (int i = 0; i < K.N; i++) {
        descriptor(i, K.mDescriptors.ptr(i));
        K.mFeatVec[(unsigned) (i / 4)].push_back((unsigned) i);
        if (i % 7 == (id % 7)) {   // a point from before; its position is two units in front of the keyframe (ComputeSceneMedianDepth reads it)
            MapPoint *p = new MapPoint();
            p->mnId = 1000000 + w.owned.size();
            for (int a = 0; a < 3; a++) p->mWorldPos[a] = K.mOw[a] + 2.f * K.mRcw(2, a);
            K.mvpMapPoints[i] = p;
            w.owned.push_back(p);
        }
    }
}
void make_world(World &w, int nfiles, char **files, float mb) {
    w.neigh.resize(nfiles);
    for (int j = 0; j < nfiles; j++) {
        KeyFrame k1;
        Problem P;
        read_problem(files[j], j == 0 ? w.cur : k1, w.neigh[j], P, mb, mb);
    }
    dress(w, w.cur, 0);
    for (int j = 0; j < nfiles; j++) dress(w, w.neigh[j], j + 1);
}

// LocalMapping::ComputeF12 (src/LocalMapping.cc:1329-1344) for the test: K1^-T [t12]x R12 K2^-1 in double, rounded once
Matrix3f compute_f12(KeyFrame *&a, KeyFrame *&b) {
    double R12[9], t12[3], tx[9], M[9], N[9], F[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            R12[3 * r + c] = 0;
            for (int k = 0; k < 3; k++) R12[3 * r + c] += (double) a->mRcw(r, k) * b->mRcw(c, k);
        }
    for (int r = 0; r < 3; r++) {
        t12[r] = a->mtcw[r];
        for (int k = 0; k < 3; k++) t12[r] -= R12[3 * r + k] * b->mtcw[k];
    }
    const double x[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};
    memcpy(tx, x, sizeof x);
    const double K1iT[9] = {1.0 / a->fx, 0, 0, 0, 1.0 / a->fy, 0, -a->cx / (double) a->fx, -a->cy / (double) a->fy, 1};
    const double K2i[9] = {1.0 / b->fx, 0, -b->cx / (double) b->fx, 0, 1.0 / b->fy, -b->cy / (double) b->fy, 0, 0, 1};
    auto mul = [](const double *A, const double *B, double *C) {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) { C[3 * r + c] = 0; for (int k = 0; k < 3; k++) C[3 * r + c] += A[3 * r + k] * B[3 * k + c]; }
    };
    mul(K1iT, tx, M); mul(M, R12, N); mul(N, K2i, F);
    Matrix3f o;
    for (int i = 0; i < 9; i++) o.m[i] = (float) F[i];
    return o;
}

struct Poll {
    int stop, calls = 0;
    bool operator()() { calls++; return stop >= 0 && calls >= stop; }
};

// the loop as the reference runs it (src/LocalMapping.cc:1009-1216), the per-pair body through the one-neighbour shell
int sequential(World &w, bool mono, int stop) {
    Poll poll{stop};
    ORBmatcher matcher(0.6, false);
    KeyFrame *cur = &w.cur;
    const float ratioFactor = 1.5f * cur->mfScaleFactor;
    int nnew = 0;
    for (size_t j = 0; j < w.neigh.size(); j++) {
        if (j > 0 && poll()) return nnew;
        KeyFrame *k2 = &w.neigh[j];
        const float b[3] = {k2->mOw[0] - cur->mOw[0], k2->mOw[1] - cur->mOw[1], k2->mOw[2] - cur->mOw[2]};
        const float baseline = std::sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
        if (!mono) { if (baseline < k2->mb) continue; }
        else if (baseline / k2->ComputeSceneMedianDepth(2) < 0.01) continue;
        Matrix3f F12 = compute_f12(cur, k2);
        std::vector<std::pair<size_t, size_t>> pairs;
        matcher.SearchForTriangulation(cur, k2, F12, pairs, false);
        std::vector<float> x3d;
        std::vector<uint8_t> status;
        if (!TriangulatePairsDevice(cur, k2, pairs, ratioFactor, x3d, status)) { fprintf(stderr, "TriangulatePairsDevice failed\n"); exit(1); }
        for (size_t i = 0; i < pairs.size(); i++) {
            if (status[i] & 15) continue;
            Vector3f X;
            for (int a = 0; a < 3; a++) X[a] = x3d[3 * i + a];
            MapPoint *p = new MapPoint(X, cur, &w.map);
            p->AddObservation(cur, pairs[i].first);
            p->AddObservation(k2, pairs[i].second);
            cur->AddMapPoint(p, pairs[i].first);
            k2->AddMapPoint(p, pairs[i].second);
            p->ComputeDistinctiveDescriptors();
            p->UpdateNormalAndDepth();
            w.map.AddMapPoint(p);
            w.recent.push_back(p);
            nnew++;
        }
    }
    return nnew;
}

long id_of(const MapPoint *p) { return p ? (long) p->mnId : -1; }

int compare(World &a, World &b) {
    int bad = a.recent.size() != b.recent.size();
    std::list<MapPoint *>::iterator ia = a.recent.begin(), ib = b.recent.begin();
    for (; ia != a.recent.end() && ib != b.recent.end(); ++ia, ++ib) {
        MapPoint *p = *ia, *q = *ib;
        bad += p->mnId != q->mnId || memcmp(&p->mWorldPos, &q->mWorldPos, sizeof p->mWorldPos) != 0 ||
               memcmp(&p->mNormalVector, &q->mNormalVector, sizeof p->mNormalVector) != 0 || p->mfMaxDistance != q->mfMaxDistance ||
               p->mfMinDistance != q->mfMinDistance || p->nObs != q->nObs || p->mObservations.size() != q->mObservations.size();
        bad += p->mObservations[&a.cur] != q->mObservations[&b.cur];
    }
    for (int i = 0; i < a.cur.N; i++) bad += id_of(a.cur.mvpMapPoints[i]) != id_of(b.cur.mvpMapPoints[i]);
    for (size_t j = 0; j < a.neigh.size(); j++)
        for (int i = 0; i < a.neigh[j].N; i++) bad += id_of(a.neigh[j].mvpMapPoints[i]) != id_of(b.neigh[j].mvpMapPoints[i]);
    return bad;
}

int batch_mode(int argc, char **argv) {
    if (argc < 8) return 2;
    const int mn = atoi(argv[2]), mono = atoi(argv[3]), stop = atoi(argv[4]);
    const float mb = (float) atof(argv[6]);
    World a, b;
    make_world(a, argc - 7, argv + 7, mb);
    make_world(b, argc - 7, argv + 7, mb);
    ygzf_host_tri_device_min = 1 << 30;   // (a): the host text, pair by pair
    const int nA = sequential(a, mono != 0, stop);
    if (mn >= 0) ygzf_host_tri_device_min = mn; else ygzf_host_tri_device_min = 64;
    std::vector<KeyFrame *> neigh;
    for (KeyFrame &k : b.neigh) neigh.push_back(&k);
    Poll poll{stop};
    const int nB = CreateNewMapPointsBatch(&b.cur, neigh, &b.map, b.recent, mono != 0, compute_f12, [&] { return poll(); });
    const int bad = compare(a, b) + (nA != nB);
    FILE *out = fopen(argv[5], "wb");
    if (!out) return 2;
    const int32_t count = (int32_t) a.recent.size();
    fwrite(&count, 4, 1, out);
    for (MapPoint *p : a.recent) {
        int32_t rec[3] = {-1, (int32_t) p->mObservations[&a.cur], -1};
        for (size_t j = 0; j < a.neigh.size(); j++)
            if (p->mObservations.count(&a.neigh[j])) { rec[0] = (int32_t) j; rec[2] = (int32_t) p->mObservations[&a.neigh[j]]; }
        fwrite(rec, 4, 3, out);
        fwrite(&p->mWorldPos, sizeof(float), 3, out);
    }
    fclose(out);
    std::printf("created %d batch %d differences %d\n", nA, nB, bad);
    if (bad) return 1;
    std::printf("tri shell ok\n");
    return 0;
}

int time_mode(int argc, char **argv) {
    if (argc < 5) return 2;
    const int reps = atoi(argv[2]);
    const float mb = (float) atof(argv[3]);
    int created = 0;
    for (int variant = 0; variant < 3; variant++) {
        ygzf_host_tri_device_min = variant == 2 ? 1 << 30 : 64;
        std::vector<double> us;
        for (int w = -1; w < 9; w++) {
            double sum = 0;
            for (int r = 0; r < reps; r++) {
                World world;
                make_world(world, argc - 4, argv + 4, mb);
                std::vector<KeyFrame *> neigh;
                for (KeyFrame &k : world.neigh) neigh.push_back(&k);
                const auto t0 = std::chrono::steady_clock::now();
                if (variant == 1) created = sequential(world, false, -1);
                else created = CreateNewMapPointsBatch(&world.cur, neigh, &world.map, world.recent, false, compute_f12, [] { return false; });
                sum += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            }
            if (w >= 0) us.push_back(sum / reps);
        }
        std::sort(us.begin(), us.end());
        std::printf("%.1f %.1f %.1f\n", us[us.size() / 2], us.front(), us.back());
    }
    std::printf("created %d\n", created);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "time")) return time_mode(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "pairs")) return pairs_mode(argc, argv);
    if (argc >= 2 && !strcmp(argv[1], "batch")) return batch_mode(argc, argv);
    fprintf(stderr, "usage: tri_shell pairs|batch ...\n");
    return 2;
}
