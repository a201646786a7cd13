// tri_host.cc -- csrc/tri_math.h as a plain host program, for tests/test_tri_host_progs.py: the text k_triangulate compiles, on one host
// thread, over the files tests/triangulate_cases.py writes.
//   tri_host pairs in.bin out.bin   float ratio | int32 nPairs | kf1 | kf2 | int32 idx1[nPairs] idx2[nPairs]
//                                   kf: int32 n nlevels stereo | float fx fy cx cy invfx invfy mbf Rcw[9] tcw[3] Ow[3] q[4] t[3] | keys n x 28 bytes |
//                                       float sigma2[nlevels] scale[nlevels] | stereo: float uRight[n] depth[n] cosStereo[n]
//                                -> float x3d[3 nPairs] | uint8 status[nPairs] | int32 sweeps[nPairs]
//   tri_host svd in.bin out.bin     float A[16] row-major -> float V[16] | float sv[4] | int32 sweeps
//   tri_host time reps in.bin ..    the one-thread yardstick of tools/triangulate_rate.py: every pair of every file (one file per neighbour) is one
//                                   pass; prints the us per pass as median, fastest, slowest of 9 windows of `reps` passes, one untimed first
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tri_math.h"

namespace {

struct Key { float x, y, size, angle, response; int32_t octave, class_id; };
static_assert(sizeof(Key) == 28, "cv::KeyPoint layout");

struct HostKf {
    ygzf::tri::Kf k;
    int n = 0, nlevels = 0, stereo = 0;
    std::vector<Key> keys;
    std::vector<float> sigma2, scale, uRight, depth, cosStereo;
};

template <typename T> void get(FILE *f, T *p, size_t n) {
    if (n && fread(p, sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
}
template <typename T> void put(FILE *f, const T *p, size_t n) {
    if (n && fwrite(p, sizeof(T), n, f) != n) { fprintf(stderr, "short write\n"); exit(2); }
}

void read_kf(FILE *f, HostKf &K) {
    int head[3];
    get(f, head, 3);
    K.n = head[0]; K.nlevels = head[1]; K.stereo = head[2];
    float s[7];
    get(f, s, 7);
    K.k.fx = s[0]; K.k.fy = s[1]; K.k.cx = s[2]; K.k.cy = s[3]; K.k.invfx = s[4]; K.k.invfy = s[5]; K.k.mbf = s[6];
    get(f, K.k.Rcw, 9); get(f, K.k.tcw, 3); get(f, K.k.Ow, 3); get(f, K.k.q, 4); get(f, K.k.t, 3);
    K.keys.resize(K.n); get(f, K.keys.data(), K.n);
    K.sigma2.resize(K.nlevels); get(f, K.sigma2.data(), K.nlevels);
    K.scale.resize(K.nlevels); get(f, K.scale.data(), K.nlevels);
    if (K.stereo) {
        K.uRight.resize(K.n); get(f, K.uRight.data(), K.n);
        K.depth.resize(K.n); get(f, K.depth.data(), K.n);
        K.cosStereo.resize(K.n); get(f, K.cosStereo.data(), K.n);
    }
}

// the gather of tri_kernels.hip's tri_feature
ygzf::tri::Feat feature(const HostKf &K, int idx) {
    if (idx < 0 || idx >= K.n) { fprintf(stderr, "index %d outside [0, %d)\n", idx, K.n); exit(2); }
    const Key &kp = K.keys[idx];
    if (kp.octave < 0 || kp.octave >= K.nlevels) { fprintf(stderr, "octave %d outside [0, %d)\n", kp.octave, K.nlevels); exit(2); }
    ygzf::tri::Feat f;
    f.x = kp.x; f.y = kp.y;
    f.uR = K.stereo ? K.uRight[idx] : -1.f;
    const bool stereo = f.uR >= 0.f;
    f.depth = stereo ? K.depth[idx] : -1.f;
    f.cosStereo = stereo ? K.cosStereo[idx] : 0.f;
    f.sigma2 = K.sigma2[kp.octave];
    f.scale = K.scale[kp.octave];
    return f;
}

struct Problem {
    float ratio = 0;
    HostKf K1, K2;
    std::vector<int32_t> idx1, idx2;
};
void read_problem(FILE *in, Problem &P) {
    int32_t n;
    get(in, &P.ratio, 1); get(in, &n, 1);
    read_kf(in, P.K1); read_kf(in, P.K2);
    P.idx1.resize(n); P.idx2.resize(n);
    get(in, P.idx1.data(), n); get(in, P.idx2.data(), n);
}

int time_mode(int argc, char **argv) {
    const int reps = atoi(argv[2]);
    std::vector<Problem> probs(argc - 3);
    size_t total = 0;
    for (int k = 3; k < argc; k++) {
        FILE *in = fopen(argv[k], "rb");
        if (!in) { fprintf(stderr, "cannot open %s\n", argv[k]); return 2; }
        read_problem(in, probs[k - 3]);
        fclose(in);
        total += probs[k - 3].idx1.size();
    }
    std::vector<float> x3d(3 * total);
    std::vector<uint8_t> status(total);
    std::vector<double> us;
    unsigned long sink = 0;
    for (int w = -1; w < 9; w++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (int r = 0; r < reps; r++) {
            size_t at = 0;
            for (const Problem &P : probs)
                for (size_t i = 0; i < P.idx1.size(); i++, at++)
                    status[at] = ygzf::tri::triangulate_pair(P.K1.k, P.K2.k, feature(P.K1, P.idx1[i]), feature(P.K2, P.idx2[i]), P.ratio, &x3d[3 * at], nullptr);
            sink += status[(size_t) r % total];
        }
        const double t = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / reps;
        if (w >= 0) us.push_back(t);
    }
    std::sort(us.begin(), us.end());
    printf("%.2f %.2f %.2f %lu\n", us[us.size() / 2], us.front(), us.back(), sink);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc >= 4 && !strcmp(argv[1], "time")) return time_mode(argc, argv);
    if (argc != 4) { fprintf(stderr, "usage: tri_host pairs|svd in out\n"); return 2; }
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    if (!strcmp(argv[1], "svd")) {
        float A[4][4], V[4][4], sv[4];
        get(in, &A[0][0], 16);
        const int32_t sweeps = ygzf::tri::jacobi_svd4(A, V, sv);
        put(out, &V[0][0], 16); put(out, sv, 4); put(out, &sweeps, 1);
    } else if (!strcmp(argv[1], "pairs")) {
        Problem P;
        read_problem(in, P);
        const size_t n = P.idx1.size();
        std::vector<int32_t> sweeps(n);
        std::vector<float> x3d(3 * n);
        std::vector<uint8_t> status(n);
        for (size_t i = 0; i < n; i++) {
            int s = 0;
            status[i] = ygzf::tri::triangulate_pair(P.K1.k, P.K2.k, feature(P.K1, P.idx1[i]), feature(P.K2, P.idx2[i]), P.ratio, &x3d[3 * i], &s);
            sweeps[i] = s;
        }
        put(out, x3d.data(), x3d.size()); put(out, status.data(), status.size()); put(out, sweeps.data(), sweeps.size());
    } else {
        fprintf(stderr, "unknown mode %s\n", argv[1]);
        return 2;
    }
    fclose(in);
    return fclose(out) ? 2 : 0;
}
