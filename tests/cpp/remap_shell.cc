// remap_shell.cc -- GPU test of the undistortion behind ygz::ORBextractor (tests/test_gpu_remap_shell.py): SetUndistortMaps +
// ComputePyramidUndistorted followed by operator()(Frame *, ...) must give the levels, keypoints and descriptors of the plain shell --
// ComputePyramid + operator()(Frame *, ...) -- on the restated image (tests/remap_cases.py), twice on one extractor; Undistort gives that image.
//   remap_shell <dir>: <dir>/meta.txt = src_w src_h w h n, raw_<k>.bin, want_<k>.bin (k < n), map_xy.bin, map_tab.bin
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "ORBextractor.h"
#include "ygz_compat.h"
#include "ygzf_pool.h"

static int bad = 0;
#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); bad++; } \
    } while (0)

static cv::Mat read_mat(const std::string &path, int rows, int cols, int type, size_t elem) {
    cv::Mat m(rows, cols, type);
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f || std::fread(m.data, elem, (size_t) rows * cols, f) != (size_t) rows * cols) { std::printf("cannot read %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
    return m;
}

static bool same(const cv::Mat &a, const cv::Mat &b) {
    if (a.rows != b.rows || a.cols != b.cols) return false;
    for (int y = 0; y < a.rows; y++)
        if (std::memcmp(a.ptr(y), b.ptr(y), (size_t) a.cols) != 0) return false;
    return true;
}

struct Result {
    std::vector<cv::Mat> levels;
    std::vector<cv::KeyPoint> keys;
    cv::Mat desc;
};

// what Frame's constructor does with an extractor (src/Frame.cc:807-813, :332-348): the pyramid, a clone of its levels, the extraction
static Result frame_of(ygz::ORBextractor &ex, const cv::Mat &img, bool undistort) {
    Result r;
    ygz::Frame F;
    if (undistort) ex.ComputePyramidUndistorted(img);
    else ex.ComputePyramid(img);
    for (const cv::Mat &l : ex.mvImagePyramid) F.mvImagePyramid.push_back(l.clone());
    F.mImGray = F.mvImagePyramid[0];
    F.mpORBextractorLeft = &ex;
    ex(&F, r.keys, r.desc, ygz::ORBextractor::ORBSLAM_KEYPOINT);
    r.levels = F.mvImagePyramid;
    return r;
}

// `remap_shell time <dir> <blocks> <calls per block>` (tools/remap_rate.py): ComputePyramid of the restated image against ComputePyramidUndistorted of the
// raw one, alternating blocks on two extractors; us per call, median [fastest .. slowest] block
static int time_mode(const std::string &dir, int blocks, int calls) {
    int sw, sh, w, h, n;
    FILE *f = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || std::fscanf(f, "%d %d %d %d %d", &sw, &sh, &w, &h, &n) != 5) return 2;
    std::fclose(f);
    const cv::Mat map1 = read_mat(dir + "/map_xy.bin", h, w, CV_16SC2, 4), map2 = read_mat(dir + "/map_tab.bin", h, w, CV_16UC1, 2);
    const cv::Mat raw = read_mat(dir + "/raw_0.bin", sh, sw, CV_8UC1, 1), want = read_mat(dir + "/want_0.bin", h, w, CV_8UC1, 1);
    ygz::ORBextractor und(1000, 1.2f, 8, 20, 7), plain(1000, 1.2f, 8, 20, 7);
    if (!und.SetUndistortMaps(map1, map2)) return 2;
    std::vector<double> t[2];
    for (int b = -1; b < blocks; b++)               // block -1 warms both up
        for (int which = 0; which < 2; which++) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int i = 0; i < calls; i++)
                if (which) und.ComputePyramidUndistorted(raw);
                else plain.ComputePyramid(want);
            const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / calls;
            if (b >= 0) t[which].push_back(us);
        }
    if (!same(und.mvImagePyramid[0], want) || ygzf_host::failure_count()) return 1;
    for (int which = 0; which < 2; which++) {
        std::sort(t[which].begin(), t[which].end());
        std::printf("%s us_per_call median %.1f fastest %.1f slowest %.1f blocks %d calls %d\n", which ? "ComputePyramidUndistorted" : "ComputePyramid", t[which][t[which].size() / 2],
                    t[which].front(), t[which].back(), blocks, calls);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    if (argc == 5 && std::string(argv[1]) == "time") return time_mode(argv[2], std::atoi(argv[3]), std::atoi(argv[4]));
    const std::string dir = argv[1];
    int sw, sh, w, h, n;
    FILE *f = std::fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || std::fscanf(f, "%d %d %d %d %d", &sw, &sh, &w, &h, &n) != 5) return 2;
    std::fclose(f);
    const cv::Mat map1 = read_mat(dir + "/map_xy.bin", h, w, CV_16SC2, 4), map2 = read_mat(dir + "/map_tab.bin", h, w, CV_16UC1, 2);
    ygz::ORBextractor und(1000, 1.2f, 8, 20, 7), plain(1000, 1.2f, 8, 20, 7);
    CHECK(!und.SetUndistortMaps(map2, map1), "maps of the wrong types were accepted");
    CHECK(!und.SetUndistortMaps(map1, cv::Mat(h, w + 1, CV_16UC1)), "maps of two sizes were accepted");
    CHECK(und.SetUndistortMaps(map1, map2), "the maps were refused");
    const unsigned failuresBefore = (unsigned) ygzf_host::failure_count();
    for (int round = 0; round < 2; round++)          // twice on one extractor: the second round meets uploaded maps and the extract-ahead habit
        for (int k = 0; k < n; k++) {
            const cv::Mat raw = read_mat(dir + "/raw_" + std::to_string(k) + ".bin", sh, sw, CV_8UC1, 1);
            const cv::Mat want = read_mat(dir + "/want_" + std::to_string(k) + ".bin", h, w, CV_8UC1, 1);
            CHECK(und.SetUndistortMaps(map1, map2), "the maps the extractor holds were refused");
            const Result a = frame_of(und, raw, true), b = frame_of(plain, want, false);
            CHECK(a.levels.size() == 8 && b.levels.size() == 8, "levels");
            CHECK(same(a.levels[0], want), "round %d image %d: level 0 is not the restated image", round, k);
            for (size_t l = 0; l < a.levels.size() && l < b.levels.size(); l++) CHECK(same(a.levels[l], b.levels[l]), "round %d image %d: level %d differs", round, k, (int) l);
            CHECK(a.keys.size() == b.keys.size() && a.keys.size() > 500, "round %d image %d: %d vs %d keypoints", round, k, (int) a.keys.size(), (int) b.keys.size());
            if (a.keys.size() == b.keys.size()) {
                CHECK(std::memcmp(a.keys.data(), b.keys.data(), a.keys.size() * sizeof(cv::KeyPoint)) == 0, "round %d image %d: keypoints differ", round, k);
                CHECK(same(a.desc, b.desc), "round %d image %d: descriptors differ", round, k);
            }
            // (the frame's level 0 is what the context holds, as after ComputePyramid: SparseImgAlign's image cache copies device to device)
            CHECK(plain.ResidentContext(b.levels[0]) != nullptr, "round %d image %d: the plain shell holds no resident image", round, k);
            CHECK(und.ResidentContext(a.levels[0]) != nullptr, "round %d image %d: no resident image after ComputePyramidUndistorted", round, k);
            cv::Mat right;
            CHECK(und.Undistort(raw, right) && same(right, want), "round %d image %d: Undistort is not the restated image", round, k);
        }
    CHECK((unsigned) ygzf_host::failure_count() == failuresBefore, "failures were reported on the way");
    if (bad) return 1;
    std::printf("remap shell ok\n");
    return 0;
}
