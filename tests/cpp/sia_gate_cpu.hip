// sia_gate_cpu.hip -- csrc/sia_gate.h on the CPU, as a stand-alone host program (tests/test_sia_host_progs.py builds it with AddressSanitizer and
// UBSan).  1. For every level size of a sweep and every float around every gate (all floats within a few ulps of 3 and n - 3, a dense sweep over
// [-2, n + 2], the small and the large values the int conversion still defines) sia_patch_inside answers as the reference's form does --
// (int) floorf, then the integer comparisons -- and returns the same ui, vi.  2. NaN, the infinities, +-3e9 and the neighbours of +-2^31 are
// outside, on either axis, and leave ui, vi untouched.  Prints the number of comparisons; exits non-zero on the first difference.
#include <climits>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include <hip/hip_runtime.h>

#include "sia_gate.h"

static bool reference_form(float u, float v, int w, int h, int &ui, int &vi) {   // only ever called with |u|, |v| < 2^31
    const int border = 3;
    const int a = (int) floorf(u), b = (int) floorf(v);
    if (a < 0 || b < 0 || a - border < 0 || b - border < 0 || a + border >= w || b + border >= h) return false;
    ui = a;
    vi = b;
    return true;
}

static std::vector<float> probes(int n) {
    std::vector<float> p;
    for (float c : {0.f, 2.f, 3.f, 4.f, (float) (n - 4), (float) (n - 3), (float) (n - 2), (float) n}) {
        float lo = c, hi = c;
        p.push_back(c);
        for (int k = 0; k < 4; k++) {
            lo = std::nextafterf(lo, -INFINITY);
            hi = std::nextafterf(hi, INFINITY);
            p.push_back(lo);
            p.push_back(hi);
        }
    }
    for (int k = -16; k <= 8 * (n + 2); k++) p.push_back(0.125f * (float) k);
    for (float c : {-0.f, 1e-30f, -1e-30f, 2.99f, 2.9999998f, -3.f, -1000.5f, 1e6f, -1e6f, 16777216.f, 16777218.f, 2147483520.f, -2147483520.f, -2147483648.f}) p.push_back(c);
    return p;
}

int main() {
    long long compared = 0;
    const int sizes[][2] = {{7, 42}, {8, 42}, {6, 6}, {7, 7}, {9, 8}, {96, 72}, {67, 50}, {509, 331}, {752, 480}, {3840, 2160}, {16777216, 7}};
    for (const auto &s : sizes) {
        const int w = s[0], h = s[1];
        const std::vector<float> pu = probes(w < 1024 ? w : 16), pv = probes(h < 1024 ? h : 16);
        std::vector<float> us = pu, vs = pv;
        if (w >= 1024)
            for (float c : probes(16))
                if (fabsf(c) < 1000.f) us.push_back(c + (float) (w - 16));   // around the right gate of a wide level
        if (h >= 1024)
            for (float c : probes(16))
                if (fabsf(c) < 1000.f) vs.push_back(c + (float) (h - 16));
        for (float u : us)
            for (float v : vs) {
                int a = -7, b = -7, c = -7, d = -7;
                const bool r = reference_form(u, v, w, h, a, b), g = ygzf::sia_patch_inside(u, v, w, h, c, d);
                compared++;
                if (r != g || a != c || b != d) {
                    fprintf(stderr, "FAILED: u %.9g v %.9g in %d x %d: reference %d (%d, %d), header %d (%d, %d)\n", u, v, w, h, r, a, b, g, c, d);
                    return 1;
                }
            }
    }
    const float bad[] = {NAN, -NAN, INFINITY, -INFINITY, 3e9f, -3e9f, 2147483648.f, std::nextafterf(2147483648.f, INFINITY), 4294967296.f, 4294967300.f, -4294967296.f,
                         std::nextafterf(-2147483648.f, -INFINITY), 3.4e38f, -3.4e38f, 1.8446744e19f};
    for (const auto &s : sizes)
        for (float x : bad)
            for (float ok : {3.f, 3.5f, (float) (s[1] < s[0] ? s[1] : s[0]) - 3.5f}) {
                int a = -7, b = -7;
                if (ygzf::sia_patch_inside(x, ok, s[0], s[1], a, b) || ygzf::sia_patch_inside(ok, x, s[0], s[1], a, b) || ygzf::sia_patch_inside(x, x, s[0], s[1], a, b) || a != -7 || b != -7) {
                    fprintf(stderr, "FAILED: %.9g is not rejected in %d x %d\n", x, s[0], s[1]);
                    return 1;
                }
                compared += 3;
            }
    printf("%lld\n", compared);
    return 0;
}
