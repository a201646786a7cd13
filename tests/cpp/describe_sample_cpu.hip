// describe_sample_cpu.hip -- host build of csrc/describe_sample.h, the arithmetic of one sample of describe_window's column pass, against the form it
// replaces: rintf of the rotated coordinates, the integer address 2 * ((18 + r) * kHbP + 18 + q) and the tap sum written out with four
// multiplications.  Built with -ffp-contract=off, as the library is.  Prints one JSON object of counts; "mismatches" must be 0.
//   * every pattern point (orb_pattern_table.h's 375 distinct ones) under (a, b) = sincos_deg of every multiple of 1/64 degree (sincos_deg restated
//     here operation for operation from csrc/extract_kernels.hip) and of 10^5 random angles;
//   * every integer point of [-13, 13]^2 under every (a, b) of multiples of 1/8 inside the unit disc: products that are multiples of 1/8, so
//     that exact .5 ties of both signs occur by the thousand (x = +-13, a = +-0.5 gives +-6.5);
//   * (v + M) - M against rintf on 10^6 random floats of (-2^22, 2^22) and on every half-integer of [-64, 64];
//   * the multiply-add chain against the written-out sum for all-0, all-65535 and 10^5 random septets of 16-bit values, in the three cv modes'
//     tap constants.
// Host code only.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "describe_sample.h"
#include "orb_pattern_table.h"

using namespace ygzf;

static long fails = 0;
#define FAIL(...)                                           \
    do {                                                    \
        if (fails++ < 10) { fprintf(stderr, __VA_ARGS__); } \
    } while (0)

static uint64_t rngState = 0x9E3779B97F4A7C15ull;
static uint32_t rnd32() {   // xorshift64*
    rngState ^= rngState >> 12;
    rngState ^= rngState << 25;
    rngState ^= rngState >> 27;
    return (uint32_t) ((rngState * 0x2545F4914F6CDD1Dull) >> 32);
}

// csrc/extract_kernels.hip's sincos_deg, operation for operation
static void sincos_deg(float angle_deg, float *c_out, float *s_out) {
    const float factorPI = (float) (3.14159265358979323846 / 180.f);
    const float angle = angle_deg * factorPI;
    const double x = (double) angle;
    const double TWO_OVER_PI = 6.36619772367581382433e-01, PIO2_1 = 1.57079632673412561417e+00, PIO2_1T = 6.07710050650619224932e-11;
    const double kd = floor(x * TWO_OVER_PI + 0.5);
    const int k = (int) kd;
    const double r = (x - kd * PIO2_1) - kd * PIO2_1T;
    const double z = r * r;
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double sr = r + (z * r) * (S1 + z * (S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))));
    const double rc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))));
    const double cr = 1.0 - (0.5 * z - z * rc);
    double s, c;
    switch (k & 3) {
        case 0: s = sr; c = cr; break;
        case 1: s = cr; c = -sr; break;
        case 2: s = -sr; c = -cr; break;
        default: s = -cr; c = sr; break;
    }
    *c_out = (float) c;
    *s_out = (float) s;
}

static long samples = 0, tiesUp = 0, tiesDown = 0, tiesNeg = 0, tiesPos = 0;
static int rMin = 0, rMax = 0, qMin = 0, qMax = 0;

// one sample both ways
static void check_sample(float x, float y, float a, float b) {
    // the form replaced: two products and one add or subtract, rintf, integer address
    volatile float rf = x * b + y * a, qf = x * a - y * b;
    const int r = (int) rintf(rf), q = (int) rintf(qf);
    const int wantByte = 2 * ((18 + r) * kHbP + 18 + q);
    float R, Q;
    ds::rotated(x, y, a, b, &R, &Q);
    const unsigned gotByte = ds::hb_byte(R, Q);
    samples++;
    for (float v : {(float) rf, (float) qf})
        if (fabsf(v - truncf(v)) == 0.5f) {
            (v < 0 ? tiesNeg : tiesPos)++;
            (rintf(v) > v ? tiesUp : tiesDown)++;
        }
    if (r < rMin) rMin = r;
    if (r > rMax) rMax = r;
    if (q < qMin) qMin = q;
    if (q > qMax) qMax = q;
    if (R != (float) r || Q != (float) q || (int) R != r || (int) Q != q)
        FAIL("point (%g, %g) a %a b %a: rounded (%g, %g), expected (%d, %d)\n", x, y, a, b, R, Q, r, q);
    else if ((int) gotByte != wantByte || ds::float_bits(ds::hb_byte_f(R, Q)) != ds::kTwo23Bits + (unsigned) wantByte)
        FAIL("point (%g, %g) a %a b %a: byte %u, expected %d\n", x, y, a, b, gotByte, wantByte);
    // the seven taps p[0] .. p[6 * kHbP] lie inside hb
    if (wantByte < 0 || wantByte + 6 * ds::kHbRowBytes + 2 > kHbBytes) FAIL("point (%g, %g) a %a b %a: byte %d outside hb\n", x, y, a, b, wantByte);
}

static void check_round(float v) {
    const float got = ds::round_even(v), want = rintf(v);
    if (memcmp(&got, &want, 4) != 0 && !(got == 0.f && want == 0.f)) FAIL("round_even(%a) = %a, rintf = %a\n", v, got, want);
}

template <unsigned K2, unsigned K3>
static void check_taps(const unsigned (&p)[7]) {
    // the expression replaced
    const int sum = 18 * (int) (p[0] + p[6]) + 34 * (int) (p[1] + p[5]) + (int) K2 * (int) (p[2] + p[4]) + (int) K3 * (int) p[3];
    const int t = (sum + 32768) >> 16;
    const bool tie = (sum & 0xFFFF) == 0x8000;
    const unsigned got = ds::tap_sum<K2, K3>(p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
    if (got != (unsigned) sum + 32768u || (int) (got >> 16) != t || ((got & 0xFFFFu) == 0u) != tie)
        FAIL("taps %u %u %u %u %u %u %u (k2 %u, k3 %u): sum %u, expected %u\n", p[0], p[1], p[2], p[3], p[4], p[5], p[6], K2, K3, got, (unsigned) sum + 32768u);
}

int main() {
    // ---- pattern points x angle grid, random angles
    long gridAngles = 0;
    for (int i = 0; i <= 360 * 64; i++, gridAngles++) {
        float a, b;
        sincos_deg((float) i / 64.0f, &a, &b);
        for (int k = 0; k < kBriefPointCount; k++) check_sample((float) kBriefPoint[2 * k], (float) kBriefPoint[2 * k + 1], a, b);
    }
    const long gridSamples = samples;
    for (int i = 0; i < 100000; i++) {
        float a, b;
        sincos_deg((float) rnd32() * (360.0f / 4294967296.0f), &a, &b);
        for (int k = 0; k < kBriefPointCount; k++) check_sample((float) kBriefPoint[2 * k], (float) kBriefPoint[2 * k + 1], a, b);
    }
    const long randomSamples = samples - gridSamples;
    // ---- exact ties: (a, b) multiples of 1/8 (those of 1/2 among them) inside the unit disc, every integer point of the pattern's range
    const long tiesBefore = tiesUp + tiesDown;
    long tieSamples = 0, x13Ties = 0;
    for (int ia = -8; ia <= 8; ia++)
        for (int ib = -8; ib <= 8; ib++) {
            if (ia * ia + ib * ib > 64) continue;
            const float a = (float) ia / 8.0f, b = (float) ib / 8.0f;
            for (int x = -13; x <= 13; x++)
                for (int y = -13; y <= 13; y++) {
                    const long t0 = tiesUp + tiesDown;
                    check_sample((float) x, (float) y, a, b);
                    tieSamples++;
                    if ((x == 13 || x == -13) && (ia == 4 || ia == -4) && tiesUp + tiesDown > t0) x13Ties++;
                }
        }
    const long handTies = tiesUp + tiesDown - tiesBefore;
    // ---- the rounding identity
    long rounds = 0;
    while (rounds < 1000000) {
        // half of them uniform over the range, half with a uniform exponent (small magnitudes, where most ties and the zeros lie)
        float v;
        if (rnd32() & 1u) v = ((float) (int) rnd32()) * (4194304.0f / 2147483648.0f);
        else v = ldexpf((float) (int) rnd32() / 2147483648.0f, (int) (rnd32() % 46u) - 23);
        if (!(fabsf(v) < 4194304.0f)) continue;
        check_round(v);
        rounds++;
    }
    long halves = 0;
    for (int h = -128; h <= 128; h++, halves++) check_round((float) h * 0.5f);
    check_round(-0.0f);
    check_round(4194303.5f);
    check_round(-4194303.5f);
    check_round(4194302.5f);
    // ---- the tap chain, in the three cv modes' constants (LEGACY_SSE2 and LEGACY_INT share (49, 55), CV_4 has (48, 56))
    long septets = 0;
    for (int i = 0; i < 100002; i++, septets++) {
        unsigned p[7];
        for (int k = 0; k < 7; k++) p[k] = i == 0 ? 0u : i == 1 ? 65535u : rnd32() >> 16;
        check_taps<49, 55>(p);   // YGZF_CV_LEGACY_SSE2
        check_taps<49, 55>(p);   // YGZF_CV_LEGACY_INT
        check_taps<48, 56>(p);   // YGZF_CV_4
    }
    // septets made to tie: a constant window c gives 257 c (both tap sets sum to 257), a tie where 257 c = 32768 mod 65536 -> c = 32768
    {
        unsigned p[7];
        for (int k = 0; k < 7; k++) p[k] = 32768u;
        if ((ds::tap_sum<49, 55>(p[0], p[1], p[2], p[3], p[4], p[5], p[6]) & 0xFFFFu) != 0u) FAIL("the constant window 32768 must tie\n");
        check_taps<49, 55>(p);
        check_taps<48, 56>(p);
    }
    printf("{\"points\": %d, \"grid_angles\": %ld, \"grid_samples\": %ld, \"random_samples\": %ld, \"hand_samples\": %ld, \"hand_ties\": %ld, "
           "\"x13_half_ties\": %ld, \"ties_rounded_up\": %ld, \"ties_rounded_down\": %ld, \"ties_negative\": %ld, \"ties_positive\": %ld, "
           "\"r_range\": [%d, %d], \"q_range\": [%d, %d], \"rounds\": %ld, \"halves\": %ld, \"septets\": %ld, \"mismatches\": %ld}\n",
           kBriefPointCount, gridAngles, gridSamples, randomSamples, tieSamples, handTies, x13Ties, tiesUp, tiesDown, tiesNeg, tiesPos, rMin, rMax, qMin,
           qMax, rounds, halves, septets, fails);
    return fails ? 1 : 0;
}
