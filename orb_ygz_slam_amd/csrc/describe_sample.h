// describe_sample.h -- the arithmetic of one sample of describe_window's column pass (csrc/extract_kernels.hip): where pattern point (x, y),
// rotated by (a, b) = (cos, sin) of the keypoint's angle, lands in the row-blurred window hb, and the 7-tap column sum taken there.  Stated so
// that the per-sample work stays on the full-rate float adder and the multiply-add unit:
//   * the rotated coordinates r_f = x * b + y * a and q_f = x * a - y * b are two products and one add or subtract each, as the oracle takes them
//     (no contraction);
//   * round(v) = (v + M) - M with M = 1.5 * 2^23 is rintf(v), ties to even, for every |v| < 2^22: v + M lies in [2^23, 2^24), where floats are the
//     integers, so the addition rounds v to an integer by the rounding mode's own rule (M is even: a tie goes to the even integer) and the
//     subtraction is exact;
//   * the byte address of hb[(18 + R) * kHbP + 18 + Q] is 80 R + 2 Q + 1476.  With 2^23 added to the constant every intermediate of the two
//     multiply-adds 80 * R + (2 * Q + C) is an integer of [2^23, 2^23 + 2^12) -- |R|, |Q| <= 18 --, hence exact, and the integer is the float's
//     bit pattern less that of 2^23: one integer subtraction, which the kernel merges with adding the wave's LDS base;
//   * the tap sum 18 (p0 + p6) + 34 (p1 + p5) + k2 (p2 + p4) + k3 p3 + 2^15 is a chain of four 24-bit multiply-adds: every operand is below
//     2^24 and the total below 2^32, so it is the same integer as any other order gives.
// Plain arithmetic that compiles for the host too: tests/cpp/describe_sample_cpu.hip runs this text against rintf and integer arithmetic over every
// pattern point and angle step (tests/test_describe_sample_cpu.py).
#ifndef YGZF_DESCRIBE_SAMPLE_H
#define YGZF_DESCRIBE_SAMPLE_H

#include "describe_lds.h"

#if defined(__HIPCC__)   // both passes of a HIP compilation see the same functions (device code calls them; the host program does too)
#define YGZF_DS_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define YGZF_DS_FN inline
#endif

namespace ygzf {
namespace ds {

constexpr float kRoundMagic = 12582912.0f;     // 1.5 * 2^23: even, ulp 1, and v + kRoundMagic stays inside [2^23, 2^24) for |v| < 2^22
constexpr int kHbCentre = 18;                  // hb row / column of the keypoint: pattern offsets reach 18 rows and columns either way
constexpr int kHbRowBytes = 2 * kHbP;          // 80
constexpr int kHbCentreByte = kHbCentre * kHbRowBytes + 2 * kHbCentre;   // 1476: byte offset of hb[18 * kHbP + 18]
constexpr unsigned kTwo23Bits = 0x4B000000u;   // bit pattern of 2^23f
constexpr float kAddrMagic = 8388608.0f + (float) kHbCentreByte;
static_assert(kHbCentreByte - kHbCentre * kHbRowBytes - 2 * kHbCentre >= 0 && kHbCentreByte + kHbCentre * kHbRowBytes + 2 * kHbCentre < 4096,
              "the byte offsets of all samples are integers of [0, 2^12)");

// rintf(v) for |v| < 2^22
YGZF_DS_FN float round_even(float v) { return (v + kRoundMagic) - kRoundMagic; }

// pattern point (x, y) under rotation (a, b): the rounded hb row and column offsets from the centre, as floats (integers of [-18, 18])
YGZF_DS_FN void rotated(float x, float y, float a, float b, float *R, float *Q) {
    *R = round_even(x * b + y * a);
    *Q = round_even(x * a - y * b);
}

// 2^23 + byte offset of hb[(18 + R) * kHbP + 18 + Q] inside hb, as a float: exact
YGZF_DS_FN float hb_byte_f(float R, float Q) { return __builtin_fmaf((float) kHbRowBytes, R, __builtin_fmaf(2.0f, Q, kAddrMagic)); }

YGZF_DS_FN unsigned float_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    unsigned u;
    __builtin_memcpy(&u, &f, 4);
    return u;
#endif
}
// the byte offset itself: base + hb_byte(...) is one subtraction where base - kTwo23Bits is formed once
YGZF_DS_FN unsigned hb_byte(float R, float Q) { return float_bits(hb_byte_f(R, Q)) - kTwo23Bits; }

// K * x + c for x < 2^24 and an inline constant K.  Written as the instruction on the device: from __umul24(K, x) + c the compiler takes the chain
// apart again, into four multiplications and two three-input additions.
template <unsigned K>
YGZF_DS_FN unsigned mad24(unsigned x, unsigned c) {
    static_assert(K <= 64, "K is an inline constant of the instruction");
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(x), "I"(K), "v"(c));
    return d;
#else
    return K * x + c;
#endif
}
template <unsigned K>
YGZF_DS_FN unsigned mad24_first(unsigned x) {   // K * x + 2^15, the rounding half coming from a scalar register
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned d;
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(d) : "v"(x), "I"(K), "s"(32768u));
    return d;
#else
    return K * x + 32768u;
#endif
}
// 7 taps {18, 34, K2, K3, K2, 34, 18} over p0 .. p6 (each < 2^16) + 2^15: the blurred value is the sum >> 16, a tie a sum whose low 16 bits are 0
template <unsigned K2, unsigned K3>
YGZF_DS_FN unsigned tap_sum(unsigned p0, unsigned p1, unsigned p2, unsigned p3, unsigned p4, unsigned p5, unsigned p6) {
    return mad24<18>(p0 + p6, mad24<34>(p1 + p5, mad24<K2>(p2 + p4, mad24_first<K3>(p3))));
}

}  // namespace ds
}  // namespace ygzf
#endif
