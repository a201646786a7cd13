// fast9_quad.h -- the arithmetic of fast9_quad (csrc/extract_kernels.hip), the byte-sliced FAST 9/16 test of four pixels per lane: the saturated
// thresholds from the centre dword, and the polarity bytes from the 16 ring dwords.  Written over four primitives -- lerp_u8, bitop3, the two
// clamped packed 16-bit operations, perm -- which are the gfx950 builtins under device compilation and plain C++ restatements of what those
// instructions compute under host compilation, so that tests/cpp/fast9_quad_cpu.hip runs the same network on the CPU over every ring mask, every
// (centre, ring, threshold) and random quads (tests/test_fast9_quad_cpu.py).  The ring assembly (LDS reads, v_alignbyte_b32) stays in the kernel.
#ifndef YGZF_FAST9_QUAD_H
#define YGZF_FAST9_QUAD_H

#if defined(__HIP_DEVICE_COMPILE__)
#define YGZF_F9_FN __device__ __forceinline__
#else
#define YGZF_F9_FN inline
#endif

namespace ygzf {
namespace f9 {

// ---- the primitives -------------------------------------------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
typedef unsigned short v2u16 __attribute__((ext_vector_type(2)));
// v_lerp_u8: per byte (a + b + (c & 1)) >> 1
YGZF_F9_FN unsigned lerp_u8(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_lerp(a, b, c); }
// v_bitop3_b32: per bit, bit (a << 2 | b << 1 | c) of the truth table
template <unsigned kTable>
YGZF_F9_FN unsigned bitop3(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_bitop3_b32(a, b, c, kTable); }
// v_pk_sub_u16 / v_pk_add_u16 with clamp: per 16-bit half, saturating at 0 / at 0xFFFF
YGZF_F9_FN unsigned pk_sub_u16_sat(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_sub_sat(__builtin_bit_cast(v2u16, a), __builtin_bit_cast(v2u16, b)));
}
YGZF_F9_FN unsigned pk_add_u16_sat(unsigned a, unsigned b) {
    return __builtin_bit_cast(unsigned, __builtin_elementwise_add_sat(__builtin_bit_cast(v2u16, a), __builtin_bit_cast(v2u16, b)));
}
// v_perm_b32: result byte i = byte sel[i] of the eight bytes {hi, lo} (0..3 from lo, 4..7 from hi)
YGZF_F9_FN unsigned perm(unsigned hi, unsigned lo, unsigned sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#else
YGZF_F9_FN unsigned lerp_u8(unsigned a, unsigned b, unsigned c) {
    unsigned r = 0;
    for (int i = 0; i < 4; i++) r |= ((((a >> (8 * i)) & 0xFFu) + ((b >> (8 * i)) & 0xFFu) + ((c >> (8 * i)) & 1u)) >> 1) << (8 * i);
    return r;
}
template <unsigned kTable>
YGZF_F9_FN unsigned bitop3(unsigned a, unsigned b, unsigned c) {
    unsigned r = 0;
    for (int i = 0; i < 32; i++) r |= ((kTable >> ((((a >> i) & 1u) << 2) | (((b >> i) & 1u) << 1) | ((c >> i) & 1u))) & 1u) << i;
    return r;
}
YGZF_F9_FN unsigned pk_sub_u16_sat(unsigned a, unsigned b) {
    const unsigned al = a & 0xFFFFu, bl = b & 0xFFFFu, ah = a >> 16, bh = b >> 16;
    return (al > bl ? al - bl : 0u) | ((ah > bh ? ah - bh : 0u) << 16);
}
YGZF_F9_FN unsigned pk_add_u16_sat(unsigned a, unsigned b) {
    const unsigned l = (a & 0xFFFFu) + (b & 0xFFFFu), h = (a >> 16) + (b >> 16);
    return (l > 0xFFFFu ? 0xFFFFu : l) | ((h > 0xFFFFu ? 0xFFFFu : h) << 16);
}
YGZF_F9_FN unsigned perm(unsigned hi, unsigned lo, unsigned sel) {   // selectors 0..7 only: the ones used here
    const unsigned long long v = ((unsigned long long) hi << 32) | lo;
    unsigned r = 0;
    for (int i = 0; i < 4; i++) r |= (unsigned) ((v >> (8 * ((sel >> (8 * i)) & 7u))) & 0xFFu) << (8 * i);
    return r;
}
#endif

// ---- thresholds -----------------------------------------------------------------------------------------------------------------------------
// Per byte of the centre dword c, saturated, on the complemented centre nc = 255 - c:
//     nhi = 255 - min(c + t, 255) = max(nc - t, 0)        nlo = 255 - max(c - t, 0) = min(nc + t, 255)
// Every byte is worked on in the HIGH byte of a 16-bit half: the odd bytes of nc are there already, the even ones after a shift by 8, and t
// sits in the high byte of both halves.  The clamped subtract saturates the half at 0 -- the low byte, whatever it holds, cannot borrow out of
// a high byte that stays >= 0 --, the clamped add saturates it at 0xFFFF exactly when the high bytes' sum passes 255 (the low byte of t's half
// is 0: no carry comes up).  One v_perm_b32 per bound picks the four high bytes.  One shift, four packed operations, two permutes; 0 <= t <= 255.
struct Thresholds { unsigned nhi, nlo; };
YGZF_F9_FN Thresholds thresholds(unsigned centre, int t) {
    const unsigned nc = ~centre;
    const unsigned ev = nc << 8, od = nc;
    const unsigned tH = ((unsigned) t << 8) * 0x10001u;
    Thresholds r;
    r.nhi = perm(pk_sub_u16_sat(od, tH), pk_sub_u16_sat(ev, tH), 0x07030501u);
    r.nlo = perm(pk_add_u16_sat(od, tH), pk_add_u16_sat(ev, tH), 0x07030501u);
    return r;
}

// ---- comparison and arc network -----------------------------------------------------------------------------------------------------------
// R[k] = ring pixel k of the four centres, one byte each.  Bit 7 of a v_lerp_u8 byte is the carry of the 9-bit sum:
//     B[k] = bit 7 of lerp(R[k], nhi, 0)   <=>  R[k] >  c + t          N[k] = bit 7 of lerp(R[k], nlo, 1)   <=>  R[k] >= c - t  (not dark)
// "9 contiguous of the circular 16": with A9[k] = B[k] & ... & B[k+8],
//     A9[k] | A9[k+1]  =  (B[k+1] & ... & B[k+8]) & (B[k] | B[k+9])
// so only the eight even k are needed, and the runs of eight are four pairs that start at odd positions (indices mod 16 on B, mod 8 on P):
//     P[i] = B[2i+1] & B[2i+2]                    8 two-input ANDs
//     Z[i] = P[i] & (B[2i] | B[2i+9])             8   a & (b | c)
//     T[i] = Z[i] & P[i+1] & P[i+2]               8   a & b & c
//     bright |= T[i] & P[i+3]                     8   a | (b & c)
// The dark side is the De Morgan mirror on N (a dark arc is nine zeros): Q = N | N, W = Q | (N & N), U = W | Q | Q, ndark &= U | Q.
// 32 operations per polarity, every one at the full issue rate (v_and_b32 / v_or_b32 / v_bitop3_b32: profiles/micro/r02_valu_issue_rates.txt).
// The bright chain is written to its end before the dark one starts: B and its pairs are dead by then.  The low 7 bits of every byte are
// don't-care throughout.  Returns per byte 1 = bright corner, 2 = dark corner, 0 = none.
YGZF_F9_FN unsigned arcs_bright(const unsigned *B) {
    unsigned P[8], T[8];
#pragma unroll
    for (int i = 0; i < 8; i++) P[i] = B[2 * i + 1] & B[(2 * i + 2) & 15];
#pragma unroll
    for (int i = 0; i < 8; i++) T[i] = bitop3<0xE0>(P[i], B[2 * i], B[(2 * i + 9) & 15]);
#pragma unroll
    for (int i = 0; i < 8; i++) T[i] = bitop3<0x80>(T[i], P[(i + 1) & 7], P[(i + 2) & 7]);
    unsigned bright = T[0] & P[3];
#pragma unroll
    for (int i = 1; i < 8; i++) bright = bitop3<0xF8>(bright, T[i], P[(i + 3) & 7]);
    return bright;
}
YGZF_F9_FN unsigned arcs_not_dark(const unsigned *N) {
    unsigned Q[8], U[8];
#pragma unroll
    for (int i = 0; i < 8; i++) Q[i] = N[2 * i + 1] | N[(2 * i + 2) & 15];
#pragma unroll
    for (int i = 0; i < 8; i++) U[i] = bitop3<0xF8>(Q[i], N[2 * i], N[(2 * i + 9) & 15]);
#pragma unroll
    for (int i = 0; i < 8; i++) U[i] = bitop3<0xFE>(U[i], Q[(i + 1) & 7], Q[(i + 2) & 7]);
    unsigned ndark = U[0] | Q[3];
#pragma unroll
    for (int i = 1; i < 8; i++) ndark = bitop3<0xE0>(ndark, U[i], Q[(i + 3) & 7]);
    return ndark;
}
YGZF_F9_FN unsigned polarity(const unsigned *R, Thresholds th) {
    unsigned B[16], N[16];
#pragma unroll
    for (int k = 0; k < 16; k++) B[k] = lerp_u8(R[k], th.nhi, 0u);
    const unsigned bright = arcs_bright(B);
#pragma unroll
    for (int k = 0; k < 16; k++) N[k] = lerp_u8(R[k], th.nlo, 0x01010101u);
    const unsigned ndark = arcs_not_dark(N);
    // bit 0 of a byte <- bit 7 of bright, bit 1 <- bit 7 of ~ndark.  (B[k] implies N[k], and two arcs of nine do not fit on a ring of sixteen:
    // a bright corner is never dark, so ~ndark needs no "& ~bright".)  One v_bitop3_b32 takes bit 0 from the one and the rest from the other.
    return bitop3<0xB1>(bright >> 7, ndark >> 6, 0x01010101u) & 0x03030303u;   // c ? a : ~b
}

}  // namespace f9
}  // namespace ygzf
#endif
