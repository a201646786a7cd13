// fast_lane_quads.h -- which quad of a cell a lane tests in which round of FAST pass 1 (fast_cell_process, csrc/extract_kernels.hip).  A cell of
// dw x dh tested pixels has nq = (dw + 3) >> 2 quads per row; the wave takes them 64 at a time in raster order, so in round k lane l holds quad
// i = 64 k + l: row y = i / nq, column q = i % nq, as long as i < nq * dh.  Two walks give that sequence without a division per round:
//   generic   (y, q) starts at (l / nq, l % nq) by a reciprocal multiply and advances by (64 / nq, 64 % nq) with a wrap of q;
//   fixed     where nq divides 64 (nq = 1, 2, 4, 8, 16: every cell 29 .. 32 px wide has 8), q = l & (nq - 1) for the whole cell and y advances by
//             64 / nq rows per round -- the last-quad mask, q's share of the quad record and the lane's column inside the window never change,
//             and the window address advances by a wave-uniform constant.
// Both keep the quad record's position bits yq = y << 2 | q << 10 and the value `end` it must stay below for the lane to hold a quad (y < dh), so
// the kernel's round is the same text over either walk and only the step differs.  Plain arithmetic that also compiles for the host:
// tests/cpp/fast_lane_quads_cpu.hip walks every cell size both ways against the definition above (tests/test_fast_lane_quads_cpu.py).
#ifndef YGZF_FAST_LANE_QUADS_H
#define YGZF_FAST_LANE_QUADS_H

#if defined(__HIPCC__)   // both passes of a HIP compilation see the same functions (device code calls them; the host program does too)
#define YGZF_LQ_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define YGZF_LQ_FN inline
#endif

namespace ygzf {
namespace lq {

// a / x for 0 <= a <= 64, 1 <= x <= 64 as (a * rcp16(x)) >> 16, exact in that range (rcp16_ok): the kernels' table kRcp16 holds rcp16(0 .. 64)
constexpr unsigned rcp16(int x) { return x > 0 ? 65536u / (unsigned) x + 1u : 0u; }
constexpr bool rcp16_ok() {
    for (int x = 1; x <= 64; x++)
        for (int a = 0; a <= 64; a++)
            if ((int) (((unsigned) a * rcp16(x)) >> 16) != a / x) return false;
    return true;
}
static_assert(rcp16_ok(), "the reciprocal multiply is not exact for 0 <= a <= 64, 1 <= x <= 64");
YGZF_LQ_FN int div_small(int a, unsigned m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (int) (__umul24((unsigned) a, m) >> 16);   // both < 2^24: full-rate multiply
#else
    return (int) (((unsigned) a * m) >> 16);
#endif
}

// pixels of quad q that belong to the cell, as a mask over fast9_quad's polarity bytes: all four, or dw - 4 (nq - 1) of them in the row's last quad
constexpr unsigned kAllFour = 0x03030303u;
YGZF_LQ_FN unsigned last_quad_mask(int dw, int nq) { return kAllFour >> (8 * (4 * nq - dw)); }

// nq divides 64 <=> nq is a power of two (1 <= nq <= 64)
YGZF_LQ_FN bool fixed_column(int nq) { return (nq & (nq - 1)) == 0; }
constexpr bool fixed_column_ok() {
    for (int nq = 1; nq <= 64; nq++)
        if (((nq & (nq - 1)) == 0) != (64 % nq == 0)) return false;
    return true;
}
static_assert(fixed_column_ok(), "fixed_column(nq) must mean that nq divides 64");

struct Walk {
    int y, q;        // the lane's quad (the generic walk steps these; the fixed walk leaves them at their first values)
    unsigned yq;     // y << 2 | q << 10: the quad record without its polarity bytes
    unsigned end;    // the lane holds a quad while yq < end  (dh << 2 | q << 10, i.e. y < dh)
    unsigned mask;   // kAllFour, or the last-quad mask where q == nq - 1
};
YGZF_LQ_FN bool active(const Walk &w) { return w.yq < w.end; }
YGZF_LQ_FN void place(Walk &w, int nq, int dh, unsigned lastMask) {   // yq, end and mask from (y, q)
    const unsigned q10 = (unsigned) w.q << 10;
    w.yq = ((unsigned) w.y << 2) | q10;
    w.end = ((unsigned) dh << 2) | q10;
    w.mask = w.q == nq - 1 ? lastMask : kAllFour;
}

// ---- generic: any nq <= 64.  m = rcp16(nq); (sy, sq) = (64 / nq, 64 % nq), the step of a round
YGZF_LQ_FN Walk start_generic(int lane, int nq, unsigned m, int dh, unsigned lastMask) {
    Walk w;
    w.y = div_small(lane, m);
    w.q = lane - w.y * nq;
    place(w, nq, dh, lastMask);
    return w;
}
YGZF_LQ_FN void step_generic(Walk &w, int nq, int sy, int sq, int dh, unsigned lastMask) {
    w.y += sy;
    w.q += sq;
    if (w.q >= nq) { w.q -= nq; w.y++; }
    place(w, nq, dh, lastMask);
}

// ---- fixed column: nq a power of two.  rows_per_round = 64 / nq
YGZF_LQ_FN int log2_quads(int nq) { return __builtin_ctz((unsigned) nq); }
YGZF_LQ_FN Walk start_fixed(int lane, int nq, int dh, unsigned lastMask) {
    Walk w;
    w.y = lane >> log2_quads(nq);
    w.q = lane & (nq - 1);
    place(w, nq, dh, lastMask);
    return w;
}
YGZF_LQ_FN void step_fixed(Walk &w, int rowsPerRound) { w.yq += (unsigned) rowsPerRound << 2; }   // y += rowsPerRound; q, end and mask stay

}  // namespace lq
}  // namespace ygzf
#endif
