// sia_gate.h -- the border test of SparseImgAlign's two patch loops (reference src/SparseImageAlign.cc:73-77 for the reference frame, :160-166
// for the current frame), stated once for k_sia_precompute / k_sia_run (align_kernels.hip) and for a host program (tests/cpp/sia_gate_cpu.hip).
#ifndef YGZF_SIA_GATE_H
#define YGZF_SIA_GATE_H
#include <math.h>

namespace ygzf {

constexpr int kSiaBorder = 3;   // patch_halfsize_ + 1

// The reference converts first and compares integers:
//     ui = (int) floorf(u);  if (ui - border < 0 || vi - border < 0 || ui + border >= w || vi + border >= h) continue;
// which is undefined from |u| = 2^31 on (a MapPoint at almost zero depth in the current camera gets there).  x86 converts such a value to INT_MIN
// and rejects it; the GPU's conversion saturates, INT_MAX + border wraps below w, the patch is accepted and read far outside the image.  Here
// the decision falls in float, BEFORE the conversion: floorf's result is brought into [-1, 2^24] (fmaxf drops a NaN: it becomes -1), which every
// int holds, and the reference's comparisons follow.  Nothing changes for a coordinate in [-1, 2^24): the same integer, the same answer.  One
// below -1 was outside at the left / top gate and still is (-1 - border < 0); one from 2^24 on was outside at the right / bottom gate and still
// is (a level has at most 2^24 columns and rows); NaN and the infinities, which the reference leaves undefined, are outside.  So the answer -- and ui,
// vi where it is true -- is the reference's wherever the reference defines one.  false leaves ui, vi untouched.
constexpr float kSiaGateLo = -1.f, kSiaGateHi = 16777216.f;
__host__ __device__ inline bool sia_patch_inside(float u, float v, int w, int h, int &ui, int &vi) {
    const int a = (int) fminf(fmaxf(floorf(u), kSiaGateLo), kSiaGateHi), b = (int) fminf(fmaxf(floorf(v), kSiaGateLo), kSiaGateHi);
    if (a - kSiaBorder < 0 || b - kSiaBorder < 0 || a + kSiaBorder >= w || b + kSiaBorder >= h) return false;
    ui = a;
    vi = b;
    return true;
}

}  // namespace ygzf
#endif
