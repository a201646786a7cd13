// kfdb_kernels.hip -- the keyframe database on the device (product code; entry points in ygzf_api_kfdb.hip).
//   k_kfdb_query   KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates (reference src/KeyFrameDatabase.cc:67-284): what the
//                  walk over the inverted file counts (mnLoopWords / mnRelocWords) and what mpVoc->score returns (DBoW2 L1Scoring::score,
//                  Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), for every stored BowVector against every query of the call
//   k_kfdb_repack  the live rows into a larger arena, packed
// The store is streamed whole for every query (a device inverted file is not kept): rows of (word id, value) ascending by id, as BowVector
// iterates.
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace ygzf {

// One wave per (slot, query); the four waves of a workgroup share the query's word ids in LDS and take slots blockIdx.x * 4 + wave, striding by
// the grid.  The lanes read 64 consecutive entries of the stored row (coalesced) and each looks its word id up in the query by binary search.
// score: the reference adds the terms of the common words in ascending word order to a double that starts at 0.0 -- the lanes of a pass hold
// ascending ids and the passes ascend, so the hit terms are added lane by lane from a ballot (wave-uniform, every lane carries the same sum).  A
// tree reduction would add in another order and round differently.  The terms hold no multiplication (nothing for the compiler to contract).
__global__ __launch_bounds__(256) void k_kfdb_query(KfdbQueryArgs A) {
    extern __shared__ unsigned sQ[];
    const int q = blockIdx.y;
    const int q0 = A.qOff[q], nq = A.qOff[q + 1] - q0;
    for (int i = threadIdx.x; i < nq; i += 256) sQ[i] = A.qIds[q0 + i];
    __syncthreads();
    const double *qv = A.qVals + q0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = blockIdx.x * 4 + wave; s < A.nSlots; s += gridDim.x * 4) {
        const KfdbSlot S = A.slots[s];
        int common = 0, first = -1;
        double sum = 0.0;
        const int len = S.live ? S.len : 0;
        for (int base = 0; base < len; base += 64) {
            const int i = base + lane;
            const bool in = i < len;
            const unsigned id = in ? A.ids[S.off + i] : 0u;
            int lo = 0, n = in ? nq : 0;
            while (n > 0) {   // lower_bound of id in the query's ids
                const int half = n >> 1;
                if (sQ[lo + half] < id) { lo += half + 1; n -= half + 1; }
                else n = half;
            }
            const bool hit = in && lo < nq && sQ[lo] == id;
            double term = 0.0;
            if (hit) {
                const double vi = qv[lo], wi = A.vals[S.off + i];          // score(query, stored): v1 is the query (KeyFrameDatabase.cc:119, :228)
                term = fabs(vi - wi) - fabs(vi) - fabs(wi);                 // ScoringObject.cpp:41
            }
            unsigned long long m = __ballot(hit);
            if (m == 0) continue;
            common += __popcll(m);
            if (first < 0) first = __builtin_amdgcn_readlane((int) id, __ffsll((long long) m) - 1);
            const int tlo = __double2loint(term), thi = __double2hiint(term);
            while (m) {
                const int b = __ffsll((long long) m) - 1;
                m &= m - 1;
                sum += __hiloint2double(__builtin_amdgcn_readlane(thi, b), __builtin_amdgcn_readlane(tlo, b));
            }
        }
        if (lane == 0) {
            const size_t o = (size_t) q * A.nSlots + s;
            A.common[o] = common;
            A.first[o] = first;
            A.score[o] = S.live ? -sum / 2.0 : 0.0;                         // ScoringObject.cpp:65; a free slot reports 0 / -1 / 0.0
        }
    }
}

void launch_kfdb_query(hipStream_t st, const KfdbQueryArgs &A, int nQueries, int maxQueryWords, int cuCount) {
    if (A.nSlots <= 0 || nQueries <= 0) return;
    int bx = (A.nSlots + 3) / 4;
    if (bx > 4 * cuCount) bx = 4 * cuCount;
    hipLaunchKernelGGL(k_kfdb_query, dim3(bx, nQueries), dim3(256), sizeof(unsigned) * (size_t) (maxQueryWords > 0 ? maxQueryWords : 1), st, A);
}

// One workgroup per slot: the row moves from its place in the old arena to newOff[slot] in the new one (free slots: nothing).
__global__ __launch_bounds__(256) void k_kfdb_repack(const KfdbSlot *slots, const long long *newOff, const unsigned *ids, const double *vals,
                                                     unsigned *idsNew, double *valsNew) {
    const KfdbSlot S = slots[blockIdx.x];
    if (!S.live) return;
    const long long d = newOff[blockIdx.x];
    for (int i = threadIdx.x; i < S.len; i += 256) {
        idsNew[d + i] = ids[S.off + i];
        valsNew[d + i] = vals[S.off + i];
    }
}

void launch_kfdb_repack(hipStream_t st, int nSlots, const KfdbSlot *slots, const long long *newOff, const unsigned *ids, const double *vals,
                        unsigned *idsNew, double *valsNew) {
    if (nSlots > 0) hipLaunchKernelGGL(k_kfdb_repack, dim3(nSlots), dim3(256), 0, st, slots, newOff, ids, vals, idsNew, valsNew);
}

}  // namespace ygzf
