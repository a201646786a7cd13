// grid_lds.h -- Frame::AssignFeaturesToGrid as one workgroup builds it in LDS (product code, device only).  Shared by the kernels that rebuild
// a frame's grid on every launch (match_kernels.hip: k_features_in_area, k_proj_search) and the one that builds a resident keyframe's grid once
// (kfstore_kernels.hip: k_kf_grid_build), so that both forms hold the same lists in the same order.  k_match_last builds the same grid
// fused with its staging pass (one read of the keys fills the grid counts and the LDS copies of position, level and descriptor) and is
// therefore not a caller.
#ifndef YGZF_GRID_LDS_H
#define YGZF_GRID_LDS_H
#include "kernels.h"
#include "wave_ops.h"

namespace ygzf {

constexpr int kMatchBlock = 1024;

// Frame::AssignFeaturesToGrid in LDS (one workgroup of kMatchBlock threads): cellStart[GRID_CELLS + 1] holds the exclusive prefix of the cell
// counts, list[cellStart[c] ..) the keypoint indices of cell c in ascending order (the reference's push_back order); cellFill (GRID_CELLS)
// and s_tmp (kMatchBlock / 64) are scratch.  Ends with a barrier.
__device__ inline void build_grid_lds(const ygzf_kp *__restrict__ keys, int n, float minX, float minY, float gridInvW, float gridInvH, int *cellStart,
                                      int *cellFill, int *list, int *s_tmp) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < GRID_CELLS; i += kMatchBlock) cellFill[i] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kMatchBlock) {
        const ygzf_kp k = keys[i];
        const int px = (int) roundf((k.x - minX) * gridInvW);     // Frame::PosInGrid (round, as the reference)
        const int py = (int) roundf((k.y - minY) * gridInvH);
        if (!(px < 0 || px >= GRID_COLS || py < 0 || py >= GRID_ROWS)) atomicAdd(&cellFill[px * GRID_ROWS + py], 1);
    }
    __syncthreads();
    {   // exclusive scan of 3072 counts: 3 per thread
        const int per = GRID_CELLS / kMatchBlock;
        int sum = 0;
        for (int k = 0; k < per; k++) sum += cellFill[tid * per + k];
        const int incl = wave_incl_scan(sum);
        if (lane == 63) s_tmp[wave] = incl;
        __syncthreads();
        int woff = 0;
        for (int w2 = 0; w2 < wave; w2++) woff += s_tmp[w2];
        int off = woff + incl - sum;
        for (int k = 0; k < per; k++) {
            const int c = cellFill[tid * per + k];
            cellStart[tid * per + k] = off;
            off += c;
        }
        if (tid == kMatchBlock - 1) cellStart[GRID_CELLS] = off;
    }
    __syncthreads();
    for (int i = tid; i < GRID_CELLS; i += kMatchBlock) cellFill[i] = cellStart[i];
    __syncthreads();
    for (int i = tid; i < n; i += kMatchBlock) {
        const ygzf_kp k = keys[i];
        const int px = (int) roundf((k.x - minX) * gridInvW);
        const int py = (int) roundf((k.y - minY) * gridInvH);
        if (!(px < 0 || px >= GRID_COLS || py < 0 || py >= GRID_ROWS)) list[atomicAdd(&cellFill[px * GRID_ROWS + py], 1)] = i;
    }
    __syncthreads();
    for (int c = tid; c < GRID_CELLS; c += kMatchBlock) {  // cells keep ascending keypoint index (push_back order)
        const int s = cellStart[c], e = cellStart[c + 1];
        for (int a = s + 1; a < e; a++) {
            const int v = list[a];
            int b = a - 1;
            while (b >= s && list[b] > v) { list[b + 1] = list[b]; b--; }
            list[b + 1] = v;
        }
    }
    __syncthreads();
}

}  // namespace ygzf
#endif
