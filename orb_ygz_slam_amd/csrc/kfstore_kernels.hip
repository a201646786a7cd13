// kfstore_kernels.hip -- the resident keyframes' grid (product code; entry points in ygzf_api_kfstore.hip).
//   k_kf_grid_build   Frame::AssignFeaturesToGrid (reference src/Frame.cc:314-330, PosInGrid :483-493) of one keyframe, once, into its row of
//                     the store's arena: the CSR that k_proj_search's workgroups otherwise rebuild in LDS on every launch
// The resident searches themselves are k_proj_search<MODE, true> (match_kernels.hip).
#include <hip/hip_runtime.h>

#include "grid_lds.h"

namespace ygzf {

static_assert(kKfGridCells == GRID_CELLS, "the stored grid is the matcher's grid");

// One workgroup: the grid is built in LDS by the code the non-resident searches run (build_grid_lds, grid_lds.h: same lists, same order) and
// written out.  list entries behind the last cell's end belong to no cell (keys outside the 64 x 48 cells): -1.
__global__ __launch_bounds__(kMatchBlock) void k_kf_grid_build(KfGridArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    __shared__ int s_tmp[kMatchBlock / 64];
    const GridPtrs G = grid_carve(dyn);
    int *cellStart = G.cellStart, *list = G.list;
    build_grid_lds(A.keys, A.n, A.minX, A.minY, A.gridInvW, A.gridInvH, G.cellStart, G.cellFill, G.list, s_tmp);
    const int total = cellStart[GRID_CELLS];
    for (int i = threadIdx.x; i <= GRID_CELLS; i += kMatchBlock) A.cellStart[i] = cellStart[i];
    for (int i = threadIdx.x; i < A.n; i += kMatchBlock) A.list[i] = i < total ? list[i] : -1;
}

hipError_t launch_kf_grid_build(hipStream_t st, const KfGridArgs &A) {
    hipError_t e = hipFuncSetAttribute((const void *) k_kf_grid_build, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxDynLds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_kf_grid_build, dim3(1), dim3(kMatchBlock), grid_lds_bytes(A.n), st, A);
    return hipSuccess;
}

}  // namespace ygzf
