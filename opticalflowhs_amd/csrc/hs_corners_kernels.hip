// hs_corners_kernels.hip -- part of libhsflow.so: the kernels of hs_kernels_corners.hip.h and their launches, a translation
// unit of its own so that its device code is a code object of its own.
#define HS_CORNERS_KERNELS
#include "hs_kernels_corners.hip.h"

namespace hsk {

// The launches of one chunk of `fields` fields (at most kCnBatchMax), always the same ones in the same order: what they do
// depends on the planes, how many there are on the size and the arguments alone.
hipError_t launch_corners(hipStream_t stream, const CnPlanes &pl, int fields)
{
    const int W = pl.W, H = pl.H;
    const unsigned n = (unsigned)fields;
    const unsigned segs_x = (unsigned)((W + kCnSegW - 1) / kCnSegW);
    const hipError_t e = hipMemsetAsync(pl.acc, 0, sizeof(CnAcc) * (size_t)fields, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_cn_score, dim3((unsigned)((W + kCnTileW - 1) / kCnTileW), (unsigned)((H + kCnTileH - 1) / kCnTileH), n), dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_cn_suppress, dim3(segs_x, (unsigned)((H + kCnSupH - 1) / kCnSupH), n), dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_cn_scan, dim3(1u, 1u, n), dim3(1024), 0, stream, pl);
    hipLaunchKernelGGL(k_cn_compact, dim3(segs_x, (unsigned)H, n), dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_cn_rank, dim3((pl.rule.max_candidates + kCnRankLanes - 1u) / kCnRankLanes, 1u, n), dim3(kCnRankLanes), 0, stream, pl);
    const unsigned cap = pl.capacity ? pl.capacity : 1u;
    hipLaunchKernelGGL(k_cn_finish, dim3((cap + 255u) / 256u, 1u, n), dim3(256), 0, stream, pl);
    return hipGetLastError();
}

} // namespace hsk
