// hs_gmotion_kernels.hip -- part of libhsflow.so: the kernels of hs_kernels_gmotion.hip.h and their launches, a translation
// unit of its own so that its device code is a code object of its own.
#define HS_GMOTION_KERNELS
#include "hs_kernels_gmotion.hip.h"

namespace hsk {

hipError_t launch_gm_accum(const dim3 &grid, hipStream_t stream, const GmPlanes &pl, GmScratch *scr, int first)
{
    hipLaunchKernelGGL(k_gm_accum, grid, dim3(256), 0, stream, pl, scr, first);
    return hipGetLastError();
}

hipError_t launch_gm_hist(const dim3 &grid, hipStream_t stream, const GmPlanes &pl, GmScratch *scr)
{
    hipLaunchKernelGGL(k_gm_hist, grid, dim3(256), 0, stream, pl, scr);
    return hipGetLastError();
}

hipError_t launch_gm_solve(hipStream_t stream, GmScratch *scr, int n, int what, int kind, int mode, float fixed_thr, float scale2, float min_thr2,
                           GmResultWords *results)
{
    hipLaunchKernelGGL(k_gm_solve, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, scr, n, what, kind, mode, fixed_thr, scale2, min_thr2, results);
    return hipGetLastError();
}

hipError_t launch_gm_apply(const dim3 &grid, hipStream_t stream, const GmPlanes &pl, const GmScratch *scr, GmResultWords *results)
{
    hipLaunchKernelGGL(k_gm_apply, grid, dim3(256), 0, stream, pl, scr, results);
    return hipGetLastError();
}

template <int C, bool STATS>
static void gm_warp(const dim3 &grid, hipStream_t stream, const hsgm::Model &m, const uint8_t *src, const uint8_t *ref, uint8_t *dst, int wide_dst,
                    long long src_stride, long long ref_stride, long long dst_stride, int W, int H, float t, int border, unsigned fill, unsigned long long *stats)
{
    hipLaunchKernelGGL((k_gm_warp<C, STATS>), grid, dim3(256), 0, stream, m, src, ref, dst, wide_dst, src_stride, ref_stride, dst_stride, W, H, t, border, fill,
                       stats);
}

hipError_t launch_gm_warp(const dim3 &grid, hipStream_t stream, int channels, const hsgm::Model &m, const uint8_t *src, const uint8_t *ref, uint8_t *dst,
                          int wide_dst, long long src_stride, long long ref_stride, long long dst_stride, int W, int H, float t, int border, unsigned fill,
                          unsigned long long *stats)
{
    if (channels == 1) {
        if (stats) gm_warp<1, true>(grid, stream, m, src, ref, dst, wide_dst, src_stride, ref_stride, dst_stride, W, H, t, border, fill, stats);
        else gm_warp<1, false>(grid, stream, m, src, ref, dst, wide_dst, src_stride, ref_stride, dst_stride, W, H, t, border, fill, stats);
    } else {
        if (stats) gm_warp<3, true>(grid, stream, m, src, ref, dst, wide_dst, src_stride, ref_stride, dst_stride, W, H, t, border, fill, stats);
        else gm_warp<3, false>(grid, stream, m, src, ref, dst, wide_dst, src_stride, ref_stride, dst_stride, W, H, t, border, fill, stats);
    }
    return hipGetLastError();
}

} // namespace hsk
