// hs_interp_kernels.hip -- part of libhsflow.so: the instantiations of the kernels of hs_kernels_interp.hip.h and their
// launches, a translation unit of its own so that its device code is a code object of its own.
#include "hs_kernels_interp.hip.h"

namespace hsk {

hipError_t launch_interp_splat(int channels, const dim3 &grid, hipStream_t stream, const float *u, const float *v, int P, const InterpFrames &fr, int W, int H,
                               unsigned long long *keys, long long plane, const InterpTimes &times)
{
    if (channels == 1) hipLaunchKernelGGL((k_interp_splat<1>), grid, dim3(256), 0, stream, u, v, P, fr, W, H, keys, plane, times);
    else hipLaunchKernelGGL((k_interp_splat<3>), grid, dim3(256), 0, stream, u, v, P, fr, W, H, keys, plane, times);
    return hipGetLastError();
}

hipError_t launch_interp_resolve(const dim3 &grid, hipStream_t stream, const unsigned long long *keys, long long plane, const float *u, const float *v, int P, int W,
                                 int H, const InterpTimes &times, const InterpFlowOut &out, long long flow_stride, long long state_stride, InterpStatsWords *stats,
                                 int unfilled_too)
{
    if (stats) hipLaunchKernelGGL((k_interp_resolve<true>), grid, dim3(256), 0, stream, keys, plane, u, v, P, W, H, times, out, flow_stride, state_stride, stats, unfilled_too);
    else hipLaunchKernelGGL((k_interp_resolve<false>), grid, dim3(256), 0, stream, keys, plane, u, v, P, W, H, times, out, flow_stride, state_stride, stats, unfilled_too);
    return hipGetLastError();
}

hipError_t launch_interp_blend(int channels, const dim3 &grid, hipStream_t stream, const InterpBlendPics &pics, long long flow_stride, const InterpFrames &fr,
                               long long ref_stride, long long dst_stride, long long cls_stride, int W, int H, InterpStatsWords *stats)
{
    if (channels == 1) {
        if (stats) hipLaunchKernelGGL((k_interp_blend<1, true>), grid, dim3(256), 0, stream, pics, flow_stride, fr, ref_stride, dst_stride, cls_stride, W, H, stats);
        else hipLaunchKernelGGL((k_interp_blend<1, false>), grid, dim3(256), 0, stream, pics, flow_stride, fr, ref_stride, dst_stride, cls_stride, W, H, stats);
    } else {
        if (stats) hipLaunchKernelGGL((k_interp_blend<3, true>), grid, dim3(256), 0, stream, pics, flow_stride, fr, ref_stride, dst_stride, cls_stride, W, H, stats);
        else hipLaunchKernelGGL((k_interp_blend<3, false>), grid, dim3(256), 0, stream, pics, flow_stride, fr, ref_stride, dst_stride, cls_stride, W, H, stats);
    }
    return hipGetLastError();
}

} // namespace hsk
