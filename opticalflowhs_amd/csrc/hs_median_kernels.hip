// hs_median_kernels.hip -- part of libhsflow.so: the instantiations of k_median_batch (hs_kernels_median.hip.h) and their
// launch, a translation unit of its own so that its device code is a code object of its own.
#include "hs_kernels_median.hip.h"

namespace hsk {

namespace {
template <int R, bool FILL>
void launch(const dim3 &grid, hipStream_t stream, const MedianBatchFields &f, long long is, long long ss, long long os, long long sos, int W, int H, int min_votes,
            MedianStatsWords *stats)
{
    if (stats) hipLaunchKernelGGL((k_median_batch<R, FILL, true>), grid, dim3(256), 0, stream, f, is, ss, os, sos, W, H, min_votes, stats);
    else hipLaunchKernelGGL((k_median_batch<R, FILL, false>), grid, dim3(256), 0, stream, f, is, ss, os, sos, W, H, min_votes, stats);
}
} // namespace

hipError_t launch_median_batch(int radius, bool fill, const dim3 &grid, hipStream_t stream, const MedianBatchFields &f, long long in_stride, long long state_stride,
                               long long out_stride, long long state_out_stride, int W, int H, int min_votes, MedianStatsWords *stats)
{
    if (radius == 1) {
        if (fill) launch<1, true>(grid, stream, f, in_stride, state_stride, out_stride, state_out_stride, W, H, min_votes, stats);
        else launch<1, false>(grid, stream, f, in_stride, state_stride, out_stride, state_out_stride, W, H, min_votes, stats);
    } else {
        if (fill) launch<2, true>(grid, stream, f, in_stride, state_stride, out_stride, state_out_stride, W, H, min_votes, stats);
        else launch<2, false>(grid, stream, f, in_stride, state_stride, out_stride, state_out_stride, W, H, min_votes, stats);
    }
    return hipGetLastError();
}

} // namespace hsk
