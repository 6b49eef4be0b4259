// hs_chain_kernels.hip -- part of libhsflow.so: the instantiations of k_chain_dense and k_chain_points
// (hs_kernels_chain.hip.h) and their launch, a translation unit of its own so that its device code is a code object of
// its own.
#include "hs_kernels_chain.hip.h"

namespace hsk {

hipError_t launch_chain_dense(const dim3 &grid, hipStream_t stream, const ChainPlanes &pl, const ChainDense &d, ChainStatsWords *stats)
{
    if (stats) hipLaunchKernelGGL((k_chain_dense<true>), grid, dim3(256), 0, stream, pl, d, stats);
    else hipLaunchKernelGGL((k_chain_dense<false>), grid, dim3(256), 0, stream, pl, d, stats);
    return hipGetLastError();
}

hipError_t launch_chain_points(const dim3 &grid, hipStream_t stream, const ChainPlanes &pl, const ChainPoints &d, ChainStatsWords *stats)
{
    if (stats) hipLaunchKernelGGL((k_chain_points<true>), grid, dim3(256), 0, stream, pl, d, stats);
    else hipLaunchKernelGGL((k_chain_points<false>), grid, dim3(256), 0, stream, pl, d, stats);
    return hipGetLastError();
}

} // namespace hsk
