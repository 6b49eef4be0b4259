// hs_regions_kernels.hip -- part of libhsflow.so: the kernels of hs_kernels_regions.hip.h and their launches, a translation
// unit of its own so that its device code is a code object of its own.
#define HS_REGIONS_KERNELS
#include "hs_kernels_regions.hip.h"

namespace hsk {

// The launches of one chunk of `fields` fields (at most kRgBatchMax), always the same ones in the same order: what they do
// depends on the planes, how many there are on the size and the arguments alone.
hipError_t launch_regions(hipStream_t stream, const RgPlanes &pl, int fields)
{
    const int W = pl.W, H = pl.H;
    const unsigned n = (unsigned)fields;
    const dim3 tiles((unsigned)((W + kRgTileW - 1) / kRgTileW), (unsigned)((H + kRgTileH - 1) / kRgTileH), n);
    const dim3 rows((unsigned)((W + 255) / 256), (unsigned)H, n);
    hipLaunchKernelGGL(k_rg_tile, tiles, dim3(256), 0, stream, pl);
    const int ndir = pl.conn == 8 ? 3 : 1;
    const long long edges = ((long long)((W - 1) / kRgTileW) * H + (long long)((H - 1) / kRgTileH) * W) * ndir;
    if (edges > 0) hipLaunchKernelGGL(k_rg_seam, dim3((unsigned)((edges + 255) / 256), 1u, n), dim3(256), 0, stream, pl, edges, ndir);
    hipLaunchKernelGGL(k_rg_flatten, rows, dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_rg_count, rows, dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_rg_scan, dim3(1u, 1u, n), dim3(1024), 0, stream, pl);
    hipLaunchKernelGGL(k_rg_number, rows, dim3(256), 0, stream, pl);
    hipLaunchKernelGGL(k_rg_relabel, rows, dim3(256), 0, stream, pl);
    const unsigned cap = pl.capacity ? pl.capacity : 1u;
    hipLaunchKernelGGL(k_rg_finish, dim3((cap + 255u) / 256u, 1u, n), dim3(256), 0, stream, pl);
    return hipGetLastError();
}

} // namespace hsk
