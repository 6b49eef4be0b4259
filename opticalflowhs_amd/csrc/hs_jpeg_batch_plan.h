// hs_jpeg_batch_plan.h -- where the scratch of a batch of JPEG encodes lies in the context's one device allocation, and
// how a batch is cut into chunks (hsflow_jpeg_encode_batch_device, hs_jpeg.hip.h).  Plain C++, no HIP:
// tests/jpeg_batch_plan_main.cpp compiles it alone.
//
// A chunk is at most `max_batch` consecutive pictures of one size, encoded by one set of launches.  The allocation holds
// `pictures` slices (the largest chunk so far), range by range:
//   [ coefficients ][ raw streams ][ bit offsets ][ stuffing offsets ][ bit lengths ][ 0xFF counts ][ size words ]
// Picture i's part of a range starts `stride` bytes behind picture i - 1's, a multiple of 256, so the kernels find it as
// base + i * stride and the raw streams of a chunk are one contiguous range: one memset.  The size words are the
// exception: 8 bytes each, behind each other, so the host reads a chunk's in one copy.  Chunks follow each other on one
// stream, so every chunk uses the slices from 0 again.  A slice's ranges are sized by the formulas of the single
// encode (jpeg_prepare): with one picture the layout is that path's own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace hsjpeg_plan {

constexpr size_t kChunkBytes = 128;    // hsk::kJpegChunk
constexpr size_t kMaxBlockBytes = 208; // hsjpeg::kMaxBlockBytes

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

// One picture's sizes, from W and H alone.
struct Slice {
    long long nb = 0;      // blocks: 6 per MCU of 16 x 16 pixels
    long long nchunks = 0; // 128-byte chunks of the raw stream
    size_t raw_bytes = 0;  // nb * 208 rounded up to whole chunks
    // bytes from one picture's part of a range to the next one's
    size_t s_coef = 0, s_raw = 0, s_off = 0, s_ffoff = 0, s_len = 0, s_ff = 0;
};

// The allocation for `pictures` slices: where each range starts.
struct Layout {
    Slice s;
    int pictures = 0;
    size_t o_coef = 0, o_raw = 0, o_off = 0, o_ffoff = 0, o_len = 0, o_ff = 0, o_size = 0;
    size_t total = 0;
};

struct Chunk {
    int first, count;
};

inline Slice slice(int W, int H)
{
    Slice s;
    const long long mw = ((long long)W + 15) / 16, mh = ((long long)H + 15) / 16;
    s.nb = 6 * mw * mh;
    s.raw_bytes = ((size_t)s.nb * kMaxBlockBytes + kChunkBytes - 1) / kChunkBytes * kChunkBytes;
    s.nchunks = (long long)(s.raw_bytes / kChunkBytes);
    s.s_coef = up256((size_t)s.nb * 128);
    s.s_raw = up256(s.raw_bytes);
    s.s_off = up256(((size_t)s.nb + 1) * 8);
    s.s_ffoff = up256(((size_t)s.nchunks + 1) * 8);
    s.s_len = up256((size_t)s.nb * 4);
    s.s_ff = up256((size_t)s.nchunks * 4);
    return s;
}

inline Layout layout(int W, int H, int pictures)
{
    Layout l;
    l.s = slice(W, H);
    l.pictures = pictures;
    const size_t n = (size_t)pictures;
    l.o_coef = 0;
    l.o_raw = l.o_coef + n * l.s.s_coef;
    l.o_off = l.o_raw + n * l.s.s_raw;
    l.o_ffoff = l.o_off + n * l.s.s_off;
    l.o_len = l.o_ffoff + n * l.s.s_ffoff;
    l.o_ff = l.o_len + n * l.s.s_len;
    l.o_size = l.o_ff + n * l.s.s_ff;
    l.total = l.o_size + up256(n * 8);
    return l;
}

// n pictures in chunks of at most max_batch, in order.
inline std::vector<Chunk> chunks(int n, int max_batch)
{
    std::vector<Chunk> out;
    for (int first = 0; first < n; first += max_batch) out.push_back(Chunk{first, n - first < max_batch ? n - first : max_batch});
    return out;
}

} // namespace hsjpeg_plan
