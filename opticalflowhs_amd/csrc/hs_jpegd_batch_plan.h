// hs_jpegd_batch_plan.h -- where everything of a batch of JPEG files lies in the context's one device allocation and
// one staging area, how large the grids are, and how the batch is cut into chunks (enqueue_jpegd_batch, hs_jpegd.hip.h:
// every decode, single or batched).  Plain C++, no HIP: tests/jpegd_batch_plan_main.cpp compiles it alone.
//
// A chunk is at most `max_batch` consecutive files, decoded by one set of launches.  Its allocation, from offset 0:
//   [ input: per file the tables and the stuffed segment, then the chunk's records ]   one copy from staging
//   [ the files' clean streams ]                                                         one memset
//   [ the files' coefficient buffers ]                                                   one memset
//   [ per file: chunk counts and offsets, subsequence states, planes, DC sums, restart positions ]
// Every range starts at a multiple of 256 bytes.  Chunks follow each other on one stream, so every chunk starts at 0
// again.  A single decode is the layout of one file with a maximum of 1: the batch maximum does not reach it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace hsjpegd_plan {

constexpr uint32_t kChunkBytes = 128; // hsjpegd::kChunk
constexpr uint32_t kGroup = 256;      // hsk::kJpegdGroup

struct Params {
    size_t table_bytes;  // sizeof(hsjpegd::Tables)
    size_t record_bytes; // sizeof(hsk::JpegdBatchRec)
    uint32_t S;          // bits per subsequence, a multiple of 32 in 32 .. 4096
    int max_batch;       // HSFLOW_JPEGD_BATCH_MAX
};

struct FileIn {
    uint64_t scan_bytes;       // below 2^28 (hsjpegd::kMaxScanBytes)
    int64_t nblocks;
    int64_t nmcu;              // mcux * mcuy
    int32_t restart_interval;  // MCUs per interval, 0: none
};

struct FileOut {
    uint32_t n, nchunks, nsubCap, nint;
    // offsets into the chunk's device allocation; o_tab and o_scan are the offsets into its staging area too
    size_t o_tab, o_scan, o_clean, o_coef, o_cr, o_cs, o_ro, o_so, o_start, o_exit, o_cnt, o_base, o_planes, o_diff, o_dcsum, o_rst;
    size_t scan_span, clean_span, coef_span; // bytes of the segment's range (zero-filled behind n), the clean stream, the coefficients
};

struct Chunk {
    int first, count;
    size_t o_recs, in_bytes;        // the records; all that is copied: [0, in_bytes)
    size_t o_clean, clean_bytes;    // the clean streams behind each other
    size_t o_coef, coef_bytes;      // the coefficient buffers behind each other
    size_t total;                   // bytes of the device allocation this chunk needs
    // grid extents: the largest of the chunk's files (0: no file takes that route)
    uint32_t g_clean, g_sub, g_rst, g_gather, g_blocks;
};

struct Plan {
    std::vector<FileOut> files;
    std::vector<Chunk> chunks;
    size_t device_bytes = 0, staging_bytes = 0; // the largest chunk's
};

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

inline uint32_t subseq_cap(uint32_t n, uint32_t S)
{
    return (uint32_t)((((uint64_t)n * 8u + S - 1u) / S + kGroup - 1u) / kGroup * kGroup) + (n ? 0u : kGroup);
}

inline Plan layout(const FileIn *in, int nfiles, const Params &p)
{
    Plan pl;
    pl.files.resize(nfiles > 0 ? (size_t)nfiles : 0);
    const size_t tab = up256(p.table_bytes);
    for (int first = 0; first < nfiles; first += p.max_batch) {
        Chunk c{};
        c.first = first;
        c.count = nfiles - first < p.max_batch ? nfiles - first : p.max_batch;
        size_t o = 0;
        for (int k = 0; k < c.count; k++) { // tables and segments
            const FileIn &fi = in[first + k];
            FileOut &f = pl.files[(size_t)(first + k)];
            f.n = (uint32_t)fi.scan_bytes;
            f.nchunks = (f.n + kChunkBytes - 1) / kChunkBytes;
            f.nsubCap = subseq_cap(f.n, p.S);
            f.nint = fi.restart_interval ? (uint32_t)((fi.nmcu + fi.restart_interval - 1) / fi.restart_interval) : 0u;
            f.o_tab = o; o += tab;
            f.o_scan = o; f.scan_span = up256((size_t)f.n + 4); o += f.scan_span;
        }
        c.o_recs = o; o += up256((size_t)c.count * p.record_bytes);
        c.in_bytes = o;
        c.o_clean = o;
        for (int k = 0; k < c.count; k++) {
            FileOut &f = pl.files[(size_t)(first + k)];
            f.o_clean = o; f.clean_span = up256((size_t)f.n + 16); o += f.clean_span;
        }
        c.clean_bytes = o - c.o_clean;
        c.o_coef = o;
        for (int k = 0; k < c.count; k++) {
            FileOut &f = pl.files[(size_t)(first + k)];
            f.o_coef = o; f.coef_span = up256((size_t)in[first + k].nblocks * 128); o += f.coef_span;
        }
        c.coef_bytes = o - c.o_coef;
        for (int k = 0; k < c.count; k++) {
            const size_t nb = (size_t)in[first + k].nblocks;
            FileOut &f = pl.files[(size_t)(first + k)];
            f.o_cr = o; o += up256((size_t)f.nchunks * 4 + 4);
            f.o_cs = o; o += up256((size_t)f.nchunks * 4 + 4);
            f.o_ro = o; o += up256(((size_t)f.nchunks + 1) * 8);
            f.o_so = o; o += up256(((size_t)f.nchunks + 1) * 8);
            f.o_start = o; o += up256((size_t)f.nsubCap * 8);
            f.o_exit = o; o += up256((size_t)f.nsubCap * 8);
            f.o_cnt = o; o += up256((size_t)f.nsubCap * 4);
            f.o_base = o; o += up256(((size_t)f.nsubCap + 1) * 8);
            f.o_planes = o; o += up256(nb * 64);
            f.o_diff = o; o += up256(nb * 4);
            f.o_dcsum = o; o += up256((nb + 1) * 8);
            f.o_rst = o; o += up256((size_t)f.nint * 4 + 4);
            const uint32_t gc = f.nchunks ? (f.nchunks + 255u) / 256u : 1u;
            if (gc > c.g_clean) c.g_clean = gc;
            if (f.nint) { if ((f.nint + 255u) / 256u > c.g_rst) c.g_rst = (f.nint + 255u) / 256u; }
            else if (f.nsubCap / kGroup > c.g_sub) c.g_sub = f.nsubCap / kGroup;
            const uint32_t gg = (uint32_t)((nb + 255) / 256), gb = (uint32_t)((nb + 31) / 32);
            if (gg > c.g_gather) c.g_gather = gg;
            if (gb > c.g_blocks) c.g_blocks = gb;
        }
        c.total = o;
        if (c.total > pl.device_bytes) pl.device_bytes = c.total;
        if (c.in_bytes > pl.staging_bytes) pl.staging_bytes = c.in_bytes;
        pl.chunks.push_back(c);
    }
    return pl;
}

} // namespace hsjpegd_plan
