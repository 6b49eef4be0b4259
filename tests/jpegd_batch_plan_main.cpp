// The batch layout of the device JPEG decoder (opticalflowhs_amd/csrc/hs_jpegd_batch_plan.h) alone, no HIP: a program
// of its own, built with AddressSanitizer and UBSan by tests/test_jpegd_batch_host.py.  argv[1]: the batch maximum
// (HSFLOW_JPEGD_BATCH_MAX of include/hsflow.h).  For a few hundred random batches:
//   every per-file range is 256-aligned, inside the chunk's total and disjoint from every other of its chunk;
//   chunks cover the batch in order, none above the maximum;
//   grid extents equal the per-file maxima;
//   one file reproduces the sizes of the single-file formulas, written out below;
//   one file with a maximum of 1 -- how hs_jpegd.hip.h lays out every single decode -- passes all of the above.
#include "hs_jpegd_batch_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

using namespace hsjpegd_plan;

#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        if (!(cond)) { std::printf("FAILED line %d: %s (batch %d)\n", __LINE__, #cond, g_batch); return 1; } \
    } while (0)

static int g_batch = -1;
static const size_t kTab = 5960, kRec = 232; // any sizes do: the layout takes them as parameters

struct Range { size_t lo, hi; };

static int check(const std::vector<FileIn> &in, uint32_t S, int maxb)
{
    const int n = (int)in.size();
    const Params p{kTab, kRec, S, maxb};
    const Plan pl = layout(in.data(), n, p);
    CHECK((int)pl.files.size() == n);
    CHECK((int)pl.chunks.size() == (n + maxb - 1) / maxb);
    int next = 0;
    size_t dev = 0, stage = 0;
    for (const Chunk &c : pl.chunks) {
        CHECK(c.first == next && c.count >= 1 && c.count <= maxb);
        CHECK(c.count == maxb || c.first + c.count == n); // only the last chunk is short
        next += c.count;
        std::vector<Range> r;
        uint32_t g_clean = 0, g_sub = 0, g_rst = 0, g_gather = 0, g_blocks = 0;
        size_t clean_sum = 0, coef_sum = 0;
        for (int k = 0; k < c.count; k++) {
            const FileIn &fi = in[(size_t)(c.first + k)];
            const FileOut &f = pl.files[(size_t)(c.first + k)];
            const size_t nb = (size_t)fi.nblocks;
            // the single-file formulas, written out
            const uint32_t nbytes = (uint32_t)fi.scan_bytes, nchunks = (nbytes + 127) / 128;
            const uint32_t nsubCap = (uint32_t)((((uint64_t)nbytes * 8u + S - 1u) / S + 255u) / 256u * 256u) + (nbytes ? 0u : 256u);
            const uint32_t nint = fi.restart_interval ? (uint32_t)((fi.nmcu + fi.restart_interval - 1) / fi.restart_interval) : 0u;
            CHECK(f.n == nbytes && f.nchunks == nchunks && f.nsubCap == nsubCap && f.nint == nint);
            CHECK(f.scan_span == up256((size_t)nbytes + 4) && f.clean_span == up256((size_t)nbytes + 16) && f.coef_span == up256(nb * 128));
            const std::pair<size_t, size_t> own[] = {
                {f.o_tab, kTab}, {f.o_scan, (size_t)nbytes + 4}, {f.o_clean, (size_t)nbytes + 16}, {f.o_coef, nb * 128},
                {f.o_cr, (size_t)nchunks * 4 + 4}, {f.o_cs, (size_t)nchunks * 4 + 4}, {f.o_ro, ((size_t)nchunks + 1) * 8}, {f.o_so, ((size_t)nchunks + 1) * 8},
                {f.o_start, (size_t)nsubCap * 8}, {f.o_exit, (size_t)nsubCap * 8}, {f.o_cnt, (size_t)nsubCap * 4}, {f.o_base, ((size_t)nsubCap + 1) * 8},
                {f.o_planes, nb * 64}, {f.o_diff, nb * 4}, {f.o_dcsum, (nb + 1) * 8}, {f.o_rst, (size_t)nint * 4}};
            for (const auto &o : own) {
                CHECK(o.first % 256 == 0 && o.first + o.second <= c.total);
                r.push_back(Range{o.first, o.first + std::max<size_t>(o.second, 1)}); // (an empty range still owns its start)
            }
            CHECK(f.o_tab + kTab <= c.in_bytes && f.o_scan + f.scan_span <= c.o_recs); // what the one copy carries
            CHECK(f.o_clean >= c.o_clean && f.o_clean + f.clean_span <= c.o_clean + c.clean_bytes); // what the two memsets cover
            CHECK(f.o_coef >= c.o_coef && f.o_coef + f.coef_span <= c.o_coef + c.coef_bytes);
            clean_sum += f.clean_span; coef_sum += f.coef_span;
            g_clean = std::max(g_clean, nchunks ? (nchunks + 255u) / 256u : 1u);
            if (nint) g_rst = std::max(g_rst, (nint + 255u) / 256u);
            else g_sub = std::max(g_sub, nsubCap / 256u);
            g_gather = std::max(g_gather, (uint32_t)((nb + 255) / 256));
            g_blocks = std::max(g_blocks, (uint32_t)((nb + 31) / 32));
        }
        CHECK(clean_sum == c.clean_bytes && coef_sum == c.coef_bytes); // ... and nothing else
        CHECK(c.o_recs % 256 == 0 && c.o_recs + (size_t)c.count * kRec <= c.in_bytes && c.in_bytes <= c.o_clean && c.in_bytes <= c.total);
        r.push_back(Range{c.o_recs, c.o_recs + (size_t)c.count * kRec});
        std::sort(r.begin(), r.end(), [](const Range &a, const Range &b) { return a.lo < b.lo; });
        for (size_t i = 1; i < r.size(); i++) CHECK(r[i - 1].hi <= r[i].lo);
        CHECK(c.g_clean == g_clean && c.g_sub == g_sub && c.g_rst == g_rst && c.g_gather == g_gather && c.g_blocks == g_blocks);
        dev = std::max(dev, c.total); stage = std::max(stage, c.in_bytes);
    }
    CHECK(next == n && pl.device_bytes == dev && pl.staging_bytes == stage);
    if (n == 1) { // the single-file path's sizes: its input copy, and its per-length allocation without the frame part
        const uint32_t nbytes = (uint32_t)in[0].scan_bytes, nchunks = (nbytes + 127) / 128, nsubCap = pl.files[0].nsubCap;
        const size_t tab_bytes = up256(kTab), in_bytes = tab_bytes + up256((size_t)nbytes + 4);
        const size_t need = in_bytes + up256((size_t)nbytes + 16) + 2 * up256((size_t)nchunks * 4 + 4) + 2 * up256(((size_t)nchunks + 1) * 8) + 2 * up256((size_t)nsubCap * 8) +
                            up256((size_t)nsubCap * 4) + up256(((size_t)nsubCap + 1) * 8);
        const size_t nb = (size_t)in[0].nblocks;
        const size_t frame = up256(nb * 128) + up256(nb * 64) + up256(nb * 4) + up256((nb + 1) * 8);
        const Chunk &c = pl.chunks[0];
        CHECK(pl.files[0].o_tab == 0 && pl.files[0].o_scan == tab_bytes && c.o_recs == in_bytes);
        CHECK(c.in_bytes == in_bytes + up256(kRec));
        CHECK(c.total == need + frame + up256(kRec) + up256((size_t)pl.files[0].nint * 4 + 4));
    }
    return 0;
}

int main(int argc, char **argv)
{
    const int maxb = argc > 1 ? std::atoi(argv[1]) : 8;
    if (maxb < 1) { std::printf("usage: %s <batch maximum>\n", argv[0]); return 2; }
    std::mt19937_64 rng(20251);
    const uint32_t Ss[] = {32, 128, 1024, 4096};
    auto file = [&](uint64_t bytes) {
        const int hs = 1 + (int)(rng() % 2), vs = hs == 2 ? 1 + (int)(rng() % 2) : 1, ncomp = rng() % 4 ? 3 : 1;
        const int64_t nmcu = 1 + (int64_t)(rng() % 9000);
        const int64_t bpm = ncomp == 1 ? 1 : hs * vs + 2;
        const int32_t ri = rng() % 3 ? 0 : 1 + (int32_t)(rng() % 40);
        return FileIn{bytes, nmcu * bpm, nmcu, ri};
    };
    int batches = 0;
    // fixed cases first: a zero-length segment alone and among others, one over the maximum, exactly the maximum
    for (uint32_t S : Ss) {
        g_batch = batches++;
        if (check({file(0)}, S, maxb)) return 1;
        for (uint64_t bytes : {0ull, 1ull, 127ull, 128ull, 700ull, 20000ull, 600000ull}) { // a single decode: n = 1, maximum 1
            g_batch = batches++;
            if (check({file(bytes)}, S, 1)) return 1;
        }
        g_batch = batches++;
        if (check({file(700), file(0), file(1), file(0)}, S, maxb)) return 1;
        for (int n : {maxb, maxb + 1, 2 * maxb + 1}) {
            std::vector<FileIn> in;
            for (int i = 0; i < n; i++) in.push_back(file(1 + rng() % 20000));
            g_batch = batches++;
            if (check(in, S, maxb)) return 1;
        }
    }
    for (int b = 0; b < 300; b++) {
        const int n = b < 60 ? 1 : 1 + (int)(rng() % (3 * (uint64_t)maxb + 2));
        std::vector<FileIn> in;
        for (int i = 0; i < n; i++) {
            const unsigned kind = (unsigned)(rng() % 8);
            const uint64_t bytes = kind == 0 ? 0 : kind == 1 ? rng() % 300 : kind == 2 ? 1 + rng() % 600000 : 1 + rng() % 20000;
            in.push_back(file(bytes));
        }
        g_batch = batches++;
        if (check(in, Ss[rng() % 4], maxb)) return 1;
    }
    std::printf("batch plan ok: %d batches, maximum %d\n", batches, maxb);
    return 0;
}
