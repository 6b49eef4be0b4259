// hs_postops.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): what the operators on a solved flow
// share on the host side -- the arrow and colour pictures, their JPEG forms, warp, forward-backward check, median and
// interpolation (hs_render / hs_color / hs_jpeg / hs_warp / hs_fb / hs_median / hs_interp.hip.h).  Three ordering rules hold for all of them
// (DESIGN.md 4.15), and this is their one home:
//   1. an owed ITER|EPS check is settled before c->cur is named: a re-run may end in the other buffer of the ping-pong, and
//      a result from a flow that a re-run would change is worth nothing (batch_device_begin; the synchronous forms call
//      settle_pending themselves, behind their own argument checks);
//   2. last_marked is false while work of an operator is in flight: that work reads the flow planes behind the marker of
//      the last solve, and hsflow_wait_solve / hsflow_flow_view_device then wait for the stream, not for the marker (every
//      enqueue_* clears the flag; only a synchronous form that has waited for its own work puts it back: sync_*);
//   3. a synchronous form waits for the context's own event, not for the stream, which the slots of a pair pipeline share
//      (sync_wait).
#pragma once

#include "hs_jpeg_batch_plan.h" // hsjpeg_plan::chunks

namespace {

// ---- the synchronous bracket -------------------------------------------------------------------------------------------
// sync_begin ... enqueue, copy out ... sync_finish.  A step in between that fails returns at once and leaves last_marked
// false: work may still be in flight, so that is the safe state (no scope guard puts the flag back).

int sync_begin(hsflow_ctx *c, bool *marked)
{
    if (!c->evRender) HS_HIP(c, hipEventCreateWithFlags(&c->evRender, hipEventDisableTiming));
    *marked = c->last_marked;
    return HSFLOW_OK;
}

// only what THIS context enqueued is waited for (the slots of a pair pipeline share streams)
int sync_wait(hsflow_ctx *c)
{
    HS_HIP(c, hipEventRecord(c->evRender, c->stream));
    HS_HIP(c, hipEventSynchronize(c->evRender));
    return HSFLOW_OK;
}

// Behind the call's last wait: nothing of it is in flight any more, the solve's marker speaks for the context again.
void sync_restore(hsflow_ctx *c, bool marked) { c->last_marked = marked; }

constexpr size_t kStatsBytes = 64; // hsflow_warp_stats, hsflow_fb_stats, hsflow_median_stats, hsflow_interp_stats: each asserts it

// The last wait, then the statistics record from page-locked memory (h) to the caller (record; NULL: none was asked for).
int sync_finish(hsflow_ctx *c, bool marked, void *record = nullptr, const void *h = nullptr)
{
    const int st = sync_wait(c);
    if (st) return st;
    if (record) std::memcpy(record, h, kStatsBytes);
    sync_restore(c, marked);
    return check_persist(c);
}

// One staging plane of a synchronous form, grown to the largest so far.  Only the synchronous forms use the staging, and
// they return behind the context's own event, so the old plane is idle; that event is waited for once more -- the context's
// own work, not the stream, which a pipeline's slots share.  (After a call that failed between its launch and its wait the
// plane may still be in use: hipFree holds until the device is idle.)
int stage_reserve(hsflow_ctx *c, uint8_t **p, size_t *have, size_t bytes)
{
    if (*have >= bytes) return HSFLOW_OK;
    if (*p && c->evRender) HS_HIP(c, hipEventSynchronize(c->evRender));
    hipFree(*p);
    *p = nullptr; *have = 0;
    HS_HIP(c, hipMalloc((void **)p, bytes));
    *have = bytes;
    return HSFLOW_OK;
}

// ---- statistics --------------------------------------------------------------------------------------------------------

// The one record of a synchronous form on the device and in page-locked memory, allocated by the first call that asks for
// statistics and kept (the dStats / hStats of hsflow_ctx's WarpScratch, FbScratch and MedianScratch).
int stats_reserve(hsflow_ctx *c, void **d, void **h)
{
    if (!*d) HS_HIP(c, hipMalloc(d, kStatsBytes));
    if (!*h) HS_HIP(c, hipHostMalloc(h, kStatsBytes, hipHostMallocDefault));
    return HSFLOW_OK;
}

int stats_copy_back(hsflow_ctx *c, void *h, const void *d)
{
    HS_HIP(c, hipMemcpyAsync(h, d, kStatsBytes, hipMemcpyDeviceToHost, c->stream));
    return HSFLOW_OK;
}

void stats_release(void *d, void *h)
{
    hipFree(d);
    if (h) hipHostFree(h);
}

// The grid of a chunk's launch: cnt pictures of units_x x units_y units each (columns of 1024 pixels x rows, or tiles x
// tiles).  With statistics every workgroup ends in atomics on its picture's one record, which the memory side serialises:
// up to 8 rows or tiles per workgroup while two workgroups per compute unit remain (hs_kernels_warp.hip.h).
void stats_rows(hsflow_ctx *c, long long units_x, long long units_y, int cnt, bool stats, dim3 *grid)
{
    const long long cus = c->num_cu > 0 ? c->num_cu : 256;
    long long per = stats ? units_x * units_y * cnt / (2 * cus) : 1;
    per = per < 1 ? 1 : per > 8 ? 8 : per;
    const long long gy = (units_y + per - 1) / per;
    *grid = dim3((unsigned)units_x, (unsigned)(gy < 65535 ? gy : 65535), (unsigned)cnt);
}

// The same, and with statistics (d_stats: the chunk's first record, or NULL) the memset of the chunk's records in front of
// the launch.
int stats_grid(hsflow_ctx *c, long long units_x, long long units_y, int cnt, void *d_stats, dim3 *grid)
{
    stats_rows(c, units_x, units_y, cnt, d_stats != nullptr, grid);
    if (d_stats) HS_HIP(c, hipMemsetAsync(d_stats, 0, kStatsBytes * (size_t)cnt, c->stream));
    return HSFLOW_OK;
}

// ---- batches -----------------------------------------------------------------------------------------------------------

// HSFLOW_JPEG_BATCH_MAX of this call: the environment's (1 .. the header's, for measuring the candidates), else the
// header's.  0: the environment's value is unusable.
int jpeg_batch_max()
{
    static_assert(HSFLOW_JPEG_BATCH_MAX >= 1 && HSFLOW_JPEG_BATCH_MAX <= hsk::kRenderBatchMax && HSFLOW_JPEG_BATCH_MAX <= hsk::kJpegBatchMax,
                  "the kernels' argument blocks hold at most 32 pictures");
    const char *e = getenv("HSFLOW_JPEG_BATCH_MAX");
    if (!e || !*e) return HSFLOW_JPEG_BATCH_MAX;
    char *rest = nullptr;
    const long v = strtol(e, &rest, 10);
    if (*rest || v < 1 || v > HSFLOW_JPEG_BATCH_MAX) return 0;
    return (int)v;
}

// The checks the batched entries share: the pairs ...
int check_batch_pairs(hsflow_ctx *c, int first_pair, int n)
{
    if (n < 1) return fail(c, HSFLOW_E_ARG, "a batch needs at least one picture");
    if (first_pair < 0 || (long long)first_pair + n > c->N) return fail(c, HSFLOW_E_ARG, "the batch's pairs exceed the context's");
    return HSFLOW_OK;
}

// ... and the chunk size of this call into *maxb.
int check_batch_max(hsflow_ctx *c, int *maxb)
{
    if (!(*maxb = jpeg_batch_max())) return fail(c, HSFLOW_E_ARG, "HSFLOW_JPEG_BATCH_MAX in the environment must be 1 .. " + std::to_string(HSFLOW_JPEG_BATCH_MAX));
    return HSFLOW_OK;
}

// What a device batch does last before it names c->cur, in this order: the statistics records' alignment (d_stats NULL:
// none, or checked by the caller at its own place), the chunk size of this call into *maxb, the owed ITER|EPS check
// settled (rule 1).  The chunks are then hsjpeg_plan::chunks(n, *maxb).
int batch_device_begin(hsflow_ctx *c, const void *d_stats, int *maxb)
{
    if (((uintptr_t)d_stats & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the statistics records must be 8-byte aligned");
    const int st = check_batch_max(c, maxb);
    if (st) return st;
    return settle_pending(c);
}

// The scratch of warp, check, median and interpolation (hsflow_destroy).
void postops_release(hsflow_ctx *c)
{
    hipFree(c->warp.src); hipFree(c->warp.ref); hipFree(c->warp.dst);
    stats_release(c->warp.dStats, c->warp.hStats);
    c->warp = hsflow_ctx::WarpScratch();
    hipFree(c->fb.mask); hipFree(c->fb.err2);
    stats_release(c->fb.dStats, c->fb.hStats);
    c->fb = hsflow_ctx::FbScratch();
    for (int k = 0; k < 2; k++) { hipFree(c->median.u[k]); hipFree(c->median.v[k]); hipFree(c->median.s[k]); }
    stats_release(c->median.dStats, c->median.hStats);
    c->median = hsflow_ctx::MedianScratch();
    hipFree(c->interp.base);
    for (uint8_t *p : c->interp.stage) hipFree(p);
    stats_release(c->interp.dStats, c->interp.hStats);
    c->interp = hsflow_ctx::InterpScratch();
}

} // namespace
