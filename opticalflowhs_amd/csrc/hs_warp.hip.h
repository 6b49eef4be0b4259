// hs_warp.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_warp*, a picture warped backwards
// by the flow where the solver left it (hs_warp_rule.h) and the residual against a reference picture.  Per chunk of at
// most HSFLOW_JPEG_BATCH_MAX pictures: one launch (hs_kernels_warp.hip.h), with statistics one memset of the chunk's
// records in front of it.  The single forms are batches of one.  A context that never warps allocates and launches
// nothing here.
#pragma once

namespace {

static_assert(sizeof(hsflow_warp_stats) == 64 && sizeof(hsflow_warp_stats) == sizeof(hsk::WarpStatsWords), "hsflow_warp_stats is 64 bytes on both sides");
static_assert(offsetof(hsflow_warp_stats, max_warped) == 40 && offsetof(hsflow_warp_stats, max_plain) == 44, "hsflow_warp_stats: the kernel's layout");
static_assert(sizeof(hswarp::Sums) <= sizeof(hsflow_warp_stats), "the host rule's sums are the head of hsflow_warp_stats");

int check_warp_params(hsflow_ctx *c, const hsflow_warp_params *wp)
{
    if (!wp || wp->struct_size != sizeof(hsflow_warp_params)) return fail(c, HSFLOW_E_ARG, "warp params null or struct_size mismatch");
    if (wp->channels != 1 && wp->channels != 3) return fail(c, HSFLOW_E_ARG, "warp channels must be 1 or 3");
    if (wp->border != HSFLOW_WARP_BORDER_CONSTANT && wp->border != HSFLOW_WARP_BORDER_REPLICATE) return fail(c, HSFLOW_E_ARG, "unknown warp border");
    if (!(std::isfinite(wp->t) && std::fabs(wp->t) <= hswarp::kMaxT)) return fail(c, HSFLOW_E_ARG, "warp t must be finite and |t| <= 1e6");
    return HSFLOW_OK;
}

unsigned warp_fill(const hsflow_warp_params &wp)
{
    unsigned fill = 0u;
    for (int k = 0; k < wp.channels; k++) fill |= (unsigned)wp.fill[k] << (8 * k);
    return fill;
}

// The checks every form shares once the pictures are known: what there is to do, the row sizes, no picture onto itself.
// own: src is the context's curr plane (channels must be 1).
int check_warp_pictures(hsflow_ctx *c, const hsflow_warp_params *wp, int W, bool own, bool has_ref, bool has_dst, bool has_stats, size_t src_stride,
                        size_t ref_stride, size_t dst_stride)
{
    if (own && wp->channels != 1) return fail(c, HSFLOW_E_ARG, "the context's own frames have one channel");
    if (!has_dst && !has_stats) return fail(c, HSFLOW_E_ARG, "neither a destination nor statistics asked for");
    const size_t rowb = (size_t)W * (size_t)wp->channels;
    if (!own && src_stride < rowb) return fail(c, HSFLOW_E_SIZE, "source stride smaller than channels*width");
    if (has_ref && ref_stride < rowb) return fail(c, HSFLOW_E_SIZE, "reference stride smaller than channels*width");
    if (has_dst && dst_stride < rowb) return fail(c, HSFLOW_E_SIZE, "destination stride smaller than channels*width");
    return HSFLOW_OK;
}

template <int C, bool STATS>
void launch_warp(hsflow_ctx *c, const dim3 &grid, const float *u, const float *v, const hsk::WarpBatchPics &pics, size_t ss, size_t rs, size_t ds,
                 const hsflow_warp_params &wp, hsk::WarpStatsWords *stats)
{
    hipLaunchKernelGGL((hsk::k_warp_batch<C, STATS>), grid, dim3(256), 0, c->stream, u, v, c->plane, pics, (long long)ss, (long long)rs, (long long)ds, c->W,
                       c->H, c->P, wp.t, wp.border, warp_fill(wp), stats);
}

// The launch for the pairs first_pair .. first_pair + cnt - 1 (cnt <= kRenderBatchMax).  d_stats: the chunk's first
// record, or NULL.  The caller has checked every argument.
int enqueue_warp_chunk(hsflow_ctx *c, int first_pair, int cnt, const hsflow_warp_params &wp, const hsk::WarpBatchPics &pics, size_t ss, size_t rs, size_t ds,
                       void *d_stats)
{
    const float *u = c->dU[c->cur] + first_pair * c->plane, *v = c->dV[c->cur] + first_pair * c->plane;
    hsk::WarpStatsWords *stats = (hsk::WarpStatsWords *)d_stats;
    dim3 grid;
    const int st = stats_grid(c, (c->W + 1023) / 1024, c->H, cnt, stats, &grid);
    if (st) return st;
    if (wp.channels == 1) {
        if (stats) launch_warp<1, true>(c, grid, u, v, pics, ss, rs, ds, wp, stats);
        else launch_warp<1, false>(c, grid, u, v, pics, ss, rs, ds, wp, stats);
    } else {
        if (stats) launch_warp<3, true>(c, grid, u, v, pics, ss, rs, ds, wp, stats);
        else launch_warp<3, false>(c, grid, u, v, pics, ss, rs, ds, wp, stats);
    }
    HS_HIP(c, hipGetLastError());
    c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
    return HSFLOW_OK;
}

} // namespace

extern "C" {

void hsflow_default_warp_params(hsflow_warp_params *wp)
{
    if (!wp) return;
    std::memset(wp, 0, sizeof(*wp));
    wp->struct_size = sizeof(*wp);
    wp->channels = 1;
    wp->border = HSFLOW_WARP_BORDER_CONSTANT;
    wp->t = 1.0f;
}

int hsflow_warp_host(const float *u, size_t u_stride, const float *v, size_t v_stride, int width, int height, const hsflow_warp_params *wp,
                     const uint8_t *src, size_t src_stride, const uint8_t *ref, size_t ref_stride, uint8_t *dst, size_t dst_stride, hsflow_warp_stats *stats)
{
    int st = check_warp_params(nullptr, wp);
    if (st) return st;
    if (!u || !v || !src) return fail(nullptr, HSFLOW_E_ARG, "hsflow_warp_host: null pointer");
    if (dst && (dst == src || dst == ref)) return fail(nullptr, HSFLOW_E_ARG, "hsflow_warp_host: the destination is the source or the reference");
    if (width < 1 || height < 1) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_warp_host: width and height must be positive");
    if (u_stride < (size_t)width * 4 || v_stride < (size_t)width * 4 || ((u_stride | v_stride) & 3u))
        return fail(nullptr, HSFLOW_E_SIZE, "hsflow_warp_host: flow stride smaller than 4*width or no multiple of 4");
    if ((st = check_warp_pictures(nullptr, wp, width, false, ref != nullptr, dst != nullptr, stats != nullptr, src_stride, ref_stride, dst_stride))) return st;
    hswarp::Sums sums;
    if (wp->channels == 1)
        hswarp::warp_rows<1>(u, u_stride, v, v_stride, width, height, wp->t, wp->border, warp_fill(*wp), src, src_stride, ref, ref_stride, dst, dst_stride,
                             stats ? &sums : nullptr);
    else
        hswarp::warp_rows<3>(u, u_stride, v, v_stride, width, height, wp->t, wp->border, warp_fill(*wp), src, src_stride, ref, ref_stride, dst, dst_stride,
                             stats ? &sums : nullptr);
    if (stats) {
        std::memset(stats, 0, sizeof(*stats));
        stats->inside = sums.inside; stats->outside = sums.outside; stats->unknown = sums.unknown;
        stats->sad_warped = sums.sad_warped; stats->sad_plain = sums.sad_plain;
        stats->max_warped = sums.max_warped; stats->max_plain = sums.max_plain;
    }
    return HSFLOW_OK;
}

int hsflow_warp_batch_device(hsflow_ctx *c, int first_pair, int n, const hsflow_warp_params *wp, const void *const *d_src, size_t src_stride,
                             const void *const *d_ref, size_t ref_stride, void *const *d_dst, size_t dst_stride, hsflow_warp_stats *d_stats)
{
    int st = check_ctx(c, 0), maxb = 0;
    if (st) return st;
    if ((st = check_batch_pairs(c, first_pair, n))) return st;
    if ((st = check_warp_params(c, wp))) return st;
    const bool own = d_src == nullptr;
    if ((st = check_warp_pictures(c, wp, c->W, own, d_ref != nullptr || own, d_dst != nullptr, d_stats != nullptr, src_stride,
                                  d_ref ? ref_stride : (size_t)c->P, dst_stride)))
        return st;
    for (int i = 0; i < n; i++) {
        if ((d_src && !d_src[i]) || (d_ref && !d_ref[i]) || (d_dst && !d_dst[i])) return fail(c, HSFLOW_E_ARG, "picture " + std::to_string(i) + ": null picture pointer");
        if (d_dst && ((d_src && d_dst[i] == d_src[i]) || (d_ref && d_dst[i] == d_ref[i])))
            return fail(c, HSFLOW_E_ARG, "picture " + std::to_string(i) + ": the destination is the source or the reference");
    }
    if ((st = batch_device_begin(c, d_stats, &maxb))) return st;
    if (own && (st = resolve_lazy_frames(c, false))) return st;
    const size_t ss = own ? (size_t)c->P : src_stride, rs = d_ref ? ref_stride : (size_t)c->P;
    for (const hsjpeg_plan::Chunk &ch : hsjpeg_plan::chunks(n, maxb)) {
        hsk::WarpBatchPics pics{};
        for (int k = 0; k < ch.count; k++) {
            const long long pair = first_pair + ch.first + k;
            pics.src[k] = own ? c->dB + pair * c->plane : (const uint8_t *)d_src[ch.first + k];
            pics.ref[k] = d_ref ? (const uint8_t *)d_ref[ch.first + k] : own ? c->dA + pair * c->plane : nullptr;
            pics.dst[k] = d_dst ? (uint8_t *)d_dst[ch.first + k] : nullptr;
            if (d_dst && word_aligned(d_dst[ch.first + k], dst_stride)) pics.wide |= 1u << k;
        }
        if ((st = enqueue_warp_chunk(c, first_pair + ch.first, ch.count, *wp, pics, ss, rs, dst_stride, d_stats ? d_stats + ch.first : nullptr))) return st;
    }
    return HSFLOW_OK;
}

int hsflow_warp_device(hsflow_ctx *c, int pair, const hsflow_warp_params *wp, const void *d_src, size_t src_stride, const void *d_ref, size_t ref_stride,
                       void *d_dst, size_t dst_stride, hsflow_warp_stats *d_stats)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    const void *const src[1] = {d_src}, *const ref[1] = {d_ref};
    void *const dst[1] = {d_dst};
    return hsflow_warp_batch_device(c, pair, 1, wp, d_src ? src : nullptr, src_stride, d_ref ? ref : nullptr, ref_stride, d_dst ? dst : nullptr, dst_stride,
                                    d_stats);
}

int hsflow_warp(hsflow_ctx *c, int pair, const hsflow_warp_params *wp, const uint8_t *src, size_t src_stride, const uint8_t *ref, size_t ref_stride,
                uint8_t *dst, size_t dst_stride, hsflow_warp_stats *stats)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if ((st = check_warp_params(c, wp))) return st;
    const bool own = src == nullptr;
    if ((st = check_warp_pictures(c, wp, c->W, own, ref != nullptr || own, dst != nullptr, stats != nullptr, src_stride, ref ? ref_stride : (size_t)c->P,
                                  dst_stride)))
        return st;
    if (dst && (dst == src || dst == ref)) return fail(c, HSFLOW_E_ARG, "the destination is the source or the reference");
    if ((st = settle_pending(c))) return st;
    if (own && (st = resolve_lazy_frames(c, false))) return st;
    const size_t rowb = (size_t)c->W * (size_t)wp->channels, bytes = rowb * c->H;
    hsflow_ctx::WarpScratch &w = c->warp;
    if (src && (st = stage_reserve(c, &w.src, &w.src_bytes, bytes))) return st;
    if (ref && (st = stage_reserve(c, &w.ref, &w.ref_bytes, bytes))) return st;
    if (dst && (st = stage_reserve(c, &w.dst, &w.dst_bytes, bytes))) return st;
    if (stats && (st = stats_reserve(c, (void **)&w.dStats, (void **)&w.hStats))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    if (src) HS_HIP(c, copy_rows_async(c, w.src, rowb, src, src_stride, rowb, c->H, hipMemcpyHostToDevice));
    if (ref) HS_HIP(c, copy_rows_async(c, w.ref, rowb, ref, ref_stride, rowb, c->H, hipMemcpyHostToDevice));
    hsk::WarpBatchPics pics{};
    pics.src[0] = own ? c->dB + pair * c->plane : w.src;
    pics.ref[0] = ref ? w.ref : own ? c->dA + pair * c->plane : nullptr;
    pics.dst[0] = dst ? w.dst : nullptr;
    pics.wide = dst ? (uint32_t)word_aligned(w.dst, rowb) : 0u;
    if ((st = enqueue_warp_chunk(c, pair, 1, *wp, pics, own ? (size_t)c->P : rowb, ref ? rowb : (size_t)c->P, rowb, stats ? w.dStats : nullptr))) return st;
    if (dst) HS_HIP(c, copy_rows_async(c, dst, dst_stride, w.dst, rowb, rowb, c->H, hipMemcpyDeviceToHost));
    if (stats && (st = stats_copy_back(c, w.hStats, w.dStats))) return st;
    return sync_finish(c, marked, stats, w.hStats);
}

} // extern "C"
