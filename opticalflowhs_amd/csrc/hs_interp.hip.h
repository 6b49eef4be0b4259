// hs_interp.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_interp* and hsflow_project_flow*,
// the frame at time t between the two frames of a pair (hs_interp_rule.h) from the flow where the solver left it.  Per
// chunk of at most HSFLOW_INTERP_BATCH_MAX TIMES of one pair: a memset of the key planes, the splat, the resolve,
// fill_passes launches of the median kernel in FILL mode (enqueue_median_chunk, hs_median.hip.h) and the blend
// (hs_kernels_interp.hip.h); with statistics one memset of the chunk's records in front.  The single forms are batches of
// one.  A context that never interpolates allocates and launches nothing here.  The three ordering rules of
// hs_postops.hip.h hold: the owed check is settled before c->cur is named, every enqueue clears last_marked, the
// synchronous form waits for the context's own event.
#pragma once

namespace {

static_assert(sizeof(hsflow_interp_stats) == 64 && sizeof(hsflow_interp_stats) == sizeof(hsk::InterpStatsWords), "hsflow_interp_stats is 64 bytes on both sides");
static_assert(sizeof(hsflow_interp_stats) == sizeof(hsinterp::Sums), "the host rule's sums are hsflow_interp_stats");
static_assert(offsetof(hsflow_interp_stats, sad) == 32 && offsetof(hsflow_interp_stats, holes) == 40 && offsetof(hsflow_interp_stats, unfilled) == 44 &&
                  offsetof(hsflow_interp_stats, max_diff) == 60,
              "hsflow_interp_stats: the kernels' layout");
static_assert(sizeof(hsflow_interp_params) == 20, "hsflow_interp_params is 20 bytes");
static_assert(HSFLOW_INTERP_BATCH_MAX == hsk::kInterpBatchMax && HSFLOW_INTERP_BATCH_MAX <= hsk::kMedianBatchMax, "one chunk of times is one chunk of the fill");
static_assert(HSFLOW_INTERP_BLENDED == hsinterp::kBlended && HSFLOW_INTERP_PREV_ONLY == hsinterp::kPrevOnly && HSFLOW_INTERP_CURR_ONLY == hsinterp::kCurrOnly &&
                  HSFLOW_INTERP_CLAMPED == hsinterp::kClamped,
              "the header's classes are the rule's");

int check_interp_params(hsflow_ctx *c, const hsflow_interp_params *ip)
{
    if (!ip || ip->struct_size != sizeof(hsflow_interp_params)) return fail(c, HSFLOW_E_ARG, "interp params null or struct_size mismatch");
    if (ip->channels != 1 && ip->channels != 3) return fail(c, HSFLOW_E_ARG, "interp channels must be 1 or 3");
    if (ip->fill_radius != 1 && ip->fill_radius != 2) return fail(c, HSFLOW_E_ARG, "interp fill_radius must be 1 or 2");
    const int side = 2 * ip->fill_radius + 1;
    if (ip->fill_min_votes < 1 || ip->fill_min_votes > side * side) return fail(c, HSFLOW_E_ARG, "interp fill_min_votes must be 1 .. (2 fill_radius + 1)^2");
    if (ip->fill_passes < 0 || ip->fill_passes > HSFLOW_MEDIAN_MAX_PASSES)
        return fail(c, HSFLOW_E_ARG, "interp fill_passes must be 0 .. " + std::to_string(HSFLOW_MEDIAN_MAX_PASSES));
    return HSFLOW_OK;
}

int check_interp_time(hsflow_ctx *c, float t)
{
    if (!(std::isfinite(t) && t >= 0.0f && t <= 1.0f)) return fail(c, HSFLOW_E_ARG, "interp t must be finite and 0 <= t <= 1");
    return HSFLOW_OK;
}

hsflow_median_params interp_fill_params(const hsflow_interp_params &ip)
{
    hsflow_median_params mp;
    mp.struct_size = sizeof(mp);
    mp.radius = ip.fill_radius;
    mp.mode = HSFLOW_MEDIAN_FILL;
    mp.min_votes = ip.fill_min_votes;
    return mp;
}

// The two frames of every form.  own: they are the context's planes (channels must be 1, curr must be absent too).
int check_interp_frames(hsflow_ctx *c, const hsflow_interp_params *ip, int W, bool own, bool has_curr, size_t prev_stride, size_t curr_stride)
{
    if (own && has_curr) return fail(c, HSFLOW_E_ARG, "the second frame without the first");
    if (!own && !has_curr) return fail(c, HSFLOW_E_ARG, "the first frame without the second");
    if (own && ip->channels != 1) return fail(c, HSFLOW_E_ARG, "the context's own frames have one channel");
    const size_t rowb = (size_t)W * (size_t)ip->channels;
    if (!own && (prev_stride < rowb || curr_stride < rowb)) return fail(c, HSFLOW_E_SIZE, "frame stride smaller than channels*width");
    return HSFLOW_OK;
}

// What the forms of the whole rule share once the optional pictures are known.
int check_interp_pictures(hsflow_ctx *c, const hsflow_interp_params *ip, int W, bool has_vp, size_t vps, bool has_vc, size_t vcs, bool has_ref, size_t rs,
                          bool has_dst, size_t ds, bool has_cls, size_t cls_s, bool has_stats)
{
    if (!has_dst && !has_cls && !has_stats) return fail(c, HSFLOW_E_ARG, "neither a picture nor a class plane nor statistics asked for");
    const size_t rowb = (size_t)W * (size_t)ip->channels;
    if ((has_vp && vps < (size_t)W) || (has_vc && vcs < (size_t)W)) return fail(c, HSFLOW_E_SIZE, "visibility stride smaller than width");
    if (has_ref && rs < rowb) return fail(c, HSFLOW_E_SIZE, "reference stride smaller than channels*width");
    if (has_dst && ds < rowb) return fail(c, HSFLOW_E_SIZE, "destination stride smaller than channels*width");
    if (has_cls && cls_s < (size_t)W) return fail(c, HSFLOW_E_SIZE, "class stride smaller than width");
    return HSFLOW_OK;
}

// ... and the outputs of the forms that stop after the fill.
int check_project_planes(hsflow_ctx *c, int W, bool has_u, bool has_v, size_t os, bool has_state, size_t sos, bool has_stats)
{
    if (has_u != has_v) return fail(c, HSFLOW_E_ARG, "the two flow outputs are asked for together or not at all");
    if (!has_u && !has_state && !has_stats) return fail(c, HSFLOW_E_ARG, "neither the flow nor the state nor statistics asked for");
    if (has_u && (os < (size_t)W * 4 || (os & 3u))) return fail(c, HSFLOW_E_SIZE, "output flow stride smaller than 4*width or no multiple of 4");
    if (has_state && sos < (size_t)W) return fail(c, HSFLOW_E_SIZE, "output state stride smaller than width");
    return HSFLOW_OK;
}

// A destination may not be one of the inputs (the blend gathers from them while other lanes write).
bool interp_is_input(const void *d, const void *const (&in)[5])
{
    for (const void *p : in)
        if (d && d == p) return true;
    return false;
}

// HSFLOW_INTERP_BATCH_MAX of this call: the environment's (1 .. the header's), else the header's.  0: unusable.
int interp_batch_max()
{
    const char *e = getenv("HSFLOW_INTERP_BATCH_MAX");
    if (!e || !*e) return HSFLOW_INTERP_BATCH_MAX;
    char *rest = nullptr;
    const long v = strtol(e, &rest, 10);
    if (*rest || v < 1 || v > HSFLOW_INTERP_BATCH_MAX) return 0;
    return (int)v;
}

// The scratch of `times` times, one block: per time plane (= pitch x height) words of keys, two pairs of fp32 planes,
// two state planes, all of pitch P like the context's planes (256-byte bases, 16-byte loads); then the fill's records.
// Grown on demand and kept.  (Work that still uses the old block: hipFree holds until the device is idle.)
int interp_reserve(hsflow_ctx *c, int times)
{
    hsflow_ctx::InterpScratch &s = c->interp;
    if (s.times >= times) return HSFLOW_OK;
    hipFree(s.base);
    s.base = nullptr;
    s.times = 0;
    const size_t plane = (size_t)c->plane;
    HS_HIP(c, hipMalloc(&s.base, (size_t)times * (plane * 26 + kStatsBytes)));
    s.times = times;
    return HSFLOW_OK;
}

struct InterpPlanes {
    unsigned long long *keys; // time i: i * plane words on
    float *u[2], *v[2];       // time i: i * plane floats on
    uint8_t *s[2];            // time i: i * plane bytes on
    hsk::MedianStatsWords *med;
};

InterpPlanes interp_planes(hsflow_ctx *c)
{
    const hsflow_ctx::InterpScratch &s = c->interp;
    const size_t all = (size_t)c->plane * s.times;
    InterpPlanes p;
    uint8_t *b = (uint8_t *)s.base;
    p.keys = (unsigned long long *)b; b += all * 8;
    for (int k = 0; k < 2; k++) { p.u[k] = (float *)b; b += all * 4; p.v[k] = (float *)b; b += all * 4; }
    for (int k = 0; k < 2; k++) { p.s[k] = b; b += all; }
    p.med = (hsk::MedianStatsWords *)b; // (all is a multiple of 64: 8-byte aligned)
    return p;
}

// One call of any device form.  project: stop after the fill, into u_out / v_out / state_out (n is 1).
struct InterpJob {
    int pair = 0, n = 1;
    const float *t = nullptr;
    const hsflow_interp_params *ip = nullptr;
    hsk::InterpFrames fr{};
    const void *const *ref = nullptr;
    void *const *dst = nullptr, *const *cls = nullptr;
    size_t ref_stride = 0, dst_stride = 0, cls_stride = 0;
    hsflow_interp_stats *d_stats = nullptr;
    bool project = false;
    float *u_out = nullptr, *v_out = nullptr;
    uint8_t *state_out = nullptr;
    size_t out_stride = 0, state_out_stride = 0;
};

// The launches of the times first .. first + cnt - 1 (cnt <= the scratch's times).  The caller has checked every argument,
// settled the owed check and reserved the scratch.
int enqueue_interp_chunk(hsflow_ctx *c, const InterpJob &job, int first, int cnt)
{
    const hsflow_interp_params &ip = *job.ip;
    const InterpPlanes sp = interp_planes(c);
    const long long plane = c->plane;
    const size_t frow = (size_t)c->P * 4, brow = (size_t)c->P;
    const float *u = c->dU[c->cur] + job.pair * plane, *v = c->dV[c->cur] + job.pair * plane;
    hsk::InterpStatsWords *stats = job.d_stats ? (hsk::InterpStatsWords *)(job.d_stats + first) : nullptr;
    hsk::InterpTimes times{};
    for (int k = 0; k < cnt; k++) times.t[k] = job.t[first + k];
    dim3 grid; // of all three kernels; the records' memset goes in front of everything
    int st = stats_grid(c, (c->W + 1023) / 1024, c->H, cnt, stats, &grid);
    if (st) return st;
    HS_HIP(c, hipMemsetAsync(sp.keys, 0xff, (size_t)plane * 8 * cnt, c->stream));
    HS_HIP(c, hsk::launch_interp_splat(ip.channels, grid, c->stream, u, v, c->P, job.fr, c->W, c->H, sp.keys, plane, times));
    c->last_marked = false; // (hs_postops.hip.h, rule 2: the flow planes are read behind the marker of the last solve)
    // stage j (0: the resolve, j >= 1: pass j of the fill) writes set j & 1 of the scratch; the last stage of a projection
    // writes the caller's planes
    const int passes = ip.fill_passes;
    auto stage_out = [&](int j, int k, float **uo, float **vo, uint8_t **so, size_t *os, size_t *sos) {
        if (job.project && j == passes) {
            *uo = job.u_out; *vo = job.v_out; *so = job.state_out; *os = job.out_stride; *sos = job.state_out_stride;
        } else {
            *uo = sp.u[j & 1] + k * plane; *vo = sp.v[j & 1] + k * plane; *os = frow; *sos = brow;
            *so = (j == passes) ? nullptr : sp.s[j & 1] + k * plane; // (the blend does not read the state)
        }
    };
    hsk::InterpFlowOut out{};
    size_t os = 0, sos = 0;
    for (int k = 0; k < cnt; k++) stage_out(0, k, &out.ut[k], &out.vt[k], &out.state[k], &os, &sos);
    HS_HIP(c, hsk::launch_interp_resolve(grid, c->stream, sp.keys, plane, u, v, c->P, c->W, c->H, times, out, (long long)os, (long long)sos, stats, passes == 0));
    const hsflow_median_params mp = interp_fill_params(ip);
    for (int j = 1; j <= passes; j++) {
        hsk::MedianBatchFields f{};
        size_t is = os, ss = sos;
        for (int k = 0; k < cnt; k++) {
            f.u[k] = out.ut[k]; f.v[k] = out.vt[k]; f.state[k] = out.state[k];
            stage_out(j, k, &out.ut[k], &out.vt[k], &out.state[k], &os, &sos);
            f.u_out[k] = out.ut[k]; f.v_out[k] = out.vt[k]; f.state_out[k] = out.state[k];
        }
        if ((st = enqueue_median_chunk(c, cnt, mp, f, is, ss, os, sos, j == passes && stats ? sp.med : nullptr))) return st;
    }
    if (passes > 0 && stats) // the fill's count of state-0 cells (below 2^32) into the records: 4 bytes each, 64 bytes apart
        HS_HIP(c, hipMemcpy2DAsync(&stats->unfilled, kStatsBytes, &sp.med->unfilled, kStatsBytes, 4, cnt, hipMemcpyDeviceToDevice, c->stream));
    if (job.project) return HSFLOW_OK;
    hsk::InterpBlendPics pics{};
    for (int k = 0; k < cnt; k++) {
        const int i = first + k;
        pics.ut[k] = out.ut[k]; pics.vt[k] = out.vt[k];
        pics.t[k] = job.t[i];
        pics.ref[k] = job.ref ? (const uint8_t *)job.ref[i] : nullptr;
        pics.dst[k] = job.dst ? (uint8_t *)job.dst[i] : nullptr;
        pics.cls[k] = job.cls ? (uint8_t *)job.cls[i] : nullptr;
        if (job.dst && word_aligned(job.dst[i], job.dst_stride)) pics.wide_dst |= 1u << k;
        if (job.cls && word_aligned(job.cls[i], job.cls_stride)) pics.wide_cls |= 1u << k;
    }
    HS_HIP(c, hsk::launch_interp_blend(ip.channels, grid, c->stream, pics, (long long)frow, job.fr, (long long)job.ref_stride, (long long)job.dst_stride,
                                       (long long)job.cls_stride, c->W, c->H, stats));
    return HSFLOW_OK;
}

// Every chunk of a job.  maxb: the chunk size of this call.
int enqueue_interp(hsflow_ctx *c, const InterpJob &job, int maxb)
{
    int st = interp_reserve(c, job.n < maxb ? job.n : maxb);
    if (st) return st;
    for (const hsjpeg_plan::Chunk &ch : hsjpeg_plan::chunks(job.n, maxb))
        if ((st = enqueue_interp_chunk(c, job, ch.first, ch.count))) return st;
    return HSFLOW_OK;
}

int interp_check_batch_max(hsflow_ctx *c, int *maxb)
{
    if (!(*maxb = interp_batch_max())) return fail(c, HSFLOW_E_ARG, "HSFLOW_INTERP_BATCH_MAX in the environment must be 1 .. " + std::to_string(HSFLOW_INTERP_BATCH_MAX));
    return HSFLOW_OK;
}

// The frames of a device job: the caller's, or the context's own planes of the pair.
hsk::InterpFrames interp_frames(hsflow_ctx *c, int pair, const void *prev, size_t ps, const void *curr, size_t cs, const void *vp, size_t vps, const void *vc,
                                size_t vcs)
{
    hsk::InterpFrames fr{};
    const bool own = prev == nullptr;
    fr.prev = own ? c->dA + pair * c->plane : (const uint8_t *)prev;
    fr.curr = own ? c->dB + pair * c->plane : (const uint8_t *)curr;
    fr.prev_stride = own ? c->P : (long long)ps;
    fr.curr_stride = own ? c->P : (long long)cs;
    fr.vis_prev = (const uint8_t *)vp; fr.vis_prev_stride = (long long)vps;
    fr.vis_curr = (const uint8_t *)vc; fr.vis_curr_stride = (long long)vcs;
    return fr;
}

// The host rule: P and F into packed planes (ut, vt of the result in fu[k], fv[k], the state in fs[k]; returns k).
struct InterpHostPlanes {
    std::vector<float> fu[2], fv[2];
    std::vector<uint8_t> fs[2];
};

int interp_host_project(const float *u, size_t us, const float *v, size_t vs, int W, int H, float t, const hsflow_interp_params &ip, const uint8_t *prev, size_t ps,
                        const uint8_t *curr, size_t cs, InterpHostPlanes &hp, hsinterp::Sums *sums)
{
    const size_t px = (size_t)W * H, frow = (size_t)W * 4, brow = (size_t)W;
    std::vector<uint64_t> keys(px);
    for (int k = 0; k < 2; k++) { hp.fu[k].resize(px); hp.fv[k].resize(px); hp.fs[k].resize(px); }
    if (ip.channels == 1) hsinterp::project_rows<1>(u, us, v, vs, W, H, t, prev, ps, curr, cs, keys.data(), hp.fu[0].data(), hp.fv[0].data(), hp.fs[0].data(), sums);
    else hsinterp::project_rows<3>(u, us, v, vs, W, H, t, prev, ps, curr, cs, keys.data(), hp.fu[0].data(), hp.fv[0].data(), hp.fs[0].data(), sums);
    for (int j = 1; j <= ip.fill_passes; j++) {
        const int a = (j - 1) & 1, b = j & 1;
        hsmed::Sums ms = {0, 0, 0, 0, 0};
        hsmed::median_rows(ip.fill_radius, hp.fu[a].data(), frow, hp.fv[a].data(), frow, hp.fs[a].data(), brow, W, H, 1, ip.fill_min_votes, hp.fu[b].data(),
                           hp.fv[b].data(), frow, hp.fs[b].data(), brow, &ms);
        sums->unfilled = (uint32_t)ms.unfilled;
    }
    return ip.fill_passes & 1;
}

} // namespace

extern "C" {

void hsflow_default_interp_params(hsflow_interp_params *ip)
{
    if (!ip) return;
    std::memset(ip, 0, sizeof(*ip));
    ip->struct_size = sizeof(*ip);
    ip->channels = 1;
    ip->fill_radius = 1;
    ip->fill_min_votes = 1;
    ip->fill_passes = 4;
}

int hsflow_project_flow_host(const float *u, size_t u_stride, const float *v, size_t v_stride, int width, int height, float t, const hsflow_interp_params *ip,
                             const uint8_t *prev, size_t prev_stride, const uint8_t *curr, size_t curr_stride, float *u_out, float *v_out, size_t out_stride,
                             uint8_t *state_out, size_t state_out_stride, hsflow_interp_stats *stats)
{
    int st = check_interp_params(nullptr, ip);
    if (st) return st;
    if ((st = check_interp_time(nullptr, t))) return st;
    if (!u || !v || !prev || !curr) return fail(nullptr, HSFLOW_E_ARG, "hsflow_project_flow_host: null pointer");
    if (width < 1 || height < 1) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_project_flow_host: width and height must be positive");
    if (u_stride < (size_t)width * 4 || v_stride < (size_t)width * 4 || ((u_stride | v_stride) & 3u))
        return fail(nullptr, HSFLOW_E_SIZE, "hsflow_project_flow_host: flow stride smaller than 4*width or no multiple of 4");
    if ((st = check_interp_frames(nullptr, ip, width, false, true, prev_stride, curr_stride))) return st;
    if ((st = check_project_planes(nullptr, width, u_out != nullptr, v_out != nullptr, out_stride, state_out != nullptr, state_out_stride, stats != nullptr))) return st;
    if ((u_out && (u_out == u || u_out == v || v_out == u || v_out == v || u_out == v_out))) return fail(nullptr, HSFLOW_E_ARG, "hsflow_project_flow_host: an output is an input");
    InterpHostPlanes hp;
    hsinterp::Sums sums;
    std::memset(&sums, 0, sizeof(sums));
    const int k = interp_host_project(u, u_stride, v, v_stride, width, height, t, *ip, prev, prev_stride, curr, curr_stride, hp, &sums);
    for (int y = 0; y < height; y++) {
        if (u_out) {
            std::memcpy((uint8_t *)u_out + (size_t)y * out_stride, hp.fu[k].data() + (size_t)y * width, (size_t)width * 4);
            std::memcpy((uint8_t *)v_out + (size_t)y * out_stride, hp.fv[k].data() + (size_t)y * width, (size_t)width * 4);
        }
        if (state_out) std::memcpy(state_out + (size_t)y * state_out_stride, hp.fs[k].data() + (size_t)y * width, (size_t)width);
    }
    if (stats) std::memcpy(stats, &sums, sizeof(*stats));
    return HSFLOW_OK;
}

int hsflow_interp_host(const float *u, size_t u_stride, const float *v, size_t v_stride, int width, int height, float t, const hsflow_interp_params *ip,
                       const uint8_t *prev, size_t prev_stride, const uint8_t *curr, size_t curr_stride, const uint8_t *vis_prev, size_t vis_prev_stride,
                       const uint8_t *vis_curr, size_t vis_curr_stride, const uint8_t *ref, size_t ref_stride, uint8_t *dst, size_t dst_stride, uint8_t *cls,
                       size_t cls_stride, hsflow_interp_stats *stats)
{
    int st = check_interp_params(nullptr, ip);
    if (st) return st;
    if ((st = check_interp_time(nullptr, t))) return st;
    if (!u || !v || !prev || !curr) return fail(nullptr, HSFLOW_E_ARG, "hsflow_interp_host: null pointer");
    if (width < 1 || height < 1) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_interp_host: width and height must be positive");
    if (u_stride < (size_t)width * 4 || v_stride < (size_t)width * 4 || ((u_stride | v_stride) & 3u))
        return fail(nullptr, HSFLOW_E_SIZE, "hsflow_interp_host: flow stride smaller than 4*width or no multiple of 4");
    if ((st = check_interp_frames(nullptr, ip, width, false, true, prev_stride, curr_stride))) return st;
    if ((st = check_interp_pictures(nullptr, ip, width, vis_prev != nullptr, vis_prev_stride, vis_curr != nullptr, vis_curr_stride, ref != nullptr, ref_stride,
                                    dst != nullptr, dst_stride, cls != nullptr, cls_stride, stats != nullptr)))
        return st;
    const void *const in[5] = {prev, curr, vis_prev, vis_curr, ref};
    if (interp_is_input(dst, in) || interp_is_input(cls, in) || (dst && dst == cls)) return fail(nullptr, HSFLOW_E_ARG, "hsflow_interp_host: a destination is an input");
    InterpHostPlanes hp;
    hsinterp::Sums sums;
    std::memset(&sums, 0, sizeof(sums));
    const int k = interp_host_project(u, u_stride, v, v_stride, width, height, t, *ip, prev, prev_stride, curr, curr_stride, hp, &sums);
    if (ip->channels == 1)
        hsinterp::blend_rows<1>(hp.fu[k].data(), hp.fv[k].data(), width, height, t, prev, prev_stride, curr, curr_stride, vis_prev, vis_prev_stride, vis_curr,
                                vis_curr_stride, ref, ref_stride, dst, dst_stride, cls, cls_stride, &sums);
    else
        hsinterp::blend_rows<3>(hp.fu[k].data(), hp.fv[k].data(), width, height, t, prev, prev_stride, curr, curr_stride, vis_prev, vis_prev_stride, vis_curr,
                                vis_curr_stride, ref, ref_stride, dst, dst_stride, cls, cls_stride, &sums);
    if (stats) std::memcpy(stats, &sums, sizeof(*stats));
    return HSFLOW_OK;
}

int hsflow_interp_batch_device(hsflow_ctx *c, int pair, int n, const float *t, const hsflow_interp_params *ip, const void *d_prev, size_t prev_stride,
                               const void *d_curr, size_t curr_stride, const void *d_vis_prev, size_t vis_prev_stride, const void *d_vis_curr, size_t vis_curr_stride,
                               const void *const *d_ref, size_t ref_stride, void *const *d_dst, size_t dst_stride, void *const *d_cls, size_t cls_stride,
                               hsflow_interp_stats *d_stats)
{
    int st = check_ctx(c, pair), maxb = 0;
    if (st) return st;
    if (n < 1) return fail(c, HSFLOW_E_ARG, "a batch needs at least one time");
    if ((st = check_interp_params(c, ip))) return st;
    if (!t) return fail(c, HSFLOW_E_ARG, "null list of times");
    for (int i = 0; i < n; i++)
        if ((st = check_interp_time(c, t[i]))) return st;
    const bool own = d_prev == nullptr;
    if ((st = check_interp_frames(c, ip, c->W, own, d_curr != nullptr, prev_stride, curr_stride))) return st;
    if ((st = check_interp_pictures(c, ip, c->W, d_vis_prev != nullptr, vis_prev_stride, d_vis_curr != nullptr, vis_curr_stride, d_ref != nullptr, ref_stride,
                                    d_dst != nullptr, dst_stride, d_cls != nullptr, cls_stride, d_stats != nullptr)))
        return st;
    for (int i = 0; i < n; i++) {
        if ((d_ref && !d_ref[i]) || (d_dst && !d_dst[i]) || (d_cls && !d_cls[i])) return fail(c, HSFLOW_E_ARG, "time " + std::to_string(i) + ": null picture pointer");
        const void *const in[5] = {d_prev, d_curr, d_vis_prev, d_vis_curr, d_ref ? d_ref[i] : nullptr};
        if ((d_dst && interp_is_input(d_dst[i], in)) || (d_cls && interp_is_input(d_cls[i], in)) || (d_dst && d_cls && d_dst[i] == d_cls[i]))
            return fail(c, HSFLOW_E_ARG, "time " + std::to_string(i) + ": a destination is an input");
    }
    if (((uintptr_t)d_stats & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the statistics records must be 8-byte aligned");
    if ((st = interp_check_batch_max(c, &maxb))) return st;
    if ((st = settle_pending(c))) return st; // (hs_postops.hip.h, rule 1)
    if (own && (st = resolve_lazy_frames(c, false))) return st;
    InterpJob job;
    job.pair = pair; job.n = n; job.t = t; job.ip = ip;
    job.fr = interp_frames(c, pair, d_prev, prev_stride, d_curr, curr_stride, d_vis_prev, vis_prev_stride, d_vis_curr, vis_curr_stride);
    job.ref = d_ref; job.ref_stride = ref_stride;
    job.dst = d_dst; job.dst_stride = dst_stride;
    job.cls = d_cls; job.cls_stride = cls_stride;
    job.d_stats = d_stats;
    return enqueue_interp(c, job, maxb);
}

int hsflow_interp_device(hsflow_ctx *c, int pair, float t, const hsflow_interp_params *ip, const void *d_prev, size_t prev_stride, const void *d_curr,
                         size_t curr_stride, const void *d_vis_prev, size_t vis_prev_stride, const void *d_vis_curr, size_t vis_curr_stride, const void *d_ref,
                         size_t ref_stride, void *d_dst, size_t dst_stride, void *d_cls, size_t cls_stride, hsflow_interp_stats *d_stats)
{
    const void *const ref[1] = {d_ref};
    void *const dst[1] = {d_dst}, *const cls[1] = {d_cls};
    return hsflow_interp_batch_device(c, pair, 1, &t, ip, d_prev, prev_stride, d_curr, curr_stride, d_vis_prev, vis_prev_stride, d_vis_curr, vis_curr_stride,
                                      d_ref ? ref : nullptr, ref_stride, d_dst ? dst : nullptr, dst_stride, d_cls ? cls : nullptr, cls_stride, d_stats);
}

int hsflow_project_flow_device(hsflow_ctx *c, int pair, float t, const hsflow_interp_params *ip, const void *d_prev, size_t prev_stride, const void *d_curr,
                               size_t curr_stride, void *d_u_out, void *d_v_out, size_t out_stride, void *d_state_out, size_t state_out_stride,
                               hsflow_interp_stats *d_stats)
{
    int st = check_ctx(c, pair), maxb = 0;
    if (st) return st;
    if ((st = check_interp_params(c, ip))) return st;
    if ((st = check_interp_time(c, t))) return st;
    const bool own = d_prev == nullptr;
    if ((st = check_interp_frames(c, ip, c->W, own, d_curr != nullptr, prev_stride, curr_stride))) return st;
    if ((st = check_project_planes(c, c->W, d_u_out != nullptr, d_v_out != nullptr, out_stride, d_state_out != nullptr, state_out_stride, d_stats != nullptr))) return st;
    if ((((uintptr_t)d_u_out | (uintptr_t)d_v_out) & 3u) != 0) return fail(c, HSFLOW_E_ARG, "the output flow planes must be 4-byte aligned");
    if (((uintptr_t)d_stats & 7u) != 0) return fail(c, HSFLOW_E_ARG, "the statistics records must be 8-byte aligned");
    {
        const size_t frow = (size_t)c->W * 4, brow = (size_t)c->W, pitchb = (size_t)c->P * 4;
        const MedSpan out[3] = {med_span(d_u_out, out_stride, frow, c->H), med_span(d_v_out, out_stride, frow, c->H), med_span(d_state_out, state_out_stride, brow, c->H)};
        if (med_overlap(out[0], out[1])) return fail(c, HSFLOW_E_ARG, "the two output flow planes overlap");
        for (int b = 0; b < 2; b++) {
            const MedSpan in[3] = {med_span(c->dU[b] + (long long)pair * c->plane, pitchb, frow, c->H), med_span(c->dV[b] + (long long)pair * c->plane, pitchb, frow, c->H),
                                   MedSpan{0, 0}};
            for (const MedSpan &o : out)
                for (const MedSpan &i : in)
                    if (med_overlap(o, i)) return fail(c, HSFLOW_E_ARG, "an output of the projection may not overlap the pair's flow");
        }
    }
    if ((st = interp_check_batch_max(c, &maxb))) return st;
    if ((st = settle_pending(c))) return st; // (hs_postops.hip.h, rule 1)
    if (own && (st = resolve_lazy_frames(c, false))) return st;
    InterpJob job;
    job.pair = pair; job.n = 1; job.t = &t; job.ip = ip;
    job.fr = interp_frames(c, pair, d_prev, prev_stride, d_curr, curr_stride, nullptr, 0, nullptr, 0);
    job.d_stats = d_stats;
    job.project = true;
    job.u_out = (float *)d_u_out; job.v_out = (float *)d_v_out; job.out_stride = out_stride;
    job.state_out = (uint8_t *)d_state_out; job.state_out_stride = state_out_stride;
    return enqueue_interp(c, job, maxb);
}

int hsflow_interp(hsflow_ctx *c, int pair, float t, const hsflow_interp_params *ip, const uint8_t *prev, size_t prev_stride, const uint8_t *curr, size_t curr_stride,
                  const uint8_t *vis_prev, size_t vis_prev_stride, const uint8_t *vis_curr, size_t vis_curr_stride, const uint8_t *ref, size_t ref_stride,
                  uint8_t *dst, size_t dst_stride, uint8_t *cls, size_t cls_stride, hsflow_interp_stats *stats)
{
    int st = check_ctx(c, pair), maxb = 0;
    if (st) return st;
    if ((st = check_interp_params(c, ip))) return st;
    if ((st = check_interp_time(c, t))) return st;
    const bool own = prev == nullptr;
    if ((st = check_interp_frames(c, ip, c->W, own, curr != nullptr, prev_stride, curr_stride))) return st;
    if ((st = check_interp_pictures(c, ip, c->W, vis_prev != nullptr, vis_prev_stride, vis_curr != nullptr, vis_curr_stride, ref != nullptr, ref_stride,
                                    dst != nullptr, dst_stride, cls != nullptr, cls_stride, stats != nullptr)))
        return st;
    const void *const in[5] = {prev, curr, vis_prev, vis_curr, ref};
    if (interp_is_input(dst, in) || interp_is_input(cls, in) || (dst && dst == cls)) return fail(c, HSFLOW_E_ARG, "a destination is an input");
    if ((st = interp_check_batch_max(c, &maxb))) return st;
    if ((st = settle_pending(c))) return st;
    if (own && (st = resolve_lazy_frames(c, false))) return st;
    const size_t rowb = (size_t)c->W * (size_t)ip->channels, brow = (size_t)c->W, bytes = rowb * c->H, bbytes = brow * c->H;
    hsflow_ctx::InterpScratch &w = c->interp;
    // the staging: 0 prev, 1 curr, 2 vis_prev, 3 vis_curr, 4 ref, 5 dst, 6 cls
    const void *host[7] = {prev, curr, vis_prev, vis_curr, ref, dst, cls};
    const size_t need[7] = {bytes, bytes, bbytes, bbytes, bytes, bytes, bbytes}, hstride[5] = {prev_stride, curr_stride, vis_prev_stride, vis_curr_stride, ref_stride};
    const size_t row[7] = {rowb, rowb, brow, brow, rowb, rowb, brow};
    for (int k = 0; k < 7; k++)
        if (host[k] && (st = stage_reserve(c, &w.stage[k], &w.stage_bytes[k], need[k]))) return st;
    if (stats && (st = stats_reserve(c, (void **)&w.dStats, (void **)&w.hStats))) return st;
    if ((st = interp_reserve(c, 1))) return st;
    bool marked = false;
    if ((st = sync_begin(c, &marked))) return st;
    for (int k = 0; k < 5; k++)
        if (host[k]) HS_HIP(c, copy_rows_async(c, w.stage[k], row[k], host[k], hstride[k], row[k], c->H, hipMemcpyHostToDevice));
    const void *const dref[1] = {w.stage[4]};
    void *const ddst[1] = {w.stage[5]}, *const dcls[1] = {w.stage[6]};
    InterpJob job;
    job.pair = pair; job.n = 1; job.t = &t; job.ip = ip;
    job.fr = interp_frames(c, pair, own ? nullptr : w.stage[0], rowb, own ? nullptr : w.stage[1], rowb, vis_prev ? w.stage[2] : nullptr, brow,
                           vis_curr ? w.stage[3] : nullptr, brow);
    job.ref = ref ? dref : nullptr; job.ref_stride = rowb;
    job.dst = dst ? ddst : nullptr; job.dst_stride = rowb;
    job.cls = cls ? dcls : nullptr; job.cls_stride = brow;
    job.d_stats = stats ? w.dStats : nullptr;
    if ((st = enqueue_interp(c, job, maxb))) return st;
    if (dst) HS_HIP(c, copy_rows_async(c, dst, dst_stride, w.stage[5], rowb, rowb, c->H, hipMemcpyDeviceToHost));
    if (cls) HS_HIP(c, copy_rows_async(c, cls, cls_stride, w.stage[6], brow, brow, c->H, hipMemcpyDeviceToHost));
    if (stats && (st = stats_copy_back(c, w.hStats, w.dStats))) return st;
    return sync_finish(c, marked, stats, w.hStats);
}

} // extern "C"
