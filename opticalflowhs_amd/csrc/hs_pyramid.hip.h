// hs_pyramid.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_solve_pyramid, the coarse-to-fine
// driver around the solver that exists (include/hsflow.h has the scheme in full, DESIGN.md 4.17 the reasons).  Level 0 is
// the context itself; every coarser level is a context of its own on the same device and stream, created by the first call
// and kept (HsPyramid).  Every level's solve is solve_impl as hsflow_solve / hsflow_solve_async run it: no solve path knows
// that a pyramid calls it.  Around the solves: k_pyr_down per level, k_pyr_step in front of every step but the first,
// k_pyr_total behind a level's last step (hs_kernels_pyramid.hip.h), and with median_radius the FILTER pass of
// hs_median.hip.h (enqueue_median_chunk) from the level's current flow buffer into its other one.
// Ordering (hs_postops.hip.h): under ITER everything is enqueued in stream order and nothing is waited for; with EPS each
// solve runs synchronously, so its flow is final before k_pyr_total / k_pyr_step read it (rule 1); last_marked is false
// behind the call (rule 2).
// A context that never calls hsflow_solve_pyramid allocates and launches nothing here.
#pragma once

struct HsPyramid {
    int levels = 0;
    int W[hspyr::kMaxLevels] = {}, H[hspyr::kMaxLevels] = {};
    hsflow_ctx *lv[hspyr::kMaxLevels] = {};  // lv[0]: the owner itself; the others are owned
    uint8_t *curr[hspyr::kMaxLevels] = {};   // each level's second frame as `down` made it (level 0: a copy of the context's)
    float *u0[hspyr::kMaxLevels] = {}, *v0[hspyr::kMaxLevels] = {}; // the base flow of the step in hand
    hsflow_pyramid_info info;
    bool ran = false;                        // info belongs to a solve
};

namespace {

static_assert(HSFLOW_PYRAMID_MAX_LEVELS == hspyr::kMaxLevels && HSFLOW_PYRAMID_MAX_WARPS == hspyr::kMaxWarps, "the header's constants are the rule's");
static_assert(sizeof(hsflow_pyramid_params) == 20, "hsflow_pyramid_params is 20 bytes");
constexpr int kVstatePyramid = 3; // hsflow_ctx::vstate: the last solve was a pyramid solve (hsflow_verify refuses)

int check_pyramid_params(hsflow_ctx *c, const hsflow_pyramid_params *pp)
{
    if (!pp || pp->struct_size != sizeof(hsflow_pyramid_params)) return fail(c, HSFLOW_E_ARG, "pyramid params null or struct_size mismatch");
    if (pp->levels < 0 || pp->levels > HSFLOW_PYRAMID_MAX_LEVELS) return fail(c, HSFLOW_E_ARG, "pyramid levels must be 0 (auto) .. " + std::to_string(HSFLOW_PYRAMID_MAX_LEVELS));
    if (pp->min_size < 1) return fail(c, HSFLOW_E_ARG, "pyramid min_size must be positive");
    if (pp->warps < 1 || pp->warps > HSFLOW_PYRAMID_MAX_WARPS) return fail(c, HSFLOW_E_ARG, "pyramid warps must be 1 .. " + std::to_string(HSFLOW_PYRAMID_MAX_WARPS));
    if (pp->median_radius < 0 || pp->median_radius > 2) return fail(c, HSFLOW_E_ARG, "pyramid median_radius must be 0, 1 or 2");
    return HSFLOW_OK;
}

int pyramid_plan(hsflow_ctx *c, int W, int H, const hsflow_pyramid_params *pp, int *n, int *widths, int *heights)
{
    const int st = check_pyramid_params(c, pp);
    if (st) return st;
    if (W < 1 || H < 1) return fail(c, HSFLOW_E_SIZE, "width and height must be positive");
    *n = hspyr::plan(W, H, pp->levels, pp->min_size, widths, heights);
    if (!*n) return fail(c, HSFLOW_E_SIZE, "pyramid levels: a level of 1 x 1 pixels cannot be halved");
    return HSFLOW_OK;
}

void pyramid_free_levels(HsPyramid *p)
{
    for (int l = 0; l < hspyr::kMaxLevels; l++) {
        if (l > 0 && p->lv[l]) hsflow_destroy(p->lv[l]);
        p->lv[l] = nullptr;
        hipFree(p->curr[l]); hipFree(p->u0[l]); hipFree(p->v0[l]);
        p->curr[l] = nullptr; p->u0[l] = p->v0[l] = nullptr;
    }
    p->levels = 0;
    p->ran = false;
}

// The level contexts and planes of this plan: kept while the plan stays, made anew when it changes.
int pyramid_reserve(hsflow_ctx *c, int n, const int *W, const int *H)
{
    if (!c->pyr) {
        c->pyr = new (std::nothrow) HsPyramid();
        if (!c->pyr) return fail(c, HSFLOW_E_OOM, "host allocation failed");
    }
    HsPyramid *p = c->pyr;
    bool same = p->levels == n;
    for (int l = 0; same && l < n; l++) same = p->W[l] == W[l] && p->H[l] == H[l];
    if (same) return HSFLOW_OK;
    HS_HIP(c, hipStreamSynchronize(c->stream)); // (the planes of the old plan may still be read)
    pyramid_free_levels(p);
    p->lv[0] = c;
    for (int l = 0; l < n; l++) {
        p->W[l] = W[l]; p->H[l] = H[l];
        if (l > 0) {
            hsflow_ctx *s = nullptr;
            const int st = hsflow_create(&s, c->device, W[l], H[l], c->N, c->stream, 0);
            if (st) { pyramid_free_levels(p); return fail(c, st, "hsflow_solve_pyramid: level " + std::to_string(l) + ": " + g_create_error); }
            // not counted in g_live_ctx, like hsflow_verify's scratch: a counted one would switch the persistent launch off for its owner
            if (s->counted) { g_live_ctx[s->device & 63]--; s->counted = false; }
            p->lv[l] = s;
        }
        const size_t px = (size_t)p->lv[l]->plane * c->N;
        hipError_t e = hipMalloc((void **)&p->curr[l], px);
        if (e == hipSuccess) e = hipMalloc((void **)&p->u0[l], px * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void **)&p->v0[l], px * sizeof(float));
        if (e != hipSuccess) {
            pyramid_free_levels(p);
            return fail(c, e == hipErrorOutOfMemory ? HSFLOW_E_OOM : HSFLOW_E_DEVICE, std::string("hsflow_solve_pyramid: level planes: ") + hipGetErrorString(e));
        }
    }
    p->levels = n;
    return HSFLOW_OK;
}

// One FILTER pass of the median over every pair's total of level L, from its current flow buffer into the other one.
int pyramid_median(hsflow_ctx *c, hsflow_ctx *L, int radius, int *launches)
{
    hsflow_median_params mp;
    hsflow_default_median_params(&mp);
    mp.radius = radius;
    const size_t pitchb = (size_t)L->P * 4;
    for (int first = 0; first < L->N; first += hsk::kMedianBatchMax) {
        const int cnt = std::min(L->N - first, (int)hsk::kMedianBatchMax);
        hsk::MedianBatchFields f{};
        for (int k = 0; k < cnt; k++) {
            const long long o = (long long)(first + k) * L->plane;
            f.u[k] = L->dU[L->cur] + o; f.v[k] = L->dV[L->cur] + o;
            f.u_out[k] = L->dU[L->cur ^ 1] + o; f.v_out[k] = L->dV[L->cur ^ 1] + o;
        }
        const int st = enqueue_median_chunk(L, cnt, mp, f, pitchb, 0, pitchb, 0, nullptr);
        if (st) return L == c ? st : fail(c, st, L->err);
        ++*launches;
    }
    L->cur ^= 1;
    return HSFLOW_OK;
}

// The steps of a planned pyramid solve (hsflow_solve_pyramid has checked every argument and settled what was owed).
int pyramid_run(hsflow_ctx *c, const hsflow_params &p, const hsflow_pyramid_params &pp, bool *curr_displaced)
{
    HsPyramid *py = c->pyr;
    const int n = py->levels, N = c->N, med = pp.median_radius;
    const bool eps = (p.term_type & HSFLOW_TERM_EPS) != 0;
    hsflow_pyramid_info &inf = py->info;
    std::memset(&inf, 0, sizeof(inf));
    inf.struct_size = sizeof(inf);
    inf.levels = n; inf.warps = pp.warps; inf.median_radius = med;
    for (int l = 0; l < n; l++) { inf.width[l] = py->W[l]; inf.height[l] = py->H[l]; }
    py->ran = false;
    hsflow_params q = p;
    q.use_previous = 0;
    q.reuse_derivatives = 0;
    // 1. the frames: level 0's second frame is kept aside (the steps of level 0 put the warped frame in its place)
    if (n > 1 || pp.warps > 1) {
        HS_HIP(c, hipMemcpyAsync(py->curr[0], c->dB, (size_t)c->plane * N, hipMemcpyDeviceToDevice, c->stream));
        *curr_displaced = true;
    }
    for (int l = 1; l < n; l++) {
        const hsflow_ctx *F = py->lv[l - 1];
        hsflow_ctx *L = py->lv[l];
        HS_HIP(c, hsk::launch_pyr_down(c->stream, N, F->dA, py->curr[l - 1], F->plane, F->P, F->W, F->H, L->dA, py->curr[l], L->plane, L->P));
        inf.down_launches++;
        if (L->cu_share != c->cu_share) { L->cu_share = c->cu_share; L->plan_cache.clear(); }
    }
    if (n > 1) HS_HIP(c, hipMemcpyAsync(py->lv[n - 1]->dB, py->curr[n - 1], (size_t)py->lv[n - 1]->plane * N, hipMemcpyDeviceToDevice, c->stream));
    // 2., 3. the steps, coarsest level first
    for (int l = n - 1; l >= 0; l--) {
        hsflow_ctx *L = py->lv[l];
        for (int k = 1; k <= pp.warps; k++) {
            const bool first = l == n - 1 && k == 1;
            if (!first) {
                const hsflow_ctx *C = k == 1 ? py->lv[l + 1] : L;
                // (the coarsest level's first total is its increment itself: no base planes yet for kPyrSameAdd)
                const int mode = k == 1 ? hsk::kPyrProlong : (med || (l == n - 1 && k == 2)) ? hsk::kPyrSame : hsk::kPyrSameAdd;
                const float *bu = mode == hsk::kPyrSameAdd ? py->u0[l] : C->dU[C->cur], *bv = mode == hsk::kPyrSameAdd ? py->v0[l] : C->dV[C->cur];
                HS_HIP(c, hsk::launch_pyr_step(c->stream, mode, N, bu, bv, L->dU[L->cur], L->dV[L->cur], C->plane, C->P, C->W, C->H, py->u0[l], py->v0[l], py->curr[l], L->dB,
                                               L->plane, L->P, L->W, L->H));
                inf.step_launches++;
            }
            L->frames_set = true;
            L->coef_valid = false;
            const int st = solve_impl(L, &q, !eps);
            if (st) return L == c ? st : fail(c, st, "hsflow_solve_pyramid: level " + std::to_string(l) + ": " + L->err);
            inf.sweeps[l][k - 1] = eps ? L->info.iterations_done : p.max_iter;
            inf.solves++;
            L->lastl.valid = false; // (the increment is about to become the total: its last_eps can no longer be measured)
            if (!first && (med || k == pp.warps)) { // (between the warps of a level the next step adds: kPyrSameAdd)
                HS_HIP(c, hsk::launch_pyr_total(c->stream, N, py->u0[l], py->v0[l], L->dU[L->cur], L->dV[L->cur], L->plane, L->P, L->W, L->H));
                inf.total_launches++;
            }
            if (med) {
                const int sm = pyramid_median(c, L, med, &inf.median_launches);
                if (sm) return sm;
            }
        }
    }
    return HSFLOW_OK;
}

// The level contexts and planes (hsflow_destroy).
void pyramid_release(hsflow_ctx *c)
{
    if (!c->pyr) return;
    pyramid_free_levels(c->pyr);
    delete c->pyr;
    c->pyr = nullptr;
}

} // namespace

extern "C" {

void hsflow_default_pyramid_params(hsflow_pyramid_params *pp)
{
    if (!pp) return;
    std::memset(pp, 0, sizeof(*pp));
    pp->struct_size = sizeof(*pp);
    pp->levels = 0;
    pp->min_size = 32;
    pp->warps = 1;
    pp->median_radius = 0;
}

int hsflow_pyramid_plan(int width, int height, const hsflow_pyramid_params *pp, int *levels, int *widths, int *heights)
{
    if (!levels) return fail(nullptr, HSFLOW_E_ARG, "hsflow_pyramid_plan: levels is null");
    int w[hspyr::kMaxLevels], h[hspyr::kMaxLevels], n = 0;
    const int st = pyramid_plan(nullptr, width, height, pp, &n, w, h);
    if (st) return st;
    *levels = n;
    for (int l = 0; l < hspyr::kMaxLevels; l++) {
        if (widths) widths[l] = l < n ? w[l] : 0;
        if (heights) heights[l] = l < n ? h[l] : 0;
    }
    return HSFLOW_OK;
}

int hsflow_pyramid_down_host(const uint8_t *src, size_t src_stride, int width, int height, uint8_t *dst, size_t dst_stride)
{
    if (!src || !dst) return fail(nullptr, HSFLOW_E_ARG, "hsflow_pyramid_down_host: null plane");
    if (width < 1 || height < 1) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_pyramid_down_host: width and height must be positive");
    if (src_stride < (size_t)width || dst_stride < (size_t)hspyr::half_up(width)) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_pyramid_down_host: stride smaller than a row");
    hspyr::down_rows(src, src_stride, width, height, dst, dst_stride);
    return HSFLOW_OK;
}

int hsflow_pyramid_prolong_host(const float *coarse, size_t coarse_stride, int width, int height, float *dst, size_t dst_stride)
{
    if (!coarse || !dst) return fail(nullptr, HSFLOW_E_ARG, "hsflow_pyramid_prolong_host: null plane");
    if (width < 1 || height < 1) return fail(nullptr, HSFLOW_E_SIZE, "hsflow_pyramid_prolong_host: width and height must be positive");
    if (coarse_stride < (size_t)hspyr::half_up(width) * 4 || dst_stride < (size_t)width * 4 || ((coarse_stride | dst_stride) & 3u))
        return fail(nullptr, HSFLOW_E_SIZE, "hsflow_pyramid_prolong_host: stride smaller than a row or no multiple of 4");
    hspyr::prolong_rows(coarse, coarse_stride, width, height, dst, dst_stride);
    return HSFLOW_OK;
}

int hsflow_solve_pyramid(hsflow_ctx *c, const hsflow_params *p, const hsflow_pyramid_params *pp)
{
    int st = check_ctx(c, 0);
    if (st) return st;
    if (!p || p->struct_size != sizeof(hsflow_params)) return fail(c, HSFLOW_E_ARG, "params null or struct_size mismatch");
    int W[hspyr::kMaxLevels], H[hspyr::kMaxLevels], n = 0;
    if ((st = pyramid_plan(c, c->W, c->H, pp, &n, W, H))) return st;
    if (p->mode != HSFLOW_MODE_CV) return fail(c, HSFLOW_E_ARG, "hsflow_solve_pyramid: HSFLOW_MODE_CV only");
    if (p->use_previous) return fail(c, HSFLOW_E_ARG, "hsflow_solve_pyramid: use_previous is not supported (every level starts from the level above)");
    if (p->profile) return fail(c, HSFLOW_E_ARG, "hsflow_solve_pyramid: profile is not supported");
    if (p->kernel == HSFLOW_KERNEL_PERSIST) return fail(c, HSFLOW_E_ARG, "hsflow_solve_pyramid: HSFLOW_KERNEL_PERSIST is not supported");
    if (c->borrowed) return fail(c, HSFLOW_E_ARG, "hsflow_solve_pyramid: not on a verify scratch context");
    const bool eps = (p->term_type & HSFLOW_TERM_EPS) != 0;
    if ((st = check_solve_args(c, *p, false))) return st;
    if (!c->frames_set) return fail(c, HSFLOW_E_STATE, "frames were not set");
    if (c->org != 0 || eps_windowed(c)) return fail(c, HSFLOW_E_STATE, "hsflow_solve_pyramid: a row origin or an Eps row window is set on this context");
    if (c->per_pair && eps && c->N > 1)
        return fail(c, HSFLOW_E_STATE, "hsflow_solve_pyramid: hsflow_set_pair_termination with EPS termination on a batch: the pairs of a level stop together");
    if (2LL * c->N > c->max_grid_z) return fail(c, HSFLOW_E_SIZE, "hsflow_solve_pyramid: too many pairs for one launch per level");
    if ((st = settle_pending(c))) return st; // an unverified asynchronous solve still needs the old inputs
    if ((st = pyramid_reserve(c, n, W, H))) return st;
    bool displaced = false;
    st = pyramid_run(c, *p, *pp, &displaced);
    // 5. the context's second frame is the caller's again; frames and flow count as changed behind the solver's back
    if (displaced) {
        const hipError_t e = hipMemcpyAsync(c->dB, c->pyr->curr[0], (size_t)c->plane * c->N, hipMemcpyDeviceToDevice, c->stream);
        if (e != hipSuccess && !st) st = fail(c, HSFLOW_E_DEVICE, std::string("hsflow_solve_pyramid: restoring the second frame: ") + hipGetErrorString(e));
    }
    c->coef_valid = false;
    c->lastl.valid = false;
    c->flow_tame = false;
    c->flow_after_mark = true;
    c->last_marked = false;
    c->vstate = st ? 2 : kVstatePyramid;
    c->last_status = st;
    if (!st) c->pyr->ran = true;
    return st;
}

int hsflow_get_pyramid_info(hsflow_ctx *c, hsflow_pyramid_info *out)
{
    if (!c) return fail(nullptr, HSFLOW_E_ARG, "null context");
    if (!out || out->struct_size != sizeof(hsflow_pyramid_info)) return fail(c, HSFLOW_E_ARG, "hsflow_get_pyramid_info: out null or struct_size mismatch");
    if (!c->pyr || !c->pyr->ran) return fail(c, HSFLOW_E_STATE, "hsflow_get_pyramid_info: no pyramid solve yet on this context");
    *out = c->pyr->info;
    return HSFLOW_OK;
}

int hsflow_pyramid_get_level(hsflow_ctx *c, int level, int pair, uint8_t *prev, size_t prev_stride, uint8_t *curr, size_t curr_stride, float *u, size_t u_stride,
                             float *v, size_t v_stride)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!c->pyr || !c->pyr->ran || c->vstate != kVstatePyramid)
        return fail(c, HSFLOW_E_STATE, "hsflow_pyramid_get_level: the last solve of this context was not a pyramid solve");
    const HsPyramid *py = c->pyr;
    if (level < 0 || level >= py->levels) return fail(c, HSFLOW_E_ARG, "hsflow_pyramid_get_level: level out of range");
    const hsflow_ctx *L = py->lv[level];
    const size_t brow = (size_t)L->W, frow = brow * 4;
    if ((prev && prev_stride < brow) || (curr && curr_stride < brow)) return fail(c, HSFLOW_E_SIZE, "frame stride smaller than the level's width");
    if ((u && (u_stride < frow || (u_stride & 3u))) || (v && (v_stride < frow || (v_stride & 3u))))
        return fail(c, HSFLOW_E_SIZE, "flow stride must be a multiple of 4 and >= 4 * the level's width");
    if ((st = settle_pending(c))) return st;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    const long long o = (long long)pair * L->plane;
    const uint8_t *dcurr = level == 0 ? c->dB : py->curr[level]; // (level 0's is the context's own again)
    if (prev) HS_HIP(c, hipMemcpy2D(prev, prev_stride, L->dA + o, (size_t)L->P, brow, L->H, hipMemcpyDeviceToHost));
    if (curr) HS_HIP(c, hipMemcpy2D(curr, curr_stride, dcurr + o, (size_t)L->P, brow, L->H, hipMemcpyDeviceToHost));
    if (u) HS_HIP(c, hipMemcpy2D(u, u_stride, L->dU[L->cur] + o, (size_t)L->P * 4, frow, L->H, hipMemcpyDeviceToHost));
    if (v) HS_HIP(c, hipMemcpy2D(v, v_stride, L->dV[L->cur] + o, (size_t)L->P * 4, frow, L->H, hipMemcpyDeviceToHost));
    return HSFLOW_OK;
}

} // extern "C"
