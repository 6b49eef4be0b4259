// hs_verify.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): hsflow_verify, the verifyResults()
// the reference left a stub (HSOpticalFlowOpenCL.cpp:894), hsflow_compare_flow_device and hsflow_compare_planes_host.
// The reference pass is the library's own plainest path -- stand-alone derivative kernel, one sweep per launch, no
// graph -- run by a second context object that borrows the owner's frames and stream and owns flow and coefficient
// planes of its own; the comparison is k_plane_compare (hs_kernels_verify.hip.h).  A context that never verifies
// allocates and launches nothing here.
#pragma once

namespace {

// Records of k_plane_compare on the device and their page-locked copy, and the event behind that copy.
int cmp_reserve(hsflow_ctx *c, int records)
{
    if (!c->evVerify) HS_HIP(c, hipEventCreateWithFlags(&c->evVerify, hipEventDisableTiming));
    if (c->cmp_cap >= records) return HSFLOW_OK;
    HS_HIP(c, hipStreamSynchronize(c->stream));
    hipFree(c->dCmp);
    if (c->hCmp) hipHostFree(c->hCmp);
    c->dCmp = c->hCmp = nullptr; c->cmp_cap = 0;
    const size_t bytes = (size_t)records * hsk::kCmpRecWords * sizeof(unsigned long long);
    HS_HIP(c, hipMalloc((void **)&c->dCmp, bytes));
    HS_HIP(c, hipHostMalloc((void **)&c->hCmp, bytes, hipHostMallocDefault));
    c->cmp_cap = records;
    return HSFLOW_OK;
}

// One comparison of two W x H planes of 32-bit elements into record `rec`, enqueued on c's stream.  Every element read
// lies inside [0, W) x [0, H) of its plane; the caller has checked the strides.
int cmp_enqueue(hsflow_ctx *c, bool words, const void *a, size_t as, const void *b, size_t bs, int rec)
{
    const int cbs = (c->W + hsk::kCmpChunk - 1) / hsk::kCmpChunk;
    const unsigned nchunks = (unsigned)((long long)cbs * c->H); // <= plane <= 2^30
    const int vec = (((uintptr_t)a | (uintptr_t)b | as | bs) & 15u) == 0;
    // eight workgroups of 256 lanes fill a CU; fewer where the plane has fewer chunks
    const unsigned grid = std::min(nchunks, (unsigned)std::max(1, c->num_cu) * 8u);
    unsigned long long *r = c->dCmp + (size_t)rec * hsk::kCmpRecWords;
    if (words)
        hipLaunchKernelGGL(hsk::k_plane_compare<true>, dim3(grid), dim3(hsk::kCmpThreads), 0, c->stream, (const char *)a, (long long)as,
                           (const char *)b, (long long)bs, c->W, c->H, cbs, nchunks, vec, r);
    else
        hipLaunchKernelGGL(hsk::k_plane_compare<false>, dim3(grid), dim3(hsk::kCmpThreads), 0, c->stream, (const char *)a, (long long)as,
                           (const char *)b, (long long)bs, c->W, c->H, cbs, nchunks, vec, r);
    HS_HIP(c, hipGetLastError());
    return HSFLOW_OK;
}

int cmp_clear(hsflow_ctx *c, int records)
{
    HS_HIP(c, hipMemsetAsync(c->dCmp, 0, (size_t)records * hsk::kCmpRecWords * sizeof(unsigned long long), c->stream));
    return HSFLOW_OK;
}

// The records back in one small copy; waits for the event behind it -- for what THIS context enqueued, not for what other
// contexts have queued on a shared stream since.
int cmp_fetch(hsflow_ctx *c, int records)
{
    HS_HIP(c, hipMemcpyAsync(c->hCmp, c->dCmp, (size_t)records * hsk::kCmpRecWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HS_HIP(c, hipEventRecord(c->evVerify, c->stream));
    HS_HIP(c, hipEventSynchronize(c->evVerify));
    return HSFLOW_OK;
}

hsflow_plane_diff cmp_record(const hsflow_ctx *c, int rec)
{
    const unsigned long long *r = c->hCmp + (size_t)rec * hsk::kCmpRecWords;
    hsflow_plane_diff d;
    d.differing = r[0]; d.failing = r[1]; d.nonfinite = r[2];
    d.first_failing = r[3] ? (int64_t)~r[3] : -1; // the kernel keeps the complement under atomicMax
    const uint32_t abs_bits = (uint32_t)(r[4] & 0xFFFFFFFFull);
    d.max_abs_diff = hsverify::as_float(abs_bits);
    d.max_ulp = (uint32_t)(r[4] >> 32);
    return d;
}

// sums, maxima, and the first failing index of the LOWEST pair that has one (pairs are visited in ascending order)
void cmp_merge(hsflow_plane_diff &into, const hsflow_plane_diff &d)
{
    into.differing += d.differing; into.failing += d.failing; into.nonfinite += d.nonfinite;
    if (into.first_failing < 0) into.first_failing = d.first_failing;
    into.max_abs_diff = std::max(into.max_abs_diff, d.max_abs_diff);
    into.max_ulp = std::max(into.max_ulp, d.max_ulp);
}

int check_plane_arg(hsflow_ctx *c, const void *p, size_t stride)
{
    if (((uintptr_t)p & 3u) || (stride & 3u) || stride < (size_t)c->W * 4)
        return fail(c, HSFLOW_E_SIZE, "planes must be 4-byte aligned, their stride a multiple of 4 and >= 4*width");
    return HSFLOW_OK;
}

// The reference pass's context: sizes, device, stream and FRAMES of its owner, flow and coefficient planes of its own.
// Not counted in g_live_ctx (a counted one would switch the persistent launch off for its owner).
int verify_reserve(hsflow_ctx *c)
{
    if (c->shadow) return HSFLOW_OK;
    hsflow_ctx *s = new (std::nothrow) hsflow_ctx();
    if (!s) return fail(c, HSFLOW_E_OOM, "host allocation failed");
    s->borrowed = true;
    s->device = c->device; s->W = c->W; s->H = c->H; s->N = c->N; s->P = c->P; s->plane = c->plane;
    s->stream = c->stream; s->own_stream = false;
    s->dA = c->dA; s->dB = c->dB;
    s->num_cu = c->num_cu; s->max_grid_z = c->max_grid_z;
    std::memset(&s->info, 0, sizeof(s->info));
    s->info.struct_size = sizeof(hsflow_info);
    s->info.width = c->W; s->info.height = c->H; s->info.n_pairs = c->N; s->info.pitch = c->P;
    const size_t px = (size_t)c->plane * c->N;
    hipError_t e = hipMalloc((void **)&s->dCoef, px * sizeof(uint32_t));
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = hipMalloc((void **)&s->dU[i], px * sizeof(float));
        if (e == hipSuccess) e = hipMalloc((void **)&s->dV[i], px * sizeof(float));
    }
    if (e == hipSuccess) e = hipMalloc((void **)&s->dEps, kMaxFuse * sizeof(unsigned));
    if (e == hipSuccess) e = hipMalloc((void **)&s->dZero, ((size_t)c->P + 64) * sizeof(float));
    // deterministic contents for padding columns, as hsflow_create
    if (e == hipSuccess) e = hipMemsetAsync(s->dZero, 0, ((size_t)c->P + 64) * sizeof(float), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(s->dCoef, 0, px * sizeof(uint32_t), c->stream);
    for (int i = 0; i < 2 && e == hipSuccess; i++) {
        e = hipMemsetAsync(s->dU[i], 0, px * sizeof(float), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(s->dV[i], 0, px * sizeof(float), c->stream);
    }
    if (e != hipSuccess) {
        hsflow_destroy(s);
        return fail(c, e == hipErrorOutOfMemory ? HSFLOW_E_OOM : HSFLOW_E_DEVICE,
                    std::string("hsflow_verify: scratch for the reference pass: ") + hipGetErrorString(e));
    }
    s->frames_set = true;
    c->shadow = s;
    return HSFLOW_OK;
}

} // namespace

extern "C" {

int hsflow_compare_planes_host(const float *a, size_t as, const float *b, size_t bs, int width, int height, hsflow_plane_diff *out)
{
    if (!a || !b || !out) return fail(nullptr, HSFLOW_E_ARG, "hsflow_compare_planes_host: null pointer");
    if (width <= 0 || height <= 0 || (as & 3u) || (bs & 3u) || as < (size_t)width * 4 || bs < (size_t)width * 4)
        return fail(nullptr, HSFLOW_E_SIZE, "hsflow_compare_planes_host: size must be positive, strides multiples of 4 and >= 4*width");
    hsflow_plane_diff d;
    std::memset(&d, 0, sizeof(d));
    d.first_failing = -1;
    uint32_t max_abs = 0u;
    for (int y = 0; y < height; y++) {
        const char *ra = (const char *)a + (size_t)y * as, *rb = (const char *)b + (size_t)y * bs;
        for (int x = 0; x < width; x++) {
            uint32_t wa, wb;
            std::memcpy(&wa, ra + (size_t)x * 4, 4);
            std::memcpy(&wb, rb + (size_t)x * 4, 4);
            const hsverify::Elem e = hsverify::classify(wa, wb);
            d.nonfinite += e.nonfinite ? 1u : 0u;
            if (!e.differing) continue;
            d.differing++;
            if (e.measured) {
                max_abs = std::max(max_abs, hsverify::as_bits(e.abs_diff));
                d.max_ulp = std::max(d.max_ulp, e.ulp);
            }
            if (e.failing) {
                d.failing++;
                if (d.first_failing < 0) d.first_failing = (int64_t)y * width + x;
            }
        }
    }
    d.max_abs_diff = hsverify::as_float(max_abs);
    *out = d;
    return HSFLOW_OK;
}

int hsflow_compare_flow_device(hsflow_ctx *c, int pair, const void *du, size_t us, const void *dv, size_t vs, hsflow_plane_diff *u,
                               hsflow_plane_diff *v)
{
    int st = check_ctx(c, pair);
    if (st) return st;
    if (!du || !dv || !u || !v) return fail(c, HSFLOW_E_ARG, "hsflow_compare_flow_device: null pointer");
    if ((st = check_plane_arg(c, du, us)) || (st = check_plane_arg(c, dv, vs))) return st;
    // a flow that a re-run would change is not worth comparing: an owed ITER|EPS check is settled first
    if ((st = settle_pending(c))) return st;
    if ((st = cmp_reserve(c, 2)) || (st = cmp_clear(c, 2))) return st;
    const size_t pb = (size_t)c->P * sizeof(float);
    if ((st = cmp_enqueue(c, false, c->dU[c->cur] + pair * c->plane, pb, du, us, 0))) return st;
    if ((st = cmp_enqueue(c, false, c->dV[c->cur] + pair * c->plane, pb, dv, vs, 1))) return st;
    if ((st = cmp_fetch(c, 2))) return st;
    *u = cmp_record(c, 0);
    *v = cmp_record(c, 1);
    return check_persist(c);
}

int hsflow_verify(hsflow_ctx *c, int pair, hsflow_verify_report *report)
{
    if (!c) return fail(nullptr, HSFLOW_E_ARG, "null context");
    if (!report || report->struct_size != sizeof(hsflow_verify_report)) return fail(c, HSFLOW_E_ARG, "hsflow_verify: report null or struct_size mismatch");
    if (pair < -1 || pair >= c->N) return fail(c, HSFLOW_E_ARG, "hsflow_verify: pair must be -1 (all) or an index below n_pairs");
    int st = check_ctx(c, 0);
    if (st) return st;
    if (c->borrowed) return fail(c, HSFLOW_E_ARG, "hsflow_verify: not on a verify scratch context");
    if ((st = settle_pending(c))) return st;
    if (c->persist_unchecked) { // an asynchronous persistent launch may have given up: its flow would be invalid
        HS_HIP(c, hipStreamSynchronize(c->stream));
        if ((st = check_persist(c))) return st;
    }
    if (c->vstate == 0) return fail(c, HSFLOW_E_STATE, "hsflow_verify: no solve yet on this context");
    if (c->vstate == 2) return fail(c, HSFLOW_E_STATE, "hsflow_verify: the last solve failed (or ended in HSFLOW_E_NOTERM): there is nothing to verify");
    if (c->vstate == 3) return fail(c, HSFLOW_E_STATE, "hsflow_verify: the last solve was a pyramid solve: the flow held is no single solve of the context's frames");
    if (c->vparams.use_previous)
        return fail(c, HSFLOW_E_STATE, "hsflow_verify: the last solve continued from an earlier flow (use_previous = 1); that starting flow is gone, "
                                       "warm starts cannot be verified");
    if (!c->frames_set || !c->coef_valid)
        return fail(c, HSFLOW_E_STATE, "hsflow_verify: frames were set or pushed since the last solve; the flow held belongs to other frames");
    if ((st = verify_reserve(c))) return st;
    hsflow_ctx *s = c->shadow;
    if (s->org != c->v_org || s->eps_row0 != c->v_eps_row0 || s->eps_rows != c->v_eps_rows) { // as the solve under test ran
        s->org = c->v_org; s->eps_row0 = c->v_eps_row0; s->eps_rows = c->v_eps_rows;
        s->plan_cache.clear();
    }
    // the plainest path: one sweep per launch behind the stand-alone derivative kernel, from zero flow, launch by launch
    hsflow_params q = c->vparams;
    q.kernel = HSFLOW_KERNEL_SIMPLE;
    q.fuse_steps = q.tile_w = q.tile_h = q.threads = q.strip_rows = 0;
    q.use_previous = q.reuse_derivatives = q.use_graph = q.profile = 0;
    s->coef_valid = false;
    s->per_pair = c->v_per_pair; // every pair's own stopping sweep, from the one-sweep kernel's Eps of that pair alone
    if ((st = solve_impl(s, &q, false))) return fail(c, st, "hsflow_verify: the reference pass failed: " + s->err);
    const int first = pair < 0 ? 0 : pair, count = pair < 0 ? c->N : 1;
    if ((st = cmp_reserve(c, 3 * count)) || (st = cmp_clear(c, 3 * count))) return st;
    const size_t pb = (size_t)c->P * sizeof(float);
    for (int k = 0; k < count; k++) {
        const long long o = (long long)(first + k) * c->plane;
        if ((st = cmp_enqueue(c, false, c->dU[c->cur] + o, pb, s->dU[s->cur] + o, pb, 3 * k))) return st;
        if ((st = cmp_enqueue(c, false, c->dV[c->cur] + o, pb, s->dV[s->cur] + o, pb, 3 * k + 1))) return st;
        if ((st = cmp_enqueue(c, true, c->dCoef + o, pb, s->dCoef + o, pb, 3 * k + 2))) return st;
    }
    if ((st = cmp_fetch(c, 3 * count))) return st;
    hsflow_verify_report r;
    std::memset(&r, 0, sizeof(r));
    r.struct_size = sizeof(r);
    r.pair = pair;
    // sweeps per pair where the pairs stop each on its own, else the batch's for every pair
    auto done = [](const hsflow_ctx *x, int i) { return x->pair_res_valid ? x->pair_res[(size_t)i].iterations_done : x->info.iterations_done; };
    bool counts_agree = true;
    if (pair >= 0) {
        r.iterations_done = done(c, pair);
        r.iterations_ref = done(s, pair);
    } else { // the counts of the lowest pair where they differ, else the maxima
        for (int i = 0; i < c->N; i++) {
            r.iterations_done = std::max(r.iterations_done, done(c, i));
            r.iterations_ref = std::max(r.iterations_ref, done(s, i));
        }
        for (int i = 0; i < c->N && counts_agree; i++)
            if (done(c, i) != done(s, i)) {
                counts_agree = false;
                r.iterations_done = done(c, i);
                r.iterations_ref = done(s, i);
            }
    }
    r.u.first_failing = r.v.first_failing = r.deriv_first = -1;
    for (int k = 0; k < count; k++) {
        const hsflow_plane_diff du = cmp_record(c, 3 * k), dv = cmp_record(c, 3 * k + 1), dd = cmp_record(c, 3 * k + 2);
        cmp_merge(r.u, du);
        cmp_merge(r.v, dv);
        r.deriv_differing += dd.differing;
        if (r.deriv_first < 0) r.deriv_first = dd.first_failing;
        if (pair < 0 && r.pair < 0 && (du.failing || dv.failing || dd.differing)) r.pair = first + k;
    }
    r.ok = r.u.failing == 0 && r.v.failing == 0 && r.deriv_differing == 0 && r.iterations_ref == r.iterations_done && counts_agree;
    *report = r;
    return HSFLOW_OK;
}

} // extern "C"
