// hs_context.hip.h -- part of libhsflow.so (one translation unit, see hsflow.hip): plan / graph types, the
// context object behind hsflow_ctx, error plumbing.
#pragma once

namespace {

constexpr int kMaxFuse = 32;        // upper bound on sweeps per fused launch
constexpr int kLdsLimit = 160 * 1024; // bytes of LDS per CU on gfx950
constexpr int kNumCU = 256;

thread_local std::string g_create_error; // last error of a call without a context, per host thread

struct FusedPlan {
    hsk::FusedGeom g;
    int NT, K, lds_bytes, tiles;
};

struct StripPlan {
    hsk::StripGeom g;
    int R, lds_bytes, tiles;
    int fold; // 0: k_jacobi_strip (256 columns, one strip per wavefront); 1: k_jacobi_fold (128 columns, two)
};

// A launch plan for T sweeps with either multi-sweep kernel.
struct JPlan {
    int kind = 0; // HSFLOW_KERNEL_FUSED, HSFLOW_KERNEL_STRIP or HSFLOW_KERNEL_FOLD
    int T = 0;
    FusedPlan f{};
    StripPlan s{};
};

// What a Jacobi launch records about Eps = max |u_k - u_{k-1}|, |v_k - v_{k-1}| (the kernels' EPS template argument).
enum class EpsMode : int {
    None = 0,
    EverySweep = 1,  // the exact Eps of every sweep
    Witness = 2,     // strip / fold: one lower bound per launch and workgroup that proves "no sweep of mine fell below epsilon"
    WitnessLast = 3, // the witness, and the exact Eps of the last sweep (two words per workgroup)
};

// Layout of the Eps words of one pass in dEpsTiles (k_eps_reduce's arguments): `slots` rows of `stride` words; the
// first n_first rows hold cnt_first valid words (one per workgroup of a full launch), the others cnt_last.
// pairs > 0: the pass is reduced PER PAIR (k_eps_reduce_pairs: one word per (slot, pair), hEps[slot * pairs + pair]); the
// words of a row are then per workgroup of a strip / fold launch, cnt_first / cnt_last = tiles per pair x pairs.
struct EpsLayout {
    int slots = 0, stride = 1, n_first = 0, cnt_first = 0, cnt_last = 0;
    int pairs = 0;
};

struct GraphKey {
    int mode, kernel, max_iter, T, tw, th, nt, lr, cur, use_prev; // lr: K (fused) or R (strip)
    float coeff;
    float eps_thr = -1.f; // >= 0: the graph of an ITER|EPS witness pass with that threshold
    bool operator<(const GraphKey &o) const
    {
        return std::tie(mode, kernel, max_iter, T, tw, th, nt, lr, cur, use_prev, coeff, eps_thr) <
               std::tie(o.mode, o.kernel, o.max_iter, o.T, o.tw, o.th, o.nt, o.lr, o.cur, o.use_prev, o.coeff, o.eps_thr);
    }
};

struct GraphEntry {
    hipGraph_t graph;
    hipGraphExec_t exec;
    int cur_after, launches;
};

// What solve_impl works out once and the three termination paths share.
struct SolveSetup {
    float coeff;        // Ilambda = fl32(1 / fl32(lambda))
    int kernel;         // kernel actually used (AUTO resolved)
    bool multi;         // several sweeps per launch (every kernel but the simple one)
    bool use_iter, use_eps;
    long long budget;   // sweep budget (huge when ITER does not apply)
    int T;              // sweeps per full launch
    JPlan plan;         // launch plan for T sweeps
    JPlan tail;         // ... and for the short last launch of budget % T sweeps (tail.T = 0: the budget has none)
    bool witness;       // ITER|EPS runs the budget as witness launches (plan and tail can; no exact pass is being forced)
    bool persist;       // the whole budget as ONE persistent launch in phases of T sweeps (HSFLOW_KERNEL_PERSIST)
    hsflow_params eff;  // the parameters of THIS call (a cached setup gets them replaced: use_previous, reuse_derivatives, use_graph
                        // and profile do not enter the plan)
};

// prepare_solve's result for one set of parameters (hsflow_ctx::plan_cache)
struct PlanKey {
    hsflow_params p;
    int async, exact;
    int t_cap; // hsflow_ctx::t_cap the plan was made under
};
struct PlanEntry {
    PlanKey key;
    SolveSetup S;
    hsflow_info info;
};

} // namespace

struct HsPyramid; // hs_pyramid.hip.h

struct hsflow_ctx {
    int device = 0;
    int W = 0, H = 0, N = 0, P = 0;
    int org = 0;         // frame row of this context's row 0, modulo 2 (hsflow_set_row_origin)
    long long plane = 0; // elements per pair plane
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint8_t *dA = nullptr, *dB = nullptr;
    uint32_t *dCoef = nullptr;
    float *dE[3] = {nullptr, nullptr, nullptr}; // CLASSIC mode: Ex, Ey, Et planes for the kernels that read planes (allocated on first use)
    bool dE_valid = false;       // ... and whether they hold the current derivatives (dCoef always does, packed)
    int coef_mode = -1;          // discretisation the current derivatives belong to
    float *dU[2] = {nullptr, nullptr}, *dV[2] = {nullptr, nullptr};
    unsigned long long *dStamps = nullptr; // diagnostic phase stamps (HSFLOW_DEBUG_STAMPS), else NULL
    unsigned *dEps = nullptr;   // kMaxFuse words: Eps sink of launches that do not collect it
    unsigned *hEps = nullptr;   // page-locked, device-visible: k_eps_reduce writes the per-sweep Eps words here
    unsigned *hEpsDev = nullptr; // the device's address of hEps
    size_t hEpsCap = 0;
    int *dPairs = nullptr;      // 3 * N indices: the identity, the list of active pairs, the lists of a chunk's replays
    unsigned *dEpsTiles = nullptr; // per-sweep, per-workgroup Eps of the launches of one solve
    size_t epsTilesCap = 0;
    float *dUb = nullptr, *dVb = nullptr; // backup of the starting flow (ITER|EPS with use_previous)
    // Caller-written flow (hs_solve.hip.h, "tame planes"): the flow planes are `tame` while this context's own CV solves
    // with Ilambda >= 1e-20 made them, from zero or from tame planes -- what the strip kernels' scaled state counts on.  A
    // write through hsflow_set_flow_device (without HSFLOW_FLOW_SOLVER_MADE) or the one-shot's upload, a solve with a
    // smaller Ilambda and a classic solve clear the flag, a measurement that finds nothing above 1e15 sets it again; a warm
    // strip / fold solve on planes that are not tame measures them first (dFlowMax: one word) and caps its launch length
    // (t_cap: 0 none, else the most sweeps a strip / fold launch of the solve being planned may have).
    bool flow_tame = true;
    unsigned *dFlowMax = nullptr, *hFlowMax = nullptr; // (the word on the device, and page-locked for its way back)
    int t_cap = 0;
    // the persistent launch (HSFLOW_KERNEL_PERSIST, hs_kernels_strip.hip.h): a third flow buffer (its phases alternate
    // between this one and the ping-pong buffer the result lands in; the starting flow stays intact), the tiles' phase
    // counters, the error word (page-locked, device-visible)
    float *dUp = nullptr, *dVp = nullptr;
    unsigned *dFlags = nullptr;
    unsigned *hErr = nullptr, *hErrDev = nullptr;
    int persist_tiles = 0;       // grid the phase counters are consistent for (0: to be cleared before the next launch)
    bool persist_off = false;    // a persistent launch timed out on this context: not used again
    bool persist_unchecked = false; // an asynchronous persistent solve whose error word has not been looked at yet
    bool counted = false;        // this context is in g_live_ctx
    int eps_row0 = 0, eps_rows = 0; // hsflow_set_eps_rows: rows whose changes count for Eps (0 rows: the whole frame)
    std::vector<float> sweep_eps;   // Eps of every sweep of the last exact (per-sweep) pass: hsflow_solve_probe hands it out
    // hsflow_set_pair_termination: under EPS termination every pair of the context stops on its own Eps (hs_solve.hip.h,
    // "per-pair stop").  What the last solve did pair by pair (hsflow_get_pair_result); empty while the batch stops as one.
    bool per_pair = false;
    struct PairResult {
        int status = 0, iterations_done = 0, eps_rerun = 0;
        float last_eps = 0.f;
        long long sweeps = 0;
        bool eps_owed = false;   // stands at the budget of an asynchronous witness pass: last_eps is measured when somebody asks
        bool in_both = false;    // took the exact pass: its final flow lies in both ping-pong buffers
    };
    std::vector<PairResult> pair_res;
    bool pair_res_valid = false;    // pair_res belongs to the last solve (a per-pair solve ran)
    long long sweeps_run = 0;       // sweeps the device ran in the last solve, speculative and repeated ones included
    bool probe_pairs = false;       // hsflow_solve_probe_pairs: the exact pass also reduces its Eps words per pair ...
    std::vector<float> sweep_eps_pairs; // ... into this, [sweep][pair]
    // hsflow_set_async_reduce: every asynchronous solve is followed by k_mark_done; the host waits for a solve by polling the
    // page-locked word (hsflow_wait_solve) instead of waiting for the stream
    unsigned *dSeq = nullptr, *hMark = nullptr, *hMarkDev = nullptr;
    float *dZero = nullptr; // one row of zeros (P floats): stands in for u and v in strip / fold launches that start from zero flow
    unsigned mark_issued = 0;       // markers enqueued so far = the value the last one will write
    bool last_marked = false;       // the last solve was followed by a marker
    bool flow_after_mark = false;   // copies into / out of the flow planes were enqueued behind that marker (hsflow_set_flow_device,
                                    // hsflow_get_flow_device, hsflow_get_flow_async): the marker no longer says "the planes are final"
    bool async_reduce = false;      // hsflow_set_async_reduce
    int cu_share = 0;            // > 0: the planners count on this many CUs only (hsflow_set_cu_share); 0: the whole chip
    int num_cu = 0;              // compute units of the device (one workgroup of the persistent launch per CU)
    int max_grid_z = 65535;      // the device's grid limit in z: launches with one layer of workgroups per pair take at most this many
    void *dScratch = nullptr;   // staging for host frames / derivative read-back (scratch_reserve)
    // hsflow_render_flow[_device] (hs_render.hip.h), allocated by the first render: the priority plane (P x H words, zero
    // between renders), the picture hsflow_render_flow draws into before it copies it out (3*W x H bytes), and the
    // event behind that copy
    unsigned *dPrio = nullptr;
    bool prio_dirty = false;    // a render failed between its two launches: clear the plane before the next one
    uint8_t *dRgb = nullptr;
    hipEvent_t evRender = nullptr;
    // hsflow_color_flow* (hs_color.hip.h), allocated by the first colour picture: one scale word per picture of a chunk
    // (the largest raw radius as a bit pattern, written and read on the device) and a page-locked word for the one the
    // synchronous form hands to its caller.  The pictures the synchronous and JPEG forms draw into are dRgb and
    // jpeg_batch.rgb, shared with the arrow drawing: everything of a context runs on one stream.
    unsigned *dColorScale = nullptr;
    unsigned *hColorScale = nullptr;
    // hsflow_warp (hs_warp.hip.h), allocated by the first synchronous warp that needs them and grown to the largest
    // picture so far: the caller's source and reference on the device, the warped picture before it is copied out, one
    // statistics record on the device and one in page-locked memory.  The device forms take the caller's memory and
    // allocate nothing.
    struct WarpScratch {
        uint8_t *src = nullptr, *ref = nullptr, *dst = nullptr;
        size_t src_bytes = 0, ref_bytes = 0, dst_bytes = 0;
        hsflow_warp_stats *dStats = nullptr, *hStats = nullptr;
    } warp;
    // hsflow_fb / hsflow_fb_planes (hs_fb.hip.h), allocated by the first synchronous check that needs them: the mask and
    // the err2 plane before they are copied out, one statistics record on the device and one in page-locked memory.  The
    // device forms take the caller's memory and allocate nothing.
    struct FbScratch {
        uint8_t *mask = nullptr, *err2 = nullptr;
        size_t mask_bytes = 0, err2_bytes = 0;
        hsflow_fb_stats *dStats = nullptr, *hStats = nullptr;
    } fb;
    // hsflow_jpeg_encode_device and the render-and-encode forms (hs_jpeg.hip.h), allocated by the first encode and kept:
    // one block of device memory carved into the coefficients (128 B per block), the blocks' bit lengths and offsets, the
    // raw stream (208 B per block), the chunks' 0xFF counts and offsets and a size word; the tables and header of every
    // quality used so far; for the synchronous forms the file on the device and a page-locked size word
    struct JpegScratch {
        void *base = nullptr;
        int16_t *coef = nullptr;
        uint32_t *len = nullptr, *raw = nullptr, *ff = nullptr;
        uint64_t *off = nullptr, *ffoff = nullptr, *size = nullptr;
        long long nb = 0, nchunks = 0;
        size_t raw_bytes = 0;
        std::map<int, hsjpeg::Tables *> tables; // by quality, device memory
        uint8_t *out = nullptr;
        size_t out_bytes = 0;
        uint64_t *hSize = nullptr;
    } jpeg;
    // hsflow_jpeg_decode_device, hsflow_jpeg_decode_batch_device and the entries built on them (hs_jpegd.hip.h), allocated
    // by the first decode and kept: one block of device memory for a chunk's files, laid out by hs_jpegd_batch_plan.h (a
    // single decode is a chunk of one) and grown to the largest chunk so far; two page-locked staging areas with the event
    // behind each one's copy; for the synchronous forms a picture on the device (its first 256 bytes hold the status
    // words), two BGR pictures, page-locked status words; hsflow_set_sequence_jpeg's status words (the first 256-byte
    // multiple) and pictures on the device, its status words in page-locked memory
    struct JpegdScratch {
        void *base = nullptr;
        size_t bytes = 0;
        uint8_t *stage[2] = {nullptr, nullptr};
        size_t stage_bytes[2] = {0, 0};
        hipEvent_t evStage[2] = {nullptr, nullptr};
        int next_slot = 0;
        uint8_t *out = nullptr;
        size_t out_bytes = 0;
        uint8_t *bgr[2] = {nullptr, nullptr};
        uint32_t *dStatus = nullptr, *hStatus = nullptr;
        hipEvent_t evDone = nullptr;
        uint8_t *seq = nullptr;
        size_t seq_bytes = 0;
        uint32_t *hSeq = nullptr;
        int hSeq_words = 0;
        bool pair_status_owed = false; // hsflow_set_frames_jpeg_async's two words are on their way into hStatus[2 .. 3],
        hipEvent_t evPair = nullptr;   // this event behind their copy; hsflow_jpeg_async_status has not asked yet
    } jpegd;
    // hsflow_verify / hsflow_compare_flow_device (hs_verify.hip.h), all allocated by the first call: the parameters of the
    // last solve asked for through the ABI and how it ended; the reference pass's own buffers, held as a second context
    // object that borrows this one's frames and stream (`shadow`; it is `borrowed`: not counted in g_live_ctx, and it frees
    // neither the frames nor the stream); the comparison records on the device and in page-locked memory; the event behind
    // their copy
    hsflow_params vparams;
    int vstate = 0;             // 0: no solve yet, 1: the last solve succeeded, 2: it failed, 3: it was a pyramid solve (hs_pyramid.hip.h)
    int last_status = 0;        // ... and what it returned (hsflow_get_pair_result on a batch that stops as one)
    bool v_per_pair = false;    // ... and whether its pairs stopped each on its own
    int v_org = 0, v_eps_row0 = 0, v_eps_rows = 0; // row origin and Eps rows that solve ran with
    hsflow_ctx *shadow = nullptr;
    bool borrowed = false;
    unsigned long long *dCmp = nullptr, *hCmp = nullptr;
    int cmp_cap = 0;            // records both hold
    hipEvent_t evVerify = nullptr;
    size_t scratch_bytes = 0;
    int cur = 0;                // which of dU/dV holds the current flow
    // hsflow_solve_async_frames_device: the caller's frames, while the solve has not yet decided who copies them (`lazy`:
    // only inside that call).  Once it has decided that its first Jacobi launch reads them in place and leaves the copy in
    // dA / dB itself, that one launch is handed them (resolve_lazy_frames, LaunchIo::frames).
    struct FrameRef {
        bool active = false;
        const uint8_t *A = nullptr, *B = nullptr;
        long long PA = 0, PB = 0; // row pitches in bytes
    } lazy;
    unsigned long long copies_elided = 0; // submissions whose frame copy rode in the first Jacobi launch (hsflow_frame_copies_elided)
    bool frames_set = false;
    bool coef_valid = false;
    hsflow_info info;
    std::string err;
    // an ITER|EPS solve enqueued by hsflow_solve_async whose early-stop check is still owed
    struct Pending {
        bool active = false;
        hsflow_params params;
        int iters = 0, launches = 0, cur0 = 0;
        EpsLayout words;        // its witness words
        bool reduced = false;   // the reduction into hEps was enqueued with the solve (async_reduce)
        unsigned mark = 0;      // ... and the marker behind it
        bool marked_by_reduce = false; // ... written by the reduction kernel's last workgroup
    } pend;
    // what it takes to measure last_eps of an asynchronous ITER|EPS solve on demand (hsflow_get_info): its last
    // launch again, from the input buffer that launch left intact, with the final sweep's Eps measured
    struct LastLaunch {
        bool valid = false;    // last_eps not measured yet
        JPlan plan;
        int zero_in = 0;
        float coeff = 0.f, eps_thr = 0.f;
        bool from_third = false; // its input lies in dUp / dVp (last phase of a persistent launch), not the other ping-pong buffer
    } lastl;
    bool force_exact = false; // the exact per-sweep pass is wanted (set while a pending solve is settled)
    // A dry run of an enqueue sequence ahead of its stream capture (run_captured): kernel attributes cannot be set inside a
    // capture, so the sequence is walked once with this set -- the launch wrappers then only raise the dynamic-LDS cap of
    // the kernel variant they would launch, and whatever else enqueues work returns at once.
    bool configuring = false;
    std::map<GraphKey, GraphEntry> graphs;
    std::vector<PlanEntry> plan_cache; // prepare_solve's results by parameters; cleared when what they rest on changes
    std::vector<hipEvent_t> events;
    // a batch of pictures drawn and encoded by one set of launches per chunk (hs_render.hip.h, hs_jpeg.hip.h,
    // hs_jpeg_batch_plan.h), allocated by the first batched call and kept: dPrio holds prio_planes priority planes (the
    // single render uses the first); one allocation for the encode scratch of `pictures` slices, separate from the single
    // encode's; for the render-and-encode forms `rgb_pictures` pictures on the device; for the synchronous form
    // `out_pictures` output slots of `slot` bytes and the chunk's size words in page-locked memory
    int prio_planes = 0;
    struct JpegBatchScratch {
        void *base = nullptr;
        int pictures = 0;
        uint8_t *rgb = nullptr;
        int rgb_pictures = 0;
        uint8_t *out = nullptr;
        size_t slot = 0;
        int out_pictures = 0;
        uint64_t *hSize = nullptr;
    } jpeg_batch;
    // hsflow_median_apply / hsflow_median (hs_median.hip.h), each piece allocated by the first call that needs it and kept:
    // packed fp32 plane pairs between the passes (apply: one; the synchronous form with several passes: two), two state
    // planes, one statistics record on the device and one in page-locked memory.  The device forms take the caller's
    // memory and allocate nothing.  (Last in the context: every other member stays where it was.)
    struct MedianScratch {
        float *u[2] = {nullptr, nullptr}, *v[2] = {nullptr, nullptr};
        uint8_t *s[2] = {nullptr, nullptr};
        hsflow_median_stats *dStats = nullptr, *hStats = nullptr;
    } median;
    // hsflow_interp* / hsflow_project_flow_device (hs_interp.hip.h): one block for `times` times of a chunk -- per time the
    // key plane, two pairs of fp32 planes and two state planes of pitch x height, then the fill's records -- allocated by
    // the first call, grown on demand and kept; for the synchronous form the caller's pictures on the device (prev, curr,
    // vis_prev, vis_curr, ref, dst, cls), one statistics record on the device and one in page-locked memory.
    struct InterpScratch {
        void *base = nullptr;
        int times = 0;
        uint8_t *stage[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        size_t stage_bytes[7] = {0, 0, 0, 0, 0, 0, 0};
        hsflow_interp_stats *dStats = nullptr, *hStats = nullptr;
    } interp;
    // hsflow_solve_pyramid (hs_pyramid.hip.h): the level contexts and planes of the last plan, allocated by the first
    // pyramid solve and kept.  NULL on a context that never ran one.
    HsPyramid *pyr = nullptr;
    // hsflow_chain_flow / hsflow_track_points (hs_chain.hip.h): the staging of the synchronous forms -- the callers' state
    // planes, start planes or points on the device and the results before they are copied out, each slot allocated by the
    // first call that needs it and grown to the largest so far -- one statistics record on the device and one in page-locked
    // memory.  The device forms take the caller's memory and allocate nothing.
    struct ChainScratch {
        uint8_t *stage[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        size_t stage_bytes[7] = {0, 0, 0, 0, 0, 0, 0};
        hsflow_chain_stats *dStats = nullptr, *hStats = nullptr;
    } chain;
    // hsflow_gmotion_* (hs_gmotion.hip.h): the kernels' records (hsk::GmScratch, one per field of the largest batch so far;
    // zero sums and histograms between calls, `dirty` while a call's launches may have been cut short), allocated by the
    // first call and grown; the staging of the synchronous forms -- 0 state, 1 mask, 2 / 3 the residual planes, 4 / 5 / 6
    // source, reference and destination of the model warp -- and one result and one warp statistics record on the device
    // and in page-locked memory.
    struct GmotionScratch {
        void *scr = nullptr;
        int cap = 0;
        bool dirty = false;
        uint8_t *stage[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        size_t stage_bytes[7] = {0, 0, 0, 0, 0, 0, 0};
        hsflow_gmotion_result *dRes = nullptr, *hRes = nullptr;
        hsflow_warp_stats *dStats = nullptr, *hStats = nullptr;
    } gmotion;
    // hsflow_regions* (hs_regions.hip.h): the kernels' scratch (per field of the largest chunk so far a parent and an area
    // plane of W * H words and one count word per 256 pixels of a row, then the hsk::RgAcc records; a call reads no word it
    // has not written itself, so nothing is cleared), allocated by the first call and grown; the staging of the synchronous
    // form -- 0 mask, 1 labels, 2 records -- and one result header on the device and in page-locked memory.
    struct RegionsScratch {
        void *scr = nullptr;
        size_t bytes = 0;
        uint8_t *stage[3] = {nullptr, nullptr, nullptr};
        size_t stage_bytes[3] = {0, 0, 0};
        hsflow_regions_result *dRes = nullptr, *hRes = nullptr;
    } regions;
    // hsflow_link_regions* (hs_link.hip.h): the kernels' scratch (per step of the largest set of launches so far the rule's
    // table of cap_a * cap_b + 2 * cap_a + 1 words, one count word per 256 cells and 2 + 2 * cap_a + cap_b words more; the
    // call's first kernel clears the table, so nothing is carried over), allocated by the first call and grown; the
    // staging of the synchronous form -- 0 labels of a, 1 labels of b, 2 links, 3 side_a, 4 side_b -- and one result header
    // on the device and in page-locked memory.
    struct LinkScratch {
        void *scr = nullptr;
        size_t bytes = 0;
        uint8_t *stage[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        size_t stage_bytes[5] = {0, 0, 0, 0, 0};
        hsflow_link_result *dRes = nullptr, *hRes = nullptr;
    } link;
    // hsflow_corners* (hs_corners.hip.h): the kernels' scratch (per field of the largest chunk so far a score plane of W * H
    // int64, 65536 candidates of 16 bytes, four ballot words and one offset word per 256 pixels of a row, then the
    // hsk::CnAcc records, which a memset in front of every set of launches clears; a call reads no other word it has not
    // written itself), allocated by the first call and grown; the staging of the synchronous form -- 0 mask, 1 records,
    // 2 xy -- and one result header on the device and in page-locked memory.
    struct CornersScratch {
        void *scr = nullptr;
        size_t bytes = 0;
        uint8_t *stage[3] = {nullptr, nullptr, nullptr};
        size_t stage_bytes[3] = {0, 0, 0};
        hsflow_corners_result *dRes = nullptr, *hRes = nullptr;
    } corners;
};

namespace {

// What a Jacobi launch is handed besides its plan and its flow planes.  The solve paths build one from their locals at the
// place of the launch; nothing of it lives in the context.  (Here, not next to EpsMode: it names hsflow_ctx::FrameRef.)
struct LaunchIo {
    unsigned *eps;         // where the launch records Eps: rows of `stride` words, one row per sweep (EverySweep) or launch
    int stride = 1;        // words per row: one per workgroup (strip / fold), else 1
    float thr = 0.f;       // witness launches: smallest float >= epsilon
    int eps_pair = 0;      // simple / LDS-tile kernel: 1 = one Eps word per (sweep, pair) instead of one per sweep
    const int *pairs = nullptr; // the launch works on these pairs only (device array of n_pairs indices), NULL: on all
    int n_pairs = 0;
    const hsflow_ctx::FrameRef *frames = nullptr; // a first launch with the derivative pass reads these, NULL: dA / dB
};

// The default: Eps into the sink nobody reads, all pairs, the context's own frames.
LaunchIo default_io(const hsflow_ctx *c) { return LaunchIo{c->dEps}; }

// One pass of a CV-mode solve: `sweeps` Jacobi sweeps from the current flow, as n launches of `plan` with a short last one
// (enqueue_pass walks it, issue_pass puts it on the stream).  The solve paths build one from their setup.
struct Pass {
    int sweeps = 0, n = 0;          // n: launches (persist: phases of the one launch)
    const JPlan *plan = nullptr, *last = nullptr; // of every launch but the last, of the last (the one-sweep kernel: NULL)
    float coeff = 0.f;
    bool zero = false;              // the pass starts from u = v = 0 (a cold start)
    bool persist = false;           // all of it as ONE persistent launch
    EpsMode eps = EpsMode::None, eps_last = EpsMode::None; // what every launch but the last records, and the last
    unsigned *eps_rows = nullptr;   // launch (phase) L records into row L of these (NULL: nothing, into the sink nobody reads) ...
    int stride = 1;                 // ... of this many words ...
    float thr = 0.f;                // ... against this threshold (LaunchIo)
    const EpsLayout *reduce = nullptr; // behind the last launch the rows are reduced into hEps ...
    bool mark = false;              // ... by a kernel whose last workgroup writes the context's marker
    bool save_start = false;        // the starting flow is kept in dUb / dVb first
    // how launch 0 is formed (form_first_launch):
    bool deriv = false, fuse = false; // the derivatives are computed; by launch 0 itself, not by a kernel of their own
    bool in_place = false;          // launch 0 reads the caller's frames, these:
    hsflow_ctx::FrameRef frames;
};

// live contexts per device (this process): the persistent launch wants the device to itself -- two persistent grids
// from two contexts could each hold part of the CUs and wait for workgroups that cannot start
std::atomic<int> g_live_ctx[64];
constexpr int kMaxPersistTiles = 4096;

hsflow_ctx *g_oneshot = nullptr; // context kept by hsflow_calc_optical_flow_hs_8u32f between calls
std::mutex g_oneshot_mutex;

int fail(hsflow_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg; else g_create_error = msg;
    return code;
}

#define HS_HIP(c, call)                                                                           \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess)                                                                     \
            return fail((c), e_ == hipErrorOutOfMemory ? HSFLOW_E_OOM : HSFLOW_E_DEVICE,          \
                        std::string(#call) + ": " + hipGetErrorString(e_));                       \
    } while (0)

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// A picture whose base and row stride are multiples of 4: the kernels move its rows as whole words (`wide`).
int word_aligned(const void *p, size_t stride) { return (((uintptr_t)p | stride) & 3u) == 0; }

} // namespace
