// HSOpticalFlowOpenCL.cpp -- see HSOpticalFlowOpenCL.hpp.  Host orchestration only; every pixel is
// computed by libhsflow.so.
#include "HSOpticalFlowOpenCL.hpp"

#include <chrono>
#include <cmath>
#include <cstring>
#include <iostream>

#include <hip/hip_runtime_api.h> // the batched "-cv -cam" route uploads its frames itself: hipMalloc / hipMemcpy / hipFree

namespace {

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Frames of the "-cam" route come from numbered files instead of a capture device:
// $HSFLOW_CAMERA_DIR/frame_0000.pgm (or .ppm / .jpg), frame_0001.pgm, ... until one is missing.
std::string camera_frame(int i)
{
    const char *dir = getenv("HSFLOW_CAMERA_DIR");
    const std::string base = std::string(dir ? dir : ".");
    char name[64];
    for (const char *ext : {"pgm", "ppm", "jpg"}) {
        snprintf(name, sizeof(name), "/frame_%04d.%s", i, ext);
        if (FILE *f = fopen((base + name).c_str(), "rb")) { fclose(f); return base + name; }
    }
    snprintf(name, sizeof(name), "/frame_%04d.pgm", i);
    return base + name;
}

// HSFLOW_RENDER_DEVICE=1: the picture is drawn on the device from the flow where the solver left it
// (hsflow_render_flow) and u, v are never downloaded; otherwise they are, and the host draws (pnm.hpp).
bool render_on_device()
{
    const char *e = getenv("HSFLOW_RENDER_DEVICE");
    return e && atoi(e) != 0;
}

// HSFLOW_VERIFY=1: every solved pair is verified on the device before its context goes away (hsflow_verify), one
// "Passed!" / "Failed" line per pair on stdout; a pair that fails makes the exit status SDK_FAILURE.
bool verify_wanted()
{
    const char *e = getenv("HSFLOW_VERIFY");
    return e && atoi(e) != 0;
}

// hsflow_verify of ctx's pair and its line; SDK_SUCCESS iff the report says ok.
int verify_pair(hsflow_ctx *ctx, int W, hsflow_verify_report &report, int pair = 0)
{
    std::memset(&report, 0, sizeof(report));
    report.struct_size = sizeof(report);
    const int st = hsflow_verify(ctx, pair, &report);
    if (st != HSFLOW_OK) {
        std::cout << "Failed: " << hsflow_last_error(ctx) << std::endl;
        return SDK_FAILURE;
    }
    std::cout << verify_line(report, W) << std::endl;
    return report.ok ? SDK_SUCCESS : SDK_FAILURE;
}

// HSFLOW_PICTURE=color: every route writes the dense colour picture (hsflow_color_flow*: the Middlebury wheel) instead
// of the arrows; "arrows", or no variable, leaves everything as it was.  0: arrows, 1: colour, -1: unusable.
int picture_kind()
{
    const char *e = getenv("HSFLOW_PICTURE");
    if (!e || !*e || strcmp(e, "arrows") == 0) return 0;
    return strcmp(e, "color") == 0 ? 1 : strcmp(e, "warp") == 0 ? 2 : strcmp(e, "fb") == 0 ? 3 : strcmp(e, "interp") == 0 ? 4 : strcmp(e, "stab") == 0 ? 5 : -1;
}

bool color_picture() { return picture_kind() == 1; }

// HSFLOW_COLOR_MAX=<float>: the colour picture's scale is that flow (HSFLOW_COLOR_SCALE_FIXED); without it the picture's
// own largest flow (AUTO).  false: the value is unusable.
bool color_params(hsflow_color_params &cp)
{
    hsflow_default_color_params(&cp);
    const char *e = getenv("HSFLOW_COLOR_MAX");
    if (!e || !*e) return true;
    char *rest = nullptr;
    const float m = strtof(e, &rest);
    if (*rest || !std::isfinite(m) || !(m > 0.f)) return false;
    cp.scale_mode = HSFLOW_COLOR_SCALE_FIXED;
    cp.max_flow = m;
    return true;
}

// HSFLOW_PICTURE=warp on the two "-hd" routes: the file holds the motion-compensated second frame -- the second input as
// loaded, colour and all, warped onto the first by the solved flow (hsflow_warp*) -- instead of a picture of the flow, and
// one line on stdout tells the residual.  HSFLOW_WARP_T=<float>: the fraction of the flow to apply (default 1).
// false: the value is unusable.
bool warp_params(hsflow_warp_params &wp)
{
    hsflow_default_warp_params(&wp);
    const char *e = getenv("HSFLOW_WARP_T");
    if (!e || !*e) return true;
    char *rest = nullptr;
    const float t = strtof(e, &rest);
    if (*rest || !std::isfinite(t) || !(std::fabs(t) <= 1e6f)) return false;
    wp.t = t;
    return true;
}

// With HSFLOW_RENDER_DEVICE=1 through hsflow_warp (the flow stays on the device), otherwise hsflow_warp_host on the flow
// that was read back; the same bytes and the same line.
int warp_picture(hsflow_ctx *ctx, const pnm::Image &first, const pnm::Image &second, const std::vector<float> &u, const std::vector<float> &v,
                 pnm::Image &out)
{
    const int W = second.width, H = second.height, C = second.channels;
    if (first.width != W || first.height != H || first.channels != C) { std::cout << "HSFLOW_PICTURE=warp: the two frames differ in kind" << std::endl; return SDK_FAILURE; }
    out.width = W; out.height = H; out.channels = C;
    out.data.resize((size_t)W * H * C);
    hsflow_warp_params wp;
    warp_params(wp);
    wp.channels = C;
    hsflow_warp_stats s;
    const size_t rowb = (size_t)W * C;
    const int st = render_on_device() ? hsflow_warp(ctx, 0, &wp, second.data.data(), rowb, first.data.data(), rowb, out.data.data(), rowb, &s)
                                      : hsflow_warp_host(u.data(), (size_t)W * 4, v.data(), (size_t)W * 4, W, H, &wp, second.data.data(), rowb,
                                                         first.data.data(), rowb, out.data.data(), rowb, &s);
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(render_on_device() ? ctx : nullptr) << std::endl; return SDK_FAILURE; }
    std::cout << "warp: inside " << s.inside << " outside " << s.outside << " unknown " << s.unknown << " sad_warped " << s.sad_warped << " sad_plain "
              << s.sad_plain << std::endl;
    return SDK_SUCCESS;
}

// HSFLOW_PICTURE=stab on the two "-hd" routes: the file holds the second input warped onto the first by the ONE global motion
// fitted to the solved flow (hsflow_gmotion_fit*, hsflow_gmotion_warp*) -- the stabilised frame -- not by the dense flow,
// and one line on stdout tells the model's six parameters and the inliers' share.
// HSFLOW_GMOTION=<translation|similarity|affine>[,<passes>[,<px>|auto]] selects the fit (default affine,3,1).
// false: the value is unusable.
bool gmotion_choice(hsflow_gmotion_params &gp)
{
    hsflow_default_gmotion_params(&gp);
    const char *e = getenv("HSFLOW_GMOTION");
    if (!e || !*e) return true;
    const std::string text(e);
    const size_t c1 = text.find(','), c2 = c1 == std::string::npos ? c1 : text.find(',', c1 + 1);
    const std::string kind = text.substr(0, c1);
    if (kind == "translation") gp.model = HSFLOW_GMOTION_TRANSLATION;
    else if (kind == "similarity") gp.model = HSFLOW_GMOTION_SIMILARITY;
    else if (kind == "affine") gp.model = HSFLOW_GMOTION_AFFINE;
    else return false;
    if (c1 == std::string::npos) return true;
    const std::string passes = text.substr(c1 + 1, c2 == std::string::npos ? c2 : c2 - c1 - 1);
    char *rest = nullptr;
    const long n = strtol(passes.c_str(), &rest, 10);
    if (passes.empty() || *rest || n < 1 || n > HSFLOW_GMOTION_MAX_PASSES) return false;
    gp.passes = (int)n;
    if (c2 == std::string::npos) return true;
    const std::string thr = text.substr(c2 + 1);
    if (thr == "auto") { gp.threshold_mode = HSFLOW_GMOTION_THRESHOLD_AUTO; return true; }
    const float px = strtof(thr.c_str(), &rest);
    if (thr.empty() || *rest || !std::isfinite(px) || !(px > 0.f)) return false;
    gp.inlier_px = px;
    return true;
}

// "<what>: model p0 .. p5 inliers <share of the frame>": the line of HSFLOW_PICTURE=stab and of the chained camera route.
static std::string gmotion_line(const char *what, const hsflow_gmotion_result &r, int W, int H)
{
    char line[256];
    snprintf(line, sizeof(line), "%s: model %.9g %.9g %.9g %.9g %.9g %.9g inliers %.4f", what, r.p[0], r.p[1], r.p[2], r.p[3], r.p[4], r.p[5],
             (double)r.cls[0] / ((double)W * H));
    return line;
}

// With HSFLOW_RENDER_DEVICE=1 through hsflow_gmotion_fit and hsflow_gmotion_warp (the flow stays on the device), otherwise
// the host rules on the flow that was read back; the same bytes and the same line.
int stab_picture(hsflow_ctx *ctx, const pnm::Image &first, const pnm::Image &second, const std::vector<float> &u, const std::vector<float> &v,
                 pnm::Image &out)
{
    const int W = second.width, H = second.height, C = second.channels;
    if (first.width != W || first.height != H || first.channels != C) { std::cout << "HSFLOW_PICTURE=stab: the two frames differ in kind" << std::endl; return SDK_FAILURE; }
    out.width = W; out.height = H; out.channels = C;
    out.data.resize((size_t)W * H * C);
    hsflow_gmotion_params gp;
    gmotion_choice(gp);
    hsflow_warp_params wp;
    hsflow_default_warp_params(&wp);
    wp.channels = C;
    hsflow_gmotion_result r;
    const size_t rowb = (size_t)W * C;
    const bool dev = render_on_device();
    int st = dev ? hsflow_gmotion_fit(ctx, 0, nullptr, 0, &gp, nullptr, 0, nullptr, nullptr, 0, &r)
                 : hsflow_gmotion_fit_host(u.data(), v.data(), (size_t)W * 4, nullptr, 0, W, H, &gp, nullptr, 0, nullptr, nullptr, 0, &r);
    if (st == HSFLOW_OK)
        st = dev ? hsflow_gmotion_warp(ctx, r.p, &wp, second.data.data(), rowb, nullptr, 0, out.data.data(), rowb, nullptr)
                 : hsflow_gmotion_warp_host(r.p, W, H, &wp, second.data.data(), rowb, nullptr, 0, out.data.data(), rowb, nullptr);
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(dev ? ctx : nullptr) << std::endl; return SDK_FAILURE; }
    std::cout << gmotion_line("stab", r, W, H) << std::endl;
    return SDK_SUCCESS;
}

// HSFLOW_PICTURE=fb on the two "-hd" routes: the context holds two pairs, the second the first one reversed
// (hsflow_set_frames_reversed), both solved by the route's own parameters; the file holds the forward-backward
// consistency mask of pair 0 against pair 1 (hsflow_fb*: 255 consistent, 0 elsewhere) as a gray picture, and one line on
// stdout tells the statistics.  HSFLOW_FB_ALPHA / HSFLOW_FB_BETA=<float> override the defaults.  false: a value is
// unusable, *which names its variable.
bool fb_params(hsflow_fb_params &fp, const char **which)
{
    hsflow_default_fb_params(&fp);
    const struct { const char *name; float *field; float top; } vars[2] = {{"HSFLOW_FB_ALPHA", &fp.alpha, 1e6f}, {"HSFLOW_FB_BETA", &fp.beta, 1e30f}};
    for (const auto &var : vars) {
        const char *e = getenv(var.name);
        if (!e || !*e) continue;
        char *rest = nullptr;
        const float x = strtof(e, &rest);
        if (*rest || !std::isfinite(x) || !(x >= 0.f && x <= var.top)) { *which = var.name; return false; }
        *var.field = x;
    }
    return true;
}

// With HSFLOW_RENDER_DEVICE=1 through hsflow_fb (the flows stay on the device), otherwise hsflow_fb_host on the four
// planes read back; the same bytes and the same line.
int fb_picture(hsflow_ctx *ctx, int W, int H, pnm::Image &out)
{
    out.width = W; out.height = H; out.channels = 1;
    out.data.resize((size_t)W * H);
    hsflow_fb_params fp;
    const char *which = nullptr;
    fb_params(fp, &which);
    hsflow_fb_stats s;
    int st;
    if (render_on_device()) {
        st = hsflow_fb(ctx, 0, 1, &fp, out.data.data(), (size_t)W, nullptr, 0, &s);
    } else {
        std::vector<float> f[4];
        for (auto &plane : f) plane.resize((size_t)W * H);
        const size_t rowb = (size_t)W * 4;
        st = hsflow_get_flow(ctx, 0, f[0].data(), rowb, f[1].data(), rowb);
        if (st == HSFLOW_OK) st = hsflow_get_flow(ctx, 1, f[2].data(), rowb, f[3].data(), rowb);
        if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
        st = hsflow_fb_host(f[0].data(), rowb, f[1].data(), rowb, f[2].data(), rowb, f[3].data(), rowb, W, H, &fp, out.data.data(), (size_t)W, nullptr, 0, &s);
        if (st != HSFLOW_OK) { std::cout << hsflow_last_error(nullptr) << std::endl; return SDK_FAILURE; }
    }
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
    const uint64_t evaluated = s.consistent + s.inconsistent;
    char mse[64];
    snprintf(mse, sizeof(mse), "%.6f", evaluated ? (double)s.sum_err2_q / (256.0 * (double)evaluated) : 0.0);
    std::cout << "fb: consistent " << s.consistent << " inconsistent " << s.inconsistent << " outside " << s.outside << " unknown " << s.unknown << " mse "
              << mse << std::endl;
    return SDK_SUCCESS;
}

// HSFLOW_PICTURE=interp on the two "-hd" routes: the file holds the frame at time t between the two input files, in their
// own channels (hsflow_interp*: the forward flow projected to t, holes filled, both frames fetched and blended), and one
// line on stdout tells the record.  HSFLOW_INTERP_T=<float in 0 .. 1> (default 0.5).  HSFLOW_INTERP_FB=1: the context
// holds the reversed pair as for HSFLOW_PICTURE=fb, and the masks of both checks (HSFLOW_FB_ALPHA / HSFLOW_FB_BETA) go
// in as vis_prev / vis_curr.  false: the value is unusable.
bool interp_time(float &t)
{
    t = 0.5f;
    const char *e = getenv("HSFLOW_INTERP_T");
    if (!e || !*e) return true;
    char *rest = nullptr;
    const float x = strtof(e, &rest);
    if (*rest || !std::isfinite(x) || !(x >= 0.f && x <= 1.f)) return false;
    t = x;
    return true;
}

bool interp_fb()
{
    const char *e = getenv("HSFLOW_INTERP_FB");
    return e && e[0] == '1';
}

// With HSFLOW_RENDER_DEVICE=1 through hsflow_interp (and hsflow_fb: the flows stay on the device), otherwise
// hsflow_interp_host (and hsflow_fb_host) on the flows read back; the same bytes and the same line.
int interp_picture(hsflow_ctx *ctx, const pnm::Image &first, const pnm::Image &second, const std::vector<float> &u, const std::vector<float> &v,
                   pnm::Image &out)
{
    const int W = second.width, H = second.height, C = second.channels;
    if (first.width != W || first.height != H || first.channels != C) { std::cout << "HSFLOW_PICTURE=interp: the two frames differ in kind" << std::endl; return SDK_FAILURE; }
    out.width = W; out.height = H; out.channels = C;
    out.data.resize((size_t)W * H * C);
    float t;
    interp_time(t);
    hsflow_interp_params ip;
    hsflow_default_interp_params(&ip);
    ip.channels = C;
    hsflow_interp_stats s;
    const size_t rowb = (size_t)W * C, frow = (size_t)W * 4;
    const bool device = render_on_device(), fb = interp_fb();
    std::vector<uint8_t> vis[2];
    int st = HSFLOW_OK;
    if (fb) {
        hsflow_fb_params fp;
        const char *which = nullptr;
        fb_params(fp, &which);
        for (auto &m : vis) m.resize((size_t)W * H);
        if (device) {
            st = hsflow_fb(ctx, 0, 1, &fp, vis[0].data(), (size_t)W, nullptr, 0, nullptr);
            if (st == HSFLOW_OK) st = hsflow_fb(ctx, 1, 0, &fp, vis[1].data(), (size_t)W, nullptr, 0, nullptr);
            if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
        } else {
            std::vector<float> ub((size_t)W * H), vb((size_t)W * H);
            if (hsflow_get_flow(ctx, 1, ub.data(), frow, vb.data(), frow) != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
            st = hsflow_fb_host(u.data(), frow, v.data(), frow, ub.data(), frow, vb.data(), frow, W, H, &fp, vis[0].data(), (size_t)W, nullptr, 0, nullptr);
            if (st == HSFLOW_OK) st = hsflow_fb_host(ub.data(), frow, vb.data(), frow, u.data(), frow, v.data(), frow, W, H, &fp, vis[1].data(), (size_t)W, nullptr, 0, nullptr);
            if (st != HSFLOW_OK) { std::cout << hsflow_last_error(nullptr) << std::endl; return SDK_FAILURE; }
        }
    }
    const uint8_t *vp = fb ? vis[0].data() : nullptr, *vc = fb ? vis[1].data() : nullptr;
    st = device ? hsflow_interp(ctx, 0, t, &ip, first.data.data(), rowb, second.data.data(), rowb, vp, (size_t)W, vc, (size_t)W, nullptr, 0, out.data.data(), rowb,
                                nullptr, 0, &s)
                : hsflow_interp_host(u.data(), frow, v.data(), frow, W, H, t, &ip, first.data.data(), rowb, second.data.data(), rowb, vp, (size_t)W, vc, (size_t)W,
                                     nullptr, 0, out.data.data(), rowb, nullptr, 0, &s);
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(device ? ctx : nullptr) << std::endl; return SDK_FAILURE; }
    std::cout << "interp: t " << t << " blended " << s.blended << " prev_only " << s.prev_only << " curr_only " << s.curr_only << " clamped " << s.clamped
              << " holes " << s.holes << " unfilled " << s.unfilled << " collisions " << s.collisions << " left " << s.left << " unknown " << s.unknown << std::endl;
    return SDK_SUCCESS;
}

// HSFLOW_MEDIAN=<radius>[,<passes>[,fill]] on the two "-hd" routes: the pair's flow is median-filtered in place
// (hsflow_median_apply: radius 1 or 2, passes 1 .. 64, default 1) before the picture is drawn.  With "fill" the context
// holds the reversed pair as for HSFLOW_PICTURE=fb, the hsflow_fb mask (HSFLOW_FB_ALPHA / HSFLOW_FB_BETA) is the state,
// only the untrusted pixels of the forward flow are replaced, and one line on stdout tells the record.
// 0: not set, 1: usable, -1: unusable.
int median_choice(int &radius, int &passes, bool &fill)
{
    radius = 1; passes = 1; fill = false;
    const char *e = getenv("HSFLOW_MEDIAN");
    if (!e || !*e) return 0;
    char *rest = nullptr;
    const long r = strtol(e, &rest, 10);
    if (rest == e || (r != 1 && r != 2)) return -1;
    radius = (int)r;
    if (!*rest) return 1;
    if (*rest != ',') return -1;
    const char *q = rest + 1;
    const long k = strtol(q, &rest, 10);
    if (rest == q || k < 1 || k > HSFLOW_MEDIAN_MAX_PASSES) return -1;
    passes = (int)k;
    if (!*rest) return 1;
    if (strcmp(rest, ",fill") != 0) return -1;
    fill = true;
    return 1;
}

// HSFLOW_PYRAMID=<levels 1 .. 8 | auto>[,<warps 1 .. 8>[,<median radius 0 .. 2>]] on the "-cv -hd" routes: the solve is the
// coarse-to-fine solve (hsflow_solve_pyramid) with the route's parameters at every level; whatever HSFLOW_PICTURE and
// HSFLOW_MEDIAN ask for works on its flow.  0: not set, 1: usable, -1: unusable.
int pyramid_choice(hsflow_pyramid_params &pp)
{
    hsflow_default_pyramid_params(&pp);
    const char *e = getenv("HSFLOW_PYRAMID");
    if (!e || !*e) return 0;
    const char *q = e;
    char *rest = nullptr;
    if (strncmp(q, "auto", 4) == 0) {
        rest = const_cast<char *>(q) + 4;
    } else {
        const long l = strtol(q, &rest, 10);
        if (rest == q || l < 1 || l > HSFLOW_PYRAMID_MAX_LEVELS) return -1;
        pp.levels = (int)l;
    }
    if (!*rest) return 1;
    if (*rest != ',') return -1;
    q = rest + 1;
    const long w = strtol(q, &rest, 10);
    if (rest == q || w < 1 || w > HSFLOW_PYRAMID_MAX_WARPS) return -1;
    pp.warps = (int)w;
    if (!*rest) return 1;
    if (*rest != ',') return -1;
    q = rest + 1;
    const long r = strtol(q, &rest, 10);
    if (rest == q || *rest || r < 0 || r > 2) return -1;
    pp.median_radius = (int)r;
    return 1;
}

// The filter of pair 0's flow in place; u, v (host copies of the flow, or null) are read again behind it.
int median_step(hsflow_ctx *ctx, int W, int H, std::vector<float> *u, std::vector<float> *v)
{
    int radius, passes;
    bool fill;
    if (median_choice(radius, passes, fill) != 1) return SDK_SUCCESS;
    hsflow_median_params mp;
    hsflow_default_median_params(&mp);
    mp.radius = radius;
    int st;
    if (!fill) {
        st = hsflow_median_apply(ctx, 0, &mp, passes, nullptr, 0, nullptr, 0, nullptr);
    } else {
        mp.mode = HSFLOW_MEDIAN_FILL;
        hsflow_fb_params fp;
        const char *which = nullptr;
        fb_params(fp, &which);
        void *dMask = nullptr, *dStats = nullptr;
        hsflow_median_stats s;
        if (hipMalloc(&dMask, (size_t)W * H) != hipSuccess || hipMalloc(&dStats, sizeof(s)) != hipSuccess) {
            (void)hipFree(dMask);
            std::cout << "hipMalloc of the median's state failed" << std::endl;
            return SDK_FAILURE;
        }
        st = hsflow_fb_device(ctx, 0, 1, &fp, dMask, (size_t)W, nullptr, 0, nullptr);
        if (st == HSFLOW_OK) st = hsflow_median_apply(ctx, 0, &mp, passes, dMask, (size_t)W, nullptr, 0, (hsflow_median_stats *)dStats);
        if (st == HSFLOW_OK) st = hsflow_synchronize(ctx);
        const bool copied = st == HSFLOW_OK && hipMemcpy(&s, dStats, sizeof(s), hipMemcpyDeviceToHost) == hipSuccess;
        (void)hipFree(dMask);
        (void)hipFree(dStats);
        if (st == HSFLOW_OK && !copied) { std::cout << "reading the median's record failed" << std::endl; return SDK_FAILURE; }
        if (st == HSFLOW_OK)
            std::cout << "median: kept " << s.kept << " filled " << s.filled << " unfilled " << s.unfilled << " newly_filled " << s.newly_filled << " changed "
                      << s.changed << std::endl;
    }
    if (st == HSFLOW_OK && u && v && !u->empty()) st = hsflow_get_flow(ctx, 0, u->data(), (size_t)W * 4, v->data(), (size_t)W * 4);
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
    return SDK_SUCCESS;
}

// HSFLOW_REGIONS=<min_area>[,<4|8>[,<join_px>]] on the two "-hd" routes: behind the solve (and HSFLOW_MEDIAN / HSFLOW_PYRAMID)
// the flow is fitted with the HSFLOW_GMOTION choice and mask values {0, 255, 0, 0} -- the pixels that do not follow the
// camera -- and that mask is labelled (hsflow_regions*): one line "regions: kept .. dropped .. foreground .. largest .." and
// at most 16 lines "region k: area .. box x0 y0 x1 y1 centre cx cy motion mu mv".  The picture is unchanged.
// 0: not set, 1: usable, -1: unusable.
constexpr uint32_t kRegionLines = 16;

int regions_choice(hsflow_regions_params &rp)
{
    hsflow_default_regions_params(&rp);
    const char *e = getenv("HSFLOW_REGIONS");
    if (!e || !*e) return 0;
    char *rest = nullptr;
    const long a = strtol(e, &rest, 10);
    if (rest == e || a < 1 || a > (1L << 30)) return -1;
    rp.min_area = (uint32_t)a;
    if (!*rest) return 1;
    if (*rest != ',') return -1;
    const char *q = rest + 1;
    const long c = strtol(q, &rest, 10);
    if (rest == q || (c != 4 && c != 8)) return -1;
    rp.connectivity = (int)c;
    if (!*rest) return 1;
    if (*rest != ',') return -1;
    q = rest + 1;
    const float j = strtof(q, &rest);
    if (rest == q || *rest || !std::isfinite(j) || !(j >= 0.f) || !std::isfinite(j * j) || (j > 0.f && !(j * j > 0.f))) return -1;
    rp.join_px = j;
    return 1;
}

// With HSFLOW_RENDER_DEVICE=1 through hsflow_gmotion_fit_device and hsflow_regions_device (mask and flow stay on the device,
// the records alone are read back), otherwise the host rules on the flow that was read back (u, v); the same lines.
int regions_step(hsflow_ctx *ctx, int W, int H, const std::vector<float> *u, const std::vector<float> *v)
{
    hsflow_regions_params rp;
    if (regions_choice(rp) != 1) return SDK_SUCCESS;
    hsflow_gmotion_params gp;
    gmotion_choice(gp);
    gp.value[0] = 0; gp.value[1] = 255; gp.value[2] = 0; gp.value[3] = 0;
    std::vector<hsflow_regions_record> recs(kRegionLines);
    hsflow_regions_result r;
    int st;
    if (render_on_device()) {
        void *dMask = nullptr, *dOut = nullptr; // dOut: the result header, then the records
        const size_t out_bytes = sizeof(r) + sizeof(hsflow_regions_record) * kRegionLines;
        if (hipMalloc(&dMask, (size_t)W * H) != hipSuccess || hipMalloc(&dOut, out_bytes) != hipSuccess) {
            (void)hipFree(dMask);
            std::cout << "hipMalloc of the regions' mask failed" << std::endl;
            return SDK_FAILURE;
        }
        std::vector<uint8_t> back(out_bytes);
        st = hsflow_gmotion_fit_device(ctx, 0, nullptr, 0, &gp, dMask, (size_t)W, nullptr, nullptr, 0, nullptr);
        if (st == HSFLOW_OK)
            st = hsflow_regions_device(ctx, 0, dMask, (size_t)W, &rp, nullptr, 0, (hsflow_regions_record *)((uint8_t *)dOut + sizeof(r)), kRegionLines,
                                       (hsflow_regions_result *)dOut);
        if (st == HSFLOW_OK) st = hsflow_synchronize(ctx);
        const bool copied = st == HSFLOW_OK && hipMemcpy(back.data(), dOut, out_bytes, hipMemcpyDeviceToHost) == hipSuccess;
        (void)hipFree(dMask);
        (void)hipFree(dOut);
        if (st == HSFLOW_OK && !copied) { std::cout << "reading the regions' records failed" << std::endl; return SDK_FAILURE; }
        if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
        memcpy(&r, back.data(), sizeof(r));
        memcpy(recs.data(), back.data() + sizeof(r), sizeof(hsflow_regions_record) * kRegionLines);
    } else {
        if (!u || !v || u->size() != (size_t)W * H) { std::cout << "HSFLOW_REGIONS: no flow in host memory" << std::endl; return SDK_FAILURE; }
        std::vector<uint8_t> mask((size_t)W * H);
        st = hsflow_gmotion_fit_host(u->data(), v->data(), (size_t)W * 4, nullptr, 0, W, H, &gp, mask.data(), (size_t)W, nullptr, nullptr, 0, nullptr);
        if (st == HSFLOW_OK)
            st = hsflow_regions_host(mask.data(), (size_t)W, u->data(), v->data(), (size_t)W * 4, W, H, &rp, nullptr, 0, recs.data(), kRegionLines, &r);
        if (st != HSFLOW_OK) { std::cout << hsflow_last_error(nullptr) << std::endl; return SDK_FAILURE; }
    }
    std::cout << "regions: kept " << r.n_regions << " dropped " << r.n_dropped << " foreground " << r.fg_px << " largest " << r.largest_area << std::endl;
    for (uint32_t k = 0; k < r.n_written; k++) {
        const hsflow_regions_record &q = recs[k];
        const double nf = q.n_flow ? 256.0 * (double)q.n_flow : 1.0;
        char line[256];
        snprintf(line, sizeof(line), "region %u: area %u box %u %u %u %u centre %.2f %.2f motion %.3f %.3f", k + 1, q.area, (unsigned)q.x0, (unsigned)q.y0,
                 (unsigned)q.x1, (unsigned)q.y1, (double)q.sum_x / q.area, (double)q.sum_y / q.area, (double)q.sum_qu / nf, (double)q.sum_qv / nf);
        std::cout << line << std::endl;
    }
    return SDK_SUCCESS;
}

// The host route of the colour picture: the rule on the host, applied to the flow that was read back.
int color_on_host(pnm::Image &imgFlow, const std::vector<float> &u, const std::vector<float> &v, int W, int H)
{
    imgFlow.width = W; imgFlow.height = H; imgFlow.channels = 3;
    imgFlow.data.resize((size_t)W * H * 3);
    hsflow_color_params cp;
    color_params(cp);
    const int st = hsflow_color_flow_host(u.data(), (size_t)W * 4, v.data(), (size_t)W * 4, W, H, &cp, imgFlow.data.data(), (size_t)W * 3, nullptr);
    if (st != HSFLOW_OK) std::cout << hsflow_last_error(nullptr) << std::endl;
    return st == HSFLOW_OK ? SDK_SUCCESS : SDK_FAILURE;
}

// The device route of both drawings, and of the colour picture: the picture of ctx's current flow into imgFlow.
int draw_on_device(hsflow_ctx *ctx, int preset, int W, int H, pnm::Image &imgFlow, int pair = 0)
{
    imgFlow.width = W; imgFlow.height = H; imgFlow.channels = 3;
    imgFlow.data.resize((size_t)W * H * 3);
    hsflow_render_params rp;
    hsflow_default_render_params(&rp, preset);
    hsflow_color_params cp;
    color_params(cp);
    const int st = color_picture() ? hsflow_color_flow(ctx, pair, &cp, imgFlow.data.data(), (size_t)W * 3, nullptr)
                                   : hsflow_render_flow(ctx, pair, &rp, imgFlow.data.data(), (size_t)W * 3);
    if (st != HSFLOW_OK) std::cout << hsflow_last_error(ctx) << std::endl;
    return st == HSFLOW_OK ? SDK_SUCCESS : SDK_FAILURE;
}

// HSFLOW_JPEG_DEVICE=1 next to HSFLOW_RENDER_DEVICE=1, and an output name ending in .jpg / .jpeg: the file itself comes
// from the device (hsflow_render_flow_jpeg) and is written as it is -- the picture never crosses, only its file.
bool jpeg_on_device(const std::string &output)
{
    const char *e = getenv("HSFLOW_JPEG_DEVICE");
    if (!render_on_device() || !e || atoi(e) == 0 || warp_wanted() || fb_wanted() || interp_wanted() || stab_wanted()) return false; // (the warped frame, the mask and the intermediate frame are written by the host's encoder)
    auto ends = [&](const char *x) {
        const size_t n = std::strlen(x);
        if (output.size() < n) return false;
        for (size_t i = 0; i < n; i++) {
            const char c = output[output.size() - n + i];
            if ((c >= 'A' && c <= 'Z' ? c + 32 : c) != x[i]) return false;
        }
        return true;
    };
    return ends(".jpg") || ends(".jpeg");
}

// The device route of the file: ctx's current flow drawn, encoded (quality 95, as cvSaveImage) and written to `output`.
int save_jpeg_from_device(hsflow_ctx *ctx, int preset, int W, int H, const std::string &output)
{
    hsflow_render_params rp;
    hsflow_default_render_params(&rp, preset);
    hsflow_color_params cp;
    color_params(cp);
    std::vector<uint8_t> file(hsflow_jpeg_bound(W, H));
    size_t n = 0;
    const int st = color_picture() ? hsflow_color_flow_jpeg(ctx, 0, &cp, 95, file.data(), file.size(), &n)
                                   : hsflow_render_flow_jpeg(ctx, 0, &rp, 95, file.data(), file.size(), &n);
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
    FILE *f = fopen(output.c_str(), "wb");
    if (!f) return SDK_FAILURE;
    const bool ok = fwrite(file.data(), 1, n, f) == n;
    return fclose(f) == 0 && ok ? SDK_SUCCESS : SDK_FAILURE;
}

} // namespace

bool picture_choice_usable()
{
    hsflow_color_params cp;
    hsflow_warp_params wp;
    hsflow_fb_params fp;
    const char *which = nullptr;
    if (picture_kind() < 0) { std::cout << "HSFLOW_PICTURE must be color, warp, fb, interp, stab or arrows" << std::endl; return false; }
    if (!fb_params(fp, &which)) { std::cout << which << " must be a finite number >= 0 (alpha at most 1e6, beta at most 1e30)" << std::endl; return false; }
    if (!color_params(cp)) { std::cout << "HSFLOW_COLOR_MAX must be a finite number > 0" << std::endl; return false; }
    if (!warp_params(wp)) { std::cout << "HSFLOW_WARP_T must be a finite number, at most 1e6 in magnitude" << std::endl; return false; }
    hsflow_gmotion_params gmp;
    if (!gmotion_choice(gmp)) { std::cout << "HSFLOW_GMOTION must be translation, similarity or affine[,<passes 1..8>[,<px>|auto]]" << std::endl; return false; }
    float t;
    if (!interp_time(t)) { std::cout << "HSFLOW_INTERP_T must be a number in 0 .. 1" << std::endl; return false; }
    int radius, passes;
    bool fill;
    if (median_choice(radius, passes, fill) < 0) { std::cout << "HSFLOW_MEDIAN must be <radius 1 or 2>[,<passes 1 .. 64>[,fill]]" << std::endl; return false; }
    hsflow_pyramid_params pp;
    if (pyramid_choice(pp) < 0) { std::cout << "HSFLOW_PYRAMID must be <levels 1 .. 8 or auto>[,<warps 1 .. 8>[,<median radius 0, 1 or 2>]]" << std::endl; return false; }
    hsflow_regions_params rgp;
    if (regions_choice(rgp) < 0) { std::cout << "HSFLOW_REGIONS must be <min_area 1 .. 2^30>[,<4 or 8>[,<join_px, a finite number >= 0>]]" << std::endl; return false; }
    return true;
}

bool pyramid_wanted()
{
    hsflow_pyramid_params pp;
    return pyramid_choice(pp) == 1;
}

bool median_wanted()
{
    int radius, passes;
    bool fill;
    return median_choice(radius, passes, fill) == 1;
}

// HSFLOW_MEDIAN=..,fill and HSFLOW_PICTURE=interp with HSFLOW_INTERP_FB=1 need the reversed pair beside the pair, as
// HSFLOW_PICTURE=fb does.
static bool reversed_pair_wanted()
{
    int radius, passes;
    bool fill;
    return fb_wanted() || (interp_wanted() && interp_fb()) || (median_choice(radius, passes, fill) == 1 && fill);
}

bool warp_wanted() { return picture_kind() == 2; }
bool stab_wanted() { return picture_kind() == 5; }

bool fb_wanted() { return picture_kind() == 3; }

bool interp_wanted() { return picture_kind() == 4; }

HSOpticalFlowOpenCL::HSOpticalFlowOpenCL(const char *name, char *src_, char *in1, char *in2, char *out, float alp,
                                         int it, int gs, char *dType)
    : SDKSample(name), alpha(alp), iterations(it), blockSizeX(gs), src(src_ ? src_ : ""), input1(in1 ? in1 : ""),
      input2(in2 ? in2 : ""), output(out ? out : "")
{
    gpu = !(dType && strcmp(dType, "CPU") == 0); // HSOpticalFlowOpenCL.hpp:157-160
}

HSOpticalFlowOpenCL::HSOpticalFlowOpenCL(const char *name, char *src_, float alp, int it, int gs, char *dType)
    : SDKSample(name), alpha(alp), iterations(it), blockSizeX(gs), src(src_ ? src_ : "")
{
    gpu = !(dType && strcmp(dType, "CPU") == 0);
}

HSOpticalFlowOpenCL::~HSOpticalFlowOpenCL() { cleanup(); }

int HSOpticalFlowOpenCL::initialize() { return SDKSample::initialize(); }
int HSOpticalFlowOpenCL::setup() { return SDK_SUCCESS; }

// The reference's stub (:894) answered SDK_SUCCESS whatever happened; before any pair has been solved that answer is kept.
int HSOpticalFlowOpenCL::verifyResults()
{
    if (!ctx || !solved) return SDK_SUCCESS;
    return verify_pair(ctx, (int)width, report);
}

int HSOpticalFlowOpenCL::cleanup()
{
    if (ctx) { hsflow_destroy(ctx); ctx = nullptr; }
    solved = false;
    return SDK_SUCCESS;
}

int HSOpticalFlowOpenCL::ensureContext(int w, int h)
{
    if (ctx && (unsigned)w == width && (unsigned)h == height) return SDK_SUCCESS;
    cleanup();
    if (hsflow_create(&ctx, 0, w, h, reversed_pair_wanted() && src == "-hd" ? 2 : 1, nullptr, 1) != HSFLOW_OK) { // (HSFLOW_PICTURE=fb, HSFLOW_MEDIAN=..,fill: the reversed pair beside it)
        std::cout << "hsflow_create: " << hsflow_last_error(nullptr) << std::endl;
        ctx = nullptr;
        return SDK_FAILURE;
    }
    width = w; height = h;
    u.assign((size_t)w * h, 0.f);
    v.assign((size_t)w * h, 0.f);
    return SDK_SUCCESS;
}

int HSOpticalFlowOpenCL::solvePair(const pnm::Image &a, const pnm::Image &b, bool streaming, bool frames_set)
{
    int st = frames_set ? HSFLOW_OK : streaming ? hsflow_push_frame_u8(ctx, 0, b.data.data(), b.width)
                       : hsflow_set_frames_u8(ctx, 0, a.data.data(), a.width, b.data.data(), b.width);
    if (st == HSFLOW_OK && reversed_pair_wanted() && src == "-hd") st = hsflow_set_frames_reversed(ctx, 1, 0);
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
    hsflow_params p;
    hsflow_default_params(&p);
    // the "-cl" route keeps the reference kernels' own discretisation (Kernels.cl: cube derivatives,
    // 1/6-1/12 mean, alpha^2) -- with the v update the reference forgot; HSFLOW_CL_AS_CV=1 switches
    // to the OpenCV discretisation with the equivalent regulariser lambda = 1/alpha^2,
    // HSFLOW_CL_AS_SHIPPED=1 to Kernels.cl as shipped (v never written: the reference's pictures)
    if (getenv("HSFLOW_CL_AS_CV")) p.lambda = 1.0f / (alpha * alpha);
    else { p.mode = getenv("HSFLOW_CL_AS_SHIPPED") ? HSFLOW_MODE_CLASSIC_AS_SHIPPED : HSFLOW_MODE_CLASSIC; p.alpha = alpha; }
    p.term_type = HSFLOW_TERM_ITER;        // the reference loop runs a fixed count (:750-751)
    p.max_iter = iterations;
    const double t0 = now_ms();
    st = hsflow_solve(ctx, &p);
    if (st == HSFLOW_OK && !render_on_device()) st = hsflow_get_flow(ctx, 0, u.data(), (size_t)width * 4, v.data(), (size_t)width * 4);
    lastMs = now_ms() - t0;
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
    solved = true;
    return SDK_SUCCESS;
}

// Arrow rendering of the reference (HSOpticalFlowOpenCL.cpp:762-770): 4-pixel grid, |u| or |v| > 0.5,
// blue dot + red full-length line.  With HSFLOW_RENDER_DEVICE=1 the device draws it (u and v stay where they are).
int HSOpticalFlowOpenCL::drawFlow(pnm::Image &imgFlow) const
{
    if (render_on_device()) return draw_on_device(ctx, HSFLOW_RENDER_CL, (int)width, (int)height, imgFlow);
    if (color_picture()) return color_on_host(imgFlow, u, v, (int)width, (int)height);
    imgFlow.width = width; imgFlow.height = height; imgFlow.channels = 3;
    imgFlow.data.assign((size_t)width * height * 3, 0);
    const int step = 4;
    for (unsigned i = 0; i < height; i += step)
        for (unsigned j = 0; j < width; j += step) {
            const float fu = u[j + (size_t)i * width], fv = v[j + (size_t)i * width];
            if (fu > 0.5f || fv > 0.5f || fu < -0.5f || fv < -0.5f) {
                pnm::filled_circle(imgFlow, j, i, 2, 0, 0, 255);
                pnm::line(imgFlow, j, i, (int)(j + fu), (int)(i + fv), 255, 0, 0);
            }
        }
    return SDK_SUCCESS;
}

// HSFLOW_JPEG_IN_DEVICE=1 on the two "-hd" routes: input files that are JPEG are handed to hsflow_set_frames_jpeg as
// they are -- decoded on the device, only their entropy-coded bytes cross PCIe -- instead of jpegb::load and an upload
// of 3 bytes per pixel.  PGM / PPM inputs, and everything without the switch, go the way they always went.
static bool jpeg_in_device()
{
    const char *e = getenv("HSFLOW_JPEG_IN_DEVICE");
    return e && e[0] == '1';
}

static bool read_jpeg_file(const std::string &path, std::vector<uint8_t> &buf)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t tmp[65536];
    size_t n;
    buf.clear();
    while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
    fclose(f);
    return buf.size() >= 2 && buf[0] == 0xFF && buf[1] == 0xD8;
}

// Both inputs as JPEG files whose headers the library accepts and that agree in size: that size, else false.
static bool jpeg_pair(const std::string &in1, const std::string &in2, std::vector<uint8_t> &f1, std::vector<uint8_t> &f2, int &W, int &H)
{
    if (!jpeg_in_device() || !read_jpeg_file(in1, f1) || !read_jpeg_file(in2, f2)) return false;
    hsflow_jpeg_info i1, i2;
    i1.struct_size = i2.struct_size = sizeof(hsflow_jpeg_info);
    if (hsflow_jpeg_read_header(f1.data(), f1.size(), &i1) != HSFLOW_OK || hsflow_jpeg_read_header(f2.data(), f2.size(), &i2) != HSFLOW_OK) return false;
    if (i1.width != i2.width || i1.height != i2.height) return false;
    W = i1.width; H = i1.height;
    return true;
}

int HSOpticalFlowOpenCL::run()
{
    if (!gpu) {
        std::cout << "dType CPU is not available in this build (GPU only)." << std::endl;
        return SDK_FAILURE;
    }
    if (!(alpha > 0.f) || iterations <= 0) {
        std::cout << "alpha and the iteration count must be positive." << std::endl;
        return SDK_FAILURE;
    }
    if (src == "-hd") {
        pnm::Image c1, c2, g1, g2;
        std::vector<uint8_t> f1, f2;
        int jw = 0, jh = 0;
        const bool from_files = jpeg_pair(input1, input2, f1, f2, jw, jh);
        if (from_files) {
            if (ensureContext(jw, jh) != SDK_SUCCESS) return SDK_FAILURE;
            if (hsflow_set_frames_jpeg(ctx, 0, f1.data(), f1.size(), f2.data(), f2.size(), 0) != HSFLOW_OK) {
                std::cout << hsflow_last_error(ctx) << std::endl;
                return SDK_FAILURE;
            }
            if (solvePair(g1, g2, false, true) != SDK_SUCCESS) return SDK_FAILURE;
        } else {
        if (!pnm::load_image(input1, c1) || !pnm::load_image(input2, c2)) {
            std::cout << "Input image error.\n";
            return -1; // HSOpticalFlowOpenCL.cpp:724,735
        }
        pnm::to_gray(c1, g1);
        pnm::to_gray(c2, g2);
        if (g1.width != g2.width || g1.height != g2.height) { std::cout << "Input image error.\n"; return -1; }
        if (ensureContext(g1.width, g1.height) != SDK_SUCCESS) return SDK_FAILURE;
        if (solvePair(g1, g2, false) != SDK_SUCCESS) return SDK_FAILURE;
        }
        std::cout << "Avg time: " << lastMs << " [ms]" << std::endl; // :755
        const int verdict = verify_wanted() ? verifyResults() : SDK_SUCCESS;
        if (median_step(ctx, (int)width, (int)height, render_on_device() ? nullptr : &u, render_on_device() ? nullptr : &v) != SDK_SUCCESS) return SDK_FAILURE;
        if (regions_step(ctx, (int)width, (int)height, render_on_device() ? nullptr : &u, render_on_device() ? nullptr : &v) != SDK_SUCCESS) return SDK_FAILURE;
        if (jpeg_on_device(output)) return save_jpeg_from_device(ctx, HSFLOW_RENDER_CL, (int)width, (int)height, output) == SDK_SUCCESS ? verdict : SDK_FAILURE;
        pnm::Image imgFlow;
        if (warp_wanted()) {
            if (from_files && (!pnm::load_image(input1, c1) || !pnm::load_image(input2, c2))) { std::cout << "Input image error.\n"; return -1; }
            if (warp_picture(ctx, c1, c2, u, v, imgFlow) != SDK_SUCCESS) return SDK_FAILURE;
        } else if (stab_wanted()) {
            if (from_files && (!pnm::load_image(input1, c1) || !pnm::load_image(input2, c2))) { std::cout << "Input image error.\n"; return -1; }
            if (stab_picture(ctx, c1, c2, u, v, imgFlow) != SDK_SUCCESS) return SDK_FAILURE;
        } else if (interp_wanted()) {
            if (from_files && (!pnm::load_image(input1, c1) || !pnm::load_image(input2, c2))) { std::cout << "Input image error.\n"; return -1; }
            if (interp_picture(ctx, c1, c2, u, v, imgFlow) != SDK_SUCCESS) return SDK_FAILURE;
        } else if (fb_wanted()) {
            if (fb_picture(ctx, (int)width, (int)height, imgFlow) != SDK_SUCCESS) return SDK_FAILURE;
        } else if (drawFlow(imgFlow) != SDK_SUCCESS) return SDK_FAILURE;
        if (!output.empty() && !pnm::save_image(output, imgFlow)) return SDK_FAILURE;
        return verdict;
    }
    // "-cam": previous frame stays on the device, only the new frame is uploaded (:810-834)
    pnm::Image prev, cur, gprev, gcur;
    if (!pnm::load_image(camera_frame(0), prev)) { std::cerr << "ERROR: capture is NULL \n"; return -1; }
    pnm::to_gray(prev, gprev);
    if (ensureContext(gprev.width, gprev.height) != SDK_SUCCESS) return SDK_FAILURE;
    double total = 0.0;
    int count = 0, verdict = SDK_SUCCESS;
    for (int i = 1; pnm::load_image(camera_frame(i), cur); i++) {
        pnm::to_gray(cur, gcur);
        if (gcur.width != gprev.width || gcur.height != gprev.height) break;
        if (solvePair(gprev, gcur, count > 0) != SDK_SUCCESS) return SDK_FAILURE;
        total += lastMs;
        count++;
        if (verify_wanted() && verifyResults() != SDK_SUCCESS) verdict = SDK_FAILURE;
        if (getenv("HSFLOW_CAMERA_OUT")) {
            pnm::Image imgFlow;
            if (drawFlow(imgFlow) != SDK_SUCCESS) return SDK_FAILURE;
            char name[64];
            snprintf(name, sizeof(name), "/flow_%04d.ppm", i);
            pnm::save_image(std::string(getenv("HSFLOW_CAMERA_OUT")) + name, imgFlow);
        }
        gprev = gcur;
    }
    if (count) std::cout << "Avg time: " << total / count << " [ms]" << std::endl; // :838
    return verdict;
}

// ---- GPU counterpart of OpticalFlowOpenCV (OpticalFlowHS/OpticalFlowOpenCV.cpp:7-52) --------------

// arrows of the CPU route: 4-pixel grid, |.| > 1, half length (OpticalFlowOpenCV.cpp:33-46, :98-111); with
// HSFLOW_PICTURE=color the dense colour picture instead
static void draw_cv_flow(pnm::Image &imgFlow, const std::vector<float> &u, const std::vector<float> &v, int W, int H)
{
    if (color_picture()) { (void)color_on_host(imgFlow, u, v, W, H); return; } // (its arguments were checked at the start)
    imgFlow.width = W; imgFlow.height = H; imgFlow.channels = 3;
    imgFlow.data.assign((size_t)W * H * 3, 0);
    for (int y = 0; y < H; y += 4)
        for (int x = 0; x < W; x += 4) {
            const float px = u[(size_t)y * W + x], py = v[(size_t)y * W + x];
            if (px > 1 || py > 1 || px < -1 || py < -1) {
                pnm::filled_circle(imgFlow, x, y, 2, 0, 0, 255);
                pnm::line(imgFlow, x, y, (int)(x + px / 2), (int)(y + py / 2), 255, 0, 0);
            }
        }
}

int OpticalFlowOpenCV::runFromImg(char *input1, char *input2, char *output, float lambda, int it)
{
    pnm::Image c1, c2;
    std::vector<uint8_t> f1, f2;
    int jw = 0, jh = 0;
    const bool from_files = jpeg_pair(input1, input2, f1, f2, jw, jh);
    if (!from_files && (!pnm::load_image(input1, c1) || !pnm::load_image(input2, c2) || c1.width != c2.width || c1.height != c2.height)) {
        std::cout << "Input image error.\n";
        return -1;
    }
    const int W = from_files ? jw : c1.width, H = from_files ? jh : c1.height;
    hsflow_ctx *ctx = nullptr;
    if (hsflow_create(&ctx, 0, W, H, reversed_pair_wanted() ? 2 : 1, nullptr, 1) != HSFLOW_OK) { std::cout << hsflow_last_error(nullptr) << std::endl; return 1; } // (fb, median fill: the reversed pair beside it)
    int st;
    const double t0 = now_ms();
    if (from_files) { // cvLoadImage + cvCvtColor + cvSmooth, all on the device
        st = hsflow_set_frames_jpeg(ctx, 0, f1.data(), f1.size(), f2.data(), f2.size(), 1);
    } else if (c1.channels == 3) { // PPM is RGB; the C ABI takes BGR like cvLoadImage delivers
        std::vector<uint8_t> b1(c1.data), b2(c2.data);
        for (size_t i = 0; i < b1.size(); i += 3) { std::swap(b1[i], b1[i + 2]); std::swap(b2[i], b2[i + 2]); }
        st = hsflow_set_frames_bgr8(ctx, 0, b1.data(), (size_t)W * 3, b2.data(), (size_t)W * 3, 1); // gray + cvSmooth(CV_BLUR,3,3)
    } else {
        st = hsflow_set_frames_gray8_blur(ctx, 0, c1.data.data(), (size_t)W, c2.data.data(), (size_t)W);
    }
    if (st == HSFLOW_OK && reversed_pair_wanted()) st = hsflow_set_frames_reversed(ctx, 1, 0);
    hsflow_params p;
    hsflow_default_params(&p);          // ITER|EPS, eps = (float)1e-6 as at OpticalFlowOpenCV.cpp:29
    p.lambda = lambda;
    p.max_iter = it;
    const bool on_device = render_on_device();
    std::vector<float> u, v;
    if (!on_device) { u.resize((size_t)W * H); v.resize((size_t)W * H); }
    hsflow_pyramid_params pyr;
    const bool pyramid = pyramid_choice(pyr) == 1; // HSFLOW_PYRAMID: the coarse-to-fine solve in the solve's place
    if (st == HSFLOW_OK) st = pyramid ? hsflow_solve_pyramid(ctx, &p, &pyr) : hsflow_solve(ctx, &p);
    if (st == HSFLOW_OK && !on_device) st = hsflow_get_flow(ctx, 0, u.data(), (size_t)W * 4, v.data(), (size_t)W * 4);
    const double ms = now_ms() - t0;
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; hsflow_destroy(ctx); return 1; }
    hsflow_verify_report report;
    const int verdict = verify_wanted() ? verify_pair(ctx, W, report) : SDK_SUCCESS; // (the context goes away below)
    if (median_step(ctx, W, H, on_device ? nullptr : &u, on_device ? nullptr : &v) != SDK_SUCCESS) { hsflow_destroy(ctx); return 1; }
    if (regions_step(ctx, W, H, on_device ? nullptr : &u, on_device ? nullptr : &v) != SDK_SUCCESS) { hsflow_destroy(ctx); return 1; }
    pnm::Image imgFlow;
    const bool file_on_device = jpeg_on_device(output ? output : "");
    if (file_on_device) {
        if (save_jpeg_from_device(ctx, HSFLOW_RENDER_CV, W, H, output) != SDK_SUCCESS) { hsflow_destroy(ctx); return 1; }
    } else if (warp_wanted()) {
        if (from_files && (!pnm::load_image(input1, c1) || !pnm::load_image(input2, c2))) { std::cout << "Input image error.\n"; hsflow_destroy(ctx); return -1; }
        if (warp_picture(ctx, c1, c2, u, v, imgFlow) != SDK_SUCCESS) { hsflow_destroy(ctx); return 1; }
    } else if (stab_wanted()) {
        if (from_files && (!pnm::load_image(input1, c1) || !pnm::load_image(input2, c2))) { std::cout << "Input image error.\n"; hsflow_destroy(ctx); return -1; }
        if (stab_picture(ctx, c1, c2, u, v, imgFlow) != SDK_SUCCESS) { hsflow_destroy(ctx); return 1; }
    } else if (interp_wanted()) {
        if (from_files && (!pnm::load_image(input1, c1) || !pnm::load_image(input2, c2))) { std::cout << "Input image error.\n"; hsflow_destroy(ctx); return -1; }
        if (interp_picture(ctx, c1, c2, u, v, imgFlow) != SDK_SUCCESS) { hsflow_destroy(ctx); return 1; }
    } else if (fb_wanted()) {
        if (fb_picture(ctx, W, H, imgFlow) != SDK_SUCCESS) { hsflow_destroy(ctx); return 1; }
    } else if (on_device && draw_on_device(ctx, HSFLOW_RENDER_CV, W, H, imgFlow) != SDK_SUCCESS) { hsflow_destroy(ctx); return 1; }
    hsflow_destroy(ctx);
    if (!on_device && !warp_wanted() && !fb_wanted() && !interp_wanted() && !stab_wanted()) draw_cv_flow(imgFlow, u, v, W, H);
    if (!file_on_device) pnm::save_image(output, imgFlow);
    std::cout << "Avg time: " << ms << " [ms]" << std::endl;
    return verdict;
}

// The camera loop of the CPU route (OpticalFlowOpenCV.cpp:56-131) on numbered frame files instead of a
// capture device ($HSFLOW_CAMERA_DIR, see camera_frame).  Faithful to the reference's loop, including
// its quirk: cvSmooth works in place and the blurred new frame becomes the next old frame (:93,:117),
// so from the second pair on the old frame enters the solver blurred TWICE.  The blurred frames never
// leave the device: from the second pair on hsflow_push_frame_ex blurs the resident new frame once more into
// the old one's plane and only the next gray frame is uploaded.
// HSFLOW_CAMERA_BATCH=n (1 .. 256) on the "-cv -cam" route: the loop below in batches of n pairs.  0: not set; -1: unusable.
static int camera_batch()
{
    const char *e = getenv("HSFLOW_CAMERA_BATCH");
    if (!e || !*e) return 0;
    char *rest = nullptr;
    const long v = strtol(e, &rest, 10);
    return *rest || v < 1 || v > 256 ? -1 : (int)v;
}

// HSFLOW_CAMERA_CHAIN=1 on the batched "-cv -cam" route: beside the flow_%04d.ppm files every batch writes chain_%04d.ppm
// (numbered like the flow picture of its last pair), the colour picture (AUTO scale) of the flow from the batch's first frame
// to its last -- every pixel followed through the batch's flows (hsflow_chain_flow) -- and prints one line
// "chain %04d: model p0 .. p5 inliers <share>", the global motion fitted to that flow (hsflow_gmotion_fit_host; HSFLOW_GMOTION
// selects the fit).  0: not set (or "0"); -1: unusable.
static int camera_chain()
{
    const char *e = getenv("HSFLOW_CAMERA_CHAIN");
    if (!e || !*e || strcmp(e, "0") == 0) return 0;
    return strcmp(e, "1") == 0 ? 1 : -1;
}

// The chained flow of ctx's m pairs into U, V (W x H, packed): HSFLOW_CHAIN_MAX_PAIRS pairs per call, a longer batch
// continues from the call before through the start planes.
static int chain_batch(hsflow_ctx *ctx, int m, int W, int H, std::vector<float> &U, std::vector<float> &V)
{
    hsflow_chain_params cp;
    hsflow_default_chain_params(&cp);
    const size_t px = (size_t)W * H, row = (size_t)W * 4;
    std::vector<float> U0, V0;
    U.resize(px); V.resize(px);
    for (int first = 0; first < m; first += HSFLOW_CHAIN_MAX_PAIRS) {
        const int n = m - first < HSFLOW_CHAIN_MAX_PAIRS ? m - first : HSFLOW_CHAIN_MAX_PAIRS;
        int pairs[HSFLOW_CHAIN_MAX_PAIRS];
        for (int k = 0; k < n; k++) pairs[k] = first + k;
        if (first) { U0.swap(U); V0.swap(V); U.resize(px); V.resize(px); }
        const int st = hsflow_chain_flow(ctx, pairs, n, nullptr, 0, first ? U0.data() : nullptr, first ? V0.data() : nullptr, row, &cp, U.data(), V.data(), row,
                                         nullptr, 0, nullptr, 0, nullptr);
        if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
    }
    return SDK_SUCCESS;
}

// HSFLOW_CAMERA_OBJECTS=<min_area>[,<share 0..256>] on the batched "-cv -cam" route: every batch writes objects_%04d.txt
// (numbered like the flow picture of its last pair), the moving objects of its pairs with ids that hold over the batch.  Per
// batch, all on the device: the fit's foreground mask of every pair (HSFLOW_GMOTION selects the fit, mask values {0, 255, 0,
// 0}), hsflow_regions_batch_device with min_area and 256 records, hsflow_link_regions_batch_device at caps 256 from each
// pair's labels to the next pair's, then hsflow_link_tracks_host with the share (default 128) on the records that came back.
// One line per region: "frame id area x0 y0 x1 y1 sum_x sum_y n_flow sum_qu sum_qv", frame the pair's old frame.  Ids start
// at 1 in every batch.  0: not set, 1: usable, -1: unusable.
constexpr uint32_t kObjectsCap = 256;

static int camera_objects(uint32_t &min_area, uint32_t &share)
{
    min_area = 1; share = 128;
    const char *e = getenv("HSFLOW_CAMERA_OBJECTS");
    if (!e || !*e) return 0;
    char *rest = nullptr;
    const long a = strtol(e, &rest, 10);
    if (rest == e || a < 1 || a > (1L << 30)) return -1;
    min_area = (uint32_t)a;
    if (!*rest) return 1;
    if (*rest != ',') return -1;
    const char *q = rest + 1;
    const long sh = strtol(q, &rest, 10);
    if (rest == q || *rest || sh < 0 || sh > 256) return -1;
    share = (uint32_t)sh;
    return 1;
}

// dBuf / dBufBytes: the batch's planes and records on the device, grown here and kept by the caller across the batches.
static int objects_batch(hsflow_ctx *ctx, int m, int W, int H, int first_frame, uint32_t min_area, uint32_t share, const std::string &path, void *&dBuf,
                         size_t &dBufBytes)
{
    hsflow_gmotion_params gp;
    gmotion_choice(gp);
    gp.value[0] = 0; gp.value[1] = 255; gp.value[2] = 0; gp.value[3] = 0;
    hsflow_regions_params rp;
    hsflow_default_regions_params(&rp);
    rp.min_area = min_area;
    hsflow_link_params lp;
    hsflow_default_link_params(&lp);
    lp.cap_a = lp.cap_b = kObjectsCap;
    const size_t px = (size_t)W * H, rec_bytes = sizeof(hsflow_regions_record) * kObjectsCap, side_bytes = sizeof(hsflow_link_side) * kObjectsCap;
    // what comes back first (heads, records, sides), then the label planes and the masks
    const size_t back_bytes = (sizeof(hsflow_regions_result) + rec_bytes + 2 * side_bytes) * (size_t)m;
    const size_t need = back_bytes + px * 5 * (size_t)m;
    if (dBufBytes < need) {
        if (dBuf) (void)hipFree(dBuf);
        dBuf = nullptr; dBufBytes = 0;
        if (hipMalloc(&dBuf, need) != hipSuccess) { std::cout << "hipMalloc of the objects' planes failed" << std::endl; return SDK_FAILURE; }
        dBufBytes = need;
    }
    uint8_t *d = (uint8_t *)dBuf;
    uint8_t *dHeads = d, *dRecs = dHeads + sizeof(hsflow_regions_result) * (size_t)m, *dSa = dRecs + rec_bytes * (size_t)m, *dSb = dSa + side_bytes * (size_t)m;
    uint8_t *dLabels = d + back_bytes, *dMasks = dLabels + px * 4 * (size_t)m;
    std::vector<void *> masks, labels, recs, sa, sb;
    for (int k = 0; k < m; k++) {
        masks.push_back(dMasks + px * (size_t)k);
        labels.push_back(dLabels + px * 4 * (size_t)k);
        recs.push_back(dRecs + rec_bytes * (size_t)k);
        sa.push_back(dSa + side_bytes * (size_t)k);
        sb.push_back(dSb + side_bytes * (size_t)k);
    }
    int st = hsflow_gmotion_fit_batch_device(ctx, 0, m, nullptr, 0, &gp, masks.data(), (size_t)W, nullptr, nullptr, 0, nullptr);
    if (st == HSFLOW_OK)
        st = hsflow_regions_batch_device(ctx, 0, m, (const void *const *)masks.data(), (size_t)W, &rp, labels.data(), (size_t)W * 4, recs.data(), kObjectsCap,
                                         (hsflow_regions_result *)dHeads);
    if (st == HSFLOW_OK && m > 1)
        st = hsflow_link_regions_batch_device(ctx, 0, m - 1, (const void *const *)labels.data(), (size_t)W * 4, &lp, nullptr, 0, sa.data(), sb.data(), nullptr);
    if (st == HSFLOW_OK) st = hsflow_synchronize(ctx);
    std::vector<uint8_t> back(back_bytes);
    const bool copied = st == HSFLOW_OK && hipMemcpy(back.data(), d, back_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
    if (!copied) { std::cout << "reading the objects' records failed" << std::endl; return SDK_FAILURE; }
    const hsflow_regions_result *heads = (const hsflow_regions_result *)back.data();
    const hsflow_regions_record *records = (const hsflow_regions_record *)(back.data() + (dRecs - d));
    const hsflow_link_side *sides_a = (const hsflow_link_side *)(back.data() + (dSa - d)), *sides_b = (const hsflow_link_side *)(back.data() + (dSb - d));
    std::vector<const hsflow_link_side *> pa, pb;
    std::vector<uint32_t> counts;
    for (int k = 0; k < m; k++) {
        counts.push_back(heads[k].n_regions);
        if (k + 1 < m) { pa.push_back(sides_a + (size_t)kObjectsCap * k); pb.push_back(sides_b + (size_t)kObjectsCap * k); }
    }
    std::vector<uint32_t> ids((size_t)m * kObjectsCap);
    if (hsflow_link_tracks_host(pa.data(), pb.data(), counts.data(), m - 1, kObjectsCap, share, ids.data(), nullptr) != HSFLOW_OK) {
        std::cout << hsflow_last_error(nullptr) << std::endl;
        return SDK_FAILURE;
    }
    FILE *f = fopen(path.c_str(), "w");
    if (!f) { std::cout << "cannot write " << path << std::endl; return SDK_FAILURE; }
    for (int k = 0; k < m; k++)
        for (uint32_t j = 0; j < heads[k].n_written; j++) {
            const hsflow_regions_record &q = records[(size_t)kObjectsCap * k + j];
            fprintf(f, "%d %u %u %u %u %u %u %llu %llu %u %lld %lld\n", first_frame + k, ids[(size_t)kObjectsCap * k + j], q.area, (unsigned)q.x0, (unsigned)q.y0,
                    (unsigned)q.x1, (unsigned)q.y1, (unsigned long long)q.sum_x, (unsigned long long)q.sum_y, q.n_flow, (long long)q.sum_qu, (long long)q.sum_qv);
        }
    fclose(f);
    return SDK_SUCCESS;
}

// HSFLOW_CAMERA_POINTS=<n>[,<quality_q16>[,<nms_r>]] on the batched "-cv -cam" route: every batch writes points_%04d.txt
// (numbered like the flow picture of its last pair).  Per batch, all on the device: the n best corners of the batch's first
// frame as the context holds it (hsflow_corners_device, pair 0, the prev plane; the defaults but for quality and radius),
// whose xy array goes as it is into hsflow_track_points_device over the batch's pairs (its first HSFLOW_CHAIN_MAX_PAIRS, if
// the batch is longer) -- no read-back in between.  One line per written corner: "rank x0 y0 score x y status age", x0 y0
// the corner, x y where the flows took it (nan once it is lost), status and age the tracker's.  0: not set, 1: usable,
// -1: unusable.
static int camera_points(uint32_t &n, uint32_t &quality, int &nms_r)
{
    hsflow_corners_params cp;
    hsflow_default_corners_params(&cp);
    n = 0; quality = cp.quality_q16; nms_r = cp.nms_r;
    const char *e = getenv("HSFLOW_CAMERA_POINTS");
    if (!e || !*e) return 0;
    char *rest = nullptr;
    const long a = strtol(e, &rest, 10);
    if (rest == e || a < 1 || a > (long)HSFLOW_CORNERS_MAX_CANDIDATES) return -1;
    n = (uint32_t)a;
    if (!*rest) return 1;
    if (*rest != ',') return -1;
    const char *q = rest + 1;
    const long qu = strtol(q, &rest, 10);
    if (rest == q || qu < 0 || qu > 65535) return -1;
    quality = (uint32_t)qu;
    if (!*rest) return 1;
    if (*rest != ',') return -1;
    q = rest + 1;
    const long r = strtol(q, &rest, 10);
    if (rest == q || *rest || r < 1 || r > 8) return -1;
    nms_r = (int)r;
    return 1;
}

// dBuf / dBufBytes: the batch's records and points on the device, grown here and kept by the caller across the batches.
static int points_batch(hsflow_ctx *ctx, int m, uint32_t n, uint32_t quality, int nms_r, const std::string &path, void *&dBuf, size_t &dBufBytes)
{
    hsflow_corners_params cp;
    hsflow_default_corners_params(&cp);
    cp.quality_q16 = quality;
    cp.nms_r = nms_r;
    hsflow_chain_params chp;
    hsflow_default_chain_params(&chp);
    // what comes back (header, records, last positions, status, age), then the corners' xy, which stays on the device
    const size_t rec_bytes = sizeof(hsflow_corners_record) * (size_t)n, xy_bytes = 8 * (size_t)n, byte_bytes = ((size_t)n + 7) & ~(size_t)7;
    const size_t back_bytes = sizeof(hsflow_corners_result) + rec_bytes + xy_bytes + 2 * byte_bytes, need = back_bytes + xy_bytes;
    if (dBufBytes < need) {
        if (dBuf) (void)hipFree(dBuf);
        dBuf = nullptr; dBufBytes = 0;
        if (hipMalloc(&dBuf, need) != hipSuccess) { std::cout << "hipMalloc of the points failed" << std::endl; return SDK_FAILURE; }
        dBufBytes = need;
    }
    uint8_t *d = (uint8_t *)dBuf;
    uint8_t *dHead = d, *dRecs = dHead + sizeof(hsflow_corners_result), *dLast = dRecs + rec_bytes, *dStatus = dLast + xy_bytes, *dAge = dStatus + byte_bytes;
    uint8_t *dXy = d + back_bytes;
    const int steps = m < HSFLOW_CHAIN_MAX_PAIRS ? m : HSFLOW_CHAIN_MAX_PAIRS;
    int pairs[HSFLOW_CHAIN_MAX_PAIRS];
    for (int k = 0; k < steps; k++) pairs[k] = k;
    int st = hsflow_corners_device(ctx, 0, 0, nullptr, 0, &cp, (hsflow_corners_record *)dRecs, n, (float *)dXy, (hsflow_corners_result *)dHead);
    if (st == HSFLOW_OK) st = hsflow_track_points_device(ctx, pairs, steps, nullptr, 0, &chp, (const float *)dXy, (int)n, nullptr, (float *)dLast, dStatus, dAge, nullptr);
    if (st == HSFLOW_OK) st = hsflow_synchronize(ctx);
    std::vector<uint8_t> back(back_bytes);
    const bool copied = st == HSFLOW_OK && hipMemcpy(back.data(), d, back_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return SDK_FAILURE; }
    if (!copied) { std::cout << "reading the points failed" << std::endl; return SDK_FAILURE; }
    const hsflow_corners_result *head = (const hsflow_corners_result *)back.data();
    const hsflow_corners_record *recs = (const hsflow_corners_record *)(back.data() + (dRecs - d));
    const float *last = (const float *)(back.data() + (dLast - d));
    const uint8_t *status = back.data() + (dStatus - d), *age = back.data() + (dAge - d);
    FILE *f = fopen(path.c_str(), "w");
    if (!f) { std::cout << "cannot write " << path << std::endl; return SDK_FAILURE; }
    auto num = [](float a) {
        char text[32];
        if (a != a) snprintf(text, sizeof(text), "nan");
        else snprintf(text, sizeof(text), "%.9g", (double)a);
        return std::string(text);
    };
    for (uint32_t k = 0; k < head->n_written; k++)
        fprintf(f, "%u %u %u %lld %s %s %u %u\n", k, (unsigned)recs[k].x, (unsigned)recs[k].y, (long long)recs[k].score, num(last[2 * k]).c_str(),
                num(last[2 * k + 1]).c_str(), (unsigned)status[k], (unsigned)age[k]);
    fclose(f);
    return SDK_SUCCESS;
}

static bool ends_with_jpg(const std::string &s) { return s.size() >= 4 && s.compare(s.size() - 4, 4, ".jpg") == 0; }

// The same loop with up to n + 1 frames read ahead: ONE hsflow_set_sequence_* call and ONE hsflow_solve per batch on a
// context of n pairs whose pairs stop on their own Eps (hsflow_set_pair_termination), as the loop's calls of
// cvCalcOpticalFlowHS do.  The first batch is the loop from its start (HSFLOW_SEQ_REBLUR: its first old frame is blurred
// once, every later one twice); a later batch starts with the frame the one before ended with, which was a new frame
// there (| HSFLOW_SEQ_REBLUR_FIRST).  A tail of m < n pairs gets a context of m pairs.  Gray frames are uploaded as they
// are; with HSFLOW_JPEG_IN_DEVICE=1 and nothing but .jpg frames the files go to the device undecoded.  The flow_%04d.ppm
// files are byte for byte those of the loop below.
// pts_n: the corners of HSFLOW_CAMERA_POINTS, 0 without it.
static int run_camera_batched(float lambda, int it, int nb, bool chain, bool objects, uint32_t obj_min_area, uint32_t obj_share, uint32_t pts_n,
                              uint32_t pts_quality, int pts_nms_r)
{
    struct Frame {
        pnm::Image gray;           // the gray frame, or
        std::vector<uint8_t> file; // the JPEG file as it is
    };
    bool files = jpeg_in_device();
    for (int i = 0; files; i++) { // every frame of the clip a .jpg?
        const std::string name = camera_frame(i);
        FILE *f = fopen(name.c_str(), "rb");
        if (!f) { files = i > 0; break; }
        fclose(f);
        if (!ends_with_jpg(name)) files = false;
    }
    int W = 0, H = 0;
    auto load = [&](int i, Frame &fr) { // false: the clip ends in front of frame i
        int w = 0, h = 0;
        if (files) {
            hsflow_jpeg_info info;
            info.struct_size = sizeof(info);
            if (!read_jpeg_file(camera_frame(i), fr.file) || hsflow_jpeg_read_header(fr.file.data(), fr.file.size(), &info) != HSFLOW_OK) return false;
            w = info.width; h = info.height;
        } else {
            pnm::Image frame;
            if (!pnm::load_image(camera_frame(i), frame)) return false;
            pnm::to_gray(frame, fr.gray); // cvCvtColor(imgTmp, img, CV_BGR2GRAY) :79,86
            w = fr.gray.width; h = fr.gray.height;
        }
        if (i == 0) { W = w; H = h; }
        return w == W && h == H;
    };
    std::vector<Frame> batch(1);
    if (!load(0, batch[0])) { std::cout << "ERROR: capture is NULL \n"; return -1; }
    hsflow_params p;
    hsflow_default_params(&p); // ITER|EPS, eps (float)1e-6 :94
    p.lambda = lambda;
    p.max_iter = it;
    const bool on_device = render_on_device();
    std::vector<float> u, v;
    if (!on_device) { u.resize((size_t)W * H); v.resize((size_t)W * H); }
    hsflow_ctx *ctx = nullptr;
    int ctx_pairs = 0;
    void *dFrames = nullptr; // the batch's gray frames on the device, packed
    size_t dBytes = 0;
    void *dObjects = nullptr; // HSFLOW_CAMERA_OBJECTS: the planes and records of objects_batch
    size_t dObjectsBytes = 0;
    void *dPoints = nullptr; // HSFLOW_CAMERA_POINTS: the records and points of points_batch
    size_t dPointsBytes = 0;
    const size_t frame_bytes = (size_t)W * H;
    auto done = [&](int code) {
        if (ctx) hsflow_destroy(ctx);
        if (dFrames) (void)hipFree(dFrames);
        if (dObjects) (void)hipFree(dObjects);
        if (dPoints) (void)hipFree(dPoints);
        return code;
    };
    double total = 0.0;
    int count = 0, verdict = SDK_SUCCESS, flags = HSFLOW_SEQ_REBLUR;
    for (bool more = true; more;) {
        while ((int)batch.size() < nb + 1) {
            Frame fr;
            if (!load(count + (int)batch.size(), fr)) { more = false; break; }
            batch.push_back(std::move(fr));
        }
        const int m = (int)batch.size() - 1;
        if (m < 1) break;
        if (m != ctx_pairs) {
            if (ctx) hsflow_destroy(ctx);
            ctx = nullptr;
            if (hsflow_create(&ctx, 0, W, H, m, nullptr, 1) != HSFLOW_OK) { std::cout << hsflow_last_error(nullptr) << std::endl; return done(1); }
            if (hsflow_set_pair_termination(ctx, 1) != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return done(1); }
            ctx_pairs = m;
        }
        const double t0 = now_ms();
        int st;
        if (files) {
            std::vector<const uint8_t *> ptrs;
            std::vector<size_t> sizes;
            for (const Frame &fr : batch) { ptrs.push_back(fr.file.data()); sizes.push_back(fr.file.size()); }
            st = hsflow_set_sequence_jpeg_ex(ctx, 0, ptrs.data(), sizes.data(), m + 1, 1, flags);
        } else {
            if (dBytes < frame_bytes * (size_t)(m + 1)) {
                if (dFrames) (void)hipFree(dFrames);
                dFrames = nullptr; dBytes = 0;
                if (hipMalloc(&dFrames, frame_bytes * (size_t)(m + 1)) != hipSuccess) { std::cout << "hipMalloc of the batch's frames failed" << std::endl; return done(1); }
                dBytes = frame_bytes * (size_t)(m + 1);
            }
            std::vector<const void *> ptrs;
            for (int j = 0; j <= m; j++) {
                void *d = (uint8_t *)dFrames + frame_bytes * (size_t)j;
                if (hipMemcpy(d, batch[(size_t)j].gray.data.data(), frame_bytes, hipMemcpyHostToDevice) != hipSuccess) { std::cout << "upload of a frame failed" << std::endl; return done(1); }
                ptrs.push_back(d);
            }
            st = hsflow_set_sequence_device_ex(ctx, 0, HSFLOW_FRAMES_GRAY8_BLUR, ptrs.data(), m + 1, (size_t)W, flags); // :92-93,118 for every pair
        }
        if (st == HSFLOW_OK) st = hsflow_solve(ctx, &p);
        if (st == HSFLOW_OK) st = hsflow_synchronize(ctx); // (the frames' buffer is written again by the next batch)
        total += now_ms() - t0;
        if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return done(1); }
        for (int k = 0; k < m; k++) {
            const int i = count + k + 1; // the pair's new frame
            if (!on_device && hsflow_get_flow(ctx, k, u.data(), (size_t)W * 4, v.data(), (size_t)W * 4) != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; return done(1); }
            hsflow_verify_report report;
            if (verify_wanted() && verify_pair(ctx, W, report, k) != SDK_SUCCESS) verdict = SDK_FAILURE;
            if (getenv("HSFLOW_CAMERA_OUT")) {
                pnm::Image imgFlow;
                if (!on_device) draw_cv_flow(imgFlow, u, v, W, H);
                else if (draw_on_device(ctx, HSFLOW_RENDER_CV, W, H, imgFlow, k) != SDK_SUCCESS) return done(1);
                char name[64];
                snprintf(name, sizeof(name), "/flow_%04d.ppm", i);
                pnm::save_image(std::string(getenv("HSFLOW_CAMERA_OUT")) + name, imgFlow);
            }
        }
        if (chain && getenv("HSFLOW_CAMERA_OUT")) {
            std::vector<float> cu, cv;
            if (chain_batch(ctx, m, W, H, cu, cv) != SDK_SUCCESS) return done(1);
            pnm::Image imgChain;
            imgChain.width = W; imgChain.height = H; imgChain.channels = 3;
            imgChain.data.resize((size_t)W * H * 3);
            hsflow_color_params cp;
            hsflow_default_color_params(&cp); // (AUTO: the picture's own largest flow)
            if (hsflow_color_flow_host(cu.data(), (size_t)W * 4, cv.data(), (size_t)W * 4, W, H, &cp, imgChain.data.data(), (size_t)W * 3, nullptr) != HSFLOW_OK) {
                std::cout << hsflow_last_error(nullptr) << std::endl;
                return done(1);
            }
            char name[64];
            snprintf(name, sizeof(name), "/chain_%04d.ppm", count + m);
            pnm::save_image(std::string(getenv("HSFLOW_CAMERA_OUT")) + name, imgChain);
            // the camera's motion over the batch: the model of the accumulated flow (HSFLOW_GMOTION selects the fit); the
            // pixels the chain lost carry NaN and are UNKNOWN to the fit
            hsflow_gmotion_params gp;
            gmotion_choice(gp);
            hsflow_gmotion_result r;
            if (hsflow_gmotion_fit_host(cu.data(), cv.data(), (size_t)W * 4, nullptr, 0, W, H, &gp, nullptr, 0, nullptr, nullptr, 0, &r) != HSFLOW_OK) {
                std::cout << hsflow_last_error(nullptr) << std::endl;
                return done(1);
            }
            snprintf(name, sizeof(name), "chain %04d", count + m);
            std::cout << gmotion_line(name, r, W, H) << std::endl;
        }
        if (objects && getenv("HSFLOW_CAMERA_OUT")) {
            char name[64];
            snprintf(name, sizeof(name), "/objects_%04d.txt", count + m);
            if (objects_batch(ctx, m, W, H, count, obj_min_area, obj_share, std::string(getenv("HSFLOW_CAMERA_OUT")) + name, dObjects, dObjectsBytes) != SDK_SUCCESS)
                return done(1);
        }
        if (pts_n && getenv("HSFLOW_CAMERA_OUT")) {
            char name[64];
            snprintf(name, sizeof(name), "/points_%04d.txt", count + m);
            if (points_batch(ctx, m, pts_n, pts_quality, pts_nms_r, std::string(getenv("HSFLOW_CAMERA_OUT")) + name, dPoints, dPointsBytes) != SDK_SUCCESS) return done(1);
        }
        count += m;
        Frame last = std::move(batch.back()); // imgOld = imgNew :118, across the batches
        batch.clear();
        batch.push_back(std::move(last));
        flags = HSFLOW_SEQ_REBLUR | HSFLOW_SEQ_REBLUR_FIRST;
    }
    if (count) std::cout << "Avg time: " << total / count << " [ms]" << std::endl; // :122 (per frame)
    return done(verdict);
}

int OpticalFlowOpenCV::runFromCamera(float lambda, int it)
{
    const int chain = camera_chain();
    if (chain < 0) { std::cout << "HSFLOW_CAMERA_CHAIN must be 0 or 1" << std::endl; return 1; }
    uint32_t obj_min_area = 1, obj_share = 128;
    const int objects = camera_objects(obj_min_area, obj_share);
    if (objects < 0) { std::cout << "HSFLOW_CAMERA_OBJECTS must be <min_area 1 .. 2^30>[,<share 0 .. 256>]" << std::endl; return 1; }
    if (objects && !getenv("HSFLOW_CAMERA_OUT")) { std::cout << "HSFLOW_CAMERA_OBJECTS needs HSFLOW_CAMERA_OUT, the directory of objects_%04d.txt" << std::endl; return 1; }
    uint32_t pts_n = 0, pts_quality = 0;
    int pts_nms_r = 0;
    const int points = camera_points(pts_n, pts_quality, pts_nms_r);
    if (points < 0) { std::cout << "HSFLOW_CAMERA_POINTS must be <n 1 .. 65536>[,<quality_q16 0 .. 65535>[,<nms_r 1 .. 8>]]" << std::endl; return 1; }
    if (points && !getenv("HSFLOW_CAMERA_OUT")) { std::cout << "HSFLOW_CAMERA_POINTS needs HSFLOW_CAMERA_OUT, the directory of points_%04d.txt" << std::endl; return 1; }
    if (const int nb = camera_batch()) {
        if (nb < 0) { std::cout << "HSFLOW_CAMERA_BATCH must be 1 .. 256" << std::endl; return 1; }
        return run_camera_batched(lambda, it, nb, chain == 1, objects == 1, obj_min_area, obj_share, points == 1 ? pts_n : 0u, pts_quality, pts_nms_r);
    }
    if (chain) { std::cout << "HSFLOW_CAMERA_CHAIN needs HSFLOW_CAMERA_BATCH=1 .. 256" << std::endl; return 1; }
    if (objects) { std::cout << "HSFLOW_CAMERA_OBJECTS needs HSFLOW_CAMERA_BATCH=1 .. 256" << std::endl; return 1; }
    if (points) { std::cout << "HSFLOW_CAMERA_POINTS needs HSFLOW_CAMERA_BATCH=1 .. 256" << std::endl; return 1; }
    pnm::Image frame, gold, gnew;
    if (!pnm::load_image(camera_frame(0), frame)) { std::cout << "ERROR: capture is NULL \n"; return -1; }
    pnm::to_gray(frame, gold);                                   // cvCvtColor(imgTmp, imgOld, CV_BGR2GRAY) :79
    const int W = gold.width, H = gold.height;
    hsflow_ctx *ctx = nullptr;
    if (hsflow_create(&ctx, 0, W, H, 1, nullptr, 1) != HSFLOW_OK) { std::cout << hsflow_last_error(nullptr) << std::endl; return 1; }
    hsflow_params p;
    hsflow_default_params(&p);                                   // ITER|EPS, eps (float)1e-6 :94
    p.lambda = lambda;
    p.max_iter = it;
    const bool on_device = render_on_device();
    std::vector<float> u, v;
    if (!on_device) { u.resize((size_t)W * H); v.resize((size_t)W * H); }
    double total = 0.0;
    int count = 0, verdict = SDK_SUCCESS;
    for (int i = 1; pnm::load_image(camera_frame(i), frame); i++) {
        pnm::to_gray(frame, gnew);
        if (gnew.width != W || gnew.height != H) break;
        const double t0 = now_ms();
        int st = i == 1 ? hsflow_set_frames_gray8_blur(ctx, 0, gold.data.data(), (size_t)W, gnew.data.data(), (size_t)W) // :92-93
                        : hsflow_push_frame_ex(ctx, 0, HSFLOW_FRAMES_GRAY8_BLUR, gnew.data.data(), (size_t)W, 1); // imgOld = imgNew (:117), blurred again (:92)
        if (st == HSFLOW_OK) st = hsflow_solve(ctx, &p);
        if (st == HSFLOW_OK && !on_device) st = hsflow_get_flow(ctx, 0, u.data(), (size_t)W * 4, v.data(), (size_t)W * 4);
        total += now_ms() - t0;
        if (st != HSFLOW_OK) { std::cout << hsflow_last_error(ctx) << std::endl; hsflow_destroy(ctx); return 1; }
        count++;
        hsflow_verify_report report;
        if (verify_wanted() && verify_pair(ctx, W, report) != SDK_SUCCESS) verdict = SDK_FAILURE;
        if (getenv("HSFLOW_CAMERA_OUT")) {
            pnm::Image imgFlow;
            if (!on_device) draw_cv_flow(imgFlow, u, v, W, H);
            else if (draw_on_device(ctx, HSFLOW_RENDER_CV, W, H, imgFlow) != SDK_SUCCESS) { hsflow_destroy(ctx); return 1; }
            char name[64];
            snprintf(name, sizeof(name), "/flow_%04d.ppm", i);
            pnm::save_image(std::string(getenv("HSFLOW_CAMERA_OUT")) + name, imgFlow);
        }
    }
    hsflow_destroy(ctx);
    if (count) std::cout << "Avg time: " << total / count << " [ms]" << std::endl; // :122 (per frame)
    return verdict;
}
