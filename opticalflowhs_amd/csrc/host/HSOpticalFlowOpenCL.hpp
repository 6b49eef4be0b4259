// HSOpticalFlowOpenCL.hpp -- drop-in for the reference's entry-point class
// (OpticalFlowHS/HSOpticalFlowOpenCL.hpp:26-264): same class name, both constructor signatures
// (:130 disk, :171 camera) and the lifecycle methods initialize / setup / run / cleanup /
// verifyResults (:239-263), so that main.cpp:104-108 and :120-124 compile unchanged.  The body no
// longer touches OpenCL: it forwards to the C ABI in include/hsflow.h (HIP on MI355X).
//
// Differences that are deliberate:
//   * both u and v are solved (the reference's kernel never updated v, Kernels.cl:84-86);
//   * planar u8 / fp32 buffers instead of float4 per pixel;
//   * no per-iteration host<->device copies;
//   * image files are binary PGM/PPM (no OpenCV highgui on this platform);
//   * dType "CPU" is refused: this build has no CPU path;
//   * verifyResults() verifies: the last pair is re-solved sweep by sweep on the device and compared there
//     (hsflow_verify).  run() calls it after every pair when HSFLOW_VERIFY=1.
// The "-cl" route runs the reference kernels' own discretisation (HSFLOW_MODE_CLASSIC, alpha);
// the "-cv" route (class OpticalFlowOpenCV below) runs the OpenCV one (graded semantics).
#pragma once
#include <string>
#include <vector>

#include "../../../include/hsflow.h"
#include "jpeg_baseline.hpp"
#include "jpeg_encode.hpp"
#include "verify_line.hpp"

#define SDK_SUCCESS 0 /* SDKUtil/include/SDKCommon.hpp:23 */
#define SDK_FAILURE 1 /* SDKUtil/include/SDKCommon.hpp:24 */

// Stand-in for the AMD APP SDK base class (SDKUtil/include/SDKApplication.hpp:12-47): only the name.
class SDKSample {
protected:
    std::string sampleName;
public:
    explicit SDKSample(const char *name) : sampleName(name ? name : "") {}
    virtual ~SDKSample() {}
    virtual int initialize() { return SDK_SUCCESS; }
};

class HSOpticalFlowOpenCL : public SDKSample {
    hsflow_ctx *ctx = nullptr;
    std::vector<float> u, v;      // flow of the last pair, planar, pitch = width (not filled with HSFLOW_RENDER_DEVICE=1)
    float alpha;                  // flow smoothness coefficient (reference: cl_float alpha)
    int iterations;
    int blockSizeX;               // "gs": accepted for compatibility (work-group size hint), unused
    unsigned width = 0, height = 0;
    bool gpu = true;
    std::string src, input1, input2, output;
    double lastMs = 0.0;
    bool solved = false;          // a pair has been solved on ctx: verifyResults has something to verify
    hsflow_verify_report report{}; // of the last verifyResults

    int ensureContext(int w, int h);
    int solvePair(const pnm::Image &a, const pnm::Image &b, bool streaming, bool frames_set = false);
    int drawFlow(pnm::Image &imgFlow) const; // host loop over u, v; HSFLOW_RENDER_DEVICE=1: hsflow_render_flow, no read-back

public:
    HSOpticalFlowOpenCL(const char *name, char *src, char *input1, char *input2, char *output, float alp,
                        int it, int gs, char *dType);
    HSOpticalFlowOpenCL(const char *name, char *src, float alp, int it, int gs, char *dType);
    ~HSOpticalFlowOpenCL();

    int initialize();      // reference: registers a dead -i option (HSOpticalFlowOpenCL.cpp:681-704)
    int setup();           // reference: no-op (:895)
    int run();             // load pair / stream frames, derivatives + iterations, draw, save
    int cleanup();         // releases the context (:849-892)
    int verifyResults();   // reference: stub returning SDK_SUCCESS (:894).  Here: hsflow_verify of the last pair solved
                           // (SDK_SUCCESS before any), one "Passed!" / "Failed" line (verify_line.hpp) on stdout
    const hsflow_verify_report &verifyReport() const { return report; }

    const std::vector<float> &flowU() const { return u; }
    const std::vector<float> &flowV() const { return v; }
    double lastSolveMs() const { return lastMs; }
};

// HSFLOW_PICTURE (color | arrows) and HSFLOW_COLOR_MAX (a finite float > 0) as every route will read them: false, after
// a message on stdout, if either holds something else.
bool picture_choice_usable();
// HSFLOW_PICTURE=warp: the file is the motion-compensated second frame (the two "-hd" routes only).
bool warp_wanted();
// HSFLOW_PICTURE=stab: the file is the second frame warped by the fitted global motion (the two "-hd" routes only).
bool stab_wanted();
// HSFLOW_PICTURE=fb: the file is the forward-backward consistency mask of the pair against its reverse (the two "-hd"
// routes only).
bool fb_wanted();
// HSFLOW_PICTURE=interp: the file is the frame at time HSFLOW_INTERP_T between the two input files (the two "-hd" routes
// only).
bool interp_wanted();
// HSFLOW_MEDIAN=<radius>[,<passes>[,fill]]: the flow is median-filtered, or its untrusted pixels filled, in place before
// the picture is drawn (the two "-hd" routes only).
bool median_wanted();
// HSFLOW_PYRAMID=<levels|auto>[,<warps>[,<median radius>]]: the solve is hsflow_solve_pyramid (the "-cv -hd" routes only).
bool pyramid_wanted();

// GPU counterpart of the reference's CPU route (OpticalFlowHS/OpticalFlowOpenCV.hpp:6-11):
// gray -> 3x3 box blur -> Horn-Schunck(lambda, ITER|EPS, eps 1e-6) -> arrows, all but the file I/O
// and the drawing on the device.
class OpticalFlowOpenCV {
public:
    int runFromImg(char *input1, char *input2, char *output, float lambda, int it);
    int runFromCamera(float lambda, int it);
};
