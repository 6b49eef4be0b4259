// main.cpp -- command line of the reference (OpticalFlowHS/main.cpp:24-148), same positional
// grammar:
//   -cl -hd  in1 in2 out alpha iterations workgroup GPU|CPU      (10 arguments)
//   -cl -cam alpha iterations workgroup GPU|CPU                  (7)
//   -cv -hd  in1 in2 out lambda iterations                       (8)
//   -cv -cam lambda iterations                                   (5)
// Images are binary PGM/PPM; the interactive getchar() pause of the original (main.cpp:87) is
// kept only when HSFLOW_PAUSE is set.
// HSFLOW_RENDER_DEVICE=1: the arrow picture is drawn on the device (hsflow_render_flow) and the flow is not
// downloaded; the files written are the same.
// HSFLOW_JPEG_DEVICE=1 with it, and an output name ending in .jpg / .jpeg (the two -hd routes): the file is encoded on
// the device too (hsflow_render_flow_jpeg) and written as it is; the same bytes.
// HSFLOW_PICTURE=color: every route writes the dense colour picture of the flow (the Middlebury wheel; include/hsflow.h,
// hsflow_color_flow*) instead of the arrows -- by the host rule from the flow read back, with HSFLOW_RENDER_DEVICE=1 drawn
// on the device, with HSFLOW_JPEG_DEVICE=1 encoded there too; the same bytes every way.  HSFLOW_COLOR_MAX=<float>: the
// flow that is fully saturated (default: the picture's own largest).  An unusable value of either: a message, exit status 1.
// HSFLOW_PICTURE=warp (the two -hd routes): the file is the motion-compensated SECOND frame instead -- the second input as
// loaded, warped onto the first by the solved flow (hsflow_warp*) -- and one line "warp: inside .. outside .. unknown ..
// sad_warped .. sad_plain .." tells the residual; by hsflow_warp_host from the flow read back, with HSFLOW_RENDER_DEVICE=1
// by hsflow_warp on the device; the same file and line.  HSFLOW_WARP_T=<float>: the fraction of the flow applied (default 1;
// finite, at most 1e6 in magnitude, else a message and exit status 1).
// HSFLOW_PICTURE=stab (the two -hd routes): the file is the second input warped onto the first by the ONE global motion fitted
// to the solved flow (hsflow_gmotion_fit*, hsflow_gmotion_warp*), not by the dense flow; one line tells the model and the
// inliers' share.  HSFLOW_GMOTION=<translation|similarity|affine>[,<passes>[,<px>|auto]] selects the fit.
// HSFLOW_REGIONS=<min_area>[,<4|8>[,<join_px>]] (the two -hd routes): behind the solve (and HSFLOW_MEDIAN / HSFLOW_PYRAMID) the
// flow is fitted with the HSFLOW_GMOTION choice, the pixels that do not follow the camera are labelled (hsflow_regions*), and
// one line "regions: kept .. dropped .. foreground .. largest .." and at most 16 lines "region k: area .. box x0 y0 x1 y1
// centre cx cy motion mu mv" tell what moves; by the host rules from the flow read back, with HSFLOW_RENDER_DEVICE=1 on the
// device with only the records read back; the same lines, the picture is unchanged (an unusable value: a message and exit
// status 1).
// HSFLOW_CAMERA_OBJECTS=<min_area>[,<share 0..256>] (the batched -cv -cam route, needs HSFLOW_CAMERA_BATCH and HSFLOW_CAMERA_OUT): every batch
// writes objects_%04d.txt -- the regions of every pair's fit mask (hsflow_regions_batch_device), linked from pair to pair on the
// device (hsflow_link_regions_batch_device) and given ids that hold over the batch (hsflow_link_tracks_host); one line "frame
// id area x0 y0 x1 y1 sum_x sum_y n_flow sum_qu sum_qv" per region.  Ids restart with every batch.
// HSFLOW_CAMERA_POINTS=<n>[,<quality_q16>[,<nms_r>]] (the same route, needs HSFLOW_CAMERA_BATCH and HSFLOW_CAMERA_OUT): every batch
// writes points_%04d.txt -- the n best corners of the batch's first frame (hsflow_corners_device), followed through the batch's
// flows (hsflow_track_points_device) with no read-back in between; one line "rank x0 y0 score x y status age" per corner.
// HSFLOW_PICTURE=fb (the two -hd routes): the pair is solved forwards and, from the same pre-processed frames, backwards
// (hsflow_set_frames_reversed), and the file is the forward-backward consistency mask (hsflow_fb*: 255 where the two flows
// cancel, 0 elsewhere) as a gray picture; one line "fb: consistent .. inconsistent .. outside .. unknown .. mse .." tells
// the statistics; by hsflow_fb_host from the flows read back, with HSFLOW_RENDER_DEVICE=1 by hsflow_fb on the device; the
// same file and line.  HSFLOW_FB_ALPHA / HSFLOW_FB_BETA=<float>: the bound's two terms (defaults 0.01 and 0.5; finite,
// 0 .. 1e6 and 0 .. 1e30, else a message and exit status 1).
// HSFLOW_PICTURE=interp (the two -hd routes): the file is the frame at time t between the two input files, in their own
// channels (hsflow_interp*: the forward flow projected to t, its holes filled, both frames fetched along it and blended);
// one line "interp: t .. blended .. prev_only .. curr_only .. clamped .. holes .. unfilled .. collisions .. left .. unknown
// .." tells the record; by hsflow_interp_host from the flow read back, with HSFLOW_RENDER_DEVICE=1 by hsflow_interp on the
// device; the same file and line.  HSFLOW_INTERP_T=<float in 0 .. 1> (default 0.5; else a message and exit status 1).
// HSFLOW_INTERP_FB=1: the pair is also solved backwards as for HSFLOW_PICTURE=fb, and the masks of both checks go in as
// the visibility planes.
// HSFLOW_MEDIAN=<radius>[,<passes>[,fill]] (the two -hd routes): the solved flow is median-filtered in place on the device
// (hsflow_median_apply; radius 1 or 2, passes 1 .. 64) before the picture that HSFLOW_PICTURE asks for is drawn.  With
// "fill" the pair is also solved backwards as for HSFLOW_PICTURE=fb, the hsflow_fb mask (HSFLOW_FB_ALPHA / HSFLOW_FB_BETA)
// is the state, only the untrusted pixels are replaced by the median of their trusted neighbours, and one line "median:
// kept .. filled .. unfilled .. newly_filled .. changed .." tells the record of the last pass.  A bad value: a message
// and exit status 1.
// HSFLOW_PYRAMID=<levels 1 .. 8 | auto>[,<warps 1 .. 8>[,<median radius 0 .. 2>]] (-cv -hd, from PPM / PGM or from JPEG files):
// the solve becomes the coarse-to-fine solve (hsflow_solve_pyramid: every level solved with the route's lambda and
// iteration count), for motions of many pixels; every HSFLOW_PICTURE and HSFLOW_MEDIAN behind it works on its flow.  On
// -cam and on -cl, and for a bad value: a message and exit status 1.  (HSFLOW_VERIFY=1 reports "Failed" for it: a pyramid's
// flow is no single solve to re-run.)
// HSFLOW_VERIFY=1: every solved pair is verified on the device (hsflow_verify: re-solved sweep by sweep, compared
// there) before its context goes away; one "Passed!" / "Failed" line per pair on stdout, the pictures are written as
// always, and the exit status is SDK_FAILURE if any pair failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "HSOpticalFlowOpenCL.hpp"

static int runCLDisk(char *argv[])
{
    // main.cpp:91-109; alpha is parsed with atoi there, kept
    HSOpticalFlowOpenCL clOpticalFlow("OpticalFlow", argv[2], argv[3], argv[4], argv[5], (float)atoi(argv[6]),
                                      atoi(argv[7]), atoi(argv[8]), argv[9]);
    int st = clOpticalFlow.initialize();
    if (!st) st = clOpticalFlow.setup();
    if (!st) st = clOpticalFlow.run();
    clOpticalFlow.cleanup();
    return st;
}

static int runCLCamera(char *argv[])
{
    HSOpticalFlowOpenCL clOpticalFlow("OpticalFlow", argv[2], (float)atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), argv[6]);
    int st = clOpticalFlow.initialize();
    if (!st) st = clOpticalFlow.setup();
    if (!st) st = clOpticalFlow.run();
    clOpticalFlow.cleanup();
    return st;
}

int main(int argc, char *argv[])
{
    int st = 0;
    if (argc == 1) {
        std::cout << "No parameters given.\n";
        return 0;
    }
    if (!picture_choice_usable()) return 1;
    if (warp_wanted() && argc >= 3 && strcmp(argv[2], "-cam") == 0) { std::cout << "HSFLOW_PICTURE=warp needs a pair of files (-hd)\n"; return 1; }
    if (stab_wanted() && argc >= 3 && strcmp(argv[2], "-cam") == 0) { std::cout << "HSFLOW_PICTURE=stab needs a pair of files (-hd)\n"; return 1; }
    if (fb_wanted() && argc >= 3 && strcmp(argv[2], "-cam") == 0) { std::cout << "HSFLOW_PICTURE=fb needs a pair of files (-hd)\n"; return 1; }
    if (interp_wanted() && argc >= 3 && strcmp(argv[2], "-cam") == 0) { std::cout << "HSFLOW_PICTURE=interp needs a pair of files (-hd)\n"; return 1; }
    if (median_wanted() && argc >= 3 && strcmp(argv[2], "-cam") == 0) { std::cout << "HSFLOW_MEDIAN needs a pair of files (-hd)\n"; return 1; }
    if (pyramid_wanted() && argc >= 3 && (strcmp(argv[2], "-cam") == 0 || strcmp(argv[1], "-cl") == 0)) { std::cout << "HSFLOW_PYRAMID needs the CV route on a pair of files (-cv -hd)\n"; return 1; }
    if (argc >= 3 && strcmp(argv[1], "-cl") == 0) {
        if (strcmp(argv[2], "-hd") == 0) {
            if (argc != 10) { std::cout << "Wrong argument list!\n"; return 0; }
            std::cout << "HIP disk!\n";
            st = runCLDisk(argv);
        } else if (strcmp(argv[2], "-cam") == 0) {
            if (argc != 7) { std::cout << "Wrong argument list!\n"; return 0; }
            std::cout << "HIP camera!\n";
            st = runCLCamera(argv);
        }
    } else if (argc >= 3 && strcmp(argv[1], "-cv") == 0) {
        OpticalFlowOpenCV e;
        if (strcmp(argv[2], "-hd") == 0) {
            if (argc != 8) { std::cout << "Wrong argument list!\n"; return 0; }
            std::cout << "CV-semantics disk!\n";
            st = e.runFromImg(argv[3], argv[4], argv[5], (float)atof(argv[6]), atoi(argv[7]));
        } else if (strcmp(argv[2], "-cam") == 0) {
            if (argc != 5) { std::cout << "Wrong argument list!\n"; return 0; }
            st = e.runFromCamera((float)atof(argv[3]), atoi(argv[4]));
        }
    }
    if (getenv("HSFLOW_PAUSE")) getchar();
    return st;
}
