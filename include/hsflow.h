/*
 * hsflow.h -- C ABI of the MI355X-native Horn-Schunck optical-flow solver (libhsflow.so).
 *
 * This is the drop-in boundary for the hot path of miczi/OpticalFlowHS:
 * everything the reference's HSOpticalFlowOpenCL::setupCL / runDerivatives / runCLKernels /
 * cleanup did through OpenCL goes through these entry points instead.  Plain pointers and
 * sizes only; no C++ or torch types.  All planes are single-channel and PLANAR (u8 frames,
 * fp32 flow) -- not the reference's float4-per-pixel layout (HSOpticalFlowOpenCL.hpp:29-41).
 *
 * Reference interfaces replaced, one by one:
 *   hsflow_create / hsflow_destroy ...... HSOpticalFlowOpenCL::setupCL  (HSOpticalFlowOpenCL.cpp:67-319)
 *                                          HSOpticalFlowOpenCL::cleanup  (HSOpticalFlowOpenCL.cpp:849-892)
 *   hsflow_set_frames_u8[_device] ....... clEnqueueWriteBuffer of inputImageBuffer1/2
 *                                          (HSOpticalFlowOpenCL.cpp:339-357); frames are what
 *                                          readInputImage produced (:4-44) but kept as u8
 *   hsflow_set_frames_device_ex ......... cvCvtColor + cvSmooth of both frames (OpticalFlowOpenCV.cpp:17,20,27-28) on
 *                                          frames that already lie in device memory, one launch per pair
 *   hsflow_push_frame[_device]_ex ....... one turn of the camera loop's frame handling (OpticalFlowOpenCV.cpp:85,92-93,
 *                                          118): the blurred new frame becomes the old one and is blurred again
 *   hsflow_pipeline_submit_device_ex .... the same pre-processing in front of every pair of a resident stream
 *   hsflow_preprocess_frame_host ........ the arithmetic of both steps on the host, for checking
 *   hsflow_solve / hsflow_solve_async ... runDerivatives() + iterations x runCLKernels()
 *                                          (HSOpticalFlowOpenCL.cpp:321-474, :476-679, loop :749-751)
 *                                          and, argument for argument, cvCalcOpticalFlowHS
 *                                          (OpenCV2.1/include/cv.h:481-483) as called at
 *                                          OpticalFlowOpenCV.cpp:29,94
 *   hsflow_get_flow[_device] ............ clEnqueueReadBuffer of uBuffer/vBuffer
 *                                          (HSOpticalFlowOpenCL.cpp:655-675); read at :765-767
 *   hsflow_get_derivatives .............. clEnqueueReadBuffer of Ex/Ey/Et (:437-468)
 *   hsflow_render_flow[_device] ......... the arrow drawing after the read-back: cvCircle + cvLine per grid point
 *                                          (OpticalFlowOpenCV.cpp:33-46, HSOpticalFlowOpenCL.cpp:759-769), from the
 *                                          flow where it lies -- no read-back
 *   hsflow_render_flow_jpeg[_device] .... cvSaveImage(output, imgFlow) behind it (OpticalFlowOpenCV.cpp:47,
 *                                          HSOpticalFlowOpenCL.cpp:771): the picture's JPEG file, encoded on the device
 *   hsflow_render_flow_batch_device, hsflow_jpeg_encode_batch_device, hsflow_render_flow_jpeg_batch[_device]
 *                                          the same drawing and cvSaveImage (OpticalFlowOpenCV.cpp:32-47,
 *                                          HSOpticalFlowOpenCL.cpp:759-771) for every pair of a context at once: one set
 *                                          of launches per batch, N files out without a round trip per pair
 *   hsflow_color_flow[_host|_device|_batch_device], hsflow_color_flow_jpeg[_device|_batch|_batch_device]
 *                                          no counterpart in the reference, whose only picture is the arrow plot: the
 *                                          DENSE field as the Middlebury colour wheel, drawn (and encoded) where the flow
 *                                          lies instead of a read-back of both fp32 planes
 *   hsflow_warp[_host|_device|_batch_device]
 *                                          no counterpart in the reference: the second frame warped backwards onto the
 *                                          first by the solved flow, and the residual |warp(curr) - prev| as exact integer
 *                                          sums, where the flow lies
 *   hsflow_fb[_host|_device|_batch_device|_planes_device|_planes], hsflow_set_frames_reversed
 *                                          no counterpart in the reference: the forward-backward consistency of the
 *                                          flows of (A, B) and (B, A), pixel by pixel -- a confidence mask, the squared
 *                                          error and exact integer statistics -- where the flows lie; the reversed pair
 *                                          from the frames that are already on the device
 *   hsflow_median[_host|_device|_batch_device|_planes_device|_apply]
 *                                          no counterpart in the reference: the median filter of the flow and the filling
 *                                          of untrusted pixels from their trusted neighbours, where the flow lies
 *   hsflow_interp[_host|_device|_batch_device], hsflow_project_flow_host, hsflow_project_flow_device
 *                                          no counterpart in the reference: the frame at time t between the two frames of
 *                                          a pair (frame-rate conversion) -- the forward flow projected to t, holes
 *                                          filled, both frames fetched and blended with occlusion -- where the flow lies
 *   hsflow_chain_flow[_host|_device], hsflow_chain_planes_device, hsflow_track_points[_host|_device]
 *                                          no counterpart in the reference: pixels and points followed through the flows
 *                                          of a whole sequence of pairs -- the accumulated flow from the first frame to
 *                                          the last, point tracks -- where the flows lie
 *   hsflow_regions[_host|_device|_batch_device|_planes_device]
 *                                          no counterpart in the reference: the moving objects of a pair -- the connected
 *                                          regions of a foreground mask (hsflow_gmotion_fit's, hsflow_fb's), optionally cut
 *                                          where neighbours move differently, each with its size, box, centroid and mean
 *                                          motion -- labelled where mask and flow lie; only the records cross PCIe
 *   hsflow_link_regions[_host|_device|_batch_device|_planes_device], hsflow_link_tracks_host
 *                                          no counterpart in the reference: the regions of consecutive pairs linked by
 *                                          the flow -- how many pixels of region a arrive in region b of the next frame --
 *                                          where labels and flow lie, and object ids over the sequence from those records
 *   hsflow_corners[_host|_device|_batch_device|_planes_device]
 *                                          cvGoodFeaturesToTrack of the reference's OpenCV 2.1, which the reference never
 *                                          calls: the points worth following, found in the gray planes where they lie and
 *                                          handed to hsflow_track_points_device without a read-back
 *   hsflow_set_frames_jpeg .............. cvLoadImage of both input files in front of it (OpticalFlowOpenCV.cpp:15,18,
 *                                          HSOpticalFlowOpenCL.cpp:721,732): the files' entropy-coded bytes cross PCIe,
 *                                          the pictures are decoded on the device
 *   hsflow_push_frame_jpeg .............. the camera loop's cvQueryFrame (OpticalFlowOpenCV.cpp:85) for a camera that
 *                                          delivers MJPEG
 *   hsflow_jpeg_decode_batch_device ..... cvLoadImage of many files at once (OpticalFlowOpenCV.cpp:15,18 for the disk
 *                                          route, :76,83 for the camera loop's frames): one set of launches per batch
 *   hsflow_set_sequence_jpeg ............ the same in front of a context of N pairs: N + 1 consecutive frames, each
 *                                          decoded once (the camera loop's cvQueryFrame at :76,83, fed with files)
 *   hsflow_set_sequence_device_ex, hsflow_set_sequence_jpeg_ex, hsflow_preprocess_sequence_host
 *                                          the camera loop's whole frame handling (OpticalFlowOpenCV.cpp:76-93,118: gray,
 *                                          blur of old and new in place, imgOld = imgNew) for N + 1 frames into a context
 *                                          of N pairs: every frame read once, one launch per HSFLOW_PRE_SEQ_MAX frames
 *   hsflow_pipeline_submit_jpeg ......... the disk route's two cvLoadImage (:15,18) in front of a pipeline slot
 *   hsflow_verify ....................... HSOpticalFlowOpenCL::verifyResults (HSOpticalFlowOpenCL.cpp:894), the hook of
 *                                          SDKUtil/include/SDKApplication.hpp that the reference left a stub
 *   hsflow_calc_optical_flow_hs_8u32f ... one-shot form with the argument list of OpenCV's
 *                                          icvCalcOpticalFlowHS_8u32fR (cv210.dll VA 0x1012e040)
 *   status codes ........................ SDK_SUCCESS 0 / SDK_FAILURE 1 (SDKUtil/include/SDKCommon.hpp:23-24)
 *                                          become 0 / enumerated non-zero
 *
 * Threading: a context is single-owner (not thread-safe); one context per (thread, device).
 * All device work of a context is issued on ONE HIP stream (given at creation, or its own).
 */
#ifndef HSFLOW_H_
#define HSFLOW_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HSFLOW_VERSION_MAJOR 0
#define HSFLOW_VERSION_MINOR 26 /* 0.26: hsflow_corners[_host|_device|_batch_device|_planes_device], hsflow_default_corners_params, hsflow_corners_params, hsflow_corners_record, hsflow_corners_result, HSFLOW_CORNERS_*; 0.25: hsflow_link_regions[_host|_device|_batch_device|_planes_device], hsflow_link_tracks_host, hsflow_default_link_params, hsflow_link_params, hsflow_link_record, hsflow_link_side, hsflow_link_result, HSFLOW_LINK_*; 0.24: hsflow_regions[_host|_device|_batch_device|_planes_device], hsflow_default_regions_params, hsflow_regions_params, hsflow_regions_record, hsflow_regions_result, HSFLOW_REGIONS_*; 0.23: hsflow_gmotion_fit[_host|_device|_batch_device|_planes_device], hsflow_gmotion_warp[_host|_device], hsflow_gmotion_compose_host, hsflow_gmotion_invert_host, hsflow_default_gmotion_params, hsflow_gmotion_params, hsflow_gmotion_result, HSFLOW_GMOTION_*; 0.22: hsflow_chain_flow[_host|_device], hsflow_chain_planes_device, hsflow_track_points[_host|_device], hsflow_default_chain_params, hsflow_chain_params, hsflow_chain_stats, HSFLOW_CHAIN_*; 0.21: hsflow_solve_pyramid, hsflow_pyramid_plan, hsflow_pyramid_down_host, hsflow_pyramid_prolong_host, hsflow_get_pyramid_info, hsflow_pyramid_get_level, hsflow_default_pyramid_params, hsflow_pyramid_params, hsflow_pyramid_info, HSFLOW_PYRAMID_*; 0.20: hsflow_interp[_host|_device|_batch_device], hsflow_project_flow_host, hsflow_project_flow_device, hsflow_pipeline_interp[_device], hsflow_default_interp_params, hsflow_interp_params, hsflow_interp_stats, HSFLOW_INTERP_*; 0.19: hsflow_median[_host|_device|_batch_device|_planes_device|_apply], hsflow_pipeline_median[_apply], hsflow_default_median_params, hsflow_median_params, hsflow_median_stats, HSFLOW_MEDIAN_*; 0.18: hsflow_fb[_host|_device|_batch_device|_planes_device|_planes], hsflow_set_frames_reversed, hsflow_pipeline_fb[_device], hsflow_default_fb_params, hsflow_fb_params, hsflow_fb_stats, HSFLOW_FB_*; 0.17: hsflow_warp[_host|_device|_batch_device], hsflow_pipeline_warp[_device], hsflow_default_warp_params, hsflow_warp_params, hsflow_warp_stats, HSFLOW_WARP_BORDER_*; 0.16: hsflow_color_flow[_host|_device|_batch_device], hsflow_color_flow_jpeg[_device|_batch|_batch_device], hsflow_pipeline_color[_device|_jpeg], hsflow_color_params, HSFLOW_COLOR_SCALE_*; 0.15: hsflow_set_flow_device_ex, HSFLOW_FLOW_SOLVER_MADE; 0.14: hsflow_set_sequence_device_ex, hsflow_set_sequence_jpeg_ex, hsflow_preprocess_sequence_host, HSFLOW_SEQ_REBLUR[_FIRST], HSFLOW_PRE_SEQ_MAX; 0.13: hsflow_jpeg_encode_batch_device, hsflow_render_flow_batch_device, hsflow_render_flow_jpeg_batch[_device], HSFLOW_JPEG_BATCH_MAX; 0.12: hsflow_jpeg_decode_batch_device, hsflow_set_sequence_jpeg, hsflow_set_frames_jpeg_async, hsflow_jpeg_async_status, hsflow_pipeline_submit_jpeg, HSFLOW_JPEGD_BATCH_MAX; 0.11: hsflow_jpeg_read_header, hsflow_jpeg_decode[_host|_device], hsflow_set_frames_jpeg, hsflow_push_frame_jpeg, HSFLOW_E_DATA; 0.10: hsflow_jpeg_*, hsflow_render_flow_jpeg[_device], hsflow_pipeline_render_jpeg; 0.9: hsflow_set_frames_device_ex, hsflow_push_frame[_device]_ex, hsflow_pipeline_submit_device_ex, hsflow_preprocess_frame_host; 0.8: hsflow_set_pair_termination, hsflow_get_pair_result, hsflow_solve_probe_pairs; 0.7: hsflow_verify, hsflow_compare_*, hsflow_pipeline_verify; 0.6: hsflow_render_*, hsflow_pipeline_render*; 0.5: hsflow_multi_*, hsflow_slab_*, hsflow_set_row_origin, hsflow_get_info_ex */

/* status codes (0 = success, like SDK_SUCCESS) */
#define HSFLOW_OK 0
#define HSFLOW_E_ARG 1     /* null pointer / bad enum / bad struct size            */
#define HSFLOW_E_SIZE 2    /* non-positive size, stride too small or misaligned    */
#define HSFLOW_E_DEVICE 3  /* a HIP call failed; text in hsflow_last_error         */
#define HSFLOW_E_OOM 4     /* host or device allocation failed                     */
#define HSFLOW_E_STATE 5   /* call order (solve before frames were set, ...)       */
#define HSFLOW_E_NOTERM 6  /* termination rule that would never stop               */
#define HSFLOW_E_DATA 7    /* a file's contents: unsupported kind, corrupt or truncated entropy-coded data */

/* termination flags: values of CV_TERMCRIT_ITER / CV_TERMCRIT_EPS (cxtypes.h:894-896) */
#define HSFLOW_TERM_ITER 1
#define HSFLOW_TERM_EPS 2

/* discretisation */
#define HSFLOW_MODE_CV 0      /* cvCalcOpticalFlowHS semantics: Sobel/8 on frame A, 4-neighbour
                                 mean, lambda (graded parity target)            */
#define HSFLOW_MODE_CLASSIC 1 /* Kernels.cl semantics: 2x2x2 cube derivatives, 1/6-1/12 mean,
                                 alpha^2, with the v update restored.
                                 ITER termination only (the reference's loop has no other rule).
                                 Kernels: SIMPLE, FUSED, STRIP (rows per lane 2..8); AUTO takes
                                 STRIP wherever the image has an aligned shape for it and
                                 2^-20 <= alpha <= 2^20, else FUSED.  All bit-identical.          */

#define HSFLOW_MODE_CLASSIC_AS_SHIPPED 2 /* Kernels.cl exactly as shipped: u_v_updateKernel writes u only
                                 (Kernels.cl:86), v stays at its starting value.  Reproduces the
                                 pictures the reference's OpenCL route wrote; for verification      */

/* Jacobi kernel selection */
#define HSFLOW_KERNEL_AUTO 0
#define HSFLOW_KERNEL_SIMPLE 1 /* one iteration per launch, straight from HBM/L2             */
#define HSFLOW_KERNEL_FUSED 2  /* `fuse_steps` iterations per launch on an LDS tile with halo */
#define HSFLOW_KERNEL_STRIP 3  /* `fuse_steps` iterations per launch on register-resident strips:
                                  a wavefront holds 256 columns x strip_rows rows in VGPRs, DPP
                                  for left/right, LDS only for strip-edge rows (AUTO picks this, or
                                  its folded form below ~1.5 Mpixel per context)              */
#define HSFLOW_KERNEL_FOLD 4   /* as STRIP, two 128-column strips per wavefront (half the LDS
                                  exchange; inner boundary swapped in registers)              */
#define HSFLOW_KERNEL_PERSIST 5 /* STRIP as ONE launch per solve: workgroups keep their tile in registers across
                                  phases of `fuse_steps` iterations and swap halos through HBM, ordered by per-tile
                                  phase counters (replaces the host loop HSOpticalFlowOpenCL.cpp:748-752 inside one
                                  kernel).  Needs every workgroup resident at once: one tile per CU at most, width
                                  a multiple of 4, ITER or asynchronous ITER|EPS, and the context must be the only one alive on its
                                  device (two persistent grids could starve each other; every wait inside is bounded
                                  and a timed-out solve is repeated launch by launch).  On request only: a phase
                                  boundary measures as dear as a kernel boundary, so AUTO keeps STRIP.
                                  HSFLOW_E_SIZE when it cannot run.  hsflow_info.kernel reports STRIP,
                                  hsflow_info.persistent the number of phases.                                  */

typedef struct hsflow_ctx hsflow_ctx;

typedef struct hsflow_params {
    uint32_t struct_size; /* = sizeof(hsflow_params); guards ABI growth                  */
    int32_t mode;         /* HSFLOW_MODE_*                                               */
    float lambda;         /* CV mode: Lagrange multiplier of cvCalcOpticalFlowHS.  Any positive
                             finite float, denormals included (1 / lambda = Inf: the flow stays
                             zero, as in the original); anything else is HSFLOW_E_ARG.  The
                             kernels use max(fl32(1 / lambda), FLT_MIN), which changes nothing
                             a pixel can see.  (The test suite holds every kernel, over this
                             whole range, to 4x the original's own distance from an all-double
                             iteration on its test frames: DESIGN.md 5; no guarantee beyond
                             them.)  Beyond lambda = 1e20 strip / fold launches have at
                             most 8 iterations (info.fuse_steps).  The three largest floats
                             (lambda > 3.4028229e38, FLT_MAX among them) are where this library
                             and the original part: there the original's alpha of a pixel with
                             Ix = Iy = 0 is fl32(1 / 2^-128) = Inf, 0 * Inf is NaN and spreads
                             one pixel per iteration; this library's coefficients of such a
                             pixel are 0 and its flow stays finite, the flow the neighbouring
                             lambda gives.  Kept on purpose                              */
    float alpha;          /* CLASSIC mode: smoothness weight (Kernels.cl:85).  Any positive
                             finite float; the update divides by fl32(alpha * alpha) + Ex^2 +
                             Ey^2 as Kernels.cl does, so the flow is the reference's bit for
                             bit, NaN included: where alpha^2 underflows to zero (alpha below
                             about 2.6e-23) a flat pixel divides 0 / 0, and below
                             alpha^2 = 255 / FLT_MAX = 7.5e-37 (alpha below about 8.7e-19) a
                             flat pixel with a frame difference divides to Inf and 0 * Inf
                             follows; alpha^2 = Inf (alpha above 1.8e19) gives zero flow.
                             The strip kernel takes 2^-40 <= fl32(alpha * alpha) <= 2^40
                             (2^-20 <= alpha <= 2^20) and is HSFLOW_E_ARG outside; AUTO then
                             runs the LDS-tile kernel                                    */
    int32_t term_type;    /* HSFLOW_TERM_ITER | HSFLOW_TERM_EPS                          */
    int32_t max_iter;     /* CvTermCriteria.max_iter                                     */
    double epsilon;       /* CvTermCriteria.epsilon (caller rounds through float if it
                             wants cvTermCriteria()'s behaviour, cxtypes.h:912).  The rule
                             is strict and decided in double over the whole range: a
                             solve stops after the first sweep with (double)Eps < epsilon.
                             With a sweep budget any value is taken: +inf or one above
                             FLT_MAX stops after sweep 1; zero, a negative one or a NaN
                             never stops and the budget runs out.  From about
                             2^(127 - 2 fuse_steps) up, and for a NaN, an ITER|EPS solve
                             measures every sweep and hsflow_solve_async returns with the
                             solve complete.  Without a budget: finite and > 0, else
                             HSFLOW_E_NOTERM                                              */
    int32_t use_previous; /* 0: u=v=0 first (reference behaviour); 1: continue from the
                             flow currently held by the context: any floats, as the
                             reference takes them.  Where a caller wrote that flow
                             (hsflow_set_flow_device, the one-shot's velx / vely), or a
                             solve with lambda > 1e20 or a classic solve left it, a strip /
                             fold solve first measures the planes (one small launch, the
                             host waits for one word -- hsflow_solve_async too) and shortens
                             its launches so that no intermediate leaves the float range;
                             info.fuse_steps reports the length taken.  Where the largest
                             finite |value| m has m + n * 255 * sqrt(lambda) >= FLT_MAX / 64
                             = 5.3e36 (n: max_iter, at most 2^20) HSFLOW_KERNEL_SIMPLE takes
                             the solve, which is then complete when the call returns.  NaN / Inf spread one
                             pixel per sweep, as in the reference, in every kernel       */
    int32_t kernel;       /* HSFLOW_KERNEL_*                                             */
    int32_t fuse_steps;   /* FUSED: iterations per launch, 0 = auto                      */
    int32_t tile_w;       /* FUSED: core tile width  (multiple of 4), 0 = auto           */
    int32_t tile_h;       /* FUSED: core tile height, 0 = auto                           */
    int32_t threads;      /* FUSED: workgroup size 256/512/1024; STRIP: 64 x wavefronts
                             per workgroup (64..1024); 0 = auto                          */
    int32_t strip_rows;   /* STRIP / FOLD: rows held per lane (1..8), 0 = auto           */
    int32_t reuse_derivatives; /* 1: skip the derivative pass if the frames did not change since
                             the last solve of this context (row-slab chunks, warm starts)   */
    int32_t use_graph;    /* 1: capture the launch sequence in a hipGraph and replay it  */
    int32_t profile;      /* 1: bracket every kernel with HIP events (see hsflow_info)   */
} hsflow_params;

typedef struct hsflow_info {
    uint32_t struct_size;
    int32_t width, height, n_pairs, pitch; /* pitch in elements, same for every plane    */
    int32_t iterations_done;  /* sweeps executed by the last solve; the same for every pair of the
                                 context while a batch stops as one (see hsflow_solve); with
                                 hsflow_set_pair_termination the maximum over the pairs        */
    float last_eps;           /* Eps of the last sweep (EPS termination only): the maximum over all
                                 pairs of the context, like every Eps of a batch that stops as one;
                                 with hsflow_set_pair_termination that of the lowest pair that ran
                                 iterations_done sweeps.  An asynchronous
                                 ITER|EPS solve does not measure it; hsflow_get_info then runs that
                                 solve's last launch once more to obtain it (NaN if the flow was
                                 changed through hsflow_set_flow_device in between)               */
    int32_t kernel;           /* kernel actually used                                     */
    int32_t fuse_steps, tile_w, tile_h, threads, groups_per_thread;
    int32_t tiles;            /* workgroups per fused launch                              */
    int32_t lds_bytes;        /* dynamic LDS per workgroup                                */
    int32_t jacobi_launches;  /* launches of the Jacobi kernel in the last solve          */
    float deriv_ms;           /* profile=1: derivative kernel time                        */
    float jacobi_ms;          /* profile=1: sum of Jacobi kernel times                    */
    float solve_ms;           /* profile=1: first event to last event of the solve        */
    int32_t eps_rerun;        /* ITER|EPS: 1 if the fast pass could not prove "no early stop"
                                 and the solve was repeated with Eps measured in every sweep
                                 (hsflow_set_pair_termination: for any pair of the context)  */
    int32_t deriv_fused;      /* 1 if the derivative pass ran inside the first Jacobi launch of the
                                 last solve instead of as a kernel of its own                    */
    int32_t persistent;       /* phases of the one persistent launch the last solve ran as
                                 (HSFLOW_KERNEL_PERSIST), 0 for a launch per `fuse_steps` iterations */
} hsflow_info;

/* --- lifecycle ---------------------------------------------------------------------------- */

/* Fills p with the defaults (CV mode, lambda 1, ITER|EPS, 100 iterations, eps 1e-6f, auto). */
void hsflow_default_params(hsflow_params *p);

/* n_pairs independent image pairs of width x height live in one context (n_pairs >= 1).  Under ITER termination
 * the pairs are independent: each one's flow is bit for bit what a context of its own computes.  Under EPS they share
 * ONE stopping sweep by default (hsflow_solve): a pair's flow then depends on the others it is solved with; with
 * hsflow_set_pair_termination every pair stops on its own Eps and is independent under EPS too.  Any n_pairs is
 * accepted here; one whose launches would exceed the device's grid limits has no plan (HSFLOW_E_SIZE at the solve).
 * device: HIP ordinal.  stream: the hipStream_t all work is issued on (e.g. torch's current
 * stream; NULL is the device's default stream).  own_stream != 0: ignore `stream` and create a
 * private non-blocking stream instead. */
int hsflow_create(hsflow_ctx **out, int device, int width, int height, int n_pairs, void *stream,
                  int own_stream);
int hsflow_destroy(hsflow_ctx *ctx); /* NULL is accepted; idempotent per handle */
/* Row-slab decomposition: the context holds rows [first_row, first_row + height) of a larger frame.
 * The Jacobi update adds its four neighbours in an order that depends on the pixel's checkerboard parity
 * (x + y) & 1 in the FRAME; telling the context where its row 0 sits (only the parity matters) makes a slab
 * compute bit for bit what the whole-frame solve computes for the same pixels.  Default 0. */
int hsflow_set_row_origin(hsflow_ctx *ctx, int first_row);

/* The launch planners count on `compute_units` CUs instead of the whole chip (0: the whole chip again).  For a context
 * whose solves run BESIDE other contexts' solves, so that each solve takes the shape that costs the least CU-time (few
 * large tiles, little halo redundancy) rather than the one that spreads a small frame over every CU to shorten its own
 * latency: at the reference's 600x480 default (main.cpp:4-8) that is the difference between 210 tiles of 88x16 and 36 of
 * 216x40 per launch.  The slots of a pair pipeline do NOT set a share by themselves (the planners' cost models picked
 * worse shapes with one than without); HSFLOW_PIPELINE_CU_SHARE=<n> makes every slot plan for n CUs, as an experiment.
 * Results are bit-identical whatever the shape. */
int hsflow_set_cu_share(hsflow_ctx *ctx, int compute_units);

/* on != 0: an asynchronous ITER|EPS solve enqueues the reduction of its witness words right behind its last launch (a
 * small kernel per solve on the context's stream) instead of leaving it to whoever settles the check, and EVERY asynchronous
 * solve is followed by a one-thread kernel that writes a running count to page-locked memory: settling and hsflow_wait_solve
 * then poll that word -- no launch, no stream-wide wait, no event record (which costs a stream of solves 6 %).  Pays where the stream is not the bottleneck -- the
 * slots of a pair pipeline set it: their streams overlap, and for small frames the host's time per pair is what bounds
 * the stream.  Off by default: back-to-back solves on ONE stream would pay the kernel and its boundary every time. */
int hsflow_set_async_reduce(hsflow_ctx *ctx, int on);

/* How a context of several pairs stops under EPS termination (HSFLOW_MODE_CV, term_type EPS or ITER|EPS).
 * per_pair = 0 (the default): the batch stops as one, on the maximum of its pairs' Eps (hsflow_solve).
 * per_pair = 1: every pair stops on its OWN Eps, as cvCalcOpticalFlowHS called pair by pair does
 * (OpticalFlowOpenCV.cpp:29,94): pair i's flow, iterations_done and last_eps (hsflow_get_pair_result) are bit for bit
 * what a one-pair context computes for the same frames with the same parameters -- mode, lambda, criteria, kernel
 * choice, use_previous, row origin, Eps rows -- through hsflow_solve and hsflow_solve_async alike (with or without
 * use_graph and hsflow_set_async_reduce), once the owed check is settled; the one exemption is the project's own, values
 * below 1e-30 between different launch shapes (HSFLOW_VERIFY_TINY).  A batch then behaves like n_pairs calls of
 * cvCalcOpticalFlowHS.
 * How: the speculative witness pass of ITER|EPS runs over ALL pairs to the budget exactly as before (same launches,
 * same graph) and its words are reduced per pair; a proven pair stands at the budget.  The pairs that are not proven --
 * and every pair where there is no witness pass: the simple and the LDS-tile kernel, EPS alone -- go through the exact
 * pass TOGETHER: chunk launches over a device list of the pairs still running (n_active x tiles_per_pair workgroups),
 * hsflow_info.fuse_steps sweeps per chunk (HSFLOW_KERNEL_SIMPLE: HSFLOW_PAIR_STOP_SIMPLE_CHUNK one-sweep launches), ONE
 * read-back of every active pair's Eps per chunk.  A pair whose stop lies in the chunk is replayed from the chunk's intact
 * input for exactly the missing sweeps and dropped from the list; the next chunk is launched for the rest.  A pair that
 * stops at sweep k therefore costs at most ceil(k / T) * T + k sweeps beyond the witness pass, and nothing once it has
 * stopped.  Its final flow is copied into the other ping-pong buffer as well, so that every entry that reads or hands out
 * a pair's flow (hsflow_get_flow*, hsflow_flow_view_device, hsflow_render_*, hsflow_compare_flow_device, hsflow_verify,
 * hsflow_set_flow_device followed by a warm start) sees that pair's final flow, however many sweeps its neighbours ran.
 * profile = 1: deriv_ms / jacobi_ms / solve_ms cover the witness pass; the chunk launches behind it are not bracketed.
 * EPS alone: the stall rule (4 096 sweeps without a new minimum of Eps) runs per pair; a stalled pair keeps its flow and
 * reports HSFLOW_E_NOTERM in hsflow_get_pair_result, and the solve returns HSFLOW_E_NOTERM after every other pair has
 * stopped.  ITER alone and the classic modes have no Eps: nothing changes.  hsflow_solve_probe* do not depend on it.
 * HSFLOW_KERNEL_PERSIST on a context of several pairs with EPS in term_type is refused while the switch is on
 * (HSFLOW_E_ARG: the one launch holds every pair to its last phase).
 * Takes effect from the next solve; settles an owed check first.  On a one-pair context it is accepted and changes
 * nothing.  The existing take-over of an owed check by a bit-identical repeat solve keeps working. */
#define HSFLOW_PAIR_STOP_SIMPLE_CHUNK 32 /* one-sweep launches between two read-backs of the per-pair exact pass (a design constant) */
int hsflow_set_pair_termination(hsflow_ctx *ctx, int per_pair);

/* What the last solve did for ONE pair of the context. */
typedef struct hsflow_pair_result {
    uint32_t struct_size;     /* = sizeof(hsflow_pair_result), set by the caller                          */
    int32_t pair;
    int32_t status;           /* HSFLOW_OK, or HSFLOW_E_NOTERM for a pair the stall rule gave up on       */
    int32_t iterations_done;  /* sweeps this pair's flow has run                                          */
    float last_eps;           /* this pair's Eps at its last sweep                                        */
    int32_t eps_rerun;        /* 1: the witness pass proved nothing for this pair; it took the exact pass */
    int64_t sweeps_executed;  /* every sweep the device ran for this pair in the last solve, speculative
                                 and repeated ones included                                               */
} hsflow_pair_result;
/* With hsflow_set_pair_termination off (and for every solve without EPS) each pair reports the batch's values, status
 * being what the solve returned.  Like hsflow_get_info it settles an owed check and measures an unmeasured last_eps.
 * HSFLOW_E_STATE before the first solve; HSFLOW_E_ARG: null pointer, wrong struct_size, bad pair. */
int hsflow_get_pair_result(hsflow_ctx *ctx, int pair, hsflow_pair_result *out);

/* Waits until the last solve of THIS context has finished and settles the early-stop check it may owe.  With
 * hsflow_set_async_reduce on, that is a poll of the marker behind the solve: unlike hsflow_synchronize it does not wait for
 * what other contexts have enqueued on the same stream since (the slots of a pair pipeline share streams); without it,
 * the same as hsflow_synchronize. */
int hsflow_wait_solve(hsflow_ctx *ctx);

/* --- building blocks for drivers that run ONE solve over several contexts (row slabs, hsflow_slab_*) ----------- */

/* Only the changes of rows [first_row, first_row + rows) count for Eps and for the witness of ITER|EPS solves (rows <= 0:
 * the whole frame again).  A row slab sets its OWNED rows: its halo rows repeat the neighbour's and go stale towards
 * the slab's edge inside a chunk, so their changes say nothing about the frame's Eps
 * (cv210.dll@0x1012ed2f-0x1012eda5 takes the maximum over the frame).  Strip and simple kernels. */
int hsflow_set_eps_rows(hsflow_ctx *ctx, int first_row, int rows);
/* Exactly params->max_iter sweeps (whatever params->term_type says: nothing stops them) with the Eps of every sweep
 * -- over the rows of hsflow_set_eps_rows, the maximum over all pairs of the context (the Eps an EPS-terminated solve
 * of the batch stops on) -- written to sweep_eps[0 .. max_iter).  Synchronous.  What a driver needs to
 * find the stopping sweep of a solve that is spread over several contexts: Eps_k of the frame = the maximum of the
 * contexts' Eps_k. */
int hsflow_solve_probe(hsflow_ctx *ctx, const hsflow_params *params, float *sweep_eps);
/* The same solve with the Eps of every sweep PER PAIR: sweep_eps[k * n_pairs + i] is pair i's Eps of sweep k over the rows
 * of hsflow_set_eps_rows -- what a one-pair context's hsflow_solve_probe returns for that pair; the maximum of a row over
 * the pairs is what hsflow_solve_probe returns.  Independent of hsflow_set_pair_termination.  The strip and the folded
 * kernel (what AUTO picks) reduce the batch pass's words per pair in one launch; the simple and the LDS-tile kernel
 * write one word per (sweep, pair) in this pass.  max_iter x n_pairs <= 2^28
 * (HSFLOW_E_SIZE). */
int hsflow_solve_probe_pairs(hsflow_ctx *ctx, const hsflow_params *params, float *sweep_eps /* [max_iter][n_pairs] */);
/* The early-stop check an asynchronous ITER|EPS solve still owes, looked at WITHOUT acting on it: waits for the stream;
 * *proven = 1 if the witness words prove that Eps stayed >= epsilon in every sweep (over the rows of
 * hsflow_set_eps_rows), 0 if they do not -- the flow of the whole budget stands either way and nothing is re-run.  A
 * proof from ANY context of a spread solve covers the frame (its Eps is the maximum).  HSFLOW_E_STATE if nothing is owed.
 * With hsflow_set_pair_termination on a context of several pairs: *proven = 1 iff EVERY pair is proven. */
int hsflow_take_verdict(hsflow_ctx *ctx, int *proven);

/* --- frames in ---------------------------------------------------------------------------- */

/* Host u8 single-channel frames, row strides in bytes (>= width).  Synchronous. */
int hsflow_set_frames_u8(hsflow_ctx *ctx, int pair, const uint8_t *prev, size_t prev_stride,
                         const uint8_t *curr, size_t curr_stride);
/* Same, but only enqueued on ctx's stream: the host buffers must stay valid and unchanged until
 * the stream has passed the copy (hsflow_synchronize).  Truly asynchronous only from page-locked
 * memory (hsflow_host_alloc / hsflow_host_register); from pageable memory HIP stages the copy. */
int hsflow_set_frames_u8_async(hsflow_ctx *ctx, int pair, const uint8_t *prev, size_t prev_stride,
                               const uint8_t *curr, size_t curr_stride);
/* Same, source already in device memory on ctx's device; enqueued on ctx's stream. */
int hsflow_set_frames_u8_device(hsflow_ctx *ctx, int pair, const void *d_prev, size_t prev_stride,
                                const void *d_curr, size_t curr_stride);
/* Host 8-bit BGR frames (3 bytes/pixel): BGR->gray then optional 3x3 box blur on the GPU, i.e.
 * the reference CPU route's pre-processing (OpticalFlowOpenCV.cpp:17,20,27-28). Synchronous. */
int hsflow_set_frames_bgr8(hsflow_ctx *ctx, int pair, const uint8_t *prev_bgr, size_t prev_stride,
                           const uint8_t *curr_bgr, size_t curr_stride, int blur3x3);
/* Host u8 gray frames, 3x3 box blur (cvSmooth CV_BLUR, replicate border) on the GPU. Synchronous. */
int hsflow_set_frames_gray8_blur(hsflow_ctx *ctx, int pair, const uint8_t *prev, size_t prev_stride,
                                 const uint8_t *curr, size_t curr_stride);
/* Asynchronous forms of the two above: only enqueued on ctx's stream, host buffers owned by the context
 * until hsflow_synchronize. */
int hsflow_set_frames_bgr8_async(hsflow_ctx *ctx, int pair, const uint8_t *prev_bgr, size_t prev_stride,
                                 const uint8_t *curr_bgr, size_t curr_stride, int blur3x3);
int hsflow_set_frames_gray8_blur_async(hsflow_ctx *ctx, int pair, const uint8_t *prev, size_t prev_stride,
                                       const uint8_t *curr, size_t curr_stride);
/* Streaming (camera loop, HSOpticalFlowOpenCL.cpp:810-834): the current frame becomes the
 * previous one on the device and only the new frame is uploaded. */
int hsflow_push_frame_u8(hsflow_ctx *ctx, int pair, const uint8_t *next, size_t next_stride);

/* Frames in another layout (the values also name the layouts a pair pipeline takes, below); the CPU route's
 * pre-processing (OpticalFlowOpenCV.cpp:17-28) then runs on the device. */
#define HSFLOW_FRAMES_GRAY8 0      /* u8 gray, as is                                          */
#define HSFLOW_FRAMES_GRAY8_BLUR 1 /* u8 gray, 3x3 box blur on the device (cvSmooth CV_BLUR)  */
#define HSFLOW_FRAMES_BGR8 2       /* 8-bit BGR (3 bytes / pixel): BGR->gray on the device    */
#define HSFLOW_FRAMES_BGR8_BLUR 3  /* BGR->gray and blur: what runFromImg does before solving */
/* Frames ALREADY IN DEVICE MEMORY on ctx's device, in any of the four layouts; row strides in bytes (>= width for gray,
 * >= 3 * width for BGR), any alignment.  Only enqueued on ctx's stream, like hsflow_set_frames_u8_device, which is what
 * HSFLOW_FRAMES_GRAY8 runs.  The other three are ONE launch per pair: both frames go through gray conversion and blur
 * in registers (a lane walks a strip of HSFLOW_PRE_STRIP_ROWS rows with a window of three rows of sums) and land in the
 * context's planes -- no gray plane in between, every source byte read once plus one halo row per strip end.  Sources
 * whose base and stride are multiples of 4 are read a word at a time, others byte by byte; the bytes written are those
 * of hsflow_set_frames_bgr8 / hsflow_set_frames_gray8_blur from the same pixels (hsflow_preprocess_frame_host).
 * HSFLOW_E_ARG: null pointer, unknown format; HSFLOW_E_SIZE: a stride below the row's bytes. */
#define HSFLOW_PRE_STRIP_ROWS 8 /* rows a lane of the fused pre-processing kernel walks (a design constant) */
int hsflow_set_frames_device_ex(hsflow_ctx *ctx, int pair, int format, const void *d_prev, size_t prev_stride,
                                const void *d_curr, size_t curr_stride);
/* The reference's camera sequence on the device: prev := reblur_prev ? box_blur3(curr) : curr, then
 * curr := pre(format, next).  reblur_prev = 1 with a *_BLUR format is the reference's loop (OpticalFlowOpenCV.cpp:92-93,
 * 118: cvSmooth works in place and the blurred new frame becomes the next old one, so from the second pair on the old
 * frame enters the solver blurred twice); reblur_prev = 0 with HSFLOW_FRAMES_GRAY8 is hsflow_push_frame_u8.  Two launches
 * in stream order into the planes the context has always had (cached graphs stay valid).  hsflow_push_frame_ex takes
 * `next` from host memory, uploads it into the context's staging and returns when everything is complete;
 * hsflow_push_frame_device_ex takes it from device memory and only enqueues.
 * HSFLOW_E_ARG: null pointer, unknown format, reblur_prev not 0 or 1; HSFLOW_E_SIZE: stride below the row's bytes;
 * HSFLOW_E_STATE: no frames were set before. */
int hsflow_push_frame_ex(hsflow_ctx *ctx, int pair, int format, const uint8_t *next, size_t stride, int reblur_prev);
int hsflow_push_frame_device_ex(hsflow_ctx *ctx, int pair, int format, const void *d_next, size_t stride, int reblur_prev);
/* The rule itself on the host, no device needed: dst = pre(format, src), bit for bit what the device entries write
 * (csrc/hs_pre_rule.h, one header for the kernel and for this).  src and dst must not overlap; dst_stride >= width.
 * HSFLOW_E_ARG: null pointer, unknown format; HSFLOW_E_SIZE: non-positive size, a stride below the row's bytes. */
int hsflow_preprocess_frame_host(int format, const uint8_t *src, size_t src_stride, int width, int height,
                                 uint8_t *dst, size_t dst_stride);

/* A SEQUENCE of frames into consecutive pairs (ABI 0.14): the reference's camera loop (OpticalFlowOpenCV.cpp:76-93,118:
 * cvQueryFrame, gray, cvSmooth of old and new IN PLACE, solve, imgOld = imgNew) in a context of N pairs.  With the
 * frames f_0 .. f_{n-1}, p_j = pre(format, f_j) and B(x) = HSFLOW_FRAMES_GRAY8_BLUR of the BYTES of x (x's own edge
 * pixels repeated -- the blur of the stored plane, not a wider filter over f_j), pair first_pair + k, 0 <= k <= n - 2,
 * receives
 *     curr = p_{k+1}
 *     prev = p_k      without HSFLOW_SEQ_REBLUR, or for k == 0 without HSFLOW_SEQ_REBLUR_FIRST
 *     prev = B(p_k)   otherwise
 * HSFLOW_SEQ_REBLUR with a *_BLUR format is the reference's loop from its start: from the second pair on the old frame
 * enters the solver blurred twice.  HSFLOW_SEQ_REBLUR | HSFLOW_SEQ_REBLUR_FIRST is the same loop continued -- f_0 was
 * the new frame of an earlier pair already -- so a long clip goes through a context in consecutive batches that share
 * one frame.  The planes are exactly those the one-pair entries write: with flags 0
 * hsflow_set_frames_device_ex(format, f_k, f_{k+1}); for a reblurred pair hsflow_set_frames_device_ex(format, f_k, f_k)
 * followed by hsflow_push_frame_device_ex(format, f_{k+1}, 1) -- which cost a pair three launches and three reads of a
 * frame.  Here every frame is read ONCE, by one launch per chunk of at most HSFLOW_PRE_SEQ_MAX frames (the frame is a
 * grid dimension; frames are independent, so chunks need no overlap), and leaves p_j and / or B(p_j) in up to two
 * planes; nothing in between exists outside registers.  Measured on an MI355X, 9 resident BGR frames into 8 pairs,
 * BGR8_BLUR, HIP events around 200 repetitions (profiles/pre_sequence_time.txt; the frames stay cache-resident between
 * repetitions): 1080p 3.3 us per pair with flags 0 against 9.8 us for 8 x hsflow_set_frames_device_ex on the parent
 * commit, 4.9 us with HSFLOW_SEQ_REBLUR against 20.7 us for the one-pair calls above; 600x480 1.9 us against 6.7 us and
 * 1.9 us against 16.1 us. */
#define HSFLOW_SEQ_REBLUR 1       /* prev of every pair but the call's first is blurred once more        */
#define HSFLOW_SEQ_REBLUR_FIRST 2 /* ... and the call's first pair too (only together with HSFLOW_SEQ_REBLUR) */
#define HSFLOW_PRE_SEQ_MAX 32 /* frames per launch (four pointers each in the kernel's argument block); the environment variable of the same name overrides it per call, 1..HSFLOW_PRE_SEQ_MAX */
/* d_frames: a host array of n_frames pointers to frames resident on ctx's device, all in `format` with rows `stride`
 * bytes apart, any alignment; the array is free on return.  Only enqueues on ctx's stream, settles an owed ITER|EPS
 * check first like every frame entry, and writes into the planes the context has always had (cached graphs stay
 * valid).  Every argument is checked before anything is enqueued; on any error no pair's frames change.
 * HSFLOW_E_ARG: a null list or entry, unknown format, n_frames < 2, first_pair < 0, first_pair + n_frames - 1 > n_pairs,
 * flags not 0, 1 or 3, HSFLOW_PRE_SEQ_MAX in the environment unusable; HSFLOW_E_SIZE: a stride below the row's bytes. */
int hsflow_set_sequence_device_ex(hsflow_ctx *ctx, int first_pair, int format, const void *const *d_frames,
                                  int n_frames, size_t stride, int flags);
/* The rule on the host, no device needed: frames are n_frames host frames, prev and curr n_frames - 1 planes each of
 * width x height bytes with rows dst_stride apart (the planes of the call's pairs).  It walks a frame the way the
 * kernel does (csrc/hs_pre_rule.h, one definition for both), so the composition of the two borders can be checked on
 * a CPU.  Sources and planes must not overlap.  HSFLOW_E_ARG: null list or entry, unknown format or flags,
 * n_frames < 2; HSFLOW_E_SIZE: non-positive size, a stride below the row's bytes. */
int hsflow_preprocess_sequence_host(int format, int flags, const uint8_t *const *frames, int n_frames, size_t stride,
                                    int width, int height, uint8_t *const *prev, uint8_t *const *curr, size_t dst_stride);

/* --- solve -------------------------------------------------------------------------------- */

/* Derivative pass + Jacobi iterations for every pair of the context.  EPS termination on a batch, by default: the Eps
 * of a sweep is the maximum over ALL pairs of the context (each over the rows of hsflow_set_eps_rows), and the whole
 * batch stops at the first sweep whose Eps is below epsilon -- every pair runs the same number of sweeps, a pair that
 * converged early goes on while its neighbours do.  cvCalcOpticalFlowHS, called per pair, stops each one on its own:
 * hsflow_set_pair_termination makes the batch do the same.
 * hsflow_solve returns
 * after the device finished; hsflow_solve_async only enqueues (no profile) and the caller
 * synchronises the stream or calls hsflow_synchronize.  Asynchronous solves take ITER termination
 * with any kernel, or ITER|EPS (the reference's call, OpticalFlowOpenCV.cpp:29) with the strip /
 * fold kernels (what AUTO picks): the early-stop check is then owed until hsflow_synchronize / hsflow_get_flow /
 * hsflow_get_info / the next solve settles it -- if the fast pass cannot prove that the stop
 * never fired, the solve is repeated exactly (hsflow_info.eps_rerun = 1), so flow copied out by
 * an earlier hsflow_get_flow_async has to be fetched again in that case.  One exception keeps a
 * stream of solves free of host round trips: an hsflow_solve_async that repeats the owed solve bit
 * for bit (same parameters, use_previous = 0; the frames cannot have changed, setting them settles)
 * recomputes the same result and takes the owed check over instead of waiting for it. */
int hsflow_solve(hsflow_ctx *ctx, const hsflow_params *params);
int hsflow_solve_async(hsflow_ctx *ctx, const hsflow_params *params);
/* hsflow_set_frames_u8_device(ctx, 0, ...) + hsflow_solve_async(ctx, params) as ONE call, for a stream of resident pairs
 * (what hsflow_pipeline_submit_device does per pair).  Same results, same state afterwards -- the context holds its own
 * copy of both frames -- but where the solve's first Jacobi launch is the strip kernel with the derivative pass in it
 * (hsflow_info.deriv_fused, kernel STRIP: frames at least one region large, up to 6 rows per lane, CV mode, no
 * profiling, not the persistent launch), the context holds one pair, both pointers are 4-byte aligned and both strides
 * multiples of 4, that launch reads the caller's planes where they lie and its core lanes store the context's copy next
 * to the derivative words: no copy kernel runs (1080 workgroups, 4 MB read and written and one more kernel in every
 * pair's chain at 1080p).  In every other case the copy kernel runs first, as with the two calls.  With use_graph the
 * first launch, which carries this call's pointers, is issued by itself and the cached graph replays the launches after
 * it: one launch and one graph launch per call, as before.  The caller's planes must stay unchanged until the solve has
 * been waited for (hsflow_wait_solve, hsflow_synchronize).  HSFLOW_KEEP_FRAME_COPY=1 in the environment: always copy. */
int hsflow_solve_async_frames_device(hsflow_ctx *ctx, const void *d_prev, size_t prev_stride, const void *d_curr,
                                     size_t curr_stride, const hsflow_params *params);
/* How many hsflow_solve_async_frames_device calls of this context went without the copy kernel so far. */
int hsflow_frame_copies_elided(hsflow_ctx *ctx, uint64_t *count);
int hsflow_synchronize(hsflow_ctx *ctx);

/* --- results out -------------------------------------------------------------------------- */

/* fp32 flow to host, row strides in bytes (multiple of 4, >= 4*width).  Synchronous. */
int hsflow_get_flow(hsflow_ctx *ctx, int pair, float *u, size_t u_stride, float *v, size_t v_stride);
/* Same, only enqueued on ctx's stream (after the solve enqueued before it); u, v are complete
 * after hsflow_synchronize.  Page-locked destination for a real overlap with other streams. */
int hsflow_get_flow_async(hsflow_ctx *ctx, int pair, float *u, size_t u_stride, float *v, size_t v_stride);
/* Row range [row0, row0+nrows) of the flow to / from device memory, on ctx's stream (used for
 * the row-slab halo exchange).  set_ writes into the flow the next
 * use_previous=1 solve continues from.  Both settle an ITER|EPS check that hsflow_solve_async still
 * owes (they wait for the stream in that case); after an ITER-only solve they only enqueue.
 * Any float may be written.  After a set_ the context no longer knows how large its flow is: the next warm strip / fold
 * solve measures the planes first (see hsflow_params.use_previous), and so does every later one unless that measurement
 * found nothing above 1e15 (then the planes count as the solver's own again) or a solve with use_previous = 0 has made
 * them anew.
 * hsflow_set_flow_device_ex (ABI 0.15) is set_ with flags.  HSFLOW_FLOW_SOLVER_MADE: the caller vouches that the rows are
 * flow that a CV solve of this library made from zero with the lambda of this context's solves -- a neighbouring row
 * slab's halo rows, a copy of this context's own flow saved earlier.  The context then keeps what it knew about its
 * planes: nothing is measured, a warm hsflow_solve_async enqueues and returns as it always did.  That is what the row-slab
 * drivers (hsflow_slab_*, slab.py) pass.  Rows that are not what the flag says can overflow inside a strip launch. */
#define HSFLOW_FLOW_SOLVER_MADE 1
/* Where the context holds the current flow of `pair`, without a copy: device pointers to row 0 and the row
 * stride in bytes (rows are `width` floats; the pitch is that of hsflow_info).  Settles an ITER|EPS check that
 * hsflow_solve_async still owes and waits for the stream -- with hsflow_set_async_reduce, for the marker behind the last
 * solve unless flow rows were copied in or out (set_flow_device, get_flow_device, get_flow_async) since, in which case
 * for the stream -- so that nothing of this context that touches the planes is left in flight; they stay valid and unchanged
 * until the next call that changes this context's flow (solve, set_flow_device).  What a consumer on the device
 * (rendering, the next stage of a pipeline) reads instead of HSOpticalFlowOpenCL.cpp:655-675's blocking read-back. */
int hsflow_flow_view_device(hsflow_ctx *ctx, int pair, const float **d_u, const float **d_v, size_t *stride_bytes);
int hsflow_get_flow_device(hsflow_ctx *ctx, int pair, int row0, int nrows, void *d_u,
                           size_t u_stride, void *d_v, size_t v_stride);
int hsflow_set_flow_device(hsflow_ctx *ctx, int pair, int row0, int nrows, const void *d_u,
                           size_t u_stride, const void *d_v, size_t v_stride);
int hsflow_set_flow_device_ex(hsflow_ctx *ctx, int pair, int row0, int nrows, const void *d_u,
                              size_t u_stride, const void *d_v, size_t v_stride, int flags);
/* Derivative planes of the last solve as fp32 (CV: Ix, Iy, It; CLASSIC: Ex, Ey, Et). */
int hsflow_get_derivatives(hsflow_ctx *ctx, int pair, float *dx, float *dy, float *dt,
                           size_t stride);
/* The pre-processed u8 frames the solver actually sees (after gray/blur), to host. */
int hsflow_get_frames_u8(hsflow_ctx *ctx, int pair, uint8_t *prev, size_t prev_stride,
                         uint8_t *curr, size_t curr_stride);

/* --- the flow picture --------------------------------------------------------------------- */

/* What the reference delivers is a picture (OpticalFlowOpenCV.cpp:33-46, HSOpticalFlowOpenCL.cpp:759-769): on a black
 * image, for the grid points in raster order (y outer, x inner; y and x multiples of `step`), with a = u[y][x],
 * b = v[y][x]:
 *   1. drawn iff a > threshold || b > threshold || a < -threshold || b < -threshold (NaN in both draws nothing);
 *   2. the dot: the 13 pixels with dx*dx + dy*dy <= 4 around (x, y) (cvCircle, radius 2, filled) in dot_rgb;
 *   3. the line from (x, y) to ((int)((float)x + a*scale), (int)((float)y + b*scale)) -- fp32 arithmetic, truncation
 *      toward zero, as cvPoint(float, float) -- in line_rgb, rasterised as OpenCV 2.1's cvLine(thickness 1) does: from
 *      the LEFT end point, error term major - 2*minor, a diagonal step while the error is negative;
 *   4. every pixel clipped to the image, and LATER WRITES WIN: a grid point's line lies over its own dot, and all of a
 *      later grid point lies over all of an earlier one.
 * The device draws exactly that, byte for byte what the host drawing of the drop-in class (csrc/host) draws from the
 * same flow, without the flow ever leaving the device: every write gets a number (2k + 1 the dot, 2k + 2 the line of
 * grid point k), a pixel shows the highest number that reached it, so the picture does not depend on the order of
 * execution.  The work per line is bounded by the image, whatever the flow's magnitude.
 * Out of the host's defined range: where an end-point coordinate (float)x + a*scale or (float)y + b*scale is not finite
 * or its magnitude is >= 2^20 -- the host's (int) conversion is undefined there -- the dot is drawn and NO line.
 * The picture is RGB, 3 bytes per pixel, rows `stride` bytes apart; the bytes of a row beyond 3*width are left alone. */
#define HSFLOW_RENDER_CV 0   /* OpticalFlowOpenCV.cpp:33-46: threshold 1, scale 0.5   */
#define HSFLOW_RENDER_CL 1   /* HSOpticalFlowOpenCL.cpp:759-769: threshold 0.5, scale 1 */
typedef struct hsflow_render_params {
    uint32_t struct_size;    /* = sizeof(hsflow_render_params)                                   */
    int32_t step;            /* grid spacing in pixels, >= 1 (the reference: 4)                  */
    float threshold, scale;  /* threshold finite and >= 0; scale finite (negative: arrows point backwards) */
    uint8_t dot_rgb[3], line_rgb[3], pad[2];
} hsflow_render_params;
/* One of the reference's two drawings: step 4, dot (0, 0, 255), line (255, 0, 0) and the preset's threshold and scale
 * (any preset other than HSFLOW_RENDER_CL gives HSFLOW_RENDER_CV). */
void hsflow_default_render_params(hsflow_render_params *rp, int preset);
/* The picture of the current flow of `pair` into device memory (on ctx's device), only enqueued on ctx's stream: two
 * launches behind whatever produced the flow; complete after hsflow_synchronize / a wait for the stream.  Settles an
 * ITER|EPS check that hsflow_solve_async still owes first (like hsflow_get_flow_device: a re-run would change the
 * flow).  Reads the flow and never changes it: pointers from hsflow_flow_view_device stay valid.  On a context with
 * hsflow_set_async_reduce, hsflow_wait_solve and hsflow_flow_view_device called after it wait for the stream -- and
 * with it for the render -- not only for the marker behind the last solve.  The first render of a context allocates a
 * plane of width x height words; contexts that never render pay nothing.
 * HSFLOW_E_ARG: null pointer, wrong struct_size, step < 1, threshold not finite or negative, scale not finite, bad pair;
 * HSFLOW_E_SIZE: stride < 3*width. */
int hsflow_render_flow_device(hsflow_ctx *ctx, int pair, const hsflow_render_params *rp, void *d_rgb, size_t stride);
/* The same into host memory, synchronous: drawn into a picture the context keeps on the device (allocated by the first
 * call), copied to rgb (6.2 MB at 1080p where both flow planes are 16.6 MB), complete on return.  Replaces the
 * read-back of u and v AND the host loop over the grid (HSOpticalFlowOpenCL.cpp:759-769).  Waits only for what this
 * context enqueued.  Page-locked destination for the full PCIe rate. */
int hsflow_render_flow(hsflow_ctx *ctx, int pair, const hsflow_render_params *rp, uint8_t *rgb, size_t stride);
/* The in-image pixels of the line (x0, y0) -> (x1, y1) on a width x height image, in drawing order, by the closed form the
 * render kernel uses to skip the part of a line outside the image (host arithmetic, no device needed): returns their
 * number and writes the first `capacity` of them to xy as x, y pairs.  -1: non-positive size or xy null. */
int hsflow_render_line_pixels(int x0, int y0, int x1, int y1, int width, int height, int32_t *xy, int capacity);

/* --- the picture's file (cvSaveImage) ------------------------------------------------------- */

/* The reference delivers a file: runFromImg ends in cvSaveImage(output, imgFlow) (OpticalFlowOpenCV.cpp:47,
 * HSOpticalFlowOpenCL.cpp:771), libjpeg with its defaults.  The file, exactly:
 *   JFIF 1.01 baseline, the Annex K quantisation tables scaled by the quality (scale = q < 50 ? 5000 / q : 200 - 2 q,
 *   (base * scale + 50) / 100 clamped to 1..255), libjpeg's 16-bit fixed-point RGB -> YCbCr, 4:2:0 chroma (2x2 box
 *   average, rounding bias alternating 1, 2 along a row; the planes padded to whole MCUs by edge replication, the
 *   DOWNSAMPLED chroma plane by repeating its last row), the "islow" forward DCT, the standard Huffman tables, luma
 *   blocks outside the component's own block grid as dummy blocks (no AC, the DC of the block before), no restart
 *   markers, the stream padded with 1-bits, 0x00 behind every 0xFF, FF D9.
 * That is byte for byte what the drop-in CLI's writer (csrc/host/jpeg_encode.hpp) writes for an RGB picture, and with
 * it what libjpeg-turbo writes at the same quality with 4:2:0 and what the reference's own output files hold.  The
 * device forms compute it where the picture lies: of a 1080p picture (6.2 MB) only the file (tens of KB for an arrow
 * picture) crosses PCIe.  The bytes do not depend on the order of execution and are the same on every run.
 * quality: 1..100, otherwise HSFLOW_E_ARG; 95 is what cvSaveImage uses.  Gray pictures, other subsamplings, optimised
 * Huffman tables and restart markers are not offered. */
#define HSFLOW_JPEG_HEADER_BYTES 623 /* SOI, JFIF, two DQT, SOF0, four DHT, SOS: the same count for every picture */
/* Bytes that always suffice: 625 + 416 * 6 * ceil(w/16) * ceil(h/16)  (1660 bits per block, every byte stuffed); 0 for a non-positive size. */
size_t hsflow_jpeg_bound(int width, int height);
/* The rule on the host, no device needed (like hsflow_preprocess_frame_host): rgb is width x height pixels of 3 bytes,
 * rows `stride` bytes apart; the file goes to jpeg[0 .. capacity) and its size to *bytes.  Reads exactly the picture's
 * pixels and writes nothing at or beyond jpeg + capacity.
 * HSFLOW_E_ARG: null pointer (jpeg may be null when capacity is 0), quality outside 1..100; HSFLOW_E_SIZE: width or
 * height outside 1..65535, stride < 3*width, or capacity below the file's size -- then *bytes still holds the size
 * needed and the first `capacity` bytes are the file's; HSFLOW_E_OOM: no host memory for the coefficients. */
int hsflow_jpeg_encode_host(const uint8_t *rgb, size_t stride, int width, int height, int quality,
                            uint8_t *jpeg, size_t capacity, size_t *bytes);
/* An RGB picture of the context's size in device memory -> JPEG bytes in device memory; only enqueued on ctx's stream
 * (seven launches and a memset, nothing read back in between; complete after hsflow_synchronize / a wait for the
 * stream).  d_bytes: a device word, 8-byte aligned, that receives the file's size.  Nothing at or beyond
 * d_jpeg + capacity is written; with capacity below the file's size *d_bytes still holds the size needed -- this form
 * cannot know and returns HSFLOW_OK: the caller compares.  With capacity >= hsflow_jpeg_bound that never happens.
 * Touches no solver state.  The first encode of a context allocates its scratch (coefficients, bit lengths and offsets,
 * the raw stream, per quality the tables and header: 18.0 MB at 1080p), kept until hsflow_destroy; contexts that never
 * encode pay nothing, and the scratch does not count for HSFLOW_KERNEL_PERSIST's "only one alive" rule.
 * HSFLOW_E_ARG: null pointer, d_bytes not 8-byte aligned, quality outside 1..100; HSFLOW_E_SIZE: stride < 3*width, a
 * context wider or higher than 65535. */
int hsflow_jpeg_encode_device(hsflow_ctx *ctx, const void *d_rgb, size_t stride, int quality,
                              void *d_jpeg, size_t capacity, uint64_t *d_bytes /* device, 8-byte aligned */);
/* hsflow_render_flow_device into the context's own picture + the encode, behind each other on the stream.  The
 * ordering rules of hsflow_render_flow_device apply word for word: an ITER|EPS check that hsflow_solve_async still
 * owes is settled first, the flow is read and never changed, and on a context with hsflow_set_async_reduce
 * hsflow_wait_solve and hsflow_flow_view_device called after it wait for the stream.  Argument errors: those of
 * hsflow_render_flow_device and of hsflow_jpeg_encode_device. */
int hsflow_render_flow_jpeg_device(hsflow_ctx *ctx, int pair, const hsflow_render_params *rp, int quality,
                                   void *d_jpeg, size_t capacity, uint64_t *d_bytes);
/* The same into host memory, synchronous: only the file's bytes cross PCIe (size word first, then that many bytes).
 * Complete on return; waits only for what this context enqueued.  HSFLOW_E_SIZE with capacity below the file's size:
 * *bytes holds the size needed and jpeg is left alone.  Keeps the file on the device (at most min(capacity,
 * hsflow_jpeg_bound) bytes, allocated on demand) and a page-locked size word until hsflow_destroy. */
int hsflow_render_flow_jpeg(hsflow_ctx *ctx, int pair, const hsflow_render_params *rp, int quality,
                            uint8_t *jpeg, size_t capacity, size_t *bytes);

/* A BATCH of pictures (ABI 0.13): what the reference does once per run at the end of runFromImg -- the drawing and
 * cvSaveImage (OpticalFlowOpenCV.cpp:32-47, HSOpticalFlowOpenCL.cpp:759-771) -- for n pictures of the context's size by
 * ONE set of launches: every kernel of the single forms takes the picture from a further grid dimension and runs the same
 * body (csrc/hs_kernels_render.hip.h, csrc/hs_kernels_jpeg.hip.h), what differs from picture to picture goes to the
 * kernels by value, and picture i's scratch is slice i of one allocation (csrc/hs_jpeg_batch_plan.h).  A batch larger
 * than HSFLOW_JPEG_BATCH_MAX runs in consecutive chunks of at most that many on the stream: per chunk one memset for the
 * raw streams, at most one for the priority planes, two render launches and seven encode launches, whatever n is.
 * Picture i's file is byte for byte that of hsflow_jpeg_encode_device / hsflow_render_flow_jpeg for the same picture or
 * pair, whatever its position, its neighbours, n, the chunking or HSFLOW_JPEG_BATCH_MAX; nothing at or beyond
 * d_jpeg[i] + capacity is written, and a picture whose file does not fit changes nothing for its neighbours.
 * Memory: the batched scratch is separate from the single encode's, so single and batched calls can be enqueued back to
 * back in any order without synchronisation.  It is allocated on demand for as many pictures as the largest chunk so
 * far (grown behind a wait for the stream), kept until hsflow_destroy, and does not count for HSFLOW_KERNEL_PERSIST's
 * "only one alive" rule; contexts that never batch pay nothing.  Per 1080p picture of a chunk: about 18 MB of scratch;
 * for the render forms a priority plane (8.3 MB); for the render-and-encode forms the picture (6.2 MB); for the
 * synchronous form the output slot (min(capacity, hsflow_jpeg_bound) bytes) -- so HSFLOW_JPEG_BATCH_MAX times that at most.
 * Every argument is checked before anything is enqueued or allocated; on an error nothing is written and
 * hsflow_last_error names the entry's index, where there is one. */
/* 16: the smallest of {4, 8, 16, 32} within 5 % of the best per-file time of one synchronous call at 1080p, n = 32
 * (profiles/jpeg_batch_time.txt, measured with the constant at 32: 0.0964, 0.0889, 0.0828, 0.0816 ms per file -- "best
 * 0.0816; the smallest maximum within 5 % of it: 16"; the parent's hsflow_render_flow_jpeg: 0.212).  Small pictures would
 * take more: at 600x480 a chunk of 32 costs 0.0160 ms per file against 0.0200 with 16 (and 0.143 one by one).  The kernels'
 * argument blocks hold 32 pictures; to measure a larger candidate build with the constant raised (tools/jpeg_batch_time.py). */
#define HSFLOW_JPEG_BATCH_MAX 16 /* pictures per set of launches; the environment variable of the same name overrides it per call, 1..HSFLOW_JPEG_BATCH_MAX */
/* n RGB pictures of the context's size in device memory (rows `stride` bytes apart, any alignment, each its own) -> n
 * files in device memory, file i into d_jpeg[i][0 .. capacity), its size into d_bytes[i]; only enqueued on ctx's stream
 * (complete after hsflow_synchronize / a wait for the stream).  The lists are host arrays, free on return.  This form
 * cannot know a file's size: with capacity below it d_bytes[i] still holds the size needed and the call has returned
 * HSFLOW_OK, as hsflow_jpeg_encode_device.  Touches no solver state.
 * HSFLOW_E_ARG: n < 1, a null list or entry, quality outside 1..100, d_bytes null or not 8-byte aligned,
 * HSFLOW_JPEG_BATCH_MAX in the environment unusable; HSFLOW_E_SIZE: stride < 3*width, a context wider or higher than 65535. */
int hsflow_jpeg_encode_batch_device(hsflow_ctx *ctx, const void *const *d_rgb, int n, size_t stride, int quality,
                                    void *const *d_jpeg, size_t capacity, uint64_t *d_bytes /* n device words, 8-byte aligned */);
/* The pictures of the pairs first_pair .. first_pair + n - 1 into device memory, pair first_pair + i into d_rgb[i]; only
 * enqueued (two launches per chunk).  Pair i reads its own flow planes and owns a priority plane of its own: the context's
 * plane grows to one per picture of a chunk.  The ordering rules of hsflow_render_flow_device apply word for word: an
 * ITER|EPS check that hsflow_solve_async still owes is settled first, the flow is read and never changed, and on a
 * context with hsflow_set_async_reduce hsflow_wait_solve and hsflow_flow_view_device called after it wait for the
 * stream.  After a solve with hsflow_set_pair_termination pair i's picture is that of its own final flow.
 * HSFLOW_E_ARG: n < 1, first_pair < 0 or first_pair + n > n_pairs, a null list or entry, render params as
 * hsflow_render_flow_device, the environment value unusable; HSFLOW_E_SIZE: stride < 3*width. */
int hsflow_render_flow_batch_device(hsflow_ctx *ctx, int first_pair, int n, const hsflow_render_params *rp,
                                    void *const *d_rgb, size_t stride);
/* hsflow_render_flow_batch_device into pictures the context keeps + hsflow_jpeg_encode_batch_device, behind each other
 * on the stream; only enqueued.  The ordering rules and argument errors of both. */
int hsflow_render_flow_jpeg_batch_device(hsflow_ctx *ctx, int first_pair, int n, const hsflow_render_params *rp, int quality,
                                         void *const *d_jpeg, size_t capacity, uint64_t *d_bytes);
/* The same into host memory, synchronous: per chunk the size words cross in ONE copy, then each file's bytes, with one
 * wait each -- two host round trips per chunk where n hsflow_render_flow_jpeg calls take 2 n.  Complete on return; waits
 * only for what this context enqueued; hsflow_wait_solve's marker speaks for the context again afterwards.
 * HSFLOW_E_SIZE if any file exceeds capacity: bytes[i] then holds the size needed for EVERY i, a buffer whose file does
 * not fit is left alone, and buffers whose files fit may have been written.  Keeps per-picture output slots of
 * min(capacity, hsflow_jpeg_bound) bytes on the device and page-locked size words until hsflow_destroy.
 * HSFLOW_E_ARG: as the device form, with jpeg / bytes null (bytes needs no alignment). */
int hsflow_render_flow_jpeg_batch(hsflow_ctx *ctx, int first_pair, int n, const hsflow_render_params *rp, int quality,
                                  uint8_t *const *jpeg, size_t capacity, size_t *bytes /* n */);

/* --- the dense colour picture (ABI 0.16) ---------------------------------------------------- */

/* The arrow picture samples one pixel in `step` squared, hides what lies below its threshold and needs a scale from the
 * caller.  The picture everybody's tools draw from a DENSE flow field is the Middlebury colour wheel (Baker et al.'s
 * colorcode.cpp; KITTI's and Sintel's tools and flow_to_image reproduce it): hue is the direction, saturation the
 * magnitude, zero flow is white, unknown flow is black.  These entries draw it where the flow lies -- of a 1080p pair
 * 6.2 MB of picture (or its file) cross PCIe where both flow planes are 16.6 MB.  The rule is csrc/hs_color_rule.h, one
 * header for the kernels and the host form; device and host give the same bytes.  All arithmetic is fp32, every operation
 * rounded on its own (fl), sqrt and / correctly rounded.
 *   The wheel: 55 entries by Middlebury's integer arithmetic -- RY 15: (255, 255 i / 15, 0); YG 6: (255 - 255 i / 6, 255, 0);
 *   GC 4: (0, 255, 255 i / 4); CB 11: (0, 255 - 255 i / 11, 255); BM 13: (255 i / 13, 0, 255); MR 6: (255, 0, 255 - 255 i / 6).
 *   One pixel, a = u[y][x], b = v[y][x]:
 *   1. unknown iff isnan(a) || isnan(b) || fabsf(a) > 1e9f || fabsf(b) > 1e9f: the pixel is (0, 0, 0) and does not count
 *      for the scale;
 *   2. r = sqrtf(fl(fl(a*a) + fl(b*b)));
 *   3. the scale m: HSFLOW_COLOR_SCALE_AUTO -- the maximum of r over the picture's known pixels, 1 if that is 0;
 *      HSFLOW_COLOR_SCALE_FIXED -- max_flow.  rad = fl(r / m);
 *   4. theta = the rule's own atan2 of (-b, -a) with C's signed-zero conventions: t = fl(min(|y|, |x|) / max(|y|, |x|)) (0 when
 *      both are 0), p = t P(t t) with a six-term polynomial P (max |p - atan t| = 1.8e-6 on [0, 1]; coefficients in the
 *      rule header), |y| > |x|: p = fl(pi/2 - p); signbit(x): p = fl(pi - p); signbit(y): p = -p;
 *   5. fk = fl(fl(fl(fl(theta / pi) + 1) * 0.5f) * 54), k0 = min((int)fk, 54), k1 = k0 == 54 ? 0 : k0 + 1, f = fl(fk - k0);
 *   6. per channel: c0 = fl(wheel[k0] / 255.0f), c1 alike; col = fl(fl(fl(1 - f) * c0) + fl(f * c1)); rad <= 1:
 *      col = fl(fl(1 - rad) + fl(rad * col)), otherwise col = fl(col * 0.75f); the byte is (int)fl(255.0f * col).
 * Three departures from the Middlebury program: the RADIUS is normalised, after the square root, not the components before
 * it -- in AUTO mode rad <= 1 then holds exactly and the pixel that sets the scale cannot fall into the "> 1" branch by
 * rounding; the atan2 is the rule's own, no library's; and the saturation 1 - rad (1 - col) is formed as
 * (1 - rad) + rad col, the same quantity but exact at both ends: zero flow is (255, 255, 255) and a pixel on the scale
 * shows the wheel's own levels, where fl(1 - fl(1 - col)) would lose a level for every wheel level 1 .. 64 and every even
 * one up to 126 (43 / 255 would come out as 42); the sum never exceeds 1.  Against the same formula in float64 every channel is within
 * one level wherever rad is not within 2^-20 of 1 (tests/test_color_host.py).  The wheel's seam is Middlebury's: flow
 * (m, +0) is (255, 0, 0), flow (m, -0) is (255, 0, 43).
 * The picture is RGB, 3 bytes per pixel, rows `stride` bytes apart; the bytes of a row beyond 3*width are left alone.  The
 * AUTO maximum is a maximum and the pixels are independent: the bytes do not depend on the order of execution.
 * Time on an MI355X (profiles/color_time.txt, device events around 200 calls): a 1080p picture 0.010 ms with a
 * fixed scale and 0.039 ms with the picture's own (the maximum pass, a memset and a second launch), 0.008 / 0.020 ms per
 * picture in a batch of 8; 600x480: 0.004 .. 0.009 / 0.013 ms alone, 0.002 / 0.009 ms in a batch of 8; hsflow_render_flow_device of the same 1080p pair 0.015 ms, a
 * device-to-device copy of 19 bytes per pixel 0.010 ms.  The kernel is bound by the rule's arithmetic (a square root and
 * three correctly rounded divisions per pixel), not by memory. */
#define HSFLOW_COLOR_SCALE_AUTO 0  /* the picture's own largest radius */
#define HSFLOW_COLOR_SCALE_FIXED 1 /* max_flow                          */
typedef struct hsflow_color_params {
    uint32_t struct_size; /* = sizeof(hsflow_color_params)                         */
    int32_t scale_mode;   /* HSFLOW_COLOR_SCALE_*                                  */
    float max_flow;       /* FIXED: the scale, finite and > 0; AUTO: not looked at */
    int32_t reserved;
} hsflow_color_params;
/* HSFLOW_COLOR_SCALE_AUTO. */
void hsflow_default_color_params(hsflow_color_params *cp);
/* The rule on the host, no device needed (like hsflow_preprocess_frame_host): u and v are width x height floats, rows
 * u_stride / v_stride BYTES apart; *scale_used (may be null) receives m.
 * HSFLOW_E_ARG: null pointer, wrong struct_size, unknown scale mode, max_flow not finite or not > 0; HSFLOW_E_SIZE:
 * non-positive size, a flow stride below 4*width or no multiple of 4, stride < 3*width. */
int hsflow_color_flow_host(const float *u, size_t u_stride, const float *v, size_t v_stride, int width, int height,
                           const hsflow_color_params *cp, uint8_t *rgb, size_t stride, float *scale_used /* may be null */);
/* The pictures of the pairs first_pair .. first_pair + n - 1 into device memory, pair first_pair + i into d_rgb[i] (any
 * alignment, each its own); only enqueued on ctx's stream, in chunks of at most HSFLOW_JPEG_BATCH_MAX pictures (the
 * environment variable of that name is honoured as for the arrow pictures): per chunk, AUTO: one memset of the chunk's
 * scale words and two launches -- the maximum is formed on the device, as the bit pattern of the non-negative float by
 * an integer atomicMax, and read there; no value goes through the host -- FIXED: one launch.  Picture i is byte for byte
 * that of hsflow_color_flow_host of pair i's flow, whatever its position, its neighbours, n or the chunking.
 * The ordering rules of hsflow_render_flow_device apply word for word: an ITER|EPS check that hsflow_solve_async still
 * owes is settled first, the flow is read and never changed, pointers from hsflow_flow_view_device stay valid, and on a
 * context with hsflow_set_async_reduce hsflow_wait_solve and hsflow_flow_view_device called after it wait for the stream.
 * After a solve with hsflow_set_pair_termination pair i's picture is that of its own final flow.  The first colour call
 * of a context allocates its scale words (128 bytes), kept until hsflow_destroy; they do not count for
 * HSFLOW_KERNEL_PERSIST's "only one alive" rule, and contexts that never colour pay nothing.  Every argument is checked
 * before anything is enqueued.
 * HSFLOW_E_ARG: null pointer, list or entry, wrong struct_size, unknown scale mode, bad max_flow, n < 1, first_pair < 0 or
 * first_pair + n > n_pairs, the environment value unusable; HSFLOW_E_SIZE: stride < 3*width. */
int hsflow_color_flow_batch_device(hsflow_ctx *ctx, int first_pair, int n, const hsflow_color_params *cp,
                                   void *const *d_rgb, size_t stride);
/* A batch of one. */
int hsflow_color_flow_device(hsflow_ctx *ctx, int pair, const hsflow_color_params *cp, void *d_rgb, size_t stride);
/* The same into host memory, synchronous: drawn into the picture the context keeps on the device (the one
 * hsflow_render_flow uses), copied to rgb, complete on return; *scale_used (may be null) receives m.  Waits only for what
 * this context enqueued.  Page-locked destination for the full PCIe rate. */
int hsflow_color_flow(hsflow_ctx *ctx, int pair, const hsflow_color_params *cp, uint8_t *rgb, size_t stride,
                      float *scale_used /* may be null */);
/* The colour picture + its file: hsflow_color_flow_batch_device into pictures the context keeps (those of
 * hsflow_render_flow_jpeg_batch*) + hsflow_jpeg_encode_batch_device, behind each other on the stream.  Capacity, size
 * words, errors and what crosses PCIe are exactly those of hsflow_render_flow_jpeg_batch_device / _batch; the single forms
 * are batches of one, with the capacity and size semantics of hsflow_render_flow_jpeg_device / hsflow_render_flow_jpeg.
 * File i is byte for byte hsflow_jpeg_encode_host of hsflow_color_flow_host's picture.  A dense picture makes a LARGE
 * file -- several hundred KB at 1080p and quality 95 where an arrow picture has tens: hsflow_jpeg_bound is the capacity
 * to pass. */
int hsflow_color_flow_jpeg_batch_device(hsflow_ctx *ctx, int first_pair, int n, const hsflow_color_params *cp, int quality,
                                        void *const *d_jpeg, size_t capacity, uint64_t *d_bytes);
int hsflow_color_flow_jpeg_batch(hsflow_ctx *ctx, int first_pair, int n, const hsflow_color_params *cp, int quality,
                                 uint8_t *const *jpeg, size_t capacity, size_t *bytes /* n */);
int hsflow_color_flow_jpeg_device(hsflow_ctx *ctx, int pair, const hsflow_color_params *cp, int quality,
                                  void *d_jpeg, size_t capacity, uint64_t *d_bytes);
int hsflow_color_flow_jpeg(hsflow_ctx *ctx, int pair, const hsflow_color_params *cp, int quality,
                           uint8_t *jpeg, size_t capacity, size_t *bytes);

/* --- a picture warped by the flow, and the residual (ABI 0.17) -------------------------------- */

/* What every consumer of a dense field does next -- frame-rate conversion, stabilisation, de-noising -- is to warp the
 * second frame backwards onto the first, and the residual that leaves, the sum of |warp(curr) - prev|, is the number that
 * says how well a flow explains its pair where there is no ground truth.  These entries do both where the flow lies,
 * without a read-back of both fp32 planes (16.6 MB for a 1080p pair).  No counterpart in the reference.  The rule is
 * csrc/hs_warp_rule.h, one header for the kernel and the host form; device and host give the same bytes.  All arithmetic
 * is fp32, every operation rounded on its own (fl).
 * The direction is the solver's: It = B - A, so curr(x + u, y + v) ~ prev(x, y): the warped picture approximates PREV.
 *   One pixel (x, y), a = u[y][x], b = v[y][x], src a u8 picture of C interleaved channels (C = 1 or 3), t the fraction of
 *   the flow to apply:
 *   1. unknown iff the colour picture's test says so (isnan(a) || isnan(b) || fabsf(a) > 1e9f || fabsf(b) > 1e9f): every
 *      channel of the pixel is fill[c];
 *   2. fx = fl((float)x + fl(a * t)), fy = fl((float)y + fl(b * t));
 *   3. outside iff !(fx >= 0 && fx <= W-1 && fy >= 0 && fy <= H-1).  HSFLOW_WARP_BORDER_CONSTANT: the pixel is fill;
 *      HSFLOW_WARP_BORDER_REPLICATE: fx and fy are clamped to those ranges and sampling goes on;
 *   4. x0 = (int)floorf(fx), x1 = min(x0 + 1, W-1), ax = fl(fx - (float)x0); y0, y1 and ay alike;
 *   5. per channel: top = fl(p00 + fl(ax * fl(p10 - p00))), bot alike from row y1, val = fl(top + fl(ay * fl(bot - top)));
 *      the byte is min((int)fl(val + 0.5f), 255).
 * So fx == W-1 exactly is inside with ax = 0; a component of 1e9 is known (and outside), the next float above it unknown;
 * t = 0 gives src itself at every known pixel; a whole-number flow gives src shifted, exactly.  Against the same formula
 * in float64 every byte is within one level (tests/test_warp_host.py).
 * The statistics are exact integers and do not depend on the order of execution: inside / outside / unknown count the
 * pixels (inside: known and not outside; the three sum to W*H); sad_warped is the sum of |warped_c - ref_c| over the
 * inside pixels and all channels, sad_plain the sum of |src_c - ref_c| over the SAME pixels, so that the two compare;
 * max_warped and max_plain are the largest single differences.  Without a reference picture the four are 0.
 * dst must not overlap src or ref.  Rows of dst beyond C*width bytes are left alone.
 * Time on an MI355X: profiles/warp_time.txt. */
#define HSFLOW_WARP_BORDER_CONSTANT 0  /* a pixel that samples outside the picture is fill */
#define HSFLOW_WARP_BORDER_REPLICATE 1 /* ... samples the nearest pixel of the picture    */
typedef struct hsflow_warp_params {
    uint32_t struct_size; /* = sizeof(hsflow_warp_params)       */
    int32_t channels;     /* 1 or 3, interleaved                 */
    int32_t border;       /* HSFLOW_WARP_BORDER_*                */
    float t;              /* finite, |t| <= 1e6                  */
    uint8_t fill[4];      /* fill[c] for channel c; [3] not used */
} hsflow_warp_params;
typedef struct hsflow_warp_stats { /* 64 bytes, the same on the device and on the host */
    uint64_t inside, outside, unknown;
    uint64_t sad_warped, sad_plain;
    uint32_t max_warped, max_plain;
    uint8_t reserved[16];
} hsflow_warp_stats;
/* channels 1, HSFLOW_WARP_BORDER_CONSTANT, t = 1, fill 0. */
void hsflow_default_warp_params(hsflow_warp_params *wp);
/* The rule on the host, no device needed: u and v are width x height floats, rows u_stride / v_stride BYTES apart; src,
 * ref and dst are width x height pixels of wp->channels bytes.  ref == NULL: the SADs and maxima are 0.  dst == NULL:
 * no picture is written (statistics only).
 * HSFLOW_E_ARG: null u, v, src or wp, wrong struct_size, channels not 1 or 3, unknown border, t not finite or |t| > 1e6,
 * neither dst nor stats, dst equal to src or ref; HSFLOW_E_SIZE: non-positive size, a flow stride below 4*width or no
 * multiple of 4, a picture stride below channels*width. */
int hsflow_warp_host(const float *u, size_t u_stride, const float *v, size_t v_stride, int width, int height,
                     const hsflow_warp_params *wp, const uint8_t *src, size_t src_stride,
                     const uint8_t *ref /* may be null */, size_t ref_stride, uint8_t *dst /* may be null */, size_t dst_stride,
                     hsflow_warp_stats *stats /* may be null */);
/* The pictures d_src[i] warped by the flow of pair first_pair + i into d_dst[i] (device memory, any alignment, each its
 * own), the statistics against d_ref[i] into d_stats[i]; only enqueued on ctx's stream, in chunks of at most
 * HSFLOW_JPEG_BATCH_MAX pictures (the environment variable of that name is honoured as for the other pictures): per chunk
 * one launch, with statistics a memset of the chunk's records in front of it -- the counters are formed on the device by
 * integer atomics, one per counter and workgroup.  Picture i and record i are those of hsflow_warp_host with pair
 * first_pair + i's flow, whatever the position, the neighbours, n or the chunking.
 * d_src == NULL: the context's own pre-processed curr planes (what hsflow_get_frames_u8 hands out); channels must then be
 * 1, src_stride is not looked at, and d_ref == NULL then means its prev planes.  With caller pictures d_ref == NULL means
 * no reference: the SADs and maxima are 0.  d_dst == NULL: a statistics-only pass that writes no picture.  d_stats ==
 * NULL: no statistics.  The pictures may have any alignment; d_stats must be a multiple of 8 (the counters are 64-bit
 * atomics).
 * The ordering rules of hsflow_render_flow_device apply word for word: an ITER|EPS check that hsflow_solve_async still
 * owes is settled first, the flow is read and never changed, and on a context with hsflow_set_async_reduce
 * hsflow_wait_solve and hsflow_flow_view_device called after it wait for the stream.  After a solve with
 * hsflow_set_pair_termination pair i is warped by its own final flow.  Nothing is allocated.  Every argument is checked
 * before anything is enqueued.
 * HSFLOW_E_ARG: null wp, a null entry of a list, wrong struct_size, channels not 1 or 3 (or 3 with the context's own
 * frames), unknown border, bad t, neither d_dst nor d_stats, d_stats no multiple of 8, d_dst[i] equal to d_src[i] or d_ref[i], n < 1, first_pair < 0
 * or first_pair + n > n_pairs, the environment value unusable; HSFLOW_E_SIZE: a stride below channels*width. */
int hsflow_warp_batch_device(hsflow_ctx *ctx, int first_pair, int n, const hsflow_warp_params *wp,
                             const void *const *d_src /* n, or NULL */, size_t src_stride,
                             const void *const *d_ref /* n, or NULL */, size_t ref_stride,
                             void *const *d_dst /* n, or NULL */, size_t dst_stride, hsflow_warp_stats *d_stats /* n on the device, or NULL */);
/* A batch of one. */
int hsflow_warp_device(hsflow_ctx *ctx, int pair, const hsflow_warp_params *wp, const void *d_src, size_t src_stride,
                       const void *d_ref, size_t ref_stride, void *d_dst, size_t dst_stride, hsflow_warp_stats *d_stats);
/* The same with pictures in host memory, synchronous: src and ref (where given) are copied to the device, the picture
 * and the record come back, complete on return.  src == NULL: the context's own frames, as above.  Waits only for what
 * this context enqueued -- except in a call that has to allocate: the staging pictures (one each for src, ref and dst,
 * as needed) are allocated by the first call that needs them and again by a call with a larger picture (hipMalloc, and
 * hipFree of the smaller one, which the runtime may hold until the device is idle, the other slots of a pipeline's lane
 * included); they are kept until hsflow_destroy (hsflow_release_cached for the one-shot's context).  Contexts that never
 * warp pay nothing. */
int hsflow_warp(hsflow_ctx *ctx, int pair, const hsflow_warp_params *wp, const uint8_t *src, size_t src_stride,
                const uint8_t *ref, size_t ref_stride, uint8_t *dst, size_t dst_stride, hsflow_warp_stats *stats);

/* --- forward-backward consistency of two flows (ABI 0.18) ------------------------------------- */

/* hsflow_warp* tell with one number how well a flow explains its pair; these entries tell, pixel by pixel, WHERE it is to
 * be trusted.  A warped pixel in an occluded or mis-estimated region is a ghost, and Horn-Schunck smooths across motion
 * boundaries, so every consumer of the warp wants this mask.  The remedy is the standard one (Sundaram, Brox and Keutzer
 * 2010): solve A->B and B->A, follow the forward vector, read the backward flow there, and call the pixel consistent where
 * the two cancel.  Done where the flows lie, without a read-back of four fp32 planes (33 MB for a 1080p pair).  No
 * counterpart in the reference.  The rule is csrc/hs_fb_rule.h, one header for the kernel and the host form; device and
 * host give the same bits.  All arithmetic is fp32, every operation rounded on its own (fl).
 *   Forward flow (uf, vf) of a pair (A, B), backward flow (ub, vb) of the pair (B, A), both W x H.  One pixel (x, y),
 *   a = uf[y][x], b = vf[y][x]:
 *   1. UNKNOWN (3) iff the colour picture's test says so (isnan(a) || isnan(b) || fabsf(a) > 1e9f || fabsf(b) > 1e9f);
 *   2. fx = fl((float)x + a), fy = fl((float)y + b); OUTSIDE (2) iff !(fx >= 0 && fx <= W-1 && fy >= 0 && fy <= H-1).
 *      There is no border option: a target outside the frame has no backward flow;
 *   3. x0 = (int)floorf(fx), x1 = min(x0 + 1, W-1), ax = fl(fx - (float)x0); y0, y1 and ay alike (the warp's taps with
 *      t = 1).  If any of the four taps of (ub, vb) is not known by the test of 1.: UNKNOWN, even where its weight is 0;
 *   4. c = the bilinear sample of ub in the warp's order: top = fl(p00 + fl(ax * fl(p10 - p00))), bot alike from row y1,
 *      c = fl(top + fl(ay * fl(bot - top))); d alike from vb;
 *   5. ex = fl(a + c), ey = fl(b + d), err2 = fl(fl(ex * ex) + fl(ey * ey));
 *      mag2 = fl(fl(fl(a * a) + fl(b * b)) + fl(fl(c * c) + fl(d * d))); bound = fl(fl(alpha * mag2) + beta).
 *      Known components are at most 1e9, so nothing overflows;
 *   6. CONSISTENT (0) iff err2 <= bound, else INCONSISTENT (1).  Classes 0 and 1 are the "evaluated" pixels.
 * So fx == W-1 exactly is inside; a forward component of 1e9 is OUTSIDE, the next float above it UNKNOWN; a whole-number
 * forward flow with the exactly opposite backward flow is CONSISTENT with err2 == 0 even with alpha = beta = 0.  Against
 * the same formula in float64 the classes agree (0 of 192 400 test pixels differed) and err2 is within 9.24e-5 of
 * (err2 + 0.5) where the backward taps are ordinary flow (tests/test_fb_host.py).
 * Outputs, each may be absent, but at least one must be asked for:
 *   mask   a u8 plane, value[class] per pixel;
 *   err2   an fp32 plane: err2 at evaluated pixels, the quiet NaN 0x7fc00000 elsewhere (the colour picture's test calls
 *          those unknown).  The squared distance on purpose: no square root, so it stays bit-exact;
 *   stats  exact integers that do not depend on the order of execution: the four class counts (they sum to W*H);
 *          sum_err2_q, the sum over evaluated pixels of (uint32_t)min(fl(err2 * 256.0f), 65535.0f) -- the squared error in
 *          1/256 px^2, saturated at 256 px^2, so that the mean squared error is sum_err2_q / (256 * evaluated);
 *          max_err2_bits, the bit pattern of the largest err2 over evaluated pixels (non-negative floats order as unsigned
 *          integers), 0 if there are none.
 * Rows of mask beyond width bytes and of err2 beyond width floats are left alone.
 * Time on an MI355X (profiles/fb_time.txt): mask + err2 + statistics of a 1080p pair in 0.052 ms with the
 * solver's flows -- 2.75 x the time of a device-to-device copy of 37 bytes per pixel, which reads 37 and writes 37 (74 bytes
 * of traffic beside the check's 32 read + 5 written), 634 x faster than reading four planes back and checking on the host
 * (32.7 ms); 0.022 ms at 600x480 (6.0 x that copy, 468 x faster than the host route). */
#define HSFLOW_FB_CONSISTENT 0
#define HSFLOW_FB_INCONSISTENT 1
#define HSFLOW_FB_OUTSIDE 2
#define HSFLOW_FB_UNKNOWN 3
typedef struct hsflow_fb_params {
    uint32_t struct_size; /* = sizeof(hsflow_fb_params)            */
    float alpha;          /* finite, 0 <= alpha <= 1e6               */
    float beta;           /* finite, 0 <= beta <= 1e30               */
    uint8_t value[4];     /* the mask's byte for class HSFLOW_FB_*   */
} hsflow_fb_params;
typedef struct hsflow_fb_stats { /* 64 bytes, the same on the device and on the host */
    uint64_t consistent, inconsistent, outside, unknown;
    uint64_t sum_err2_q;
    uint32_t max_err2_bits;
    uint8_t reserved[20];
} hsflow_fb_stats;
/* alpha 0.01, beta 0.5 (Sundaram, Brox and Keutzer 2010), value {255, 0, 0, 0}: a confidence mask.  NULL is ignored. */
void hsflow_default_fb_params(hsflow_fb_params *fp);
/* The rule on the host, no device needed: four planes of width x height floats, rows *_stride BYTES apart.  mask, err2
 * and stats may each be null.
 * HSFLOW_E_ARG: a null flow plane or fp, wrong struct_size, alpha or beta out of range, nothing asked for;
 * HSFLOW_E_SIZE: a non-positive size, a float stride below 4*width or no multiple of 4, a mask stride below width. */
int hsflow_fb_host(const float *uf, size_t uf_stride, const float *vf, size_t vf_stride, const float *ub, size_t ub_stride,
                   const float *vb, size_t vb_stride, int width, int height, const hsflow_fb_params *fp,
                   uint8_t *mask /* may be null */, size_t mask_stride, float *err2 /* may be null */, size_t err2_stride,
                   hsflow_fb_stats *stats /* may be null */);
/* Check i reads the flow of pair fwd_pairs[i] forwards and that of pair bwd_pairs[i] backwards (host arrays of n, free on
 * return; any pair may appear any number of times) into d_mask[i], d_err2[i] and d_stats[i] (device memory); only enqueued
 * on ctx's stream, in chunks of at most HSFLOW_JPEG_BATCH_MAX checks (the environment variable of that name is honoured
 * as for the other pictures): per chunk one launch, with statistics a memset of the chunk's records in front of it -- the
 * counters are formed on the device by integer atomics, one per counter and workgroup.  Output i is that of
 * hsflow_fb_host with the two pairs' flows, whatever the position, the neighbours, n or the chunking.
 * d_mask, d_err2, d_stats: each may be NULL, not all three.  The mask may have any alignment; d_err2[i] and err2_stride
 * must be multiples of 4, d_stats a multiple of 8 (the counters are 64-bit atomics).
 * The ordering rules of hsflow_warp_batch_device apply word for word: an ITER|EPS check that hsflow_solve_async still
 * owes is settled first, the flow is read and never changed, and on a context with hsflow_set_async_reduce
 * hsflow_wait_solve and hsflow_flow_view_device called after it wait for the stream.  After a solve with
 * hsflow_set_pair_termination every pair's own final flow is read.  Nothing is allocated.  Every argument is checked
 * before anything is enqueued.
 * HSFLOW_E_ARG: null fp or pair list, a null entry of an output list, wrong struct_size, alpha or beta out of range,
 * nothing asked for, a pair out of range, n < 1, d_err2[i] no multiple of 4, d_stats no multiple of 8, the environment
 * value unusable; HSFLOW_E_SIZE: a mask stride below width, an err2 stride below 4*width or no multiple of 4. */
int hsflow_fb_batch_device(hsflow_ctx *ctx, int n, const int *fwd_pairs, const int *bwd_pairs, const hsflow_fb_params *fp,
                           void *const *d_mask /* n, or NULL */, size_t mask_stride, void *const *d_err2 /* n, or NULL */, size_t err2_stride,
                           hsflow_fb_stats *d_stats /* n on the device, or NULL */);
/* A batch of one. */
int hsflow_fb_device(hsflow_ctx *ctx, int fwd_pair, int bwd_pair, const hsflow_fb_params *fp, void *d_mask, size_t mask_stride,
                     void *d_err2, size_t err2_stride, hsflow_fb_stats *d_stats);
/* The same with the backward flow from caller planes on ctx's device: width x height floats each, 4-byte aligned, rows
 * b_stride bytes apart (a multiple of 4, at least 4*width) -- another context's hsflow_flow_view_device, or a flow from
 * elsewhere.  The caller orders that producer before ctx's stream.  HSFLOW_E_ARG: a null or misaligned plane;
 * HSFLOW_E_SIZE: a bad b_stride; else as above. */
int hsflow_fb_planes_device(hsflow_ctx *ctx, int fwd_pair, const void *d_ub, const void *d_vb, size_t b_stride,
                            const hsflow_fb_params *fp, void *d_mask, size_t mask_stride, void *d_err2, size_t err2_stride,
                            hsflow_fb_stats *d_stats);
/* The results in host memory, synchronous: complete on return.  Waits only for an event behind its own work, like
 * hsflow_warp -- except in a call that has to allocate: the staging (a mask, an err2 plane, a record, as needed) is
 * allocated by the first call that needs it and kept until hsflow_destroy (hsflow_release_cached for the one-shot's
 * context).  Contexts that never check pay nothing. */
int hsflow_fb(hsflow_ctx *ctx, int fwd_pair, int bwd_pair, const hsflow_fb_params *fp, uint8_t *mask, size_t mask_stride,
              float *err2, size_t err2_stride, hsflow_fb_stats *stats);
/* hsflow_fb with the backward flow from caller planes on ctx's device, as hsflow_fb_planes_device takes them. */
int hsflow_fb_planes(hsflow_ctx *ctx, int fwd_pair, const void *d_ub, const void *d_vb, size_t b_stride, const hsflow_fb_params *fp,
                     uint8_t *mask, size_t mask_stride, float *err2, size_t err2_stride, hsflow_fb_stats *stats);
/* The reversed pair of a bidirectional solve: pair dst_pair receives prev = src_pair's pre-processed curr plane and
 * curr = its prev plane, by device copies on ctx's stream, so the frames are uploaded and pre-processed once.  It goes
 * the way of hsflow_set_frames_u8_device: an owed check is settled first, dst_pair's coefficients are rebuilt by its next
 * solve, cached graphs stay valid.  "Frames were set" is one flag per context: the caller sees to it that src_pair itself
 * has frames -- a source pair that never received any, while another pair did, is copied as it lies, without an error.
 * HSFLOW_E_ARG: a bad pair, dst_pair == src_pair; HSFLOW_E_STATE: no frames were set in the context. */
int hsflow_set_frames_reversed(hsflow_ctx *ctx, int dst_pair, int src_pair);

/* --- median filter and hole filling of the flow (ABI 0.19) ------------------------------------ */

/* hsflow_fb* end with a mask that says "this vector is not to be trusted"; these entries act on it.  Horn-Schunck smooths
 * across motion boundaries and leaves outliers at occlusions, and the standard remedy has two parts: a median filter of
 * the field (Sun, Roth and Black 2010) and filling the untrusted pixels from their trusted neighbours.  Done where the
 * flow lies, without a read-back and an upload of both fp32 planes (16.6 MB each way for a 1080p pair).  No counterpart
 * in the reference.  The rule is csrc/hs_median_rule.h, one header for the kernel and the host form; the median is a
 * selection on integers, so device and host give the same bits.
 *   Inputs: flow planes u, v (W x H fp32), an optional u8 state plane, radius r in {1, 2} (window 3x3 or 5x5), a mode and
 *   min_votes in 1 .. (2r+1)^2.  One pass at the pixel p = (x, y), a = u[p], b = v[p]:
 *   1. known(p) is the colour picture's test: !(isnan(a) || isnan(b) || fabsf(a) > 1e9f || fabsf(b) > 1e9f);
 *   2. the input state s(p): 0 (INVALID) if !known(p) or the state byte is 0; 2 (FILLED) if the byte is 2; 1 (KEPT) for
 *      any other non-zero byte, or when no state plane is given.  So the default mask of hsflow_fb (255 = consistent) can
 *      be passed as it is;
 *   3. the voters are the pixels q of the (2r+1)^2 window around p that lie inside the frame and have s(q) != 0.  The
 *      window is clipped at the frame, not replicated; p itself votes if it is valid; n is the number of voters;
 *   4. the median of a component is taken over the integer keys key(f) = bits(f) ^ ((bits(f) >> 31) ? 0xffffffff :
 *      0x80000000), an order-preserving map in which -0.0 < +0.0: the voter key of rank (n - 1) >> 1 in ascending order
 *      (the lower median), mapped back to its bits.  u and v are filtered independently, so the output vector need not
 *      be any input vector;
 *   5. HSFLOW_MEDIAN_FILTER: if n >= min_votes the output is the two medians and s_out = s if s != 0, else 2; otherwise
 *      the output is the input bits and s_out = s;
 *   6. HSFLOW_MEDIAN_FILL: if s != 0 the output is the input bits and s_out = s; if s == 0 and n >= min_votes the output
 *      is the two medians and s_out = 2; otherwise the input bits (NaNs are copied bit for bit) and s_out = 0;
 *   7. `passes` k >= 1: pass j + 1 reads pass j's output flow and output state.
 * So a window of {-0.0, +0.0} gives -0.0; a component of 1e9 votes, the next float above it does not; the corner pixel
 * of a 5x5 window has at most 9 voters; a hole pixel at Chebyshev depth d inside an otherwise valid field is filled, with
 * min_votes 1, in pass ceil(d / r).
 * Outputs, each may be absent, but at least one must be asked for:
 *   the two flow planes, together or not at all;
 *   the output state plane, bytes 0 UNFILLED, 1 KEPT, 2 FILLED -- a valid input state, so passes can be chained;
 *   stats  exact integers about the LAST pass: kept, filled, unfilled count s_out (they sum to W*H); newly_filled counts
 *          s == 0 -> s_out == 2 in that pass; changed counts the pixels whose output bits differ from that pass's input
 *          bits in u or v.  The reserved bytes are zero.
 * Rows of the outputs beyond width elements are left alone.  An output may not overlap an input.
 * Time on an MI355X (profiles/median_time.txt), one pass over a 1080p pair's flow into caller planes:
 * 0.016 ms with the 3x3 window and 0.050 ms with the 5x5 one (0.018 and 0.052 ms filling from the hsflow_fb mask), with
 * the record 0.011 .. 0.013 ms more; hsflow_median_apply with four passes 0.076 and 0.196 ms.  That is 4.2 x and 13 x the
 * time of a device-to-device copy of both planes (8 bytes per pixel read, 8 written): the selection, not the memory,
 * bounds the pass.  Against the host route (hsflow_get_flow, hsflow_median_host, upload and hsflow_set_flow_device: 75.5
 * and 244 ms) a pass is 4700 and 4900 times faster; at 600x480 0.006 and 0.015 ms, 1.7 x and 4.0 x the copy, 1300 and
 * 2400 times faster than the host route. */
#define HSFLOW_MEDIAN_FILTER 0
#define HSFLOW_MEDIAN_FILL 1
#define HSFLOW_MEDIAN_UNFILLED 0
#define HSFLOW_MEDIAN_KEPT 1
#define HSFLOW_MEDIAN_FILLED 2
#define HSFLOW_MEDIAN_MAX_PASSES 64
typedef struct hsflow_median_params {
    uint32_t struct_size; /* = sizeof(hsflow_median_params)        */
    int32_t radius;       /* 1 (3x3) or 2 (5x5)                      */
    int32_t mode;         /* HSFLOW_MEDIAN_FILTER or HSFLOW_MEDIAN_FILL */
    int32_t min_votes;    /* 1 .. (2 radius + 1)^2                   */
} hsflow_median_params;
typedef struct hsflow_median_stats { /* 64 bytes, the same on the device and on the host */
    uint64_t kept, filled, unfilled;
    uint64_t newly_filled;
    uint64_t changed;
    uint8_t reserved[24];
} hsflow_median_stats;
/* radius 1, HSFLOW_MEDIAN_FILTER, min_votes 1.  NULL is ignored. */
void hsflow_default_median_params(hsflow_median_params *mp);
/* The rule on the host, no device needed: `passes` passes (1 .. HSFLOW_MEDIAN_MAX_PASSES) over two planes of width x
 * height floats, rows *_stride BYTES apart; state may be null (every known pixel is KEPT).  u_out / v_out (together),
 * state_out and stats may each be null, not all.  With several passes the planes between them are the call's own.
 * HSFLOW_E_ARG: a null flow plane or mp, wrong struct_size, radius not 1 or 2, an unknown mode, min_votes or passes out
 * of range, nothing asked for, one flow output without the other, an output that overlaps (or is) an input;
 * HSFLOW_E_SIZE: a non-positive size, a float stride below 4*width or no multiple of 4, a byte stride below width. */
int hsflow_median_host(const float *u, size_t u_stride, const float *v, size_t v_stride, const uint8_t *state /* may be null */,
                       size_t state_stride, int width, int height, const hsflow_median_params *mp, int passes,
                       float *u_out /* may be null */, float *v_out /* may be null */, size_t out_stride,
                       uint8_t *state_out /* may be null */, size_t state_out_stride, hsflow_median_stats *stats /* may be null */);
/* ONE pass over the flows of the pairs first_pair .. first_pair + n - 1: field i reads the flow of pair first_pair + i
 * and d_state[i] into d_u_out[i], d_v_out[i], d_state_out[i] and d_stats[i] (device memory; the lists are host arrays of
 * n, free on return); only enqueued on ctx's stream, in chunks of at most HSFLOW_JPEG_BATCH_MAX fields (the environment
 * variable of that name is honoured as for the pictures): per chunk one launch, with statistics a memset of the chunk's
 * records in front of it -- the counters are formed on the device by integer atomics, one per counter and workgroup.
 * Output i is that of hsflow_median_host with that pair's flow, whatever the position, the neighbours, n or the chunking.
 * d_state, d_u_out + d_v_out, d_state_out, d_stats: each may be NULL, the outputs not all three.  The byte planes may
 * have any alignment; d_u_out[i], d_v_out[i] and out_stride must be multiples of 4, d_stats a multiple of 8 (the counters
 * are 64-bit atomics).
 * The ordering rules of hsflow_fb_batch_device apply word for word: an ITER|EPS check that hsflow_solve_async still owes
 * is settled first, the flow is read and never changed, and on a context with hsflow_set_async_reduce hsflow_wait_solve
 * and hsflow_flow_view_device called after it wait for the stream.  After a solve with hsflow_set_pair_termination every
 * pair's own final flow is read.  Nothing is allocated.  Every argument is checked before anything is enqueued.
 * HSFLOW_E_ARG: null mp, a null entry of a list, wrong struct_size, radius, mode or min_votes out of range, nothing asked
 * for, one flow output without the other, an output that overlaps an input of the batch, a pair out of range, n < 1, a
 * flow output no multiple of 4, d_stats no multiple of 8, the environment value unusable; HSFLOW_E_SIZE: a byte stride
 * below width, out_stride below 4*width or no multiple of 4. */
int hsflow_median_batch_device(hsflow_ctx *ctx, int first_pair, int n, const hsflow_median_params *mp,
                               const void *const *d_state /* n, or NULL */, size_t state_stride, void *const *d_u_out /* n, or NULL */,
                               void *const *d_v_out /* n, or NULL */, size_t out_stride, void *const *d_state_out /* n, or NULL */,
                               size_t state_out_stride, hsflow_median_stats *d_stats /* n on the device, or NULL */);
/* A batch of one. */
int hsflow_median_device(hsflow_ctx *ctx, int pair, const hsflow_median_params *mp, const void *d_state, size_t state_stride,
                         void *d_u_out, void *d_v_out, size_t out_stride, void *d_state_out, size_t state_out_stride,
                         hsflow_median_stats *d_stats);
/* One pass over caller planes on ctx's device: width x height floats each, 4-byte aligned, rows in_stride bytes apart (a
 * multiple of 4, at least 4*width).  The output state (0 / 1 / 2) is a valid input state, so a caller chains passes by
 * calling again with the outputs as inputs and fresh outputs.  The caller orders the planes' producer before ctx's stream.
 * HSFLOW_E_ARG: a null or misaligned plane; HSFLOW_E_SIZE: a bad in_stride; else as above. */
int hsflow_median_planes_device(hsflow_ctx *ctx, const hsflow_median_params *mp, const void *d_u, const void *d_v, size_t in_stride,
                                const void *d_state /* or NULL */, size_t state_stride, void *d_u_out, void *d_v_out, size_t out_stride,
                                void *d_state_out, size_t state_out_stride, hsflow_median_stats *d_stats);
/* `passes` passes (1 .. HSFLOW_MEDIAN_MAX_PASSES) whose result REPLACES the pair's flow in the context, so every later
 * picture, warp, check and use_previous = 1 solve reads it.  Only enqueued.  d_state (or NULL), d_state_out (or NULL, the
 * last pass's state) and d_stats (or NULL, the last pass's record) are device memory as above.  The flow goes to and fro
 * between the pair's planes and a scratch of one pair of fp32 planes, the states between two byte planes; the first call
 * that needs them allocates them, and they are kept until hsflow_destroy (hsflow_release_cached for the one-shot's
 * context).  Contexts that never filter pay nothing.  For the context's knowledge of its planes it goes the way of
 * hsflow_set_flow_device: an owed check is settled first, the planes count as the caller's (the next warm strip / fold
 * solve measures them), cached graphs stay valid, and hsflow_flow_view_device called after it waits for the stream.
 * HSFLOW_E_ARG: as hsflow_median_device, passes out of range, d_state_out overlapping d_state or the pair's planes. */
int hsflow_median_apply(hsflow_ctx *ctx, int pair, const hsflow_median_params *mp, int passes, const void *d_state /* or NULL */,
                        size_t state_stride, void *d_state_out /* or NULL */, size_t state_out_stride, hsflow_median_stats *d_stats /* or NULL */);
/* `passes` passes over the pair's flow with everything in host memory, synchronous: complete on return.  It does not
 * change the context's flow.  Waits only for an event behind its own work, like hsflow_fb -- except in a call that has
 * to allocate: the staging (up to two pairs of fp32 planes, two byte planes, a record) is shared with hsflow_median_apply
 * and kept like it. */
int hsflow_median(hsflow_ctx *ctx, int pair, const hsflow_median_params *mp, int passes, const uint8_t *state /* or NULL */,
                  size_t state_stride, float *u /* or NULL */, float *v /* or NULL */, size_t out_stride, uint8_t *state_out /* or NULL */,
                  size_t state_out_stride, hsflow_median_stats *stats /* or NULL */);

/* --- the frame at time t between the two frames of a pair (ABI 0.20) --------------------------- */

/* Frame-rate conversion, the consumer that hsflow_warp* name: the picture at time t, 0 <= t <= 1, between the two frames
 * of a pair (A, B) = (prev, curr), by the interpolation algorithm of Baker et al. ("A Database and Evaluation Methodology
 * for Optical Flow", IJCV 2011, section 3.3.2), the paper the colour wheel follows.  hsflow_warp with a fractional t reads
 * the vector at the pixel the picture is drawn at, not the vector that ARRIVES there, takes one frame only and knows
 * nothing of occlusion; this operator projects the forward flow to time t, fills the holes, fetches both frames along
 * the projected vector and blends them, or takes one frame alone where the other does not see the point.  Nothing of it
 * is in the reference.  The rule is csrc/hs_interp_rule.h, one header for the kernels and the host form.  All arithmetic
 * is fp32, every operation rounded on its own (fl); the integer parts are exact; device and host give the same bits.
 * Inputs: the forward flow (u, v), W x H fp32; the pictures prev and curr of C in {1, 3} interleaved u8 channels;
 * optional u8 planes vis_prev (on A's grid) and vis_curr (on B's grid), non-zero = "this pixel is visible in the other
 * frame" -- the default masks of hsflow_fb of (fwd, bwd) and of (bwd, fwd) can be passed as they are; t; the fill's
 * radius, min_votes and passes.
 *   P, projection.  The source pixel p = (x, y), a = u[p], b = v[p]:
 *   1. !known(a, b) (the colour picture's test): p contributes nothing and is counted `unknown`;
 *   2. the cost of p: the warp's taps of (a, b) at t = 1 with HSFLOW_WARP_BORDER_CONSTANT; not inside: 1023; else the sum
 *      over the channels of |prev_c[p] - the warp's bilinear byte of curr_c| (0 .. 765): the photo-consistency of (a, b);
 *   3. hx = fl(fl((float)x + fl(a * t)) + 0.5f), hy alike.  If !(hx >= 0 && hx < (float)W && hy >= 0 && hy < (float)H), on
 *      the floats, p is counted `left`; else its cell is q = ((int)floorf(hx), (int)floorf(hy));
 *   4. key = (uint64)cost << 32 | (uint32)(y * W + x); a cell keeps the MINIMUM key of all sources that land on it -- the
 *      lowest cost, at equal cost the lower source index -- whatever the order of arrival;
 *   5. a cell with a key receives the bits of (u, v) of that key's source and state 1; an empty cell is a hole: +0.0,
 *      +0.0, state 0.  `holes` counts the empty cells, `collisions` is (sources that landed) - (cells hit).
 *   F, fill.  fill_passes passes (0 .. HSFLOW_MEDIAN_MAX_PASSES) of HSFLOW_MEDIAN_FILL with fill_radius and fill_min_votes
 *      over (ut, vt, state): a hole at Chebyshev distance d from the nearest hit cell is filled in pass ceil(d / radius)
 *      (min_votes 1) and gets state 2.  `unfilled` counts the state-0 cells afterwards; their vector is still +0.0, so
 *      such a pixel is a plain cross-fade.
 *   B, blend.  The output pixel (x, y) with the filled vector (a, b), wA = fl(1.0f - t), wB = t:
 *   1. tA = the warp's taps of (a, b) at the fraction -t, tB = at the fraction wA, both with HSFLOW_WARP_BORDER_REPLICATE;
 *      inA / inB: the warp's class is inside;
 *   2. per channel fa = the bilinear value of prev at tA in the warp's order but UNROUNDED -- top = fl(p00 + fl(ax * fl(p10
 *      - p00))), bot alike, fa = fl(top + fl(ay * fl(bot - top))) -- and fb alike from curr at tB: one rounding per
 *      output byte (with the taps rounded to bytes first, the rounding noise alone makes low-contrast frames worse than
 *      a cross-fade);
 *   3. the nearest tap of a side is (ax >= 0.5f ? x1 : x0, ay >= 0.5f ? y1 : y0);
 *   4. class.  inA && inB: occA iff vis_prev is given and its byte at tA's nearest tap is 0, occB alike with vis_curr at
 *      tB; occA && !occB: HSFLOW_INTERP_PREV_ONLY; occB && !occA: HSFLOW_INTERP_CURR_ONLY; else HSFLOW_INTERP_BLENDED.
 *      Only inA: PREV_ONLY.  Only inB: CURR_ONLY.  Neither: HSFLOW_INTERP_CLAMPED, the blend of the two clamped samples;
 *   5. BLENDED / CLAMPED: m = fl(fl(wA * fa) + fl(wB * fb)); PREV_ONLY: m = fa; CURR_ONLY: m = fb;
 *      byte = min((int)fl(m + 0.5f), 255).
 * Without vis planes t = 0 gives prev and t = 1 gives curr byte for byte, whatever the flow; a constant whole-number flow
 * (dx, dy) with t dx and t dy whole gives in the interior the exact mix of the two shifted pictures.  There is no fill
 * colour and no border option: every pixel gets a plausible value.  Against the same formula of step B in float64 every
 * byte is within one level (tests/test_interp_host.py).
 * hsflow_interp_stats: blended + prev_only + curr_only + clamped = W*H; sad is the sum of |byte - ref| over all pixels
 * and channels against an optional reference picture (the interpolation error of the Middlebury benchmark), max_diff the
 * largest single difference, both 0 without one; hit cells + holes = W*H; landed + left + unknown = W*H.  The entries
 * that stop after F leave the first five and max_diff 0. */
#define HSFLOW_INTERP_BLENDED 0
#define HSFLOW_INTERP_PREV_ONLY 1
#define HSFLOW_INTERP_CURR_ONLY 2
#define HSFLOW_INTERP_CLAMPED 3
#define HSFLOW_INTERP_BATCH_MAX 8 /* times per set of launches; HSFLOW_INTERP_BATCH_MAX=<1..8> in the environment: fewer */
typedef struct hsflow_interp_params {
    uint32_t struct_size;   /* = sizeof(hsflow_interp_params)                 */
    int32_t channels;       /* 1 or 3, interleaved                            */
    int32_t fill_radius;    /* 1 or 2                                         */
    int32_t fill_min_votes; /* 1 .. (2 fill_radius + 1)^2                     */
    int32_t fill_passes;    /* 0 .. HSFLOW_MEDIAN_MAX_PASSES                  */
} hsflow_interp_params;
typedef struct hsflow_interp_stats { /* 64 bytes, the same on the device and on the host */
    uint64_t blended, prev_only, curr_only, clamped;
    uint64_t sad;
    uint32_t holes, unfilled, collisions, left, unknown, max_diff;
} hsflow_interp_stats;
/* channels 1, fill_radius 1, fill_min_votes 1, fill_passes 4.  NULL is ignored. */
void hsflow_default_interp_params(hsflow_interp_params *ip);
/* Steps P and F on the host, no device needed: the flow at time t as two fp32 planes (together or not at all, rows
 * out_stride bytes apart), the state plane (0 unfilled, 1 hit, 2 filled) and the record, at least one of them.  With
 * t = 1 this is the flow on B's grid -- what a camera loop hands to the next pair (hsflow_set_flow_device and
 * use_previous).  Writes 4*width bytes of every output flow row, width bytes of every state row and nothing else.
 * HSFLOW_E_ARG: a null input, params, t outside [0, 1] or not finite, nothing asked for; HSFLOW_E_SIZE: a stride. */
int hsflow_project_flow_host(const float *u, size_t u_stride, const float *v, size_t v_stride, int width, int height, float t,
                             const hsflow_interp_params *ip, const uint8_t *prev, size_t prev_stride, const uint8_t *curr, size_t curr_stride,
                             float *u_out /* may be null */, float *v_out /* may be null */, size_t out_stride, uint8_t *state_out /* may be null */,
                             size_t state_out_stride, hsflow_interp_stats *stats /* may be null */);
/* The whole rule on the host, no device needed.  vis_prev, vis_curr, ref, dst, cls and stats may each be null, but one of
 * dst, cls (the class plane, one byte HSFLOW_INTERP_* per pixel) and stats must be asked for.  Writes channels*width
 * bytes of every row of dst, width bytes of every row of cls and nothing else.  HSFLOW_E_ARG / HSFLOW_E_SIZE as
 * hsflow_interp_batch_device. */
int hsflow_interp_host(const float *u, size_t u_stride, const float *v, size_t v_stride, int width, int height, float t,
                       const hsflow_interp_params *ip, const uint8_t *prev, size_t prev_stride, const uint8_t *curr, size_t curr_stride,
                       const uint8_t *vis_prev, size_t vis_prev_stride, const uint8_t *vis_curr, size_t vis_curr_stride, const uint8_t *ref,
                       size_t ref_stride, uint8_t *dst, size_t dst_stride, uint8_t *cls, size_t cls_stride, hsflow_interp_stats *stats);
/* n intermediate frames of ONE pair (slow motion) at the times t[0 .. n) (host memory, read during the call) from the
 * pair's flow where it lies: per chunk of at most HSFLOW_INTERP_BATCH_MAX times one memset of the key planes, the splat
 * (one 64-bit atomicMin per landed source), the resolve, fill_passes launches of the median kernel in FILL mode and the
 * blend; the time is the launches' batch axis.  Picture i, class plane i and record i are those of hsflow_interp_host
 * with t[i], whatever n and the chunking.  Everything is device memory on the context's device, any alignment (word
 * stores where base and stride are multiples of 4); d_stats: n records, 8-byte aligned.  d_prev == NULL: the context's
 * own pre-processed frames of the pair (d_curr must be NULL too, channels 1).  d_ref[i]: the true frame at t[i], for
 * sad / max_diff.  Only enqueued on the context's stream; the ordering rules of hsflow_warp_batch_device apply word for
 * word (an owed ITER|EPS check is settled first; hsflow_wait_solve afterwards waits for this work too).  The flow is not
 * changed.  Scratch: 26 bytes per pixel of pitch x height and time of the chunk (keys, two pairs of fp32 planes and two
 * state planes for the fill's ping-pong), allocated by the first call for min(n, chunk) times, grown on demand and kept
 * until hsflow_destroy: contexts that never interpolate pay nothing.  A call that has to allocate or grow the scratch
 * (the first one, and the first with more times per chunk than any before) is not "only enqueued": freeing the old
 * block waits until the whole device is idle, earlier chunks of this context and other streams' work included.  Call
 * once with the largest n (up to the chunk size) ahead of a latency-critical loop.  Every argument is checked before anything is
 * enqueued.  HSFLOW_E_ARG: null params or list entry, struct_size, channels, a t outside [0, 1] or not finite, fill
 * parameters out of range, neither pictures nor class planes nor records asked for, misaligned records, a destination
 * equal to an input, d_curr without d_prev or the reverse, the chunk size in the environment; HSFLOW_E_SIZE: a stride
 * below the row's bytes.
 * Time on an MI355X (profiles/interp_time.txt), BGR pictures of a 1080p pair: one time 0.183 ms, with
 * reference and statistics 0.228 ms, eight times in one call 1.25 ms (0.156 each); 600x480: 0.058 ms, eight 0.198 ms.
 * That is 19 x a device-to-device copy of the bytes moved and 7 x two hsflow_warp_device calls, and 1400 x faster than
 * the host route (hsflow_get_flow + hsflow_interp_host, 263 ms).  Kernel by kernel at 1080p, one time, from a kernel
 * trace: the key planes' memset 0.009, splat 0.047 (1 channel: 0.044), resolve 0.032 (with statistics 0.035), each of
 * the four fill passes 0.0195, blend 0.023 (with reference and statistics 0.048) ms; eight times: 0.368, 0.264, 0.112 per
 * pass and 0.146 ms; 600x480: 0.0081, 0.0055, 0.0087 per pass and 0.0073 ms.  The splat is bound by its 64-bit minima:
 * the same gather without them (hsflow_warp's kernel) takes 0.013 ms, the 2.07 M atomics about 0.033 ms (45 G per
 * second), and a launch of eight times takes eight times as long. */
int hsflow_interp_batch_device(hsflow_ctx *ctx, int pair, int n, const float *t, const hsflow_interp_params *ip, const void *d_prev,
                               size_t prev_stride, const void *d_curr, size_t curr_stride, const void *d_vis_prev /* or NULL */,
                               size_t vis_prev_stride, const void *d_vis_curr /* or NULL */, size_t vis_curr_stride,
                               const void *const *d_ref /* n, or NULL */, size_t ref_stride, void *const *d_dst /* n, or NULL */, size_t dst_stride,
                               void *const *d_cls /* n, or NULL */, size_t cls_stride, hsflow_interp_stats *d_stats /* n on the device, or NULL */);
/* A batch of one. */
int hsflow_interp_device(hsflow_ctx *ctx, int pair, float t, const hsflow_interp_params *ip, const void *d_prev, size_t prev_stride,
                         const void *d_curr, size_t curr_stride, const void *d_vis_prev, size_t vis_prev_stride, const void *d_vis_curr,
                         size_t vis_curr_stride, const void *d_ref, size_t ref_stride, void *d_dst, size_t dst_stride, void *d_cls, size_t cls_stride,
                         hsflow_interp_stats *d_stats);
/* One time with everything in host memory, synchronous: complete on return.  prev == NULL: the context's own frames.
 * Waits only for an event behind its own work, like hsflow_warp -- except in a call that has to allocate its staging. */
int hsflow_interp(hsflow_ctx *ctx, int pair, float t, const hsflow_interp_params *ip, const uint8_t *prev, size_t prev_stride, const uint8_t *curr,
                  size_t curr_stride, const uint8_t *vis_prev, size_t vis_prev_stride, const uint8_t *vis_curr, size_t vis_curr_stride,
                  const uint8_t *ref, size_t ref_stride, uint8_t *dst, size_t dst_stride, uint8_t *cls, size_t cls_stride, hsflow_interp_stats *stats);
/* Steps P and F of the pair's flow on the device: what hsflow_project_flow_host gives from that flow, into device memory
 * (fp32 planes 4-byte aligned, out_stride a multiple of 4).  Only enqueued, like hsflow_interp_device; the outputs may
 * not be the pair's own planes.  d_prev == NULL: the context's own frames. */
int hsflow_project_flow_device(hsflow_ctx *ctx, int pair, float t, const hsflow_interp_params *ip, const void *d_prev, size_t prev_stride,
                               const void *d_curr, size_t curr_stride, void *d_u_out /* or NULL */, void *d_v_out /* or NULL */, size_t out_stride,
                               void *d_state_out /* or NULL */, size_t state_out_stride, hsflow_interp_stats *d_stats /* or NULL */);

/* --- pixels and points followed through a sequence of flows (ABI 0.22) -------------------------- */

/* A context holds a whole sequence (hsflow_set_sequence_*: N + 1 frames in N pairs), and every operator above works on
 * one pair.  These entries say where a pixel of frame 0 is in frame n: long-range correspondence, accumulated camera
 * motion, point tracks.  Composition is not the sum of the planes -- the vector of pair k is read where the pixel has
 * ARRIVED in frame k (on a field that rotates by 0.02 rad per pair, 96x64, eight pairs, 8 x flow is off by up to 0.60 px,
 * the chain by 1.1e-6 px).  Done where the flows lie, in ONE launch with the trajectory in registers, without a read-back
 * of 2 n fp32 planes.  No counterpart in the reference.  The rule is csrc/hs_chain_rule.h, one header for the kernels and
 * the host forms; device and host give the same bits.  All arithmetic is fp32, every operation rounded on its own (fl).
 *   Flow planes (u_k, v_k), k = 0 .. n-1, all W x H, n = 1 .. HSFLOW_CHAIN_MAX_PAIRS.  Optional state planes s_k (u8,
 *   non-zero = trusted: the default mask of hsflow_fb as it is; a NULL list or a NULL entry: no test for that plane).
 *   One step, advance(a, b, x, y, k), where (a, b) is what was accumulated and (x, y) where it started:
 *   1. UNKNOWN (3) iff the colour picture's test says so of (a, b) (NaN, or a magnitude above 1e9);
 *   2. fx = fl((float)x + a), fy = fl((float)y + b); LEFT (1) iff !(fx >= 0 && fx <= W-1 && fy >= 0 && fy <= H-1);
 *   3. x0 = (int)floorf(fx), x1 = min(x0 + 1, W-1), ax = fl(fx - (float)x0); y0, y1, ay alike (the warp's taps with t = 1).
 *      UNKNOWN iff any of the four taps of (u_k, v_k) is not known, even where its weight is 0;
 *   4. UNTRUSTED (2) iff plane k has a state plane and any of its four taps is zero;
 *   5. c = the bilinear sample of u_k in the warp's order (hsflow_fb, step 4), d of v_k; a' = fl(a + c), b' = fl(b + d);
 *      UNKNOWN iff (a', b') is not known, else ALIVE (0) with (a', b').
 *   Dense chain, pixel (x, y): WITHOUT start planes the start is (u_0, v_0)[y][x] verbatim -- no sampling, no addition, so
 *   n = 1 is a copy, -0.0 included -- UNKNOWN if not known, else UNTRUSTED if s_0[y][x] == 0, and the pixel advances through
 *   planes 1 .. n-1.  WITH start planes (U0, V0) the start is (U0, V0)[y][x], UNKNOWN if not known, no state is tested at
 *   the start, and the pixel advances through all of 0 .. n-1.  The first class other than ALIVE is final; the walk ends.
 *   Outputs, each may be absent, but at least one must be asked for; U and V together or not at all:
 *     U, V    fp32 planes: the accumulated flow from frame 0 to frame n; the quiet NaN 0x7fc00000 in both where the pixel
 *             is not ALIVE.  The last plane's vector may point outside the frame: only "known" is asked of the result, so
 *             an ALIVE pixel is known to the colour picture;
 *     status  a u8 plane, value[class]; with the default {255, 0, 0, 0} it is a state plane for hsflow_median* and
 *             hsflow_interp* as it is;
 *     age     a u8 plane: the number of planes of this call the pixel passed (n iff ALIVE; the verbatim start is plane 0);
 *     stats   exact integers that do not depend on the order of execution: cls[4], the class counts (they sum to W*H);
 *             sum_age; max_mag2_bits, the bit pattern of the largest fl(fl(U*U) + fl(V*V)) over ALIVE, 0 if there are none.
 *   A longer chain continues from the U, V of the call before through the start planes: 32 + k planes in two calls are,
 *   bit for bit, what one walk through all of them gives at every pixel that is ALIVE after the first call.  Pixels lost
 *   in the first call carry the NaN and come back UNKNOWN from the second, whatever their class was.
 *   Points: a point is a position (px, py) in frame 0, two floats.  UNKNOWN if not known; else it advances through ALL n
 *   planes with advance(px, py, 0, 0, k), so what accumulates is the position.  Row j of the track (m points of two floats)
 *   is the position after j planes for j <= age and the NaN bits beyond; row 0 is the start as given.  last: the position
 *   after n planes, the NaN bits unless ALIVE.  For points max_mag2_bits is the squared distance from the start,
 *   fl(fl(dx*dx) + fl(dy*dy)) with dx = fl(px_n - px_0), over ALIVE.  m = 1 .. 2^24.
 * Rows of U and V beyond width floats and of status and age beyond width bytes are left alone.
 * Not covered: the tickets of a pair pipeline, hsflow_multi_* and slabs.  A pipeline user takes the
 * hsflow_pipeline_flow_device pointers after hsflow_pipeline_wait and calls hsflow_chain_planes_device on a context of
 * their own.
 * Time on an MI355X (profiles/chain_time.txt): U and V through 8 pairs of 1080p flows in 0.105 ms (0.147 ms
 * with status and statistics) -- 0.62 x the seven mask-only hsflow_fb_planes_device launches that do the same gathers,
 * 27 x a device-to-device copy of two planes, 2200 x faster than reading the pairs back and chaining on the host (236 ms);
 * 32 pairs in 0.626 ms; 0.023 ms for 8 pairs at 600x480.  262 144 points with full tracks through 8 pairs in 0.026 ms. */
#define HSFLOW_CHAIN_MAX_PAIRS 32
#define HSFLOW_CHAIN_ALIVE 0
#define HSFLOW_CHAIN_LEFT 1
#define HSFLOW_CHAIN_UNTRUSTED 2
#define HSFLOW_CHAIN_UNKNOWN 3
typedef struct hsflow_chain_params {
    uint32_t struct_size; /* = sizeof(hsflow_chain_params)              */
    uint8_t value[4];     /* the status byte for class HSFLOW_CHAIN_*    */
    int32_t reserved[2];  /* 0                                           */
} hsflow_chain_params;
typedef struct hsflow_chain_stats { /* 64 bytes, the same on the device and on the host */
    uint64_t cls[4], sum_age;
    uint32_t max_mag2_bits;
    uint8_t reserved[20];
} hsflow_chain_stats;
/* value {255, 0, 0, 0}: a confidence mask.  NULL is ignored. */
void hsflow_default_chain_params(hsflow_chain_params *cp);
/* The rule on the host, no device needed: u, v: n planes each of width x height floats, rows flow_stride BYTES apart (one
 * stride for all); state: NULL or n entries, each NULL or a plane of rows state_stride bytes apart; U0, V0: the start
 * planes (rows start_stride bytes apart) or both NULL.  U, V, status, age and stats may each be null.
 * HSFLOW_E_ARG: null cp, wrong struct_size, n out of 1 .. 32, a null list or list entry of u or v, a flow plane that is not
 * 4-byte aligned, one start plane without the other, one of U and V without the other, nothing asked for, an output that
 * overlaps an input plane; HSFLOW_E_SIZE: a non-positive size, a float stride below 4*width or no multiple of 4, a byte
 * stride below width. */
int hsflow_chain_flow_host(int n, const float *const *u, const float *const *v, size_t flow_stride, const uint8_t *const *state /* may be null */,
                           size_t state_stride, int width, int height, const float *U0 /* may be null */, const float *V0, size_t start_stride,
                           const hsflow_chain_params *cp, float *U /* may be null */, float *V, size_t out_stride, uint8_t *status /* may be null */,
                           size_t status_stride, uint8_t *age /* may be null */, size_t age_stride, hsflow_chain_stats *stats /* may be null */);
/* Points by the rule on the host: xy[m][2] in; track[n + 1][m][2], last[m][2], status[m], age[m] and stats may each be
 * null, not all.  Errors as above, and HSFLOW_E_ARG: m out of 1 .. 2^24, null xy, a float array that is not 4-byte aligned. */
int hsflow_track_points_host(int n, const float *const *u, const float *const *v, size_t flow_stride, const uint8_t *const *state /* may be null */,
                             size_t state_stride, int width, int height, const hsflow_chain_params *cp, const float *xy, int m, float *track, float *last,
                             uint8_t *status, uint8_t *age, hsflow_chain_stats *stats);
/* The dense chain of n planes anywhere on ctx's device, of the context's width and height: d_u, d_v (and d_state) are
 * host arrays of n device pointers, free on return.  Only enqueued on ctx's stream: one launch, with statistics a memset
 * of the record in front of it.  The outputs are those of hsflow_chain_flow_host from the same planes.  The flow planes,
 * the start planes, d_U and d_V are 4-byte aligned and their strides multiples of 4 (16-byte alignment of base and stride
 * lets the kernel move 16 bytes at a time); status and age may have any alignment; d_stats a multiple of 8 (the counters
 * are 64-bit atomics).  The caller orders the producers of the planes before ctx's stream.
 * The ordering rules of hsflow_fb_batch_device apply word for word: an ITER|EPS check that hsflow_solve_async still owes
 * is settled first, and on a context with hsflow_set_async_reduce hsflow_wait_solve and hsflow_flow_view_device called
 * after it wait for the stream.  Nothing is allocated.  Every argument is checked before anything is enqueued.
 * HSFLOW_E_ARG and HSFLOW_E_SIZE as hsflow_chain_flow_host, and HSFLOW_E_ARG: d_stats no multiple of 8. */
int hsflow_chain_planes_device(hsflow_ctx *ctx, int n, const void *const *d_u, const void *const *d_v, size_t flow_stride,
                               const void *const *d_state /* n or NULL; a NULL entry: no test for that plane */, size_t state_stride,
                               const void *d_U0, const void *d_V0, size_t start_stride /* or NULL, NULL */, const hsflow_chain_params *cp, void *d_U,
                               void *d_V, size_t out_stride, void *d_status, size_t status_stride, void *d_age, size_t age_stride,
                               hsflow_chain_stats *d_stats);
/* The same through the context's own flows: plane k is the flow of pair pairs[k] (a host array of n, free on return; any
 * pair may appear any number of times).  The flow is read and never changed; after a solve with
 * hsflow_set_pair_termination every pair contributes its own final flow.  The outputs may not lie in the context's flow
 * planes.  HSFLOW_E_ARG also: null pairs, a pair out of range. */
int hsflow_chain_flow_device(hsflow_ctx *ctx, const int *pairs, int n, const void *const *d_state, size_t state_stride, const void *d_U0,
                             const void *d_V0, size_t start_stride, const hsflow_chain_params *cp, void *d_U, void *d_V, size_t out_stride,
                             void *d_status, size_t status_stride, void *d_age, size_t age_stride, hsflow_chain_stats *d_stats);
/* The same with state planes and start planes from host memory and the results in host memory, synchronous: complete on
 * return.  Waits only for an event behind its own work, like hsflow_fb -- except in a call that has to allocate: the
 * staging is allocated by the first call that needs a piece, grown to the largest so far and kept until hsflow_destroy
 * (hsflow_release_cached for the one-shot's context).  Contexts that never chain pay nothing. */
int hsflow_chain_flow(hsflow_ctx *ctx, const int *pairs, int n, const uint8_t *const *state, size_t state_stride, const float *U0, const float *V0,
                      size_t start_stride, const hsflow_chain_params *cp, float *U, float *V, size_t out_stride, uint8_t *status, size_t status_stride,
                      uint8_t *age, size_t age_stride, hsflow_chain_stats *stats);
/* m points through the context's own flows, everything in device memory: d_xy[m][2] in; d_track[n + 1][m][2], d_last[m][2],
 * d_status[m], d_age[m], d_stats each may be NULL, not all.  One launch, one lane per point; the float arrays are 4-byte
 * aligned (8-byte alignment lets the kernel move a point at a time).  Ordering, allocation and errors as
 * hsflow_chain_flow_device, and HSFLOW_E_ARG: m out of 1 .. 2^24, null d_xy, a misaligned float array, an output that
 * overlaps the points, a state plane or the context's flow. */
int hsflow_track_points_device(hsflow_ctx *ctx, const int *pairs, int n, const void *const *d_state, size_t state_stride,
                               const hsflow_chain_params *cp, const float *d_xy, int m, float *d_track, float *d_last, uint8_t *d_status,
                               uint8_t *d_age, hsflow_chain_stats *d_stats);
/* The same from and to host memory, synchronous like hsflow_chain_flow. */
int hsflow_track_points(hsflow_ctx *ctx, const int *pairs, int n, const uint8_t *const *state, size_t state_stride, const hsflow_chain_params *cp,
                        const float *xy, int m, float *track, float *last, uint8_t *status, uint8_t *age, hsflow_chain_stats *stats);

/* --- camera motion from the flow (0.23) ------------------------------------------------------ */

/* The single global motion that explains a flow field -- the camera's -- fitted where the flow lies, by a trimmed least
 * squares; with it a mask of the pixels that follow it (or of those that do not: the moving foreground), the flow
 * relative to the camera, and a picture warped by the model alone (stabilisation).  No counterpart in the reference.  The
 * rule is csrc/hs_gmotion_rule.h, one header for the kernels and the host forms; device and host give the same bits.
 *   Model.  p[6], fp32; with X = x - (W-1)/2, Y = y - (H-1)/2:
 *     mu = fl(fl(p0 + fl(p1 * X)) + fl(p2 * Y)),  mv = fl(fl(p3 + fl(p4 * X)) + fl(p5 * Y))
 *   TRANSLATION: p1 = p2 = p4 = p5 = 0; SIMILARITY: p1 = p5, p2 = -p4; AFFINE: all six.
 *   Classes of a pixel with flow (a, b), the first that applies:
 *     UNKNOWN (3)    the colour picture's test says so (NaN, a magnitude above 1e9), or |a| or |b| above 2048 px;
 *     UNTRUSTED (2)  a state plane is given and its byte is 0;
 *     OUTLIER (1) / INLIER (0) by r2 = fl(fl(ru * ru) + fl(rv * rv)) <= T, ru = fl(a - mu), rv = fl(b - mv); equality is an
 *                    inlier.
 *   Fit.  `passes` passes (1 .. 8): pass 0 takes every pixel that is neither UNKNOWN nor UNTRUSTED, pass j >= 1 the inliers
 *   under the model of pass j-1 and the threshold T_j.  Every pass sums exact integers (the flow quantised to 1/256 px,
 *   ties to even; doubled centred coordinates), so the order of accumulation cannot matter; from the twelve sums the
 *   model follows in double precision by one fixed sequence of + - * / and is rounded to fp32.
 *   Threshold.  FIXED: T_j = fl(inlier_px * inlier_px).  AUTO: T_j = max(min_thr2, fl(scale2 * E)), E the upper edge of the
 *   bin that holds the median of r2 under the model of pass j-1 in an exact histogram of four bins per octave over all
 *   pixels that are neither UNKNOWN nor UNTRUSTED; one more read of the flow per pass.
 *   Degenerate sets -- fewer than 3 (AFFINE) or 2 (SIMILARITY) pixels, all on one row, one column or one line -- fall back
 *   AFFINE -> SIMILARITY -> TRANSLATION -> the zero model (no pixel); the result's flags then carry
 *   HSFLOW_GMOTION_FLAG_FALLBACK, and HSFLOW_GMOTION_USED(flags) is the kind that was fitted by the last pass.
 *   Outputs under the model of the last pass and the threshold after it, each may be absent, at least one asked for:
 *     result  64 bytes: p[6], the threshold, flags, cls[4] (the class counts; they sum to W*H);
 *     mask    a u8 plane, value[class]; the default {255, 0, 0, 0} is a state plane for hsflow_median*, hsflow_interp* and
 *             hsflow_chain_* as it is, {0, 255, 0, 0} the moving foreground;
 *     res_u, res_v  fp32 planes fl(a - mu), fl(b - mv): the motion relative to the camera, ready for hsflow_color_flow*; the
 *             quiet NaN 0x7fc00000 in both where the pixel is UNKNOWN, and in place of any NaN.  Both or neither.
 *   Rows of the mask beyond width bytes and of the residual planes beyond width floats are left alone.
 *   Frames wider or higher than HSFLOW_GMOTION_MAX_SIDE are refused (HSFLOW_E_SIZE): up to there no sum can overflow.
 *   Warp by a model: dst(x, y) is src sampled by the rule of hsflow_warp with (a, b) = (mu, mv)(x, y) and the warp's t,
 *   border and fill; statistics as hsflow_warp_stats.  No flow plane is read.  channels 1 or 3, as hsflow_warp.
 *   Compose and invert work on positions: a model maps the centred position (X, Y) to (X + mu, Y + mv).
 * Time on an MI355X (profiles/gmotion_time.txt): one 1080p pair, AFFINE, FIXED, in 0.028 ms with one pass and
 * 0.060 ms with three (AUTO 0.054 / 0.144 ms); mask and residual planes add 0.002 ms; 8 pairs in one batch 0.130 ms for
 * three passes; 15 x a device-to-device copy of both planes, 392 x faster than reading the flow back and fitting on the
 * host (23.4 ms).  A 1080p BGR picture warped by a model in 0.0125 ms, 0.92 x hsflow_warp_device. */
#define HSFLOW_GMOTION_TRANSLATION 0
#define HSFLOW_GMOTION_SIMILARITY 1
#define HSFLOW_GMOTION_AFFINE 2
#define HSFLOW_GMOTION_ZERO 3 /* only as HSFLOW_GMOTION_USED: no pixel to fit */
#define HSFLOW_GMOTION_THRESHOLD_FIXED 0
#define HSFLOW_GMOTION_THRESHOLD_AUTO 1
#define HSFLOW_GMOTION_INLIER 0
#define HSFLOW_GMOTION_OUTLIER 1
#define HSFLOW_GMOTION_UNTRUSTED 2
#define HSFLOW_GMOTION_UNKNOWN 3
#define HSFLOW_GMOTION_MAX_PASSES 8
#define HSFLOW_GMOTION_MAX_SIDE 16384
#define HSFLOW_GMOTION_FLAG_FALLBACK 1u
#define HSFLOW_GMOTION_USED(flags) (((flags) >> 8) & 3u)
typedef struct hsflow_gmotion_params {
    uint32_t struct_size;   /* = sizeof(hsflow_gmotion_params)                      */
    int32_t model;          /* HSFLOW_GMOTION_TRANSLATION / _SIMILARITY / _AFFINE      */
    int32_t passes;         /* 1 .. HSFLOW_GMOTION_MAX_PASSES                          */
    int32_t threshold_mode; /* HSFLOW_GMOTION_THRESHOLD_FIXED / _AUTO                  */
    float inlier_px;        /* FIXED: finite, > 0, its square finite and > 0           */
    float scale2;           /* AUTO: in (0, 1e6]                                       */
    float min_thr2;         /* AUTO: finite, > 0                                       */
    uint8_t value[4];       /* the mask's byte for class HSFLOW_GMOTION_INLIER ...     */
    int32_t reserved[2];    /* 0                                                       */
} hsflow_gmotion_params;
typedef struct hsflow_gmotion_result { /* 64 bytes, the same on the device and on the host */
    float p[6];
    float threshold; /* the T the outputs were classified under */
    uint32_t flags;  /* HSFLOW_GMOTION_FLAG_FALLBACK | kind used << 8 */
    uint64_t cls[4];
} hsflow_gmotion_result;
/* AFFINE, 3 passes, FIXED with inlier_px 1, scale2 6, min_thr2 1/16, value {255, 0, 0, 0}.  NULL is ignored. */
void hsflow_default_gmotion_params(hsflow_gmotion_params *gp);
/* The rule on the host, no device needed: u, v of width x height floats, rows flow_stride BYTES apart; state NULL or a u8
 * plane.  mask, res_u / res_v and result may each be null, not all.
 * HSFLOW_E_ARG: null gp, wrong struct_size, unknown model or threshold mode, passes out of 1 .. 8, reserved not 0, a
 * threshold field of the chosen mode that is not finite or not positive, a null or not 4-byte aligned flow plane, one
 * residual plane without the other, nothing asked for, an output that overlaps an input;  HSFLOW_E_SIZE: a non-positive
 * size, a side above 16384, a float stride below 4*width or no multiple of 4, a byte stride below width. */
int hsflow_gmotion_fit_host(const float *u, const float *v, size_t flow_stride, const uint8_t *state /* may be null */, size_t state_stride, int width,
                            int height, const hsflow_gmotion_params *gp, uint8_t *mask /* may be null */, size_t mask_stride, float *res_u /* may be null */,
                            float *res_v, size_t res_stride, hsflow_gmotion_result *result /* may be null */);
/* Planes anywhere on ctx's device, of the context's width and height -- the U and V of hsflow_chain_planes_device, the
 * pointers of hsflow_pipeline_flow_device.  Only enqueued on ctx's stream: per pass one accumulation and one solve launch
 * (AUTO: a histogram and a second solve launch more), then one launch for the outputs; no memset in between.  The outputs
 * are those of hsflow_gmotion_fit_host from the same planes.  Flow and residual planes are 4-byte aligned, their strides
 * multiples of 4 (16-byte alignment of base and stride lets the kernels move 16 bytes at a time); byte planes may have any
 * alignment; d_result a multiple of 8 (the counts are 64-bit atomics).  The caller orders the producers of the planes
 * before ctx's stream.  The ordering rules of hsflow_fb_batch_device apply word for word.  The kernels' records (1152
 * bytes per field of the largest batch so far) are allocated by the first call and kept until hsflow_destroy.  Every
 * argument is checked before anything is enqueued.  Errors as the host form, and HSFLOW_E_ARG: d_result no multiple of 8. */
int hsflow_gmotion_fit_planes_device(hsflow_ctx *ctx, const void *d_u, const void *d_v, size_t flow_stride, const void *d_state, size_t state_stride,
                                     const hsflow_gmotion_params *gp, void *d_mask, size_t mask_stride, void *d_res_u, void *d_res_v, size_t res_stride,
                                     hsflow_gmotion_result *d_result);
/* The flows of the pairs first_pair .. first_pair + n - 1 of the context by ONE set of launches (32 pairs per set).  d_state,
 * d_mask, d_res_u, d_res_v: NULL, or host arrays of n device pointers, free on return, whose entries may be NULL (no
 * state test / no such output for that pair); d_results: NULL or n records.  The flow is read and never changed; no output
 * may lie in the context's flow planes.  HSFLOW_E_ARG also: n < 1, first_pair < 0, first_pair + n > n_pairs. */
int hsflow_gmotion_fit_batch_device(hsflow_ctx *ctx, int first_pair, int n, const void *const *d_state, size_t state_stride,
                                    const hsflow_gmotion_params *gp, void *const *d_mask, size_t mask_stride, void *const *d_res_u, void *const *d_res_v,
                                    size_t res_stride, hsflow_gmotion_result *d_results);
/* A batch of one. */
int hsflow_gmotion_fit_device(hsflow_ctx *ctx, int pair, const void *d_state, size_t state_stride, const hsflow_gmotion_params *gp, void *d_mask,
                              size_t mask_stride, void *d_res_u, void *d_res_v, size_t res_stride, hsflow_gmotion_result *d_result);
/* The same with the state plane from host memory and the outputs in host memory, synchronous: complete on return.  Waits
 * only for an event behind its own work, like hsflow_fb; the staging is allocated by the first call that needs a piece,
 * grown and kept until hsflow_destroy. */
int hsflow_gmotion_fit(hsflow_ctx *ctx, int pair, const uint8_t *state, size_t state_stride, const hsflow_gmotion_params *gp, uint8_t *mask,
                       size_t mask_stride, float *res_u, float *res_v, size_t res_stride, hsflow_gmotion_result *result);
/* A picture warped by the model (six floats in host memory) on the host: wp, src, ref, dst and stats as hsflow_warp_host.
 * HSFLOW_E_ARG: a null model or source, a parameter that is not finite, and as hsflow_warp_host; HSFLOW_E_SIZE: a
 * non-positive size, a side above 16384, a stride below channels*width. */
int hsflow_gmotion_warp_host(const float *model, int width, int height, const hsflow_warp_params *wp, const uint8_t *src, size_t src_stride,
                             const uint8_t *ref /* may be null */, size_t ref_stride, uint8_t *dst /* may be null */, size_t dst_stride,
                             hsflow_warp_stats *stats /* may be null */);
/* The same on pictures in device memory, of the context's size; only enqueued (one launch, with statistics a memset of the
 * record in front of it); d_stats a multiple of 8.  Ordering as hsflow_warp_device. */
int hsflow_gmotion_warp_device(hsflow_ctx *ctx, const float *model, const hsflow_warp_params *wp, const void *d_src, size_t src_stride, const void *d_ref,
                               size_t ref_stride, void *d_dst, size_t dst_stride, hsflow_warp_stats *d_stats);
/* The same from and to host memory, synchronous like hsflow_warp. */
int hsflow_gmotion_warp(hsflow_ctx *ctx, const float *model, const hsflow_warp_params *wp, const uint8_t *src, size_t src_stride, const uint8_t *ref,
                        size_t ref_stride, uint8_t *dst, size_t dst_stride, hsflow_warp_stats *stats);
/* out = "first m1, then m2" on positions; in double, rounded to fp32.  out may be m1 or m2.  HSFLOW_E_ARG: a null
 * pointer, a parameter that is not finite. */
int hsflow_gmotion_compose_host(const float *m1, const float *m2, float *out);
/* out = the inverse map of m.  HSFLOW_E_ARG also: the linear part I + [[p1, p2], [p4, p5]] is singular. */
int hsflow_gmotion_invert_host(const float *m, float *out);

/* --- moving objects from the flow: connected regions (0.24) ---------------------------------- */

/* What moves in the scene, as a list: the connected regions of a foreground mask -- hsflow_gmotion_fit's mask with value
 * {0, 255, 0, 0}, hsflow_fb's mask, a status plane of hsflow_chain_* -- labelled where mask and flow lie, each region with
 * its size, box, centroid sums and motion sums, so that a tracker, a region-of-interest encoder or an alarm reads a few
 * records instead of the mask and both flow planes.  No counterpart in the reference.  The rule is
 * csrc/hs_regions_rule.h, one header for the kernels and the host form; device and host give the same bits.
 *   Foreground.  A pixel whose mask byte lies in fg_lo .. fg_hi inclusive (defaults 1 .. 255); with no mask every pixel.
 *   Connectivity.  4 or 8.
 *   Join.  join_px == 0: two adjacent foreground pixels are always joined.  join_px > 0 (needs flow): only when both
 *   flows are known by hsflow_gmotion_fit's test (no NaN, no magnitude above 1e9, |a| and |b| at most 2048) and
 *     fl(fl(du * du) + fl(dv * dv)) <= fl(join_px * join_px),  du = fl(ua - ub), dv = fl(va - vb);
 *   equality joins; the test gives the same bits from either end.  A foreground pixel with unknown flow is then a region of
 *   its own.
 *   Regions.  The connected components of that graph; a region's root is the smallest y * W + x among its pixels.
 *   Numbering.  Regions of fewer than min_area (>= 1) pixels are dropped: label 0, as background, and no number.  The kept
 *   ones are numbered 1, 2, ... in ascending order of their roots.
 *   Outputs, each may be absent, at least one asked for:
 *     labels   an int32 plane, stride a multiple of 4; bytes of a row beyond 4 * width are left alone;
 *     records  `capacity` records of 64 bytes; record k-1 belongs to region k for k <= capacity, records from
 *              min(n_regions, capacity) on are left alone; regions above the capacity are still numbered in labels.
 *              sum_x / area, sum_y / area is the centroid; n_flow counts the region's pixels whose flow is known (0 with
 *              no flow planes), sum_qu, sum_qv are their flow quantised as the fit does, rint(fl(a * 256)) with ties to
 *              even, so the mean motion is sum / (256 * n_flow);
 *     result   64 bytes: n_regions, n_written = min(n_regions, capacity), n_dropped (regions below min_area), flags
 *              (HSFLOW_REGIONS_FLAG_OVERFLOW: n_regions > capacity), fg_px, dropped_px, unknown_flow_px (foreground
 *              pixels whose flow is unknown; 0 with no flow planes), largest_area and largest_label (a tie goes to the
 *              smaller label; 0, 0 with no region).  capacity counts whether or not a record array is given.
 *   Every sum is an exact integer, so the order of accumulation cannot matter.  Frames wider or higher than
 *   HSFLOW_REGIONS_MAX_SIDE are refused (HSFLOW_E_SIZE): up to there no sum can overflow (the rule header has the proof).
 * Time on an MI355X (profiles/regions_time.txt), one 1080p pair, labels, 64 records and the header: the
 * fit's foreground mask of the benchmark's pair (8767 regions) in 0.241 ms, 8 pairs in one batch 0.885 ms; a random mask at
 * the percolation threshold (60210 regions) 1.39 ms; the full mask (ONE region) 4.12 ms, of which 3.4 ms are the records'
 * atomics, every wavefront on one record; 34 x a device-to-device copy of mask and label plane; reading mask and flow back
 * and labelling on the host takes 9.2 ms, 31.6 ms and 49.5 ms for the three masks, 38 x, 23 x and 12 x the device's time. */
#define HSFLOW_REGIONS_MAX_SIDE 16384
#define HSFLOW_REGIONS_FLAG_OVERFLOW 1u
typedef struct hsflow_regions_params {
    uint32_t struct_size; /* = sizeof(hsflow_regions_params)      */
    int32_t connectivity; /* 4 or 8                               */
    int32_t fg_lo, fg_hi; /* 0 <= fg_lo <= fg_hi <= 255           */
    uint32_t min_area;    /* >= 1                                 */
    float join_px;        /* finite, >= 0, its square finite      */
    int32_t reserved[2];  /* 0                                    */
} hsflow_regions_params;
typedef struct hsflow_regions_record { /* 64 bytes, the same on the device and on the host */
    uint32_t root, area;     /* the smallest y * W + x of the region; its pixels */
    uint16_t x0, y0, x1, y1; /* the box, inclusive */
    uint64_t sum_x, sum_y;
    uint32_t n_flow, reserved0;
    int64_t sum_qu, sum_qv;
    uint64_t reserved1;
} hsflow_regions_record;
typedef struct hsflow_regions_result { /* 64 bytes, the same on the device and on the host */
    uint32_t n_regions, n_written, n_dropped, flags;
    uint64_t fg_px, dropped_px, unknown_flow_px;
    uint32_t largest_area, largest_label;
    uint64_t reserved[2];
} hsflow_regions_result;
/* connectivity 8, foreground 1 .. 255, min_area 1, join_px 0.  NULL is ignored. */
void hsflow_default_regions_params(hsflow_regions_params *rp);
/* The rule on the host, no device needed: mask NULL or a u8 plane of width x height, rows mask_stride bytes apart; u, v
 * both NULL or fp32 planes, rows flow_stride BYTES apart.  labels, records and result may each be null, not all.
 * HSFLOW_E_ARG: null rp, wrong struct_size, reserved not 0, connectivity neither 4 nor 8, fg_lo > fg_hi or outside
 * 0 .. 255, min_area 0, join_px negative, not finite or with a square that is not finite or is 0 while join_px is not,
 * join_px > 0 without flow planes, one flow plane without the other, a flow or label plane that is not 4-byte aligned,
 * records or result not 8-byte aligned, nothing asked for, an output that overlaps an input or another output;
 * HSFLOW_E_SIZE: a non-positive size, a side above 16384, a mask stride below width, a flow or labels stride below
 * 4*width or no multiple of 4, a capacity above 2^30. */
int hsflow_regions_host(const uint8_t *mask /* may be null */, size_t mask_stride, const float *u /* may be null */, const float *v, size_t flow_stride,
                        int width, int height, const hsflow_regions_params *rp, int32_t *labels /* may be null */, size_t labels_stride,
                        hsflow_regions_record *records /* may be null */, uint32_t capacity, hsflow_regions_result *result /* may be null */);
/* Planes anywhere on ctx's device, of the context's width and height.  Only enqueued on ctx's stream: a fixed sequence of
 * eight launches (seven for a frame that is one tile of 64 x 16) that does not depend on the data, no memset, no wait on
 * the host and none between workgroups.  The outputs are those of hsflow_regions_host from the same planes.  d_records and
 * d_result are multiples of 8 (64-bit atomics).  The caller orders the producers of the planes before ctx's stream.  The
 * ordering rules of hsflow_fb_batch_device apply word for word.  The scratch -- per field of the largest set of launches
 * so far two planes of 4 * width * height bytes and 4 bytes per 256 pixels of a row -- is allocated by the first call,
 * grown and kept until hsflow_destroy.  Every argument is checked before anything is enqueued.  Errors as the host form. */
int hsflow_regions_planes_device(hsflow_ctx *ctx, const void *d_mask, size_t mask_stride, const void *d_u, const void *d_v, size_t flow_stride,
                                 const hsflow_regions_params *rp, void *d_labels, size_t labels_stride, hsflow_regions_record *d_records, uint32_t capacity,
                                 hsflow_regions_result *d_result);
/* The pairs first_pair .. first_pair + n - 1 of the context, each with the context's own flow of that pair, by ONE set of
 * launches (8 pairs per set).  d_mask, d_labels, d_records: NULL, or host arrays of n device pointers, free on return,
 * whose entries may be NULL (every pixel foreground / no such output for that pair); every record array has `capacity`
 * records; d_results: NULL or n headers.  The flow is read and never changed; no output may lie in the context's flow
 * planes.  HSFLOW_E_ARG also: n < 1, first_pair < 0, first_pair + n > n_pairs. */
int hsflow_regions_batch_device(hsflow_ctx *ctx, int first_pair, int n, const void *const *d_mask, size_t mask_stride, const hsflow_regions_params *rp,
                                void *const *d_labels, size_t labels_stride, void *const *d_records, uint32_t capacity, hsflow_regions_result *d_results);
/* A batch of one. */
int hsflow_regions_device(hsflow_ctx *ctx, int pair, const void *d_mask, size_t mask_stride, const hsflow_regions_params *rp, void *d_labels,
                          size_t labels_stride, hsflow_regions_record *d_records, uint32_t capacity, hsflow_regions_result *d_result);
/* The same with the mask from host memory and the outputs in host memory, synchronous: complete on return.  Waits only for
 * events behind its own work, like hsflow_gmotion_fit; only the n_written records cross.  The staging is allocated by the
 * first call that needs a piece, grown and kept until hsflow_destroy. */
int hsflow_regions(hsflow_ctx *ctx, int pair, const uint8_t *mask, size_t mask_stride, const hsflow_regions_params *rp, int32_t *labels, size_t labels_stride,
                   hsflow_regions_record *records, uint32_t capacity, hsflow_regions_result *result);

/* --- moving objects through a sequence: regions linked across pairs (0.25) ------------------- */

/* Which region of frame k + 1 is which region of frame k: every labelled pixel of frame k is followed along the flow of the
 * pair k -> k + 1 and counted where it arrives, so that a tracker reads a few hundred bytes per pair instead of two label
 * planes and a flow field.  No counterpart in the reference.  The rule is csrc/hs_link_rule.h, one header for the kernels
 * and the host form; device and host give the same bytes.
 *   Inputs of a step.  Two int32 label planes A (frame k) and B (frame k + 1) of width x height -- hsflow_regions*'s or any
 *   other; a value <= 0 is background -- the flow (u, v) of the pair, and two caps cap_a, cap_b >= 1 with
 *   cap_a * cap_b <= HSFLOW_LINK_MAX_CELLS.
 *   Pixel (x, y) with a = A[y][x] > 0:
 *     a > cap_a: it counts into the header's over_a_px and does nothing else;
 *     it lands where hsflow_interp's projection at t = 1 puts it: hx = fl(fl((float)x + u) + 0.5f), hy alike, the pixel
 *     (floor hx, floor hy) -- the same function, so the half-pixel tie is the interpolation operator's, bit for bit;
 *     a flow that is not known (NaN, a magnitude above 1e9) or a landing outside the frame: it counts into gone_px of a;
 *     b = B at the landing pixel; b <= 0 or b > cap_b: it counts into unmatched_px of a; else it is ONE VOTE for (a, b).
 *   Outputs, each may be absent, at least one asked for:
 *     links    link_capacity records of 16 bytes, one per cell (a, b) with px > 0 votes, in ascending order of (a, b);
 *              records from min(n_links, link_capacity) on are left alone;
 *     side_a   cap_a records of 32 bytes, all written; record a-1: px, the pixels of label a (= gone_px + unmatched_px + the
 *              votes of row a); n_links, the non-zero cells of the row; best, the b of the largest cell (a tie goes to the
 *              smaller b; 0 with no vote) and best_px, its votes; gone_px, unmatched_px;
 *     side_b   cap_b records of the same struct over the columns: px the arrivals, best the a that sends most (a tie to the
 *              smaller a), gone_px = unmatched_px = 0;
 *     result   64 bytes: n_links, n_written = min(n_links, link_capacity), flags (HSFLOW_LINK_FLAG_OVERFLOW:
 *              n_links > link_capacity), n_mutual (the pairs with best(a) == b and best(b) == a), and the totals voted_px,
 *              gone_px, unmatched_px, over_a_px.  link_capacity counts whether or not a link array is given.  A link array with
 *              link_capacity 0 is no output: alone it is "nothing asked for".
 *   Every quantity is an exact integer count, so the order of arrival cannot matter.
 * Time on an MI355X (profiles/link_time.txt), one 1080p step with 256 links, both sides and the header:
 * both planes ONE region, every pixel voting, 0.051 ms at caps 64; the label planes of the benchmark pair's fit mask 0.042
 * ms at caps 64 and 0.057 ms at caps 256 (of its 8767 regions only those within the caps vote; the rest returns after the
 * label), 8 such steps in one batch 0.086 ms; random labels at caps 4096 x 4096 0.57 ms; 5 x a device-to-device copy of
 * two label planes.  Reading the planes and the flow back and linking on the host takes 9 .. 15 ms, 21 .. 30 ms and 95 ..
 * 120 ms for the three: two to three orders of magnitude more. */
#define HSFLOW_LINK_MAX_CELLS (1u << 24)
#define HSFLOW_LINK_FLAG_OVERFLOW 1u
typedef struct hsflow_link_params {
    uint32_t struct_size; /* = sizeof(hsflow_link_params)                              */
    uint32_t cap_a;       /* >= 1: labels of A above it count into over_a_px           */
    uint32_t cap_b;       /* >= 1: labels of B above it are unmatched; cap_a * cap_b <= HSFLOW_LINK_MAX_CELLS */
    uint32_t reserved;    /* 0                                                         */
} hsflow_link_params;
typedef struct hsflow_link_record { /* 16 bytes, the same on the device and on the host */
    uint32_t a, b, px, reserved;
} hsflow_link_record;
typedef struct hsflow_link_side { /* 32 bytes, the same on the device and on the host */
    uint32_t px, n_links, best, best_px, gone_px, unmatched_px, reserved[2];
} hsflow_link_side;
typedef struct hsflow_link_result { /* 64 bytes, the same on the device and on the host */
    uint32_t n_links, n_written, flags, n_mutual;
    uint64_t voted_px, gone_px, unmatched_px, over_a_px;
    uint64_t reserved[2];
} hsflow_link_result;
/* cap_a 64, cap_b 64.  NULL is ignored. */
void hsflow_default_link_params(hsflow_link_params *lp);
/* The rule on the host, no device needed: labels_a, labels_b int32 planes of width x height, rows stride_a / stride_b BYTES
 * apart; u, v fp32 planes, rows flow_stride BYTES apart.  links, side_a, side_b and result may each be null, not all.
 * HSFLOW_E_ARG: null lp, wrong struct_size, reserved not 0, a cap of 0, a null label or flow plane, a label or flow plane
 * that is not 4-byte aligned, links, sides or result not 8-byte aligned, nothing asked for, an output that overlaps an
 * input or another output; HSFLOW_E_SIZE: a non-positive size, a side above 16384, a stride below 4*width or no multiple of
 * 4, a cap above 2^30, cap_a * cap_b or link_capacity above HSFLOW_LINK_MAX_CELLS. */
int hsflow_link_regions_host(const int32_t *labels_a, size_t stride_a, const int32_t *labels_b, size_t stride_b, const float *u, const float *v,
                             size_t flow_stride, int width, int height, const hsflow_link_params *lp, hsflow_link_record *links /* may be null */,
                             uint32_t link_capacity, hsflow_link_side *side_a /* may be null */, hsflow_link_side *side_b /* may be null */,
                             hsflow_link_result *result /* may be null */);
/* Planes anywhere on ctx's device, of the context's width and height.  Only enqueued on ctx's stream: a fixed sequence of
 * eight launches that does not depend on the data, no memset call, no wait on the host and none between workgroups.  The
 * outputs are those of hsflow_link_regions_host from the same planes.  The caller orders the producers of the planes before
 * ctx's stream.  The ordering rules of hsflow_fb_batch_device apply word for word.  The scratch -- per step of the largest
 * set of launches so far 4 * (cap_a * cap_b + 2 * cap_a + 1) bytes and a few words per cap -- is allocated by the first
 * call, grown and kept until hsflow_destroy.  Every argument is checked before anything is enqueued.  Errors as the host
 * form. */
int hsflow_link_regions_planes_device(hsflow_ctx *ctx, const void *d_labels_a, size_t stride_a, const void *d_labels_b, size_t stride_b, const void *d_u,
                                      const void *d_v, size_t flow_stride, const hsflow_link_params *lp, hsflow_link_record *d_links, uint32_t link_capacity,
                                      hsflow_link_side *d_side_a, hsflow_link_side *d_side_b, hsflow_link_result *d_result);
/* n_steps steps: step i links plane i to plane i + 1 of d_labels -- a host array of n_steps + 1 device pointers, free on
 * return, none NULL, rows labels_stride bytes apart -- by the context's own flow of the pair first_pair + i.  The steps of
 * a chunk run in ONE set of launches; a chunk is min(8, HSFLOW_LINK_MAX_CELLS / (cap_a * cap_b)) steps, at least 1, so the
 * cell scratch stays within 64 MiB.  The caps are arguments: no header of hsflow_regions_batch_device has to be read back in
 * between.  d_links, d_side_a, d_side_b: NULL, or host arrays of n_steps device pointers whose entries may be NULL; every
 * link array has link_capacity records; d_results: NULL or n_steps headers.  The flow is read and never changed; no output
 * may lie in the context's flow planes.  HSFLOW_E_ARG also: n_steps < 1, first_pair < 0, first_pair + n_steps > n_pairs. */
int hsflow_link_regions_batch_device(hsflow_ctx *ctx, int first_pair, int n_steps, const void *const *d_labels, size_t labels_stride,
                                     const hsflow_link_params *lp, void *const *d_links, uint32_t link_capacity, void *const *d_side_a, void *const *d_side_b,
                                     hsflow_link_result *d_results);
/* A batch of one step. */
int hsflow_link_regions_device(hsflow_ctx *ctx, int pair, const void *d_labels_a, const void *d_labels_b, size_t labels_stride, const hsflow_link_params *lp,
                               hsflow_link_record *d_links, uint32_t link_capacity, hsflow_link_side *d_side_a, hsflow_link_side *d_side_b,
                               hsflow_link_result *d_result);
/* The same with the label planes from host memory and the outputs in host memory, synchronous: complete on return.  Waits
 * only for events behind its own work, like hsflow_regions; only the n_written links cross.  The staging is allocated by
 * the first call that needs a piece, grown and kept until hsflow_destroy. */
int hsflow_link_regions(hsflow_ctx *ctx, int pair, const int32_t *labels_a, size_t stride_a, const int32_t *labels_b, size_t stride_b,
                        const hsflow_link_params *lp, hsflow_link_record *links, uint32_t link_capacity, hsflow_link_side *side_a, hsflow_link_side *side_b,
                        hsflow_link_result *result);
/* Object ids over a chain of steps from the side records alone, on the host.  side_a[i], side_b[i]: the `cap` records of
 * step i (frame i -> frame i + 1), i < n_steps; n_regions[k]: the regions of frame k, k <= n_steps; ids: (n_steps + 1) * cap
 * words, ids[k * cap + label - 1].  Frame 0's regions get the ids 1 .. min(n_regions[0], cap).  In step i region b of frame
 * i + 1, b ascending, continues the id of a = side_b[i][b-1].best iff a != 0, side_a[i][a-1].best == b and
 * (uint64)best_px * 256 >= (uint64)min_share_256 * px of that record; otherwise it gets the next fresh id.  Slots above
 * min(n_regions[k], cap) get 0.  *n_tracks (may be null): the ids handed out.  HSFLOW_E_ARG: a null array or entry,
 * n_steps < 0, cap 0, min_share_256 above 256; HSFLOW_E_SIZE: cap above 2^30. */
int hsflow_link_tracks_host(const hsflow_link_side *const *side_a, const hsflow_link_side *const *side_b, const uint32_t *n_regions, int n_steps, uint32_t cap,
                            uint32_t min_share_256, uint32_t *ids, uint32_t *n_tracks);

/* --- which points to follow: corner detection (0.26) ----------------------------------------- */

/* The corners of a u8 gray frame -- the points hsflow_track_points* is worth feeding -- found where the frames lie.  The rule
 * is csrc/hs_corners_rule.h, one header for the host form and the kernels; everything in it is an integer, so the device
 * and the host agree byte for byte whatever the order of execution.  OpenCV 2.1 has cvGoodFeaturesToTrack for this; its
 * floating point and its sequential greedy pass over a sorted list are deliberately not reproduced.  A pixel's index is
 * y * width + x.
 *   Gradients.  The 3 x 3 Sobel pair with coordinates clamped to the frame: Ix, Iy in -1020 .. 1020.
 *   Structure tensor.  A = sum Ix^2, B = sum Ix Iy, C = sum Iy^2 over the (2 block_r + 1)^2 window, block_r in 1 .. 3, the
 *   window's coordinates clamped to the frame as well.
 *   Score, an int64.  HSFLOW_CORNERS_MIN_EIGEN: S = (A + C) - ceil(sqrt((A - C)^2 + 4 B^2)), twice the smaller eigenvalue
 *   rounded down, the root an exact integer root; S >= 0.  HSFLOW_CORNERS_HARRIS: S = 25 (A C - B^2) - (A + C)^2, the
 *   Harris measure with k = 1 / 25 scaled by 25; |S| < 7e16.
 *   Allowed.  A pixel whose mask byte lies in fg_lo .. fg_hi (no mask: every pixel) and that lies at least `border` pixels
 *   from every frame edge.  A pixel that is not allowed is no corner and does not count towards the maximum; it still
 *   competes in the suppression, so a mask never creates corners.
 *   Threshold.  smax = max(0, max S over the allowed pixels); T = max(min_score, (smax >> 16) * quality_q16).
 *   Strong.  Allowed and S >= T.
 *   Survivors.  A strong pixel p that beats every other pixel q of the frame with max(|dx|, |dy|) <= nms_r (1 .. 8): p beats
 *   q iff S_p > S_q, or S_p == S_q and index_p < index_q.  No two survivors are closer than nms_r + 1 in either axis: the
 *   operator's minimum distance.
 *   Candidates.  The first max_candidates (1 .. HSFLOW_CORNERS_MAX_CANDIDATES) survivors in ascending index; more
 *   survivors set HSFLOW_CORNERS_FLAG_TRUNCATED (the remedy: a higher quality, a larger radius).
 *   Corners.  The candidates by descending S, ties by ascending index; the first `capacity` are the output.
 *   Outputs, each may be absent, at least one asked for:
 *     records  `capacity` records of 16 bytes, record k the corner of rank k; records from n_written on are left alone;
 *     xy       `capacity` pairs of floats, ((float)x, (float)y) for rank k < n_written, both floats of every later pair
 *              the quiet NaN 0x7fc00000: the array goes to hsflow_track_points_device with m = capacity as it is and the
 *              empty slots come back UNKNOWN.  All capacity pairs are written;
 *     result   64 bytes: n_survivors, n_candidates = min(n_survivors, max_candidates), n_written = min(n_candidates,
 *              capacity), flags (TRUNCATED; HSFLOW_CORNERS_FLAG_OVERFLOW: n_candidates > capacity), smax, threshold,
 *              allowed_px, strong_px.  capacity counts whether or not an array is given.
 *   Not covered: the tickets of a pair pipeline, hsflow_multi_* and slabs have no corners entry.
 * Time on an MI355X (profiles/corners_time.txt): see the summary there. */
#define HSFLOW_CORNERS_MIN_EIGEN 0
#define HSFLOW_CORNERS_HARRIS 1
#define HSFLOW_CORNERS_MAX_SIDE 16384
#define HSFLOW_CORNERS_MAX_CANDIDATES 65536u
#define HSFLOW_CORNERS_MAX_CAPACITY (1u << 24)
#define HSFLOW_CORNERS_FLAG_OVERFLOW 1u
#define HSFLOW_CORNERS_FLAG_TRUNCATED 2u
typedef struct hsflow_corners_params { /* 64 bytes */
    uint32_t struct_size;    /* = sizeof(hsflow_corners_params)            */
    int32_t kind;            /* HSFLOW_CORNERS_MIN_EIGEN or _HARRIS        */
    int32_t block_r;         /* 1 .. 3                                     */
    int32_t nms_r;           /* 1 .. 8                                     */
    uint32_t quality_q16;    /* 0 .. 65535, in 1 / 65536 of the maximum    */
    int32_t border;          /* >= 0                                       */
    int32_t fg_lo, fg_hi;    /* 0 <= fg_lo <= fg_hi <= 255                 */
    uint32_t max_candidates; /* 1 .. HSFLOW_CORNERS_MAX_CANDIDATES         */
    uint32_t reserved0;      /* 0                                          */
    int64_t min_score;       /* >= 1                                       */
    uint64_t reserved[2];    /* 0                                          */
} hsflow_corners_params;
typedef struct hsflow_corners_record { /* 16 bytes, the same on the device and on the host */
    uint16_t x, y;
    uint32_t index; /* y * width + x */
    int64_t score;
} hsflow_corners_record;
typedef struct hsflow_corners_result { /* 64 bytes, the same on the device and on the host */
    uint32_t n_survivors, n_candidates, n_written, flags;
    int64_t smax, threshold;
    uint64_t allowed_px, strong_px;
    uint64_t reserved[2];
} hsflow_corners_result;
/* MIN_EIGEN, block_r 1, nms_r 3, quality_q16 655 (about 1 %), border 0, mask bytes 1 .. 255, max_candidates 65536,
 * min_score 1.  NULL is ignored. */
void hsflow_default_corners_params(hsflow_corners_params *cp);
/* The rule on the host, no device needed: gray a u8 plane of width x height, rows stride bytes apart; mask NULL or such a
 * plane, rows mask_stride bytes apart.  records, xy and result may each be null, not all.
 * HSFLOW_E_ARG: null gray or cp, wrong struct_size, reserved not 0, an unknown kind, block_r outside 1 .. 3, nms_r outside
 * 1 .. 8, quality_q16 above 65535, border negative, fg_lo > fg_hi or outside 0 .. 255, max_candidates outside
 * 1 .. 65536, min_score below 1, records or result not 8-byte aligned, xy not 4-byte aligned, nothing asked for, an output
 * that overlaps an input or another output;
 * HSFLOW_E_SIZE: a non-positive size, a side above 16384, a gray or mask stride below width, a capacity above 2^24. */
int hsflow_corners_host(const uint8_t *gray, size_t stride, int width, int height, const uint8_t *mask /* may be null */, size_t mask_stride,
                        const hsflow_corners_params *cp, hsflow_corners_record *records /* may be null */, uint32_t capacity, float *xy /* may be null */,
                        hsflow_corners_result *result /* may be null */);
/* Planes anywhere on ctx's device, of the context's width and height.  Only enqueued on ctx's stream: one memset of 32 bytes
 * per field and a fixed sequence of six launches that does not depend on the data, no wait on the host and none between
 * workgroups, nothing read back.  The outputs are those of hsflow_corners_host from the same planes.  The caller orders the
 * producers of the planes before ctx's stream.  The ordering rules of hsflow_fb_batch_device apply word for word.  The
 * scratch -- per field of the largest set of launches so far a score plane of 8 * width * height bytes, 36 bytes per 256
 * pixels of a row and 1 MiB of candidates -- is allocated by the first call, grown and kept until hsflow_destroy; a context
 * that never asks for corners pays nothing.  Every argument is checked before anything is enqueued.  Errors as the host
 * form. */
int hsflow_corners_planes_device(hsflow_ctx *ctx, const void *d_gray, size_t stride, const void *d_mask, size_t mask_stride, const hsflow_corners_params *cp,
                                 hsflow_corners_record *d_records, uint32_t capacity, float *d_xy, hsflow_corners_result *d_result);
/* The pairs first_pair .. first_pair + n - 1 of the context, each with the context's own pre-processed gray plane of that
 * pair -- which 0: the prev frame, 1: the curr frame; what hsflow_get_frames_u8 hands out -- by ONE set of launches (8
 * pairs per set).  d_mask, d_records, d_xy: NULL, or host arrays of n device pointers, free on return, whose entries may be
 * NULL (every pixel passes / no such output for that pair); d_results: NULL or n headers.  The frames are read and never
 * changed; no output may lie in them.  HSFLOW_E_ARG also: n < 1, first_pair < 0, first_pair + n > n_pairs, which neither 0
 * nor 1; HSFLOW_E_STATE: no frames were set. */
int hsflow_corners_batch_device(hsflow_ctx *ctx, int first_pair, int n, int which, const void *const *d_mask, size_t mask_stride,
                                const hsflow_corners_params *cp, void *const *d_records, uint32_t capacity, void *const *d_xy, hsflow_corners_result *d_results);
/* A batch of one. */
int hsflow_corners_device(hsflow_ctx *ctx, int pair, int which, const void *d_mask, size_t mask_stride, const hsflow_corners_params *cp,
                          hsflow_corners_record *d_records, uint32_t capacity, float *d_xy, hsflow_corners_result *d_result);
/* The same with the mask from host memory and the outputs in host memory, synchronous: complete on return.  Waits only for
 * events behind its own work, like hsflow_regions; only the n_written records cross, and all capacity pairs of xy.  The
 * staging is allocated by the first call that needs a piece, grown and kept until hsflow_destroy. */
int hsflow_corners(hsflow_ctx *ctx, int pair, int which, const uint8_t *mask, size_t mask_stride, const hsflow_corners_params *cp,
                   hsflow_corners_record *records, uint32_t capacity, float *xy, hsflow_corners_result *result);

/* --- the input files (cvLoadImage)---------------------------------------------------------- */

/* The reference reads its two frames with cvLoadImage(path, 1) (OpticalFlowOpenCV.cpp:15,18, HSOpticalFlowOpenCL.cpp:721,
 * 732): libjpeg with its defaults -- baseline Huffman decoding, the "islow" inverse DCT, "fancy" triangle upsampling of
 * the chroma planes (plain replication for planes at most 2 samples wide), the 16-bit fixed-point YCbCr -> RGB
 * conversion -- into 3 bytes per pixel, B first.  The rule is csrc/hs_jpegd_rule.h, one header for the host form and the
 * kernels; its pixels are those of the drop-in CLI's reader (csrc/host/jpeg_baseline.hpp, held to libjpeg-turbo by
 * tests/test_jpeg.py) for every file both accept.
 * Accepted: SOF0 / SOF1 with 8-bit samples, 1 or 3 components, luma sampling 1x1, 2x1 or 2x2 with 1x1 chroma, one
 * interleaved scan, 8- and 16-bit quantisation tables, restart intervals.  Everything else is HSFLOW_E_DATA from the
 * header alone: progressive, lossless, arithmetic and 12-bit files, other sampling factors, a second frame header, a
 * missing table, an empty scan header, an entropy-coded segment of 256 MB or more.
 * Stricter than that reader in the entropy-coded data: a decode that consumes a bit at or beyond the segment's end is
 * an error (status word 2, "truncated"; the reader pads with zeros), and so is a code of no table, a DC category
 * above 11, a zero run past coefficient 63, or a de-quantised coefficient beyond +-1151 -- what an 8x8 block of 8-bit
 * samples can produce with an 8-bit quantiser, and what the 32-bit inverse DCT carries -- (status word 1, "corrupt").
 * The device form decodes a file without restart intervals by self-synchronising speculation: the unstuffed segment is
 * cut into subsequences of HSFLOW_JPEGD_SUBSEQ_BITS bits that are decoded at once from guessed states and repaired
 * until every one starts where its predecessor ended; with restart intervals every interval is decoded on its own.
 * The pixels depend on neither. */
#define HSFLOW_JPEGD_SUBSEQ_BITS 1024 /* a multiple of 32; the environment variable of the same name overrides it per call, 32..4096 */
#define HSFLOW_JPEG_ORDER_BGR 0 /* what cvLoadImage(..., 1) returns and HSFLOW_FRAMES_BGR8 takes */
#define HSFLOW_JPEG_ORDER_RGB 1
typedef struct hsflow_jpeg_info {
    uint32_t struct_size; /* sizeof(hsflow_jpeg_info), set by the caller */
    int32_t width, height, components; /* components: 1 or 3 */
    int32_t h_samp, v_samp;            /* luma sampling factors; chroma is 1x1 */
    int32_t restart_interval;          /* MCUs per restart interval, 0: none */
    int32_t subseq_bits;               /* bits per subsequence a device decode of this file runs with now; 0 with restart intervals */
    int64_t blocks;                    /* 8x8 blocks in the scan, MCU padding included */
    uint64_t scan_offset, scan_bytes;  /* the entropy-coded segment within the file, up to the marker that ends it */
} hsflow_jpeg_info;
/* The header alone, on the host.  HSFLOW_E_ARG: null pointer, struct_size; HSFLOW_E_DATA: see above. */
int hsflow_jpeg_read_header(const uint8_t *file, size_t bytes, hsflow_jpeg_info *info);
/* The rule on the host, no device needed: pix receives width x height pixels of 3 bytes, rows `stride` apart, in
 * `order`.  info may be null.  Writes exactly the picture's pixels, and none unless it returns HSFLOW_OK.
 * HSFLOW_E_ARG: null file or pix, unknown order, struct_size; HSFLOW_E_SIZE: stride < 3*width; HSFLOW_E_DATA: the header
 * or the entropy-coded data (hsflow_last_error(NULL) says which); HSFLOW_E_OOM. */
int hsflow_jpeg_decode_host(const uint8_t *file, size_t bytes, int order, uint8_t *pix, size_t stride, hsflow_jpeg_info *info);
/* A file in HOST memory -> its picture in device memory; only enqueued on ctx's stream (a copy of the entropy-coded
 * segment and the tables from page-locked staging of the library's own -- the caller's buffer is free on return; two
 * staging areas, so two decodes can be enqueued back to back and a third waits for the first one's copy --, three
 * memsets and, as a chunk of one file of the batched path below, eleven launches without restart intervals, eight with;
 * nothing read back in between).  The picture
 * must have the context's size, else HSFLOW_E_SIZE.  HSFLOW_E_DATA is returned at once for what the header shows;
 * d_status, a device word, receives what only the bit stream shows: 0 ok, 1 corrupt, 2 truncated (the pixels are then
 * undefined, but nothing outside the picture's width x height x 3 bytes is written either way).
 * Touches no solver state: an owed ITER|EPS check stays owed.  The first decode of a context allocates its scratch
 * (by the file's block count coefficients, component planes, DC sums: 19.8 MB for a 1080p file at 4:4:4; by its length
 * the segment, the clean stream and the subsequences' states; grown on demand behind a wait for the stream, and the one
 * allocation the batched entry grows), kept until hsflow_destroy; contexts that never
 * decode pay nothing, and the scratch does not count for HSFLOW_KERNEL_PERSIST's "only one alive" rule.
 * HSFLOW_E_ARG: null pointer, unknown order, d_status not 4-byte aligned, HSFLOW_JPEGD_SUBSEQ_BITS in the environment
 * not a multiple of 32 in 32..4096; HSFLOW_E_SIZE: stride < 3*width, a picture of another size. */
int hsflow_jpeg_decode_device(hsflow_ctx *ctx, const uint8_t *file, size_t bytes, int order, void *d_pix, size_t stride,
                              uint32_t *d_status /* device word: 0 ok, 1 corrupt, 2 truncated */);
/* The same into host memory, synchronous; a non-zero status word becomes HSFLOW_E_DATA and pix is left alone.  The
 * device-side picture has pix's alignment modulo 4 and its row padding modulo 4, so the stores are those the device form
 * would use.  For checking. */
int hsflow_jpeg_decode(hsflow_ctx *ctx, const uint8_t *file, size_t bytes, int order, uint8_t *pix, size_t stride);
/* Both files into BGR pictures the context keeps on the device, then exactly hsflow_set_frames_device_ex(BGR8 or
 * BGR8_BLUR) on them.  Synchronous like hsflow_set_frames_bgr8.  On HSFLOW_E_DATA (either file) and HSFLOW_E_SIZE the
 * context's frames are unchanged.  Like every frame entry it settles an owed ITER|EPS check first. */
int hsflow_set_frames_jpeg(hsflow_ctx *ctx, int pair, const uint8_t *prev, size_t prev_bytes, const uint8_t *curr, size_t curr_bytes,
                           int blur3x3);
/* The same in front of hsflow_push_frame_device_ex: the camera sequence fed with MJPEG frames. */
int hsflow_push_frame_jpeg(hsflow_ctx *ctx, int pair, const uint8_t *next, size_t bytes, int blur3x3, int reblur_prev);

/* Many files by the same launches.  Files are independent, so n of them decoded side by side take about as long as
 * the longest one: every decode kernel's grid carries the file as a further dimension and reads a per-file record from
 * device memory (csrc/hs_kernels_jpegd.hip.h); hsflow_jpeg_decode_device above is a chunk of one through the same kernels.
 * A batch larger than HSFLOW_JPEGD_BATCH_MAX is decoded in consecutive chunks of at most that many: per chunk one copy
 * from page-locked staging (every file's tables and segment, the records), three memsets and eleven launches for files
 * without restart intervals, eight for files with, twelve for a chunk that mixes the two.  The constant bounds
 * the scratch: a 1080p file takes 19.8 MB (4:4:4; 10.0 MB at 4:2:0: coefficients, planes, DC sums by its own block
 * count) plus about 2.4 times its entropy-coded bytes at the default HSFLOW_JPEGD_SUBSEQ_BITS (segment and clean
 * stream 2, chunk words 0.19, 28 bytes per subsequence 0.22; at 32 bits per subsequence those 28 bytes make it about
 * 9.2 times), so HSFLOW_JPEGD_BATCH_MAX times that at most (a batch of fewer files
 * allocates for as many as it has), grown on demand
 * behind a wait for the stream and kept until hsflow_destroy. */
/* 32: the smallest of {4, 8, 16, 32} within 5 % of the best per-file time at 1080p (profiles/jpegd_batch_time.txt: 0.633,
 * 0.345, 0.201, 0.145 ms per file against 2.31 ms alone).  32 x 11.2 MB = 358 MB of scratch for 1080p files of 500 KB at
 * 4:2:0, about 670 MB at 4:4:4.  The environment variable of the same name overrides it per call, 1..32: that is how the
 * candidates are measured (tools/jpegd_batch_time.py). */
#define HSFLOW_JPEGD_BATCH_MAX 32
/* n files in HOST memory, each of the context's picture size (what cvLoadImage does for OpticalFlowOpenCV.cpp:15,18 and
 * the camera loop's frames, :76,83) -> n pictures in device memory at d_pix[0 .. n), rows `stride` bytes apart, in
 * `order`; only enqueued on ctx's stream.  files, bytes and d_pix are host arrays of n entries; the files' buffers
 * and the arrays are free on return.  Two calls can be enqueued back to back, and behind or in front of
 * hsflow_jpeg_decode_device, with no synchronisation in between: staging is reused behind an event.
 * Every header is parsed and every argument checked before anything is enqueued: on an error d_status, the pictures
 * and the context are untouched, and hsflow_last_error names the file's index ("file 3: ...").  d_status[i], a device
 * word, receives what only file i's bit stream shows (0 ok, 1 corrupt, 2 truncated); a bad file changes nothing for
 * the others, and nothing outside any picture's width x height x 3 bytes is written.  A file's pixels are those of
 * hsflow_jpeg_decode_device, whatever its position, its neighbours, n, the chunking or HSFLOW_JPEGD_SUBSEQ_BITS.
 * Touches no solver state: an owed ITER|EPS check stays owed.
 * HSFLOW_E_ARG: n < 1, a null list or entry, unknown order, d_status not 4-byte aligned, HSFLOW_JPEGD_SUBSEQ_BITS or
 * HSFLOW_JPEGD_BATCH_MAX in the environment unusable; HSFLOW_E_DATA: a header; HSFLOW_E_SIZE: stride < 3*width, a picture of another size. */
int hsflow_jpeg_decode_batch_device(hsflow_ctx *ctx, const uint8_t *const *files, const size_t *bytes, int n,
                                    int order, void *const *d_pix, size_t stride, uint32_t *d_status /* n device words */);
/* n_files >= 2 consecutive frames (the camera loop's cvQueryFrame, OpticalFlowOpenCV.cpp:76,83, fed with files) into
 * the pairs first_pair .. first_pair + n_files - 2: pair k is (file k, file k + 1).  Every file is decoded once, as one
 * batch, into BGR pictures the context keeps; each pair then gets exactly hsflow_set_frames_device_ex(BGR8 or
 * BGR8_BLUR), so its planes are those of hsflow_set_frames_jpeg(ctx, first_pair + k, file k, file k + 1, blur3x3).
 * Synchronous, and like every frame entry it settles an owed ITER|EPS check first.  All or nothing: on HSFLOW_E_DATA
 * (any file, header or bit stream), HSFLOW_E_SIZE and HSFLOW_E_ARG (first_pair + n_files - 1 > n_pairs, n_files < 2,
 * null entries) no pair's frames change.  The same as hsflow_set_sequence_jpeg_ex with flags 0. */
int hsflow_set_sequence_jpeg(hsflow_ctx *ctx, int first_pair, const uint8_t *const *files, const size_t *bytes,
                             int n_files, int blur3x3);
/* The same with the camera loop's frame handling (ABI 0.14; OpticalFlowOpenCV.cpp:76-93,118 fed with files): the batched
 * decode into the context's BGR pictures, then hsflow_set_sequence_device_ex(BGR8 or BGR8_BLUR, flags) -- ONE launch
 * per HSFLOW_PRE_SEQ_MAX frames where there were n_files - 1, every picture read once.  flags: 0, HSFLOW_SEQ_REBLUR or
 * HSFLOW_SEQ_REBLUR | HSFLOW_SEQ_REBLUR_FIRST; a reblurred pair's planes are those of hsflow_set_frames_jpeg(file k,
 * file k) + hsflow_push_frame_jpeg(file k + 1, blur3x3, 1).  Synchronous and all or nothing as above; also HSFLOW_E_ARG
 * for unknown flags. */
int hsflow_set_sequence_jpeg_ex(hsflow_ctx *ctx, int first_pair, const uint8_t *const *files, const size_t *bytes,
                                int n_files, int blur3x3, int flags);
/* hsflow_set_frames_jpeg without the wait, what hsflow_pipeline_submit_jpeg is made of: both headers are checked at
 * once (HSFLOW_E_DATA / _SIZE / _ARG: nothing enqueued, the frames unchanged); then the two files are decoded as a batch
 * of two into the context's BGR pictures, the two status words are copied to page-locked memory, and
 * hsflow_set_frames_device_ex follows, all on ctx's stream.  hsflow_jpeg_async_status waits for that copy alone and
 * returns HSFLOW_E_DATA if either bit stream was bad (the pair's planes and a solve enqueued behind them are then
 * meaningless).  It answers once per hsflow_set_frames_jpeg_async, for the latest one: HSFLOW_E_STATE with no such call
 * before or when that call's status has been asked for already.  The two words are the pair's own, on the device and on
 * the host: hsflow_jpeg_decode, hsflow_set_frames_jpeg, hsflow_push_frame_jpeg and the batch entries in between do not
 * change what it answers. */
int hsflow_set_frames_jpeg_async(hsflow_ctx *ctx, int pair, const uint8_t *prev, size_t prev_bytes, const uint8_t *curr,
                                 size_t curr_bytes, int blur3x3);
int hsflow_jpeg_async_status(hsflow_ctx *ctx);

/* --- is it right?  (verifyResults) -------------------------------------------------------- */

/* The reference's class has a verifyResults() like every SDK sample (SDKUtil/include/SDKApplication.hpp) and left it
 * a stub that returns SDK_SUCCESS (HSOpticalFlowOpenCL.cpp:894).  Here it is real, and needs no second implementation to
 * compare with: every fast path of this library (LDS tile, register strip, folded strip, the persistent launch,
 * launches replayed from a hipGraph, the derivative pass folded into the first launch, the speculative ITER|EPS pass)
 * is specified to give, bit for bit, what the one-sweep-per-launch kernel behind the stand-alone derivative kernel
 * gives.  hsflow_verify runs exactly that on the frames the context holds, into memory of its own, compares on the
 * device (k_plane_compare) and hands back a report of 120 bytes -- no plane is downloaded.
 *
 * The comparison rule (csrc/hs_verify_rule.h, one header for the kernel and for hsflow_compare_planes_host), for one
 * pair of fp32 values a (what the context holds) and b (the reference side):
 *   differing    the 32 bits differ: +0 and -0 differ, two NaNs with the same bits do not;
 *   failing      differing and not covered by the one exemption this project has (the strip
 *                kernels carry a scaled state inside a launch, so flow that would be denormal keeps bits that depend
 *                on where the launch boundaries fall): a differing pair is exempt iff both values are finite and
 *                fabsf(a) < HSFLOW_VERIFY_TINY && fabsf(b) < HSFLOW_VERIFY_TINY;
 *   nonfinite    a is NaN or Inf, whether or not it differs;
 *   max_abs_diff the maximum of fabsf(a - b) over the differing pairs whose two values are finite, 0 if there is none;
 *   max_ulp      the maximum over the same pairs of the distance on the ordered integer line (i = bits; if (i < 0)
 *                i = INT32_MIN - i; distance as unsigned): a flip of the lowest mantissa bit is 1 apart.  +0 against -0
 *                is the one differing pair that is 0 apart and 0 in max_abs_diff: differing, exempt, not failing;
 *   first_failing the lowest raster index y * width + x of a failing element, -1 if there is none.
 * Counts, maxima and a minimum only: a record is the same on every run, whatever the order of execution. */
#define HSFLOW_VERIFY_TINY 1e-30f /* "bit for bit, except where both values lie below 1e-30" */
typedef struct hsflow_plane_diff { /* 40 bytes */
    uint64_t differing, failing, nonfinite;
    int64_t first_failing;
    float max_abs_diff;
    uint32_t max_ulp;
} hsflow_plane_diff;

/* The rule over two planes in HOST memory (the same header compiled for the host; no device needed).  Strides in
 * bytes, multiples of 4 and >= 4 * width.  HSFLOW_E_ARG: null pointer; HSFLOW_E_SIZE: size or stride. */
int hsflow_compare_planes_host(const float *a, size_t a_stride, const float *b, size_t b_stride, int width, int height,
                               hsflow_plane_diff *out);

/* The context's CURRENT flow of `pair` (side a) against planes the caller holds in device memory on the context's
 * device (side b; 4-byte aligned, strides in bytes, multiples of 4 and >= 4 * width; 16-byte alignment of base and
 * stride gets the kernel's wide loads).  What a consumer on the device otherwise does through hsflow_get_flow and a
 * loop on the host.  Synchronous: complete on return; waits only for what this context enqueued.  Settles an ITER|EPS
 * check that hsflow_solve_async still owes first, reads the flow and never changes it: pointers from
 * hsflow_flow_view_device stay valid (the ordering rules of hsflow_render_flow_device apply word for word).  The first
 * call allocates a few hundred bytes on the device and in page-locked memory. */
int hsflow_compare_flow_device(hsflow_ctx *ctx, int pair, const void *d_u, size_t u_stride, const void *d_v, size_t v_stride,
                               hsflow_plane_diff *u, hsflow_plane_diff *v);

typedef struct hsflow_verify_report { /* 120 bytes */
    uint32_t struct_size;    /* = sizeof(hsflow_verify_report), set by the caller                             */
    int32_t ok;              /* 1 iff u.failing == 0 && v.failing == 0 && deriv_differing == 0 &&
                                iterations_ref == iterations_done                                             */
    int32_t pair;            /* pair = -1 calls: the lowest pair with a failing element (flow or derivative
                                words), -1 if none; else the pair asked for                                   */
    int32_t iterations_done; /* sweeps of the solve under test (iterations_done of hsflow_get_info)           */
    int32_t iterations_ref;  /* sweeps the reference pass ran: its own stopping sweep under EPS                */
    int32_t reserved;
    hsflow_plane_diff u, v;  /* pair = -1: counts summed and maxima over all pairs; first_failing is the raster
                                index within the lowest pair in which that plane fails                        */
    uint64_t deriv_differing; /* packed derivative words that differ from the stand-alone derivative kernel's  */
    int64_t deriv_first;      /* raster index of the first one (pair = -1: in the lowest such pair), -1 if none */
} hsflow_verify_report;

/* Is the flow this context holds NOW what a sweep-by-sweep solve of the frames it holds, with the parameters of its
 * last solve, produces?  (hsflow_solve, hsflow_solve_async, a pipeline slot's solve; hsflow_solve_probe counts as an
 * ITER solve of max_iter sweeps.)
 * The reference pass: the stand-alone derivative kernel into a coefficient plane of its own, then the one-sweep kernel
 * of the mode (HSFLOW_KERNEL_SIMPLE), launch by launch -- no hipGraph, no derivative pass inside a Jacobi launch, no
 * speculation -- from zero flow, with the same mode, lambda / alpha, term_type, max_iter, epsilon, row origin and Eps
 * rows.  Under EPS it finds its OWN stopping sweep from Eps measured in every sweep (iterations_ref).  It always covers
 * every pair of the context, because under EPS a batch stops as one.  After a solve whose pairs stopped each on its own
 * (hsflow_set_pair_termination) it finds EVERY pair's own stopping sweep, from the one-sweep kernel's Eps of that pair
 * alone: pair = i reports pair i's iterations_done / iterations_ref; pair = -1 is ok only if every pair's counts agree,
 * and reports the counts of the lowest pair where they differ, else the maxima.  Then k_plane_compare over the flow planes
 * (a = the context's, b = the reference's) and over the packed derivative words, of `pair`, or of all pairs aggregated
 * (pair = -1).
 * It leaves the context as it found it: flow, derivatives, hsflow_info, pointers handed out by
 * hsflow_flow_view_device, the cached graphs and plans, and what hsflow_get_info needs to measure last_eps later.  Its
 * scratch (two flow buffers and a coefficient plane, context-sized) is allocated by the first call and kept until
 * hsflow_destroy; contexts that never verify pay nothing, and the scratch does not count as a context for
 * HSFLOW_KERNEL_PERSIST's "only one alive" rule.  Like a render it first settles an ITER|EPS check that
 * hsflow_solve_async still owes.  Synchronous: complete on return.  A check, not a hot path: at max_iter launches it
 * costs several solves.
 * Writing the flow through hsflow_set_flow_device is NOT a refusal: the flow held now is what is compared.
 * HSFLOW_E_ARG: null pointer, wrong struct_size, pair outside [-1, n_pairs).  HSFLOW_E_STATE, with a text that says
 * which: no solve yet; the last solve failed or ended in HSFLOW_E_NOTERM; the last solve had use_previous = 1 (its
 * starting flow is gone: warm starts cannot be verified); frames were set or pushed since the last solve.
 * Out of scope: hsflow_multi_* and hsflow_slab_* (a slab's contexts refuse anyway: their solves are warm-started
 * chunks), and flow that is not finite (lambda beyond ~1e30): NaNs of different bits fail, and nonfinite > 0 in the
 * report says why. */
int hsflow_verify(hsflow_ctx *ctx, int pair, hsflow_verify_report *report);

/* --- introspection ------------------------------------------------------------------------ */

int hsflow_get_info(hsflow_ctx *ctx, hsflow_info *info);
/* measure_last_eps = 0: as hsflow_get_info, but last_eps of an asynchronous ITER|EPS solve is left as it is
 * (NaN until measured) instead of running that solve's last launch again; 1: hsflow_get_info. */
int hsflow_get_info_ex(hsflow_ctx *ctx, hsflow_info *info, int measure_last_eps);
const char *hsflow_last_error(hsflow_ctx *ctx); /* ctx may be NULL: last create() error */
const char *hsflow_status_string(int status);
int hsflow_version(void); /* major*1000 + minor */
int hsflow_device_count(int *count);

/* --- page-locked host memory (staging for the async copies) ------------------------------- */

/* The reference aliased host planes into the device with CL_MEM_USE_HOST_PTR
 * (HSOpticalFlowOpenCL.cpp:184-228); here the caller keeps ownership of its host buffers and may
 * page-lock them so that uploads / downloads overlap the solver. */
int hsflow_host_alloc(void **out, size_t bytes);   /* hipHostMalloc */
int hsflow_host_free(void *p);                     /* NULL accepted */
int hsflow_host_register(void *p, size_t bytes);   /* page-lock memory the caller allocated */
int hsflow_host_unregister(void *p);

/* --- pair pipeline: host frames in, host flow out, copies overlapped with solves ----------- */

/* Independent pairs streamed through ONE device (BASELINE config C4, SURVEY.md 8e: "one host
 * thread + >= 2 streams per GPU, double-buffered staging").  The pipeline owns `depth` single-pair
 * contexts, each on its own stream; submit() enqueues upload -> solve -> download of one pair on
 * the next slot and returns at once, so that the upload of pair i+1 and the download of pair i-1
 * run beside the solve of pair i.  It replaces the per-pair body of the reference's run()
 * (HSOpticalFlowOpenCL.cpp:744-767: write frames, derivatives, iterations, read u, v).
 * The host buffers of a submitted pair belong to the pipeline until wait(ticket) returned; use
 * page-locked memory for them.  Termination: ITER, or ITER|EPS (strip / fold kernel) -- whatever
 * hsflow_solve_async accepts; a pair whose early stop fired is re-solved inside wait().
 * Single-owner like a context; one pipeline per (thread, device). */
typedef struct hsflow_pipeline hsflow_pipeline;
int hsflow_pipeline_create(hsflow_pipeline **out, int device, int width, int height, int depth);
/* The same with the `depth` slots spread over `lanes` streams (slot k on stream k mod lanes; 1 <= lanes <= depth;
 * hsflow_pipeline_create: lanes = depth, which is what host-memory pairs want -- upload, solve and download of three
 * pairs on three queues).  For pairs that are already in device memory TWO lanes with 4 - 8 slots are the shape to use:
 * two solves side by side is what fills the chip's gaps, and the further slots keep both streams' queues
 * full while the host settles and refills the oldest slot -- 0.125 ms per 1080p / 100 pair against 0.139 with two slots
 * on two streams. */
/* With THREE OR MORE lanes the pipeline picks the launch shape itself for a pair whose caller left it to the planner (CV
 * mode, kernel AUTO, fuse_steps = strip_rows = threads = tile_w = tile_h = 0, ITER in term_type, max_iter > 0) when the
 * frame is at least 256 x 80 and at most 1.5 Mpixel: the strip kernel with min(20, max_iter) sweeps per launch, 5 rows
 * per lane and 1024 threads per workgroup (768 where 1024 would leave fewer than ~50 tiles) -- the shape that costs the
 * least CU-time while other slots' solves share the chip.  hsflow_pipeline_info reports it.  The flow is bit-identical to
 * that of the planner's shape, except for values below ~1e-30 (flow decaying to nothing on synthetic flat frames), whose
 * last bits depend on where the launch boundaries fall.  HSFLOW_PIPELINE_AUTO_SHAPE=0 turns this off. */
int hsflow_pipeline_create_lanes(hsflow_pipeline **out, int device, int width, int height, int depth, int lanes);
int hsflow_pipeline_destroy(hsflow_pipeline *pl); /* drains first; NULL accepted */
/* ticket (optional out): 0, 1, 2, ... in submission order.  Blocks only while the slot it is
 * about to reuse (ticket - depth) is still running.  With three or more lanes the launch shape may be the
 * pipeline's own (hsflow_pipeline_create_lanes). */
int hsflow_pipeline_submit(hsflow_pipeline *pl, const uint8_t *prev, size_t prev_stride,
                           const uint8_t *curr, size_t curr_stride, float *u, size_t u_stride,
                           float *v, size_t v_stride, const hsflow_params *params, uint64_t *ticket);
/* Same with the frames in another layout; the CPU route's pre-processing (OpticalFlowOpenCV.cpp:17-28)
 * then runs on the device as part of the pair's queue. */
/* (format: HSFLOW_FRAMES_*, above; HSFLOW_FRAMES_GRAY8 is hsflow_pipeline_submit) */
int hsflow_pipeline_submit_ex(hsflow_pipeline *pl, int format, const uint8_t *prev, size_t prev_stride,
                              const uint8_t *curr, size_t curr_stride, float *u, size_t u_stride,
                              float *v, size_t v_stride, const hsflow_params *params, uint64_t *ticket);
/* The same for a stream of pairs that are ALREADY IN DEVICE MEMORY (a decoder's or a camera's output, the frames of a
 * resident sequence): the slot gets its own copy of the frames (hsflow_solve_async_frames_device: written by the solve's
 * first launch where that can read the caller's planes, by a copy kernel ahead of it otherwise), the flow stays in the slot and is handed
 * out by hsflow_pipeline_flow_device -- no host buffer anywhere.  This is the reference's camera loop
 * (OpticalFlowOpenCV.cpp:91-95: fresh frames, ITER|EPS, every pair) at the speed of the solver: while pair k's
 * early-stop check is still owed, pair k+1 is already running on the next slot's stream; the check is looked at when
 * somebody asks for pair k (wait / flow_device / info / the slot's reuse `depth` submissions later), and a pair whose
 * early stop fired is re-solved from its slot's frames, which nothing has touched.  The caller's frame buffers must
 * be complete when submit is called (they are read by work enqueued on the slot's stream) and may be reused once
 * any later call on the pipeline has returned that waited for this ticket. */
int hsflow_pipeline_submit_device(hsflow_pipeline *pl, const void *d_prev, size_t prev_stride, const void *d_curr,
                                  size_t curr_stride, const hsflow_params *params, uint64_t *ticket);
/* The same for resident frames in any HSFLOW_FRAMES_* layout.  HSFLOW_FRAMES_GRAY8 is hsflow_pipeline_submit_device, the
 * in-place read included.  The other three run hsflow_set_frames_device_ex and hsflow_solve_async on the slot: the fused
 * pre-processing launch takes the place of the copy kernel in the pair's chain, and everything behind it (tickets, the
 * re-solve of a pair whose early stop fired, hsflow_pipeline_frames_u8 / _render / _verify) works from the slot's
 * pre-processed planes, as after hsflow_pipeline_submit_ex.  The caller's buffers: as for hsflow_pipeline_submit_device. */
int hsflow_pipeline_submit_device_ex(hsflow_pipeline *pl, int format, const void *d_prev, size_t prev_stride, const void *d_curr,
                                     size_t curr_stride, const hsflow_params *params, uint64_t *ticket);
/* The same for a pair of JPEG FILES in host memory (the disk route's two cvLoadImage, OpticalFlowOpenCV.cpp:15,18; a
 * camera that delivers MJPEG, :76,83): both files are decoded as a batch of two on the slot's stream into pictures the
 * slot's context owns (hsflow_set_frames_jpeg_async); the pre-processing of hsflow_set_frames_device_ex and
 * hsflow_solve_async follow on the same stream, and the flow stays in the slot as with hsflow_pipeline_submit_device.
 * Never waits for the device except for a free slot.  The files' buffers are free on return.  What the headers show
 * (HSFLOW_E_DATA, HSFLOW_E_SIZE) is returned here, and the slot stays free: no ticket is issued.  What only a bit stream
 * shows is read when the ticket is waited for: hsflow_pipeline_wait, _flow_device, _info, _frames_u8, _verify and
 * _render* of that ticket return HSFLOW_E_DATA; other tickets, earlier or later, on the same lane or not, are unaffected
 * (the slot's reuse `depth` submissions later does not report it; hsflow_pipeline_drain does).  With
 * hsflow_pipeline_render_jpeg of the ticket: files in, a file out, no picture crossing PCIe. */
int hsflow_pipeline_submit_jpeg(hsflow_pipeline *pl, const uint8_t *prev, size_t prev_bytes, const uint8_t *curr,
                                size_t curr_bytes, int blur3x3, const hsflow_params *params, uint64_t *ticket);
/* wait(ticket) + where that pair's flow lies (hsflow_flow_view_device of its slot): valid until `depth` further
 * pairs have been submitted.  HSFLOW_E_STATE if the slot has been reused already. */
int hsflow_pipeline_flow_device(hsflow_pipeline *pl, uint64_t ticket, const float **d_u, const float **d_v, size_t *stride_bytes);
int hsflow_pipeline_wait(hsflow_pipeline *pl, uint64_t ticket); /* u, v of that pair are complete */
/* wait(ticket) + the picture of that pair's flow (hsflow_render_flow / hsflow_render_flow_device of its slot, on the
 * slot's stream): a pair whose early stop fired has been re-solved by then.  Both return when the picture is complete,
 * after device-resident and host-buffer submits alike.  HSFLOW_E_STATE if the slot has been reused already; argument
 * errors as hsflow_render_flow_device. */
int hsflow_pipeline_render(hsflow_pipeline *pl, uint64_t ticket, const hsflow_render_params *rp, uint8_t *rgb, size_t stride);
int hsflow_pipeline_render_device(hsflow_pipeline *pl, uint64_t ticket, const hsflow_render_params *rp, void *d_rgb, size_t stride);
/* The same three for the dense colour picture (hsflow_color_flow, hsflow_color_flow_device, hsflow_color_flow_jpeg of the
 * ticket's slot): complete on return, HSFLOW_E_STATE if the slot has been reused already, otherwise their errors. */
int hsflow_pipeline_color(hsflow_pipeline *pl, uint64_t ticket, const hsflow_color_params *cp, uint8_t *rgb, size_t stride,
                          float *scale_used /* may be null */);
int hsflow_pipeline_color_device(hsflow_pipeline *pl, uint64_t ticket, const hsflow_color_params *cp, void *d_rgb, size_t stride);
int hsflow_pipeline_color_jpeg(hsflow_pipeline *pl, uint64_t ticket, const hsflow_color_params *cp, int quality,
                               uint8_t *jpeg, size_t capacity, size_t *bytes);
/* wait(ticket) + hsflow_warp / hsflow_warp_device of the ticket's slot: complete on return, HSFLOW_E_STATE if the slot has
 * been reused already, otherwise their errors. */
int hsflow_pipeline_warp(hsflow_pipeline *pl, uint64_t ticket, const hsflow_warp_params *wp, const uint8_t *src, size_t src_stride,
                         const uint8_t *ref, size_t ref_stride, uint8_t *dst, size_t dst_stride, hsflow_warp_stats *stats);
int hsflow_pipeline_warp_device(hsflow_pipeline *pl, uint64_t ticket, const hsflow_warp_params *wp, const void *d_src, size_t src_stride,
                                const void *d_ref, size_t ref_stride, void *d_dst, size_t dst_stride, hsflow_warp_stats *d_stats);
/* wait(both tickets) + the forward-backward check of ticket_fwd's flow against ticket_bwd's (hsflow_fb_planes /
 * hsflow_fb_planes_device on the forward slot, the backward slot's flow in place): complete on return, HSFLOW_E_STATE if
 * either slot has been reused. */
int hsflow_pipeline_fb(hsflow_pipeline *pl, uint64_t ticket_fwd, uint64_t ticket_bwd, const hsflow_fb_params *fp, uint8_t *mask, size_t mask_stride,
                       float *err2, size_t err2_stride, hsflow_fb_stats *stats);
int hsflow_pipeline_fb_device(hsflow_pipeline *pl, uint64_t ticket_fwd, uint64_t ticket_bwd, const hsflow_fb_params *fp, void *d_mask,
                              size_t mask_stride, void *d_err2, size_t err2_stride, hsflow_fb_stats *d_stats);
/* wait(ticket) + hsflow_median of that pair's flow on its slot (host memory, the slot's flow unchanged) and
 * hsflow_median_apply (the slot's flow replaced; device memory): both complete on return, HSFLOW_E_STATE if the slot has
 * been reused. */
int hsflow_pipeline_median(hsflow_pipeline *pl, uint64_t ticket, const hsflow_median_params *mp, int passes, const uint8_t *state, size_t state_stride,
                           float *u, float *v, size_t out_stride, uint8_t *state_out, size_t state_out_stride, hsflow_median_stats *stats);
int hsflow_pipeline_median_apply(hsflow_pipeline *pl, uint64_t ticket, const hsflow_median_params *mp, int passes, const void *d_state,
                                 size_t state_stride, void *d_state_out, size_t state_out_stride, hsflow_median_stats *d_stats);
/* wait(ticket) + hsflow_interp / hsflow_interp_device of the ticket's slot (the ticket's pair is the FORWARD pair): complete
 * on return, HSFLOW_E_STATE if the slot has been reused. */
int hsflow_pipeline_interp(hsflow_pipeline *pl, uint64_t ticket, float t, const hsflow_interp_params *ip, const uint8_t *prev, size_t prev_stride,
                           const uint8_t *curr, size_t curr_stride, const uint8_t *vis_prev, size_t vis_prev_stride, const uint8_t *vis_curr,
                           size_t vis_curr_stride, const uint8_t *ref, size_t ref_stride, uint8_t *dst, size_t dst_stride, uint8_t *cls,
                           size_t cls_stride, hsflow_interp_stats *stats);
int hsflow_pipeline_interp_device(hsflow_pipeline *pl, uint64_t ticket, float t, const hsflow_interp_params *ip, const void *d_prev, size_t prev_stride,
                                  const void *d_curr, size_t curr_stride, const void *d_vis_prev, size_t vis_prev_stride, const void *d_vis_curr,
                                  size_t vis_curr_stride, const void *d_ref, size_t ref_stride, void *d_dst, size_t dst_stride, void *d_cls,
                                  size_t cls_stride, hsflow_interp_stats *d_stats);
/* wait(ticket) + the JPEG file of that pair's picture (hsflow_render_flow_jpeg of its slot): complete on return.
 * HSFLOW_E_STATE if the slot has been reused already; otherwise the errors of hsflow_render_flow_jpeg. */
int hsflow_pipeline_render_jpeg(hsflow_pipeline *pl, uint64_t ticket, const hsflow_render_params *rp, int quality,
                                uint8_t *jpeg, size_t capacity, size_t *bytes);
/* wait(ticket) -- a pair whose early stop fired has been re-solved by then -- + hsflow_verify of that pair on its slot:
 * what the slot actually ran is verified, including a launch shape the pipeline chose itself (three or more lanes).
 * HSFLOW_E_STATE if the slot has been reused already. */
int hsflow_pipeline_verify(hsflow_pipeline *pl, uint64_t ticket, hsflow_verify_report *report);
/* wait(ticket) + the slot's own copy of that pair's frames into host memory (hsflow_get_frames_u8 of its slot): what a
 * re-solve, a verify or a render of that ticket works from.  HSFLOW_E_STATE if the slot has been reused already. */
int hsflow_pipeline_frames_u8(hsflow_pipeline *pl, uint64_t ticket, uint8_t *prev, size_t prev_stride, uint8_t *curr,
                              size_t curr_stride);
/* wait(ticket) + iterations_done, last_eps, eps_rerun ... of that pair; HSFLOW_E_STATE once a later
 * pair has finished on the same slot (ask before submitting `depth` more pairs). */
int hsflow_pipeline_info(hsflow_pipeline *pl, uint64_t ticket, hsflow_info *info);
int hsflow_pipeline_drain(hsflow_pipeline *pl);                 /* wait for everything submitted */
int hsflow_pipeline_depth(hsflow_pipeline *pl);
/* Submissions so far whose frame copy rode in the solve's first launch (sum of hsflow_frame_copies_elided over the slots). */
int hsflow_pipeline_copies_elided(hsflow_pipeline *pl, uint64_t *count);
const char *hsflow_pipeline_last_error(hsflow_pipeline *pl);    /* pl may be NULL: create() error */

/* --- several GPUs from one host process ----------------------------------------------------- */

/* Independent pairs over the GPUs of a node (BASELINE config C4): one pair pipeline of `depth` slots per
 * device, each driven by a host thread of its own; pair i goes to devices[i mod ndev]; no collective.  What the
 * reference's run() did per pair on one device (HSOpticalFlowOpenCL.cpp:744-767), spread over the node.  A device may
 * be listed more than once.  submit() never blocks on the device; the host buffers of a pair (page-locked for
 * overlapped copies) belong to the library until wait(ticket) / drain() returned.  format: HSFLOW_FRAMES_*.
 * Single-owner: submit / wait / drain / destroy from one thread. */
typedef struct hsflow_multi hsflow_multi;
int hsflow_multi_create(hsflow_multi **out, const int *devices, int ndev, int width, int height, int depth);
int hsflow_multi_destroy(hsflow_multi *m); /* drains first; NULL accepted */
int hsflow_multi_devices(hsflow_multi *m);
int hsflow_multi_submit(hsflow_multi *m, int format, const uint8_t *prev, size_t prev_stride, const uint8_t *curr, size_t curr_stride,
                        float *u, size_t u_stride, float *v, size_t v_stride, const hsflow_params *params, uint64_t *ticket);
int hsflow_multi_wait(hsflow_multi *m, uint64_t ticket);
int hsflow_multi_drain(hsflow_multi *m);
const char *hsflow_multi_last_error(hsflow_multi *m); /* m may be NULL: create() error */

/* ONE large frame in row slabs over several GPUs (BASELINE config C5): slab k holds a contiguous range
 * of rows plus `halo` rows either side on devices[k]; the sweeps run in chunks of <= halo and after every chunk
 * neighbouring slabs swap `halo` rows of u and v device to device (peer copies over xGMI, ordered by events; the host
 * only enqueues) -- k-row halos every k sweeps instead of one row per sweep: the same bytes in k times fewer
 * messages.  The result is bit-identical to the whole-frame solve on one GPU (hsflow_set_row_origin keeps each slab
 * on the frame's checkerboard).  Termination: ITER, or ITER|EPS as the reference calls the solver
 * (OpticalFlowOpenCV.cpp:29,94 -- hsflow_default_params as they are): the frame's Eps is the maximum over the slabs'
 * owned rows, so a chunk that ANY slab's witness vouches for holds no stop; when none does, the solve is replayed to
 * that chunk and measured sweep by sweep, the maximum taken on the host between chunks, and it ends on the sweep the
 * one-context solve ends on.  use_previous continues from the flow of the last solve (halos refreshed first).  A
 * device may be listed more than once -- listing each device TWICE gives every GPU two sub-slabs on streams of their
 * own, so that one's peer copies run under the other's sweeps (hsflow_slab_create_overlapped does that).  The
 * one-process-per-GPU form of the same scheme, with RCCL send / recv, is opticalflowhs_amd/slab.py.
 * The cross-device copies (hipMemcpyPeerAsync) have only ever run between slabs that share a card (one-GPU boxes). */
typedef struct hsflow_slab hsflow_slab;
int hsflow_slab_create(hsflow_slab **out, const int *devices, int nslab, int width, int height, int halo);
int hsflow_slab_destroy(hsflow_slab *s); /* NULL accepted */
int hsflow_slab_count(hsflow_slab *s);
int hsflow_slab_rows(hsflow_slab *s, int k, int *lo, int *hi); /* rows [lo, hi) slab k owns */
int hsflow_slab_set_frames_u8(hsflow_slab *s, const uint8_t *prev, size_t prev_stride, const uint8_t *curr, size_t curr_stride);
int hsflow_slab_solve(hsflow_slab *s, const hsflow_params *params); /* returns after every device finished */
int hsflow_slab_exchanges(hsflow_slab *s);                          /* halo exchanges of the last solve */
int hsflow_slab_iterations_done(hsflow_slab *s);                    /* sweeps of the last solve (< max_iter: the early stop fired) */
int hsflow_slab_eps_measured(hsflow_slab *s);                       /* 1: no slab's witness held, Eps was measured sweep by sweep */
/* 2 * ndev slabs, devices[k] holding slabs 2k and 2k+1 (see above). */
int hsflow_slab_create_overlapped(hsflow_slab **out, const int *devices, int ndev, int width, int height, int halo);
int hsflow_slab_get_flow(hsflow_slab *s, float *u, size_t u_stride, float *v, size_t v_stride);
const char *hsflow_slab_last_error(hsflow_slab *s); /* s may be NULL: create() error */

/* --- coarse-to-fine solves: a pyramid over the solver ---------------------------------------- */

/* Horn-Schunck linearises the brightness equation, so one solve finds motions of about a pixel.  hsflow_solve_pyramid
 * solves at several scales, coarsest first, and at every further step warps the second frame by the flow so far and solves
 * for the INCREMENT.  Every solve is an ordinary hsflow_solve of the level's frames from zero flow with the caller's
 * hsflow_params; each solve regularises the increment only (DESIGN.md 4.17 names that limit).  For a context of W x H:
 *   Levels   level 0 is the context; level l+1 is ceil(W_l / 2) x ceil(H_l / 2).  levels = 0 (auto): as many levels as keep
 *            min(W_l, H_l) >= min_size, at most HSFLOW_PYRAMID_MAX_LEVELS, level 0 always.  levels = 1 .. 8: as given; a
 *            level of 1 x 1 pixels cannot be halved: HSFLOW_E_SIZE.
 *   down     prev_l and curr_l, l >= 1, from level l-1, for u8 planes of W x H:
 *              dst(x, y) = (sum_{i,j=-2..2} k_i k_j src(clamp(2x+i, 0, W-1), clamp(2y+j, 0, H-1)) + 128) >> 8, k = (1, 4, 6, 4, 1):
 *            exact integers (hsflow_pyramid_down_host is the same rule on the host).
 *   prolong  a coarse plane c of Wc x Hc floats to a fine one of W x H, Wc = ceil(W/2), Hc = ceil(H/2), all fp32, every
 *            operation rounded on its own:
 *              h(x, r)   = c(x>>1, r) for even x;  fl(fl(c(k, r) + c(min(k+1, Wc-1), r)) * 0.5f), k = x>>1, for odd x
 *              g(x, y)   = h(x, y>>1) for even y;  fl(fl(h(x, r) + h(x, min(r+1, Hc-1))) * 0.5f), r = y>>1, for odd y
 *              dst(x, y) = fl(2 * g(x, y))
 *            Even positions copy; a NaN or an Inf beside them stays where it is (hsflow_pyramid_prolong_host).
 *   Steps, coarsest level first, `warps` steps per level:
 *     - the first step of the coarsest level: total = solve(prev, curr) from zero.  No addition and no warp: with
 *       levels = 1, warps = 1, median_radius = 0 the call is hsflow_solve bit for bit, -0.0 included.
 *     - every further step: the base flow (u0, v0) is prolong(total of level l+1) for the first step of a level, the
 *       level's total so far for a later one; w = the warp rule of hsflow_warp on curr_l with (u0, v0), one channel, t = 1,
 *       HSFLOW_WARP_BORDER_REPLICATE, where an unknown pixel (NaN, or a magnitude above 1e9) takes curr_l's own byte at
 *       (x, y); (du, dv) = solve(prev_l, w) from zero; total = fl(u0 + du), fl(v0 + dv).
 *     - median_radius 1 or 2: every total, the coarsest level's and the last one included, takes one pass of the median
 *       rule (hsflow_median_host: that radius, HSFLOW_MEDIAN_FILTER, min_votes 1, no state plane) as soon as it is formed.
 *   Afterwards the total of level 0 is the context's flow: hsflow_get_flow*, hsflow_flow_view_device, render, colour, warp,
 *   fb, median, interp and a later use_previous = 1 solve see it as they see any flow.  The context's frames are the
 *   caller's (the second frame is put back when the call's work has run); the context treats them as changed -- a following
 *   solve with reuse_derivatives = 1 recomputes the derivatives -- and treats its flow as caller-written, the way
 *   hsflow_set_flow_device leaves it.  hsflow_get_info reports the finest level's last solve; hsflow_verify returns
 *   HSFLOW_E_STATE until the next plain solve.
 * The call covers all pairs of the context.  The level contexts (levels >= 1) and their planes are created by the first call
 * and kept until hsflow_destroy; they are made anew when the plan changes; they share the context's device, stream and CU
 * share.  A context that never calls it pays nothing.  With ITER termination the call only enqueues (like
 * hsflow_solve_async); with HSFLOW_TERM_EPS in term_type every solve is settled before its flow is read: ONE HOST WAIT PER
 * STEP.  Not covered: pair-pipeline tickets, hsflow_multi_* and slabs. */
#define HSFLOW_PYRAMID_MAX_LEVELS 8
#define HSFLOW_PYRAMID_MAX_WARPS 8
typedef struct hsflow_pyramid_params {
    uint32_t struct_size;  /* = sizeof(hsflow_pyramid_params) */
    int32_t levels;        /* 0: auto (min_size decides); 1 .. HSFLOW_PYRAMID_MAX_LEVELS: as given */
    int32_t min_size;      /* auto: the smaller side of the coarsest level is at least this (>= 1) */
    int32_t warps;         /* steps per level, 1 .. HSFLOW_PYRAMID_MAX_WARPS */
    int32_t median_radius; /* 0: none; 1, 2: a 3x3 / 5x5 median of every total */
} hsflow_pyramid_params;
/* levels 0, min_size 32, warps 1, median_radius 0.  NULL is ignored.  (Measured with the CPU oracle: a coarsest level of
 * 20 x 16 raised the error of a (9, 6) px shift on 320 x 256 from 0.24 to 1.27 px; hence 32.) */
void hsflow_default_pyramid_params(hsflow_pyramid_params *pp);
/* The plan of a width x height context, no device needed: *levels, and widths[l], heights[l] for l < *levels (arrays of
 * HSFLOW_PYRAMID_MAX_LEVELS entries, the rest zero; either may be NULL).  HSFLOW_E_ARG: pp NULL or its struct_size wrong,
 * levels outside 0 .. 8, min_size < 1, warps outside 1 .. 8, median_radius outside 0 .. 2, levels NULL.  HSFLOW_E_SIZE:
 * width or height < 1, or explicit levels beyond a level of 1 x 1. */
int hsflow_pyramid_plan(int width, int height, const hsflow_pyramid_params *pp, int *levels, int *widths, int *heights);
/* `down` on the host: src is width x height bytes, dst receives ceil(width/2) bytes in each of ceil(height/2) rows and
 * nothing else.  Strides in bytes.  HSFLOW_E_ARG: a NULL plane; HSFLOW_E_SIZE: width or height < 1, a stride smaller than
 * its row. */
int hsflow_pyramid_down_host(const uint8_t *src, size_t src_stride, int width, int height, uint8_t *dst, size_t dst_stride);
/* `prolong` on the host: width x height is the FINE size, coarse holds ceil(width/2) x ceil(height/2) floats.  Strides in
 * bytes, multiples of 4.  HSFLOW_E_ARG: a NULL plane; HSFLOW_E_SIZE: width or height < 1, a stride smaller than its row or
 * no multiple of 4. */
int hsflow_pyramid_prolong_host(const float *coarse, size_t coarse_stride, int width, int height, float *dst, size_t dst_stride);
/* The pyramid solve of every pair of the context (above).
 *   HSFLOW_E_ARG    params NULL or its struct_size wrong; pp as for hsflow_pyramid_plan; a mode other than HSFLOW_MODE_CV;
 *                   use_previous set; profile = 1; HSFLOW_KERNEL_PERSIST; whatever hsflow_solve refuses in params
 *   HSFLOW_E_SIZE   explicit levels beyond a level of 1 x 1; more pairs than half the device's grid limit in z
 *   HSFLOW_E_STATE  frames not set; a row origin (hsflow_set_row_origin) or an Eps row window (hsflow_set_eps_rows) other
 *                   than the default; hsflow_set_pair_termination on, with EPS in term_type and more than one pair
 *   HSFLOW_E_NOTERM as hsflow_solve, from any level;  HSFLOW_E_OOM / HSFLOW_E_DEVICE: the level contexts, or a HIP call
 * A refusal leaves the context's flow as it was.  A failure inside a level leaves the flow unspecified and the frames the
 * caller's. */
int hsflow_solve_pyramid(hsflow_ctx *ctx, const hsflow_params *params, const hsflow_pyramid_params *pp);
/* What the last pyramid solve did. */
typedef struct hsflow_pyramid_info {
    uint32_t struct_size; /* = sizeof(hsflow_pyramid_info), set by the caller */
    int32_t levels, warps, median_radius;
    int32_t width[HSFLOW_PYRAMID_MAX_LEVELS], height[HSFLOW_PYRAMID_MAX_LEVELS];
    int32_t sweeps[HSFLOW_PYRAMID_MAX_LEVELS][HSFLOW_PYRAMID_MAX_WARPS]; /* [level][step]: sweeps of that solve (ITER: max_iter; with EPS: where it stopped) */
    int32_t solves;          /* levels * warps */
    int32_t down_launches;   /* k_pyr_down: levels - 1 */
    int32_t step_launches;   /* k_pyr_step: solves - 1 */
    int32_t total_launches;  /* k_pyr_total */
    int32_t median_launches; /* the median kernel, on behalf of the pyramid */
    int32_t reserved[3];
} hsflow_pyramid_info;
/* HSFLOW_E_ARG: out NULL or its struct_size wrong; HSFLOW_E_STATE: no pyramid solve has succeeded on this context. */
int hsflow_get_pyramid_info(hsflow_ctx *ctx, hsflow_pyramid_info *out);
/* Synchronous copy-out of one level after the last pyramid solve: its frames (curr is the ORIGINAL curr_l, not the warped
 * one) and its total flow, for one pair.  Each pointer may be NULL; strides in bytes (flow: multiples of 4).  This is what
 * lets a caller say which level went wrong.  HSFLOW_E_ARG: level or pair out of range; HSFLOW_E_SIZE: a stride smaller than
 * the level's row; HSFLOW_E_STATE: the context's last solve was not a successful pyramid solve.  (Level 0's planes are the
 * context's own: what changed them since shows.) */
int hsflow_pyramid_get_level(hsflow_ctx *ctx, int level, int pair, uint8_t *prev, size_t prev_stride, uint8_t *curr, size_t curr_stride, float *u,
                             size_t u_stride, float *v, size_t v_stride);

/* Planner introspection, no device needed: the kernel, sweeps per launch, tile shape, workgroup size,
 * tiles per launch, LDS bytes and launch count hsflow_solve would use for a context of this size with
 * these parameters (same code path as the solver's own planning; text of a refusal in
 * hsflow_last_error(NULL)).  info->struct_size must be set. */
int hsflow_plan_query(int width, int height, int n_pairs, const hsflow_params *params, hsflow_info *info);

/* --- one-shot ------------------------------------------------------------------------------ */

/* Same argument list as OpenCV's inner routine behind cvCalcOpticalFlowHS: strides in bytes,
 * term_type/max_iter/epsilon = CvTermCriteria.  Uploads, solves and downloads on device 0, on a
 * context the library keeps between calls while width and height stay the same (the reference
 * calls cvCalcOpticalFlowHS once per camera frame, OpticalFlowOpenCV.cpp:94); serialised by a
 * mutex.  use_previous != 0 reads velx/vely as the starting flow. */
int hsflow_calc_optical_flow_hs_8u32f(const uint8_t *prev, const uint8_t *curr, int img_step,
                                      int width, int height, int use_previous, float *velx,
                                      float *vely, int vel_step, float lambda, int term_type,
                                      int max_iter, double epsilon);

/* Frees the context kept by hsflow_calc_optical_flow_hs_8u32f (optional; e.g. before unloading). */
void hsflow_release_cached(void);

#ifdef __cplusplus
}
#endif
#endif /* HSFLOW_H_ */
