"""opticalflowhs_amd -- MI355X-native Horn-Schunck optical flow (hot path of miczi/OpticalFlowHS).

Layout: csrc/ holds the HIP kernels and the C ABI (include/hsflow.h); solver.py is the host-side
mirror of the reference interface; pipeline.py streams pairs through one GPU with overlapped copies, slab.py is the multi-GPU row-slab driver.  The package has
no CPU fallback: importing it without libhsflow.so raises.
"""
from . import _lib
from ._lib import (COLOR_SCALE_AUTO, COLOR_SCALE_FIXED, WARP_BORDER_CONSTANT, WARP_BORDER_REPLICATE, FB_CONSISTENT, FB_INCONSISTENT, FB_OUTSIDE, FB_UNKNOWN, CHAIN_ALIVE, CHAIN_LEFT, CHAIN_UNTRUSTED, CHAIN_UNKNOWN, CHAIN_MAX_PAIRS, HsflowChainParams, HsflowChainStats, MEDIAN_FILTER, MEDIAN_FILL, MEDIAN_UNFILLED, MEDIAN_KEPT, MEDIAN_FILLED, MEDIAN_MAX_PASSES, HsflowMedianParams, HsflowMedianStats, HsflowInterpParams, HsflowInterpStats, HsflowPyramidParams, HsflowPyramidInfo, PYRAMID_MAX_LEVELS, PYRAMID_MAX_WARPS, INTERP_BLENDED, INTERP_PREV_ONLY, INTERP_CURR_ONLY, INTERP_CLAMPED, INTERP_BATCH_MAX, HsflowColorParams, HsflowWarpParams, HsflowWarpStats, HsflowFbParams, HsflowFbStats, HsflowError, HsflowPairResult, HsflowPlaneDiff, HsflowVerifyReport, VERIFY_TINY, PRE_STRIP_ROWS, JPEGD_BATCH_MAX, JPEG_BATCH_MAX, PRE_SEQ_MAX, SEQ_REBLUR, SEQ_REBLUR_FIRST, RENDER_CL, RENDER_CV, KERNEL_AUTO, KERNEL_FUSED, KERNEL_SIMPLE, KERNEL_STRIP, KERNEL_FOLD, KERNEL_PERSIST, MODE_CLASSIC, MODE_CLASSIC_AS_SHIPPED, MODE_CV,
                   TERM_EPS, TERM_ITER)
from .solver import HSFlow, TermCriteria, calc_optical_flow_hs, color_flow_host, compare_planes, make_color_params, make_warp_params, warp_host, warp_stats_from, make_fb_params, fb_host, fb_stats_from, make_chain_params, chain_flow_host, track_points_host, chain_stats_from, make_median_params, median_host, median_stats_from, make_interp_params, interp_host, project_flow_host, interp_stats_from, make_pyramid_params, pyramid_plan, pyramid_down_host, pyramid_prolong_host, encode_jpeg, jpeg_bound, jpeg_decode_host, jpeg_read_header, make_params, make_render_params, plan_query, preprocess_frame, preprocess_sequence, term_criteria
from .pipeline import PairPipeline, pinned_empty
from .multi import MultiPairs, SlabFrame

__all__ = ["HSFlow", "PairPipeline", "MultiPairs", "SlabFrame", "pinned_empty", "make_params", "make_render_params", "make_color_params", "make_warp_params", "warp_host", "warp_stats_from", "WARP_BORDER_CONSTANT", "WARP_BORDER_REPLICATE", "HsflowWarpParams", "HsflowWarpStats", "make_interp_params", "interp_host", "project_flow_host", "interp_stats_from", "HsflowInterpParams", "HsflowInterpStats", "INTERP_BLENDED", "INTERP_PREV_ONLY", "INTERP_CURR_ONLY", "INTERP_CLAMPED", "INTERP_BATCH_MAX", "make_pyramid_params", "pyramid_plan", "pyramid_down_host", "pyramid_prolong_host", "HsflowPyramidParams", "HsflowPyramidInfo", "PYRAMID_MAX_LEVELS", "PYRAMID_MAX_WARPS", "make_fb_params", "fb_host", "fb_stats_from", "FB_CONSISTENT", "FB_INCONSISTENT", "FB_OUTSIDE", "FB_UNKNOWN", "HsflowFbParams", "HsflowFbStats", "make_chain_params", "chain_flow_host", "track_points_host", "chain_stats_from", "CHAIN_ALIVE", "CHAIN_LEFT", "CHAIN_UNTRUSTED", "CHAIN_UNKNOWN", "CHAIN_MAX_PAIRS", "HsflowChainParams", "HsflowChainStats", "make_median_params", "median_host", "median_stats_from", "MEDIAN_FILTER", "MEDIAN_FILL", "MEDIAN_UNFILLED", "MEDIAN_KEPT", "MEDIAN_FILLED", "MEDIAN_MAX_PASSES", "HsflowMedianParams", "HsflowMedianStats", "color_flow_host", "COLOR_SCALE_AUTO", "COLOR_SCALE_FIXED", "HsflowColorParams", "plan_query", "compare_planes", "preprocess_frame", "preprocess_sequence", "encode_jpeg", "jpeg_bound", "jpeg_decode_host", "jpeg_read_header", "PRE_STRIP_ROWS", "JPEGD_BATCH_MAX", "JPEG_BATCH_MAX", "PRE_SEQ_MAX", "SEQ_REBLUR", "SEQ_REBLUR_FIRST", "HsflowPlaneDiff", "HsflowPairResult", "HsflowVerifyReport", "VERIFY_TINY", "RENDER_CV", "RENDER_CL", "TermCriteria", "term_criteria", "calc_optical_flow_hs", "HsflowError",
           "TERM_ITER", "TERM_EPS", "MODE_CV", "MODE_CLASSIC", "MODE_CLASSIC_AS_SHIPPED", "KERNEL_AUTO", "KERNEL_SIMPLE",
           "KERNEL_FUSED", "KERNEL_STRIP", "KERNEL_FOLD", "KERNEL_PERSIST", "OP_SLOTS_PER_PIXEL_SWEEP"]

# Wave64 VALU lane-operations one pixel costs per Jacobi sweep in the multi-sweep kernels' arithmetic (csrc/hs_kernels_strip.hip.h,
# cross_rows + strip_row_update): 2 + 2 additions for the two neighbour sums (one shared diagonal cross sum and one combining
# addition per plane), 4 fused multiply-adds for the update, 1 multiplication that carries the constant term to the next sweep's
# scale.  bench.py prices the VALU-issue roofline with it.  The straightforward form of the same update (3 + 3 additions, round 1)
# costs 11; bench.py reports the fraction at that accounting beside it so that rounds stay comparable.
OP_SLOTS_PER_PIXEL_SWEEP = 9
OP_SLOTS_PER_PIXEL_SWEEP_STRAIGHTFORWARD = 11

_lib.load()  # fail loudly at import time if the HIP library is absent
