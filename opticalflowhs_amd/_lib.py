"""ctypes binding of libhsflow.so (the C ABI declared in include/hsflow.h).

There is NO fallback: if the HIP library is missing or a symbol is absent this raises.  The
product path never touches oracle/.
"""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HSFLOW_LIB_PATH") or os.path.join(HERE, "libhsflow.so")  # override: diagnostic builds

# status codes / enums of include/hsflow.h
OK, E_ARG, E_SIZE, E_DEVICE, E_OOM, E_STATE, E_NOTERM, E_DATA = range(8)
TERM_ITER, TERM_EPS = 1, 2
MODE_CV, MODE_CLASSIC, MODE_CLASSIC_AS_SHIPPED = 0, 1, 2
KERNEL_AUTO, KERNEL_SIMPLE, KERNEL_FUSED, KERNEL_STRIP, KERNEL_FOLD, KERNEL_PERSIST = 0, 1, 2, 3, 4, 5
FRAMES_GRAY8, FRAMES_GRAY8_BLUR, FRAMES_BGR8, FRAMES_BGR8_BLUR = 0, 1, 2, 3
RENDER_CV, RENDER_CL = 0, 1
COLOR_SCALE_AUTO, COLOR_SCALE_FIXED = 0, 1
WARP_BORDER_CONSTANT, WARP_BORDER_REPLICATE = 0, 1
FB_CONSISTENT, FB_INCONSISTENT, FB_OUTSIDE, FB_UNKNOWN = 0, 1, 2, 3
CHAIN_ALIVE, CHAIN_LEFT, CHAIN_UNTRUSTED, CHAIN_UNKNOWN = 0, 1, 2, 3  # HSFLOW_CHAIN_*
CHAIN_MAX_PAIRS = 32  # HSFLOW_CHAIN_MAX_PAIRS
GMOTION_TRANSLATION, GMOTION_SIMILARITY, GMOTION_AFFINE, GMOTION_ZERO = 0, 1, 2, 3  # HSFLOW_GMOTION_*
GMOTION_THRESHOLD_FIXED, GMOTION_THRESHOLD_AUTO = 0, 1
GMOTION_INLIER, GMOTION_OUTLIER, GMOTION_UNTRUSTED, GMOTION_UNKNOWN = 0, 1, 2, 3
GMOTION_MAX_PASSES, GMOTION_MAX_SIDE, GMOTION_FLAG_FALLBACK = 8, 16384, 1
REGIONS_MAX_SIDE, REGIONS_FLAG_OVERFLOW = 16384, 1  # HSFLOW_REGIONS_*
MEDIAN_FILTER, MEDIAN_FILL = 0, 1
MEDIAN_UNFILLED, MEDIAN_KEPT, MEDIAN_FILLED = 0, 1, 2
MEDIAN_MAX_PASSES = 64  # HSFLOW_MEDIAN_MAX_PASSES
INTERP_BLENDED, INTERP_PREV_ONLY, INTERP_CURR_ONLY, INTERP_CLAMPED = 0, 1, 2, 3
INTERP_BATCH_MAX = 8  # HSFLOW_INTERP_BATCH_MAX
PYRAMID_MAX_LEVELS, PYRAMID_MAX_WARPS = 8, 8  # HSFLOW_PYRAMID_MAX_LEVELS, HSFLOW_PYRAMID_MAX_WARPS
JPEG_ORDER_BGR, JPEG_ORDER_RGB = 0, 1
JPEGD_SUBSEQ_BITS = 1024  # HSFLOW_JPEGD_SUBSEQ_BITS
JPEGD_BATCH_MAX = 32  # HSFLOW_JPEGD_BATCH_MAX
JPEG_BATCH_MAX = 16  # HSFLOW_JPEG_BATCH_MAX
SEQ_REBLUR, SEQ_REBLUR_FIRST = 1, 2  # HSFLOW_SEQ_*
PRE_SEQ_MAX = 32  # HSFLOW_PRE_SEQ_MAX
FRAME_FORMATS = {"gray": FRAMES_GRAY8, "gray_blur": FRAMES_GRAY8_BLUR, "bgr": FRAMES_BGR8, "bgr_blur": FRAMES_BGR8_BLUR}


class HsflowParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("mode", ctypes.c_int32),
                ("lambda_", ctypes.c_float), ("alpha", ctypes.c_float),
                ("term_type", ctypes.c_int32), ("max_iter", ctypes.c_int32),
                ("epsilon", ctypes.c_double), ("use_previous", ctypes.c_int32),
                ("kernel", ctypes.c_int32), ("fuse_steps", ctypes.c_int32),
                ("tile_w", ctypes.c_int32), ("tile_h", ctypes.c_int32),
                ("threads", ctypes.c_int32), ("strip_rows", ctypes.c_int32),
                ("reuse_derivatives", ctypes.c_int32), ("use_graph", ctypes.c_int32),
                ("profile", ctypes.c_int32)]


class HsflowInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("width", ctypes.c_int32),
                ("height", ctypes.c_int32), ("n_pairs", ctypes.c_int32), ("pitch", ctypes.c_int32),
                ("iterations_done", ctypes.c_int32), ("last_eps", ctypes.c_float),
                ("kernel", ctypes.c_int32), ("fuse_steps", ctypes.c_int32),
                ("tile_w", ctypes.c_int32), ("tile_h", ctypes.c_int32), ("threads", ctypes.c_int32),
                ("groups_per_thread", ctypes.c_int32), ("tiles", ctypes.c_int32),
                ("lds_bytes", ctypes.c_int32), ("jacobi_launches", ctypes.c_int32),
                ("deriv_ms", ctypes.c_float), ("jacobi_ms", ctypes.c_float),
                ("solve_ms", ctypes.c_float), ("eps_rerun", ctypes.c_int32),
                ("deriv_fused", ctypes.c_int32), ("persistent", ctypes.c_int32)]


class HsflowRenderParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("step", ctypes.c_int32),
                ("threshold", ctypes.c_float), ("scale", ctypes.c_float),
                ("dot_rgb", ctypes.c_uint8 * 3), ("line_rgb", ctypes.c_uint8 * 3), ("pad", ctypes.c_uint8 * 2)]


class HsflowColorParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("scale_mode", ctypes.c_int32), ("max_flow", ctypes.c_float), ("reserved", ctypes.c_int32)]


class HsflowWarpParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("channels", ctypes.c_int32), ("border", ctypes.c_int32), ("t", ctypes.c_float),
                ("fill", ctypes.c_uint8 * 4)]


class HsflowWarpStats(ctypes.Structure):
    _fields_ = [("inside", ctypes.c_uint64), ("outside", ctypes.c_uint64), ("unknown", ctypes.c_uint64), ("sad_warped", ctypes.c_uint64),
                ("sad_plain", ctypes.c_uint64), ("max_warped", ctypes.c_uint32), ("max_plain", ctypes.c_uint32), ("reserved", ctypes.c_uint8 * 16)]


class HsflowFbParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("alpha", ctypes.c_float), ("beta", ctypes.c_float), ("value", ctypes.c_uint8 * 4)]


class HsflowFbStats(ctypes.Structure):
    _fields_ = [("consistent", ctypes.c_uint64), ("inconsistent", ctypes.c_uint64), ("outside", ctypes.c_uint64), ("unknown", ctypes.c_uint64),
                ("sum_err2_q", ctypes.c_uint64), ("max_err2_bits", ctypes.c_uint32), ("reserved", ctypes.c_uint8 * 20)]


class HsflowChainParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("value", ctypes.c_uint8 * 4), ("reserved", ctypes.c_int32 * 2)]


class HsflowChainStats(ctypes.Structure):
    _fields_ = [("cls", ctypes.c_uint64 * 4), ("sum_age", ctypes.c_uint64), ("max_mag2_bits", ctypes.c_uint32), ("reserved", ctypes.c_uint8 * 20)]


assert ctypes.sizeof(HsflowChainParams) == 16 and ctypes.sizeof(HsflowChainStats) == 64


class HsflowGmotionParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("model", ctypes.c_int32), ("passes", ctypes.c_int32), ("threshold_mode", ctypes.c_int32),
                ("inlier_px", ctypes.c_float), ("scale2", ctypes.c_float), ("min_thr2", ctypes.c_float), ("value", ctypes.c_uint8 * 4),
                ("reserved", ctypes.c_int32 * 2)]


class HsflowGmotionResult(ctypes.Structure):
    _fields_ = [("p", ctypes.c_float * 6), ("threshold", ctypes.c_float), ("flags", ctypes.c_uint32), ("cls", ctypes.c_uint64 * 4)]

    def as_dict(self):
        return {"p": [float(x) for x in self.p], "threshold": float(self.threshold), "flags": int(self.flags),
                "fallback": bool(self.flags & GMOTION_FLAG_FALLBACK), "used": (int(self.flags) >> 8) & 3, "cls": [int(x) for x in self.cls]}


assert ctypes.sizeof(HsflowGmotionParams) == 40 and ctypes.sizeof(HsflowGmotionResult) == 64


class HsflowRegionsParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("connectivity", ctypes.c_int32), ("fg_lo", ctypes.c_int32), ("fg_hi", ctypes.c_int32),
                ("min_area", ctypes.c_uint32), ("join_px", ctypes.c_float), ("reserved", ctypes.c_int32 * 2)]


class HsflowRegionsRecord(ctypes.Structure):
    _fields_ = [("root", ctypes.c_uint32), ("area", ctypes.c_uint32), ("x0", ctypes.c_uint16), ("y0", ctypes.c_uint16), ("x1", ctypes.c_uint16),
                ("y1", ctypes.c_uint16), ("sum_x", ctypes.c_uint64), ("sum_y", ctypes.c_uint64), ("n_flow", ctypes.c_uint32), ("reserved0", ctypes.c_uint32),
                ("sum_qu", ctypes.c_int64), ("sum_qv", ctypes.c_int64), ("reserved1", ctypes.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class HsflowRegionsResult(ctypes.Structure):
    _fields_ = [("n_regions", ctypes.c_uint32), ("n_written", ctypes.c_uint32), ("n_dropped", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("fg_px", ctypes.c_uint64), ("dropped_px", ctypes.c_uint64), ("unknown_flow_px", ctypes.c_uint64), ("largest_area", ctypes.c_uint32),
                ("largest_label", ctypes.c_uint32), ("reserved", ctypes.c_uint64 * 2)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}
        d["overflow"] = bool(self.flags & REGIONS_FLAG_OVERFLOW)
        return d


assert ctypes.sizeof(HsflowRegionsParams) == 32 and ctypes.sizeof(HsflowRegionsRecord) == 64 and ctypes.sizeof(HsflowRegionsResult) == 64


CORNERS_MIN_EIGEN = 0             # HSFLOW_CORNERS_MIN_EIGEN
CORNERS_HARRIS = 1                # HSFLOW_CORNERS_HARRIS
CORNERS_MAX_SIDE = 16384          # HSFLOW_CORNERS_MAX_SIDE
CORNERS_MAX_CANDIDATES = 65536    # HSFLOW_CORNERS_MAX_CANDIDATES
CORNERS_MAX_CAPACITY = 1 << 24    # HSFLOW_CORNERS_MAX_CAPACITY
CORNERS_FLAG_OVERFLOW = 1         # HSFLOW_CORNERS_FLAG_OVERFLOW
CORNERS_FLAG_TRUNCATED = 2        # HSFLOW_CORNERS_FLAG_TRUNCATED


class HsflowCornersParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("kind", ctypes.c_int32), ("block_r", ctypes.c_int32), ("nms_r", ctypes.c_int32),
                ("quality_q16", ctypes.c_uint32), ("border", ctypes.c_int32), ("fg_lo", ctypes.c_int32), ("fg_hi", ctypes.c_int32),
                ("max_candidates", ctypes.c_uint32), ("reserved0", ctypes.c_uint32), ("min_score", ctypes.c_int64), ("reserved", ctypes.c_uint64 * 2)]


class HsflowCornersRecord(ctypes.Structure):
    _fields_ = [("x", ctypes.c_uint16), ("y", ctypes.c_uint16), ("index", ctypes.c_uint32), ("score", ctypes.c_int64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class HsflowCornersResult(ctypes.Structure):
    _fields_ = [("n_survivors", ctypes.c_uint32), ("n_candidates", ctypes.c_uint32), ("n_written", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("smax", ctypes.c_int64), ("threshold", ctypes.c_int64), ("allowed_px", ctypes.c_uint64), ("strong_px", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64 * 2)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}
        d["overflow"] = bool(self.flags & CORNERS_FLAG_OVERFLOW)
        d["truncated"] = bool(self.flags & CORNERS_FLAG_TRUNCATED)
        return d


assert ctypes.sizeof(HsflowCornersParams) == 64 and ctypes.sizeof(HsflowCornersRecord) == 16 and ctypes.sizeof(HsflowCornersResult) == 64


LINK_MAX_CELLS = 1 << 24  # HSFLOW_LINK_MAX_CELLS
LINK_FLAG_OVERFLOW = 1    # HSFLOW_LINK_FLAG_OVERFLOW


class HsflowLinkParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("cap_a", ctypes.c_uint32), ("cap_b", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class HsflowLinkRecord(ctypes.Structure):
    _fields_ = [("a", ctypes.c_uint32), ("b", ctypes.c_uint32), ("px", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class HsflowLinkSide(ctypes.Structure):
    _fields_ = [("px", ctypes.c_uint32), ("n_links", ctypes.c_uint32), ("best", ctypes.c_uint32), ("best_px", ctypes.c_uint32),
                ("gone_px", ctypes.c_uint32), ("unmatched_px", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class HsflowLinkResult(ctypes.Structure):
    _fields_ = [("n_links", ctypes.c_uint32), ("n_written", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("n_mutual", ctypes.c_uint32),
                ("voted_px", ctypes.c_uint64), ("gone_px", ctypes.c_uint64), ("unmatched_px", ctypes.c_uint64), ("over_a_px", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64 * 2)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}
        d["overflow"] = bool(self.flags & LINK_FLAG_OVERFLOW)
        return d


assert ctypes.sizeof(HsflowLinkParams) == 16 and ctypes.sizeof(HsflowLinkRecord) == 16 and ctypes.sizeof(HsflowLinkSide) == 32 and ctypes.sizeof(HsflowLinkResult) == 64


class HsflowMedianParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("radius", ctypes.c_int32), ("mode", ctypes.c_int32), ("min_votes", ctypes.c_int32)]


class HsflowMedianStats(ctypes.Structure):
    _fields_ = [("kept", ctypes.c_uint64), ("filled", ctypes.c_uint64), ("unfilled", ctypes.c_uint64), ("newly_filled", ctypes.c_uint64),
                ("changed", ctypes.c_uint64), ("reserved", ctypes.c_uint8 * 24)]


class HsflowInterpParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("channels", ctypes.c_int32), ("fill_radius", ctypes.c_int32), ("fill_min_votes", ctypes.c_int32),
                ("fill_passes", ctypes.c_int32)]


class HsflowInterpStats(ctypes.Structure):
    _fields_ = [("blended", ctypes.c_uint64), ("prev_only", ctypes.c_uint64), ("curr_only", ctypes.c_uint64), ("clamped", ctypes.c_uint64),
                ("sad", ctypes.c_uint64), ("holes", ctypes.c_uint32), ("unfilled", ctypes.c_uint32), ("collisions", ctypes.c_uint32),
                ("left", ctypes.c_uint32), ("unknown", ctypes.c_uint32), ("max_diff", ctypes.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class HsflowPyramidParams(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("levels", ctypes.c_int32), ("min_size", ctypes.c_int32), ("warps", ctypes.c_int32),
                ("median_radius", ctypes.c_int32)]


class HsflowPyramidInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("levels", ctypes.c_int32), ("warps", ctypes.c_int32), ("median_radius", ctypes.c_int32),
                ("width", ctypes.c_int32 * PYRAMID_MAX_LEVELS), ("height", ctypes.c_int32 * PYRAMID_MAX_LEVELS),
                ("sweeps", (ctypes.c_int32 * PYRAMID_MAX_WARPS) * PYRAMID_MAX_LEVELS), ("solves", ctypes.c_int32), ("down_launches", ctypes.c_int32),
                ("step_launches", ctypes.c_int32), ("total_launches", ctypes.c_int32), ("median_launches", ctypes.c_int32), ("reserved", ctypes.c_int32 * 3)]


class HsflowPlaneDiff(ctypes.Structure):
    _fields_ = [("differing", ctypes.c_uint64), ("failing", ctypes.c_uint64), ("nonfinite", ctypes.c_uint64),
                ("first_failing", ctypes.c_int64), ("max_abs_diff", ctypes.c_float), ("max_ulp", ctypes.c_uint32)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class HsflowVerifyReport(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("ok", ctypes.c_int32), ("pair", ctypes.c_int32),
                ("iterations_done", ctypes.c_int32), ("iterations_ref", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("u", HsflowPlaneDiff), ("v", HsflowPlaneDiff),
                ("deriv_differing", ctypes.c_uint64), ("deriv_first", ctypes.c_int64)]


class HsflowPairResult(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("pair", ctypes.c_int32), ("status", ctypes.c_int32),
                ("iterations_done", ctypes.c_int32), ("last_eps", ctypes.c_float), ("eps_rerun", ctypes.c_int32),
                ("sweeps_executed", ctypes.c_int64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


class HsflowJpegInfo(ctypes.Structure):
    _fields_ = [("struct_size", ctypes.c_uint32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("components", ctypes.c_int32),
                ("h_samp", ctypes.c_int32), ("v_samp", ctypes.c_int32), ("restart_interval", ctypes.c_int32), ("subseq_bits", ctypes.c_int32),
                ("blocks", ctypes.c_int64), ("scan_offset", ctypes.c_uint64), ("scan_bytes", ctypes.c_uint64)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "struct_size"}


VERIFY_TINY = 1e-30  # HSFLOW_VERIFY_TINY
PAIR_STOP_SIMPLE_CHUNK = 32  # HSFLOW_PAIR_STOP_SIMPLE_CHUNK
PRE_STRIP_ROWS = 8  # HSFLOW_PRE_STRIP_ROWS

_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
_pp = ctypes.POINTER(HsflowParams)
_rp = ctypes.POINTER(HsflowRenderParams)
_cp = ctypes.POINTER(HsflowColorParams)
_fp = ctypes.POINTER(ctypes.c_float)
_wp = ctypes.POINTER(HsflowWarpParams)
_ws = ctypes.POINTER(HsflowWarpStats)
_bp = ctypes.POINTER(HsflowFbParams)
_bs = ctypes.POINTER(HsflowFbStats)
_ip = ctypes.POINTER(ctypes.c_int)
_mp = ctypes.POINTER(HsflowMedianParams)
_ms = ctypes.POINTER(HsflowMedianStats)
_np = ctypes.POINTER(HsflowInterpParams)
_ns = ctypes.POINTER(HsflowInterpStats)
_yp = ctypes.POINTER(HsflowPyramidParams)
_hp = ctypes.POINTER(HsflowChainParams)
_hs = ctypes.POINTER(HsflowChainStats)
_gp = ctypes.POINTER(HsflowGmotionParams)
_gr = ctypes.POINTER(HsflowGmotionResult)
_rgp = ctypes.POINTER(HsflowRegionsParams)
_rgr = ctypes.POINTER(HsflowRegionsResult)
_cnp = ctypes.POINTER(HsflowCornersParams)
_cnr = ctypes.POINTER(HsflowCornersResult)
_lnp = ctypes.POINTER(HsflowLinkParams)
_lnr = ctypes.POINTER(HsflowLinkResult)
_f = ctypes.c_float
_dp = ctypes.POINTER(HsflowPlaneDiff)
_vr = ctypes.POINTER(HsflowVerifyReport)
_ji = ctypes.POINTER(HsflowJpegInfo)

# name -> (restype, argtypes).  tests/test_abi.py checks this table against include/hsflow.h.
PROTOTYPES = {
    "hsflow_default_params": (None, [_pp]),
    "hsflow_create": (_i, [ctypes.POINTER(_vp), _i, _i, _i, _i, _vp, _i]),
    "hsflow_destroy": (_i, [_vp]),
    "hsflow_set_row_origin": (_i, [_vp, _i]),
    "hsflow_set_cu_share": (_i, [_vp, _i]),
    "hsflow_set_async_reduce": (_i, [_vp, _i]),
    "hsflow_set_eps_rows": (_i, [_vp, _i, _i]),
    "hsflow_solve_probe": (_i, [_vp, _pp, ctypes.POINTER(ctypes.c_float)]),
    "hsflow_solve_probe_pairs": (_i, [_vp, _pp, ctypes.POINTER(ctypes.c_float)]),
    "hsflow_set_pair_termination": (_i, [_vp, _i]),
    "hsflow_get_pair_result": (_i, [_vp, _i, ctypes.POINTER(HsflowPairResult)]),
    "hsflow_take_verdict": (_i, [_vp, ctypes.POINTER(_i)]),
    "hsflow_set_frames_u8": (_i, [_vp, _i, _vp, _sz, _vp, _sz]),
    "hsflow_set_frames_u8_async": (_i, [_vp, _i, _vp, _sz, _vp, _sz]),
    "hsflow_set_frames_u8_device": (_i, [_vp, _i, _vp, _sz, _vp, _sz]),
    "hsflow_set_frames_bgr8": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _i]),
    "hsflow_set_frames_gray8_blur": (_i, [_vp, _i, _vp, _sz, _vp, _sz]),
    "hsflow_set_frames_bgr8_async": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _i]),
    "hsflow_set_frames_gray8_blur_async": (_i, [_vp, _i, _vp, _sz, _vp, _sz]),
    "hsflow_push_frame_u8": (_i, [_vp, _i, _vp, _sz]),
    "hsflow_set_frames_device_ex": (_i, [_vp, _i, _i, _vp, _sz, _vp, _sz]),
    "hsflow_push_frame_ex": (_i, [_vp, _i, _i, _vp, _sz, _i]),
    "hsflow_push_frame_device_ex": (_i, [_vp, _i, _i, _vp, _sz, _i]),
    "hsflow_preprocess_frame_host": (_i, [_i, _vp, _sz, _i, _i, _vp, _sz]),
    "hsflow_solve": (_i, [_vp, _pp]),
    "hsflow_solve_async": (_i, [_vp, _pp]),
    "hsflow_solve_async_frames_device": (_i, [_vp, _vp, _sz, _vp, _sz, _pp]),
    "hsflow_frame_copies_elided": (_i, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "hsflow_synchronize": (_i, [_vp]),
    "hsflow_wait_solve": (_i, [_vp]),
    "hsflow_get_flow": (_i, [_vp, _i, _vp, _sz, _vp, _sz]),
    "hsflow_get_flow_async": (_i, [_vp, _i, _vp, _sz, _vp, _sz]),
    "hsflow_flow_view_device": (_i, [_vp, _i, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_sz)]),
    "hsflow_get_flow_device": (_i, [_vp, _i, _i, _i, _vp, _sz, _vp, _sz]),
    "hsflow_set_flow_device": (_i, [_vp, _i, _i, _i, _vp, _sz, _vp, _sz]),
    "hsflow_set_flow_device_ex": (_i, [_vp, _i, _i, _i, _vp, _sz, _vp, _sz, _i]),
    "hsflow_get_derivatives": (_i, [_vp, _i, _vp, _vp, _vp, _sz]),
    "hsflow_get_frames_u8": (_i, [_vp, _i, _vp, _sz, _vp, _sz]),
    "hsflow_default_render_params": (None, [_rp, _i]),
    "hsflow_render_flow_device": (_i, [_vp, _i, _rp, _vp, _sz]),
    "hsflow_render_flow": (_i, [_vp, _i, _rp, _vp, _sz]),
    "hsflow_jpeg_bound": (_sz, [_i, _i]),
    "hsflow_jpeg_encode_host": (_i, [_vp, _sz, _i, _i, _i, _vp, _sz, ctypes.POINTER(_sz)]),
    "hsflow_jpeg_encode_device": (_i, [_vp, _vp, _sz, _i, _vp, _sz, _vp]),
    "hsflow_render_flow_jpeg_device": (_i, [_vp, _i, _rp, _i, _vp, _sz, _vp]),
    "hsflow_render_flow_jpeg": (_i, [_vp, _i, _rp, _i, _vp, _sz, ctypes.POINTER(_sz)]),
    "hsflow_jpeg_encode_batch_device": (_i, [_vp, _vp, _i, _sz, _i, _vp, _sz, _vp]),
    "hsflow_render_flow_batch_device": (_i, [_vp, _i, _i, _rp, _vp, _sz]),
    "hsflow_render_flow_jpeg_batch_device": (_i, [_vp, _i, _i, _rp, _i, _vp, _sz, _vp]),
    "hsflow_render_flow_jpeg_batch": (_i, [_vp, _i, _i, _rp, _i, _vp, _sz, ctypes.POINTER(_sz)]),
    "hsflow_default_color_params": (None, [_cp]),
    "hsflow_color_flow_host": (_i, [_vp, _sz, _vp, _sz, _i, _i, _cp, _vp, _sz, _fp]),
    "hsflow_color_flow_batch_device": (_i, [_vp, _i, _i, _cp, _vp, _sz]),
    "hsflow_color_flow_device": (_i, [_vp, _i, _cp, _vp, _sz]),
    "hsflow_color_flow": (_i, [_vp, _i, _cp, _vp, _sz, _fp]),
    "hsflow_color_flow_jpeg_batch_device": (_i, [_vp, _i, _i, _cp, _i, _vp, _sz, _vp]),
    "hsflow_color_flow_jpeg_batch": (_i, [_vp, _i, _i, _cp, _i, _vp, _sz, ctypes.POINTER(_sz)]),
    "hsflow_color_flow_jpeg_device": (_i, [_vp, _i, _cp, _i, _vp, _sz, _vp]),
    "hsflow_color_flow_jpeg": (_i, [_vp, _i, _cp, _i, _vp, _sz, ctypes.POINTER(_sz)]),
    "hsflow_default_warp_params": (None, [_wp]),
    "hsflow_warp_host": (_i, [_vp, _sz, _vp, _sz, _i, _i, _wp, _vp, _sz, _vp, _sz, _vp, _sz, _ws]),
    "hsflow_warp_batch_device": (_i, [_vp, _i, _i, _wp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_warp_device": (_i, [_vp, _i, _wp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_warp": (_i, [_vp, _i, _wp, _vp, _sz, _vp, _sz, _vp, _sz, _ws]),
    "hsflow_default_fb_params": (None, [_bp]),
    "hsflow_fb_host": (_i, [_vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _i, _i, _bp, _vp, _sz, _vp, _sz, _bs]),
    "hsflow_fb_batch_device": (_i, [_vp, _i, _ip, _ip, _bp, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_fb_device": (_i, [_vp, _i, _i, _bp, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_fb_planes_device": (_i, [_vp, _i, _vp, _vp, _sz, _bp, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_fb": (_i, [_vp, _i, _i, _bp, _vp, _sz, _vp, _sz, _bs]),
    "hsflow_fb_planes": (_i, [_vp, _i, _vp, _vp, _sz, _bp, _vp, _sz, _vp, _sz, _bs]),
    "hsflow_set_frames_reversed": (_i, [_vp, _i, _i]),
    "hsflow_default_median_params": (None, [_mp]),
    "hsflow_median_host": (_i, [_vp, _sz, _vp, _sz, _vp, _sz, _i, _i, _mp, _i, _vp, _vp, _sz, _vp, _sz, _ms]),
    "hsflow_median_batch_device": (_i, [_vp, _i, _i, _mp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_median_device": (_i, [_vp, _i, _mp, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_median_planes_device": (_i, [_vp, _mp, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_median_apply": (_i, [_vp, _i, _mp, _i, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_median": (_i, [_vp, _i, _mp, _i, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _ms]),
    "hsflow_default_interp_params": (None, [_np]),
    "hsflow_project_flow_host": (_i, [_vp, _sz, _vp, _sz, _i, _i, _f, _np, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _ns]),
    "hsflow_interp_host": (_i, [_vp, _sz, _vp, _sz, _i, _i, _f, _np, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _ns]),
    "hsflow_interp_batch_device": (_i, [_vp, _i, _i, _fp, _np, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_interp_device": (_i, [_vp, _i, _f, _np, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_interp": (_i, [_vp, _i, _f, _np, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _ns]),
    "hsflow_project_flow_device": (_i, [_vp, _i, _f, _np, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_default_pyramid_params": (None, [_yp]),
    "hsflow_default_chain_params": (None, [_hp]),
    "hsflow_chain_flow_host": (_i, [_i, _vp, _vp, _sz, _vp, _sz, _i, _i, _vp, _vp, _sz, _hp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _hs]),
    "hsflow_track_points_host": (_i, [_i, _vp, _vp, _sz, _vp, _sz, _i, _i, _hp, _vp, _i, _vp, _vp, _vp, _vp, _hs]),
    "hsflow_chain_planes_device": (_i, [_vp, _i, _vp, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _hp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_chain_flow_device": (_i, [_vp, _ip, _i, _vp, _sz, _vp, _vp, _sz, _hp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_chain_flow": (_i, [_vp, _ip, _i, _vp, _sz, _vp, _vp, _sz, _hp, _vp, _vp, _sz, _vp, _sz, _vp, _sz, _hs]),
    "hsflow_track_points_device": (_i, [_vp, _ip, _i, _vp, _sz, _hp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "hsflow_track_points": (_i, [_vp, _ip, _i, _vp, _sz, _hp, _vp, _i, _vp, _vp, _vp, _vp, _hs]),
    "hsflow_default_gmotion_params": (None, [_gp]),
    "hsflow_gmotion_fit_host": (_i, [_vp, _vp, _sz, _vp, _sz, _i, _i, _gp, _vp, _sz, _vp, _vp, _sz, _gr]),
    "hsflow_gmotion_fit_planes_device": (_i, [_vp, _vp, _vp, _sz, _vp, _sz, _gp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "hsflow_gmotion_fit_batch_device": (_i, [_vp, _i, _i, _vp, _sz, _gp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "hsflow_gmotion_fit_device": (_i, [_vp, _i, _vp, _sz, _gp, _vp, _sz, _vp, _vp, _sz, _vp]),
    "hsflow_gmotion_fit": (_i, [_vp, _i, _vp, _sz, _gp, _vp, _sz, _vp, _vp, _sz, _gr]),
    "hsflow_gmotion_warp_host": (_i, [_fp, _i, _i, _wp, _vp, _sz, _vp, _sz, _vp, _sz, _ws]),
    "hsflow_gmotion_warp_device": (_i, [_vp, _fp, _wp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_gmotion_warp": (_i, [_vp, _fp, _wp, _vp, _sz, _vp, _sz, _vp, _sz, _ws]),
    "hsflow_gmotion_compose_host": (_i, [_fp, _fp, _fp]),
    "hsflow_gmotion_invert_host": (_i, [_fp, _fp]),
    "hsflow_default_regions_params": (None, [_rgp]),
    "hsflow_regions_host": (_i, [_vp, _sz, _vp, _vp, _sz, _i, _i, _rgp, _vp, _sz, _vp, ctypes.c_uint32, _rgr]),
    "hsflow_regions_planes_device": (_i, [_vp, _vp, _sz, _vp, _vp, _sz, _rgp, _vp, _sz, _vp, ctypes.c_uint32, _vp]),
    "hsflow_regions_batch_device": (_i, [_vp, _i, _i, _vp, _sz, _rgp, _vp, _sz, _vp, ctypes.c_uint32, _vp]),
    "hsflow_regions_device": (_i, [_vp, _i, _vp, _sz, _rgp, _vp, _sz, _vp, ctypes.c_uint32, _vp]),
    "hsflow_regions": (_i, [_vp, _i, _vp, _sz, _rgp, _vp, _sz, _vp, ctypes.c_uint32, _rgr]),
    "hsflow_default_corners_params": (None, [_cnp]),
    "hsflow_corners_host": (_i, [_vp, _sz, _i, _i, _vp, _sz, _cnp, _vp, ctypes.c_uint32, _vp, _cnr]),
    "hsflow_corners_planes_device": (_i, [_vp, _vp, _sz, _vp, _sz, _cnp, _vp, ctypes.c_uint32, _vp, _vp]),
    "hsflow_corners_batch_device": (_i, [_vp, _i, _i, _i, _vp, _sz, _cnp, _vp, ctypes.c_uint32, _vp, _vp]),
    "hsflow_corners_device": (_i, [_vp, _i, _i, _vp, _sz, _cnp, _vp, ctypes.c_uint32, _vp, _vp]),
    "hsflow_corners": (_i, [_vp, _i, _i, _vp, _sz, _cnp, _vp, ctypes.c_uint32, _vp, _cnr]),
    "hsflow_default_link_params": (None, [_lnp]),
    "hsflow_link_regions_host": (_i, [_vp, _sz, _vp, _sz, _vp, _vp, _sz, _i, _i, _lnp, _vp, ctypes.c_uint32, _vp, _vp, _lnr]),
    "hsflow_link_regions_planes_device": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _vp, _sz, _lnp, _vp, ctypes.c_uint32, _vp, _vp, _vp]),
    "hsflow_link_regions_batch_device": (_i, [_vp, _i, _i, _vp, _sz, _lnp, _vp, ctypes.c_uint32, _vp, _vp, _vp]),
    "hsflow_link_regions_device": (_i, [_vp, _i, _vp, _vp, _sz, _lnp, _vp, ctypes.c_uint32, _vp, _vp, _vp]),
    "hsflow_link_regions": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _lnp, _vp, ctypes.c_uint32, _vp, _vp, _lnr]),
    "hsflow_link_tracks_host": (_i, [_vp, _vp, _vp, _i, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp]),
    "hsflow_pyramid_plan": (_i, [_i, _i, _yp, _ip, _ip, _ip]),
    "hsflow_pyramid_down_host": (_i, [_vp, _sz, _i, _i, _vp, _sz]),
    "hsflow_pyramid_prolong_host": (_i, [_vp, _sz, _i, _i, _vp, _sz]),
    "hsflow_solve_pyramid": (_i, [_vp, _pp, _yp]),
    "hsflow_get_pyramid_info": (_i, [_vp, ctypes.POINTER(HsflowPyramidInfo)]),
    "hsflow_pyramid_get_level": (_i, [_vp, _i, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz]),
    "hsflow_jpeg_read_header": (_i, [_vp, _sz, _ji]),
    "hsflow_jpeg_decode_host": (_i, [_vp, _sz, _i, _vp, _sz, _ji]),
    "hsflow_jpeg_decode_device": (_i, [_vp, _vp, _sz, _i, _vp, _sz, _vp]),
    "hsflow_jpeg_decode": (_i, [_vp, _vp, _sz, _i, _vp, _sz]),
    "hsflow_set_frames_jpeg": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _i]),
    "hsflow_push_frame_jpeg": (_i, [_vp, _i, _vp, _sz, _i, _i]),
    "hsflow_jpeg_decode_batch_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, _vp]),
    "hsflow_set_sequence_jpeg": (_i, [_vp, _i, _vp, _vp, _i, _i]),
    "hsflow_set_sequence_jpeg_ex": (_i, [_vp, _i, _vp, _vp, _i, _i, _i]),
    "hsflow_set_sequence_device_ex": (_i, [_vp, _i, _i, _vp, _i, _sz, _i]),
    "hsflow_preprocess_sequence_host": (_i, [_i, _i, _vp, _i, _sz, _i, _i, _vp, _vp, _sz]),
    "hsflow_set_frames_jpeg_async": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _i]),
    "hsflow_jpeg_async_status": (_i, [_vp]),
    "hsflow_render_line_pixels": (_i, [_i, _i, _i, _i, _i, _i, ctypes.POINTER(ctypes.c_int32), _i]),
    "hsflow_compare_planes_host": (_i, [_vp, _sz, _vp, _sz, _i, _i, _dp]),
    "hsflow_compare_flow_device": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _dp, _dp]),
    "hsflow_verify": (_i, [_vp, _i, _vr]),
    "hsflow_pipeline_verify": (_i, [_vp, ctypes.c_uint64, _vr]),
    "hsflow_get_info": (_i, [_vp, ctypes.POINTER(HsflowInfo)]),
    "hsflow_get_info_ex": (_i, [_vp, ctypes.POINTER(HsflowInfo), _i]),
    "hsflow_last_error": (ctypes.c_char_p, [_vp]),
    "hsflow_status_string": (ctypes.c_char_p, [_i]),
    "hsflow_version": (_i, []),
    "hsflow_device_count": (_i, [ctypes.POINTER(_i)]),
    "hsflow_release_cached": (None, []),
    "hsflow_plan_query": (_i, [_i, _i, _i, _pp, ctypes.POINTER(HsflowInfo)]),
    "hsflow_host_alloc": (_i, [ctypes.POINTER(_vp), _sz]),
    "hsflow_host_free": (_i, [_vp]),
    "hsflow_host_register": (_i, [_vp, _sz]),
    "hsflow_host_unregister": (_i, [_vp]),
    "hsflow_pipeline_create": (_i, [ctypes.POINTER(_vp), _i, _i, _i, _i]),
    "hsflow_pipeline_create_lanes": (_i, [ctypes.POINTER(_vp), _i, _i, _i, _i, _i]),
    "hsflow_pipeline_destroy": (_i, [_vp]),
    "hsflow_pipeline_submit": (_i, [_vp, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _pp, ctypes.POINTER(ctypes.c_uint64)]),
    "hsflow_pipeline_submit_ex": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _pp, ctypes.POINTER(ctypes.c_uint64)]),
    "hsflow_pipeline_submit_device": (_i, [_vp, _vp, _sz, _vp, _sz, _pp, ctypes.POINTER(ctypes.c_uint64)]),
    "hsflow_pipeline_submit_device_ex": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _pp, ctypes.POINTER(ctypes.c_uint64)]),
    "hsflow_pipeline_submit_jpeg": (_i, [_vp, _vp, _sz, _vp, _sz, _i, _pp, ctypes.POINTER(ctypes.c_uint64)]),
    "hsflow_pipeline_flow_device": (_i, [_vp, ctypes.c_uint64, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.POINTER(_sz)]),
    "hsflow_pipeline_wait": (_i, [_vp, ctypes.c_uint64]),
    "hsflow_pipeline_render": (_i, [_vp, ctypes.c_uint64, _rp, _vp, _sz]),
    "hsflow_pipeline_render_jpeg": (_i, [_vp, ctypes.c_uint64, _rp, _i, _vp, _sz, ctypes.POINTER(_sz)]),
    "hsflow_pipeline_render_device": (_i, [_vp, ctypes.c_uint64, _rp, _vp, _sz]),
    "hsflow_pipeline_color": (_i, [_vp, ctypes.c_uint64, _cp, _vp, _sz, _fp]),
    "hsflow_pipeline_color_jpeg": (_i, [_vp, ctypes.c_uint64, _cp, _i, _vp, _sz, ctypes.POINTER(_sz)]),
    "hsflow_pipeline_color_device": (_i, [_vp, ctypes.c_uint64, _cp, _vp, _sz]),
    "hsflow_pipeline_warp": (_i, [_vp, ctypes.c_uint64, _wp, _vp, _sz, _vp, _sz, _vp, _sz, _ws]),
    "hsflow_pipeline_warp_device": (_i, [_vp, ctypes.c_uint64, _wp, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_pipeline_fb": (_i, [_vp, ctypes.c_uint64, ctypes.c_uint64, _bp, _vp, _sz, _vp, _sz, _bs]),
    "hsflow_pipeline_fb_device": (_i, [_vp, ctypes.c_uint64, ctypes.c_uint64, _bp, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_pipeline_median": (_i, [_vp, ctypes.c_uint64, _mp, _i, _vp, _sz, _vp, _vp, _sz, _vp, _sz, _ms]),
    "hsflow_pipeline_median_apply": (_i, [_vp, ctypes.c_uint64, _mp, _i, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_pipeline_interp": (_i, [_vp, ctypes.c_uint64, _f, _np, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _ns]),
    "hsflow_pipeline_interp_device": (_i, [_vp, ctypes.c_uint64, _f, _np, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _vp]),
    "hsflow_pipeline_info": (_i, [_vp, ctypes.c_uint64, ctypes.POINTER(HsflowInfo)]),
    "hsflow_pipeline_drain": (_i, [_vp]),
    "hsflow_pipeline_depth": (_i, [_vp]),
    "hsflow_pipeline_copies_elided": (_i, [_vp, ctypes.POINTER(ctypes.c_uint64)]),
    "hsflow_pipeline_frames_u8": (_i, [_vp, ctypes.c_uint64, _vp, _sz, _vp, _sz]),
    "hsflow_pipeline_last_error": (ctypes.c_char_p, [_vp]),
    "hsflow_multi_create": (_i, [ctypes.POINTER(_vp), ctypes.POINTER(_i), _i, _i, _i, _i]),
    "hsflow_multi_destroy": (_i, [_vp]),
    "hsflow_multi_devices": (_i, [_vp]),
    "hsflow_multi_submit": (_i, [_vp, _i, _vp, _sz, _vp, _sz, _vp, _sz, _vp, _sz, _pp, ctypes.POINTER(ctypes.c_uint64)]),
    "hsflow_multi_wait": (_i, [_vp, ctypes.c_uint64]),
    "hsflow_multi_drain": (_i, [_vp]),
    "hsflow_multi_last_error": (ctypes.c_char_p, [_vp]),
    "hsflow_slab_create": (_i, [ctypes.POINTER(_vp), ctypes.POINTER(_i), _i, _i, _i, _i]),
    "hsflow_slab_destroy": (_i, [_vp]),
    "hsflow_slab_count": (_i, [_vp]),
    "hsflow_slab_rows": (_i, [_vp, _i, ctypes.POINTER(_i), ctypes.POINTER(_i)]),
    "hsflow_slab_set_frames_u8": (_i, [_vp, _vp, _sz, _vp, _sz]),
    "hsflow_slab_solve": (_i, [_vp, _pp]),
    "hsflow_slab_exchanges": (_i, [_vp]),
    "hsflow_slab_iterations_done": (_i, [_vp]),
    "hsflow_slab_eps_measured": (_i, [_vp]),
    "hsflow_slab_create_overlapped": (_i, [ctypes.POINTER(_vp), ctypes.POINTER(_i), _i, _i, _i, _i]),
    "hsflow_slab_get_flow": (_i, [_vp, _vp, _sz, _vp, _sz]),
    "hsflow_slab_last_error": (ctypes.c_char_p, [_vp]),
    "hsflow_calc_optical_flow_hs_8u32f": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _i,
                                               ctypes.c_float, _i, _i, ctypes.c_double]),
}

_lib = None


def load():
    """Returns the loaded library; raises ImportError if it cannot be loaded (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so (same soname as
    # /opt/rocm's).  Loading torch first makes libhsflow.so bind to that copy; the other order
    # would put two runtimes in the process and the second one finds no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "opticalflowhs_amd: %s is missing -- build it with `python opticalflowhs_amd/build.py` "
            "(hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # e.g. libamdhip64 not found
        raise ImportError("opticalflowhs_amd: cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise ImportError("opticalflowhs_amd: %s does not export %s" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


class HsflowError(RuntimeError):
    def __init__(self, status, message):
        RuntimeError.__init__(self, "hsflow status %d: %s" % (status, message))
        self.status = status
