"""Host-side mirror of the reference's solver interface, over the C ABI (include/hsflow.h).

`calc_optical_flow_hs` has the argument list of cvCalcOpticalFlowHS (OpenCV2.1/include/cv.h:481-483)
as the reference calls it (OpticalFlowHS/OpticalFlowOpenCV.cpp:29); `HSFlow` is the resident-context
form that the reference's HSOpticalFlowOpenCL class plays (setupCL once, then per pair
runDerivatives + iterations x runCLKernels; HSOpticalFlowOpenCL.cpp:744-751).
Everything here runs on the GPU through libhsflow.so; there is no CPU path in this package.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from ._lib import (HsflowCornersParams, HsflowCornersRecord, HsflowCornersResult, HsflowLinkParams, HsflowLinkRecord, HsflowLinkSide, HsflowLinkResult, HsflowRegionsParams, HsflowRegionsRecord, HsflowRegionsResult, HsflowGmotionParams, HsflowGmotionResult, GMOTION_TRANSLATION, GMOTION_SIMILARITY, GMOTION_AFFINE, GMOTION_THRESHOLD_FIXED, GMOTION_THRESHOLD_AUTO, COLOR_SCALE_AUTO, COLOR_SCALE_FIXED, WARP_BORDER_CONSTANT, WARP_BORDER_REPLICATE, HsflowColorParams, HsflowWarpParams, HsflowWarpStats, HsflowFbParams, HsflowFbStats, HsflowChainParams, HsflowChainStats, CHAIN_MAX_PAIRS, HsflowMedianParams, HsflowMedianStats, HsflowInterpParams, HsflowInterpStats, HsflowPyramidParams, HsflowPyramidInfo, MEDIAN_FILTER, MEDIAN_FILL, HsflowError, HsflowInfo, HsflowPairResult, HsflowParams, HsflowPlaneDiff, HsflowRenderParams, HsflowVerifyReport, RENDER_CL, RENDER_CV, KERNEL_AUTO, KERNEL_FUSED, KERNEL_SIMPLE, KERNEL_STRIP, KERNEL_FOLD, KERNEL_PERSIST,
                   MODE_CLASSIC, MODE_CV, TERM_EPS, TERM_ITER)

TermCriteria = collections.namedtuple("TermCriteria", "type max_iter epsilon")


def term_criteria(type_, max_iter, epsilon):
    """cvTermCriteria(): epsilon is rounded through fp32 (OpenCV2.1/include/cxtypes.h:904-915)."""
    return TermCriteria(int(type_), int(max_iter), float(np.float32(epsilon)))


def _ptr(x):
    """Device or host pointer of a numpy array / torch tensor / raw int."""
    if isinstance(x, int):
        return ctypes.c_void_p(x)
    if isinstance(x, np.ndarray):
        return ctypes.c_void_p(x.ctypes.data)
    if hasattr(x, "data_ptr"):
        return ctypes.c_void_p(x.data_ptr())
    raise TypeError("expected numpy array, tensor or int pointer, got %r" % type(x))


def _is_device_tensor(x):
    return hasattr(x, "is_cuda") and bool(x.is_cuda)


def make_params(lam=1.0, max_iter=100, epsilon=1e-6, term_type=TERM_ITER | TERM_EPS,
                use_previous=False, mode=MODE_CV, alpha=1.0, kernel=KERNEL_AUTO, fuse_steps=0,
                tile_w=0, tile_h=0, threads=0, strip_rows=0, reuse_derivatives=False, use_graph=False,
                profile=False):
    p = HsflowParams()
    _lib.load().hsflow_default_params(ctypes.byref(p))
    p.mode = mode
    p.lambda_ = lam
    p.alpha = alpha
    p.term_type = term_type
    p.max_iter = max_iter
    p.epsilon = epsilon
    p.use_previous = 1 if use_previous else 0
    p.kernel = kernel
    p.fuse_steps = fuse_steps
    p.tile_w = tile_w
    p.tile_h = tile_h
    p.threads = threads
    p.strip_rows = strip_rows
    p.reuse_derivatives = 1 if reuse_derivatives else 0
    p.use_graph = 1 if use_graph else 0
    p.profile = 1 if profile else 0
    return p


def make_render_params(route="cv", step=None, threshold=None, scale=None, dot_rgb=None, line_rgb=None):
    """hsflow_render_params of one of the reference's two drawings -- route "cv" (OpticalFlowOpenCV.cpp:33-46:
    threshold 1, half-length lines) or "cl" (HSOpticalFlowOpenCL.cpp:759-769: threshold 0.5, full-length lines), both on a
    4-pixel grid with blue dots and red lines -- with any field replaced."""
    if route not in ("cv", "cl"):
        raise ValueError("route must be 'cv' or 'cl'")
    rp = HsflowRenderParams()
    _lib.load().hsflow_default_render_params(ctypes.byref(rp), RENDER_CL if route == "cl" else RENDER_CV)
    if step is not None:
        rp.step = int(step)
    if threshold is not None:
        rp.threshold = threshold
    if scale is not None:
        rp.scale = scale
    for name, val in (("dot_rgb", dot_rgb), ("line_rgb", line_rgb)):
        if val is not None:
            if len(val) != 3:
                raise ValueError("%s must be three bytes" % name)
            setattr(rp, name, (ctypes.c_uint8 * 3)(*[int(t) for t in val]))
    return rp


def make_color_params(max_flow=None):
    """hsflow_color_params of the dense colour picture (the Middlebury wheel): max_flow=None takes the scale from the
    picture itself (HSFLOW_COLOR_SCALE_AUTO), a number fixes it (HSFLOW_COLOR_SCALE_FIXED; finite and > 0)."""
    cp = HsflowColorParams()
    _lib.load().hsflow_default_color_params(ctypes.byref(cp))
    if max_flow is not None:
        cp.scale_mode = COLOR_SCALE_FIXED
        cp.max_flow = max_flow
    return cp


def make_warp_params(channels=1, t=1.0, border="constant", fill=0):
    """hsflow_warp_params of a backward warp by the flow: `channels` 1 or 3 (interleaved), `t` the fraction of the flow to
    apply (1: the second frame onto the first), `border` "constant" (a pixel that samples outside the picture, or whose
    flow is unknown, is `fill`) or "replicate" (outside samples take the nearest pixel), `fill` one level or one per
    channel."""
    wp = HsflowWarpParams()
    _lib.load().hsflow_default_warp_params(ctypes.byref(wp))
    wp.channels = int(channels)
    wp.t = t
    if isinstance(border, str):
        if border not in ("constant", "replicate"):
            raise ValueError("border must be 'constant' or 'replicate'")
        border = WARP_BORDER_REPLICATE if border == "replicate" else WARP_BORDER_CONSTANT
    wp.border = int(border)
    levels = [int(fill)] * 3 if np.isscalar(fill) else [int(f) for f in fill]
    if len(levels) > 4 or any(not 0 <= f <= 255 for f in levels):
        raise ValueError("fill must be at most 4 levels of 0 .. 255")
    for k, f in enumerate(levels):
        wp.fill[k] = f
    return wp


def _warp_image(img, height, width, what, device):
    """(pointer, row stride in bytes, channels) of a picture for the warp entries: uint8, (H, W), (H, W, 1) or (H, W, 3),
    packed pixels, any row stride; a NumPy array, or with device=True a CUDA tensor."""
    shape = tuple(img.shape)
    if device != _is_device_tensor(img) or (not device and not isinstance(img, np.ndarray)):
        raise ValueError("%s must be %s" % (what, "a CUDA uint8 tensor" if device else "a uint8 NumPy array"))
    channels = 1 if len(shape) == 2 else shape[2] if len(shape) == 3 else 0
    if str(img.dtype) not in ("uint8", "torch.uint8") or shape[:2] != (height, width) or channels not in (1, 3):
        raise ValueError("%s must be uint8 of shape (height, width), (height, width, 1) or (height, width, 3)" % what)
    strides = tuple(img.stride()) if device else img.strides
    if strides[1] != channels or (len(shape) == 3 and channels == 3 and strides[2] != 1):
        raise ValueError("%s must have packed pixels" % what)
    return _ptr(img), strides[0], channels


def _warp_args(height, width, src, ref, out, device, params, t, border, fill):
    """The pictures of one warp call as ((pointer, stride) of src, of ref, of out, params); absent pictures are (None, 0)."""
    pics = [(_warp_image(x, height, width, what, device) if x is not None else (None, 0, None))
            for x, what in ((src, "src"), (ref, "ref"), (out, "out"))]
    given = set(c for _, _, c in pics if c is not None)
    if len(given) > 1:
        raise ValueError("src, ref and out must have the same number of channels")
    channels = given.pop() if given else 1
    if params is None:
        params = make_warp_params(channels, t, border, fill)
    elif given and params.channels != channels:
        raise ValueError("params.channels does not match the pictures")
    return tuple((p, s) for p, s, _ in pics) + (params,)


def _stats_record(cls, want, device, device_index):
    """(record, pointer) of one statistics record of `cls` (64 bytes) where `want`, else (None, None): on the device a CUDA
    uint8 tensor, else the ctypes record."""
    if not want:
        return None, None
    if device:
        import torch
        rec = torch.empty(ctypes.sizeof(cls), dtype=torch.uint8, device="cuda:%d" % device_index)  # (the library clears it)
        return rec, _ptr(rec)
    rec = cls()
    return rec, ctypes.byref(rec)


def _check_stats_tensor(stats, n, cls):
    """The pointer of a device batch's statistics: None, or of a contiguous CUDA uint8 tensor that holds n records of `cls`."""
    if stats is None:
        return None
    if not _is_device_tensor(stats) or str(stats.dtype) != "torch.uint8" or not stats.is_contiguous() or stats.numel() < n * ctypes.sizeof(cls):
        raise ValueError("stats must be a contiguous CUDA uint8 tensor of at least n * 64 bytes")
    return _ptr(stats)


def _plane_lists(items, n, what, unit, read):
    """One list of a device batch as (pointer array, the one row stride, what `read` gave): items None (absent: (None, 0,
    [])), a tensor (n, ...) or a list of n tensors; read(x): (pointer, row stride, ...) of one of them; `what` and `unit`
    word the error."""
    if items is None:
        return None, 0, []
    got = [read(items[i]) for i in range(len(items))]
    if len(got) != n or len(set(g[1] for g in got)) > 1:
        raise ValueError("%s must hold one %s, all of one row stride" % (what, unit))
    return (ctypes.c_void_p * max(n, 1))(*[g[0].value for g in got]), got[0][1] if got else 0, got


def _warp_call(height, width, device_index, src, ref, out, params, t, border, fill, return_stats, picture):
    """What `HSFlow.warp` and `PairPipeline.warp` share: decides between the host and the device form, allocates `out`
    where a picture is wanted and none was given, and the statistics record.  Returns (device, the C call's arguments
    from the params on, out, stats)."""
    device = any(_is_device_tensor(x) for x in (src, ref, out))
    if not picture:
        out = None
    elif out is None:
        shape = tuple(src.shape) if src is not None else (height, width)
        if device:
            import torch
            out = torch.empty(shape, dtype=torch.uint8, device="cuda:%d" % device_index)
        else:
            out = np.empty(shape, np.uint8)
    (sp, ss), (rp, rs), (op, os_), wp = _warp_args(height, width, src, ref, out, device, params, t, border, fill)
    stats, sref = _stats_record(HsflowWarpStats, return_stats, device, device_index)
    return device, (ctypes.byref(wp), sp, ss, rp, rs, op, os_, sref), out, stats


def make_interp_params(channels=1, fill_radius=1, fill_min_votes=1, fill_passes=4):
    """hsflow_interp_params of the frame between the two frames of a pair: `channels` 1 or 3 (interleaved), and the hole
    filling of the projected flow -- `fill_passes` passes (0 .. MEDIAN_MAX_PASSES) of the median rule in FILL mode with
    `fill_radius` (1 or 2) and `fill_min_votes`."""
    ip = HsflowInterpParams()
    _lib.load().hsflow_default_interp_params(ctypes.byref(ip))
    ip.channels, ip.fill_radius, ip.fill_min_votes, ip.fill_passes = int(channels), int(fill_radius), int(fill_min_votes), int(fill_passes)
    return ip


def _interp_call(height, width, device_index, prev, curr, vis_prev, vis_curr, ref, out, classes, stats, params, device):
    """What `HSFlow.interp`, `PairPipeline.interp` and `interp_host` share.  out / classes: False or None (absent), True
    (allocated here) or the array to fill; stats True or False.  Returns (device, the C call's arguments from the params
    on, out, classes, stats)."""
    if (prev is None) != (curr is None):
        raise ValueError("prev and curr are given together or not at all")
    device = bool(device) or any(_is_device_tensor(x) for x in (prev, curr, vis_prev, vis_curr, ref, out, classes))
    pshape = tuple(prev.shape) if prev is not None else (height, width)
    made = []
    for x, shape in ((out, pshape), (classes, (height, width))):
        if x is None or x is False:
            x = None
        elif x is True and device:
            import torch
            x = torch.empty(shape, dtype=torch.uint8, device="cuda:%d" % device_index)
        elif x is True:
            x = np.empty(shape, np.uint8)
        made.append(x)
    out, classes = made
    pics = [(_warp_image(x, height, width, what, device) if x is not None else (None, 0, None))
            for x, what in ((prev, "prev"), (curr, "curr"), (ref, "ref"), (out, "out"))]
    given = set(c for _, _, c in pics if c is not None)
    if len(given) > 1:
        raise ValueError("prev, curr, ref and out must have the same number of channels")
    channels = given.pop() if given else 1
    if params is None:
        params = make_interp_params(channels)
    elif given and params.channels != channels:
        raise ValueError("params.channels does not match the pictures")
    planes = [(_plane(x, height, width, "uint8", what, device) if x is not None else (None, 0))
              for x, what in ((vis_prev, "vis_prev"), (vis_curr, "vis_curr"), (classes, "classes"))]
    rec, sref = _stats_record(HsflowInterpStats, stats, device, device_index)
    (pp, ps, _), (cp, cs, _), (rp, rs, _), (op, os_, _) = pics
    (vpp, vps), (vcp, vcs), (kp, ks) = planes
    return device, (ctypes.byref(params), pp, ps, cp, cs, vpp, vps, vcp, vcs, rp, rs, op, os_, kp, ks, sref), out, classes, rec


def _project_call(height, width, device_index, prev, curr, flow, state, stats, params, device):
    """What `HSFlow.project_flow` and `project_flow_host` share; flow / state: False, True or (for flow) a pair (u, v) of
    planes, (for state) the plane to fill.  Returns (the C call's arguments from the params on, u, v, state, stats)."""
    if (prev is None) != (curr is None):
        raise ValueError("prev and curr are given together or not at all")
    pics = [(_warp_image(x, height, width, what, device) if x is not None else (None, 0, None)) for x, what in ((prev, "prev"), (curr, "curr"))]
    given = set(c for _, _, c in pics if c is not None)
    if len(given) > 1:
        raise ValueError("prev and curr must have the same number of channels")
    if params is None:
        params = make_interp_params(given.pop() if given else 1)

    def new(dtype):
        if device:
            import torch
            return torch.empty((height, width), dtype=getattr(torch, dtype), device="cuda:%d" % device_index)
        return np.empty((height, width), dtype)
    u = v = None
    if flow is True:
        u, v = new("float32"), new("float32")
    elif flow:
        u, v = flow
    state = new("uint8") if state is True else (None if state is None or state is False else state)
    (up, us), (vp, vs) = [(_plane(x, height, width, "float32", "flow output", device) if x is not None else (None, 0)) for x in (u, v)]
    if u is not None and us != vs:
        raise ValueError("the two flow outputs share one row stride")
    sp, ss = _plane(state, height, width, "uint8", "state", device) if state is not None else (None, 0)
    rec, sref = _stats_record(HsflowInterpStats, stats, device, device_index)
    (pp, ps, _), (cp, cs, _) = pics
    return (ctypes.byref(params), pp, ps, cp, cs, up, vp, us, sp, ss, sref), u, v, state, rec


def make_fb_params(alpha=0.01, beta=0.5, values=(255, 0, 0, 0)):
    """hsflow_fb_params of a forward-backward check: a pixel is consistent where |f + b(x + f)|^2 <= alpha (|f|^2 + |b|^2) +
    beta (alpha finite in 0 .. 1e6, beta in 0 .. 1e30); `values`: the mask's byte for the classes consistent,
    inconsistent, outside, unknown."""
    fp = HsflowFbParams()
    _lib.load().hsflow_default_fb_params(ctypes.byref(fp))
    fp.alpha, fp.beta = alpha, beta
    levels = [int(x) for x in values]
    if len(levels) != 4 or any(not 0 <= x <= 255 for x in levels):
        raise ValueError("values must be 4 levels of 0 .. 255")
    for k, x in enumerate(levels):
        fp.value[k] = x
    return fp


def _plane(x, height, width, dtype, what, device):
    """(pointer, row stride in bytes) of a plane of the check or the median: (H, W) of `dtype`, elements packed, any row stride."""
    if device != _is_device_tensor(x) or (not device and not isinstance(x, np.ndarray)):
        raise ValueError("%s must be %s" % (what, "a CUDA tensor" if device else "a NumPy array"))
    if str(x.dtype) not in (dtype, "torch." + dtype) or tuple(x.shape) != (height, width):
        raise ValueError("%s must be %s of shape (height, width)" % (what, dtype))
    size = 4 if dtype in ("float32", "int32") else 1
    strides = tuple(st * size for st in x.stride()) if device else x.strides
    if strides[1] != size:
        raise ValueError("%s must have packed elements" % what)
    return _ptr(x), strides[0]


def _fb_call(height, width, device_index, mask, err2, stats, params, alpha, beta, values, device):
    """What `HSFlow.fb`, `PairPipeline.fb` and `fb_host` share: mask / err2 each False or None (absent), True (allocated
    here) or the plane to fill; stats True or False.  Returns (device, the C call's arguments from the params on, mask,
    err2, stats)."""
    device = bool(device) or any(_is_device_tensor(x) for x in (mask, err2))
    planes = []
    for x, dtype in ((mask, "uint8"), (err2, "float32")):
        if x is None or x is False:
            x = None
        elif x is True and device:
            import torch
            x = torch.empty((height, width), dtype=getattr(torch, dtype), device="cuda:%d" % device_index)
        elif x is True:
            x = np.empty((height, width), dtype)
        planes.append(x)
    mask, err2 = planes
    mp, ms = _plane(mask, height, width, "uint8", "mask", device) if mask is not None else (None, 0)
    ep, es = _plane(err2, height, width, "float32", "err2", device) if err2 is not None else (None, 0)
    fp = params if params is not None else make_fb_params(alpha, beta, values)
    rec, sref = _stats_record(HsflowFbStats, stats, device, device_index)
    return device, (ctypes.byref(fp), mp, ms, ep, es, sref), mask, err2, rec


def make_gmotion_params(model="affine", passes=3, threshold="fixed", inlier_px=1.0, scale2=6.0, min_thr2=0.0625, values=(255, 0, 0, 0)):
    """hsflow_gmotion_params of a global-motion fit: `model` "translation", "similarity" or "affine" (or the GMOTION_*
    constant); `passes` 1 .. 8 of the trimmed least squares; `threshold` "fixed" (a pixel is an inlier within `inlier_px`
    of the model) or "auto" (the squared threshold is `scale2` times the median squared residual, at least `min_thr2`);
    `values`: the mask's byte for the classes inlier, outlier, untrusted, unknown.  include/hsflow.h has the rule."""
    gp = HsflowGmotionParams()
    _lib.load().hsflow_default_gmotion_params(ctypes.byref(gp))
    if isinstance(model, str):
        kinds = {"translation": GMOTION_TRANSLATION, "similarity": GMOTION_SIMILARITY, "affine": GMOTION_AFFINE}
        if model not in kinds:
            raise ValueError("model must be 'translation', 'similarity' or 'affine'")
        model = kinds[model]
    if isinstance(threshold, str):
        if threshold not in ("fixed", "auto"):
            raise ValueError("threshold must be 'fixed' or 'auto'")
        threshold = GMOTION_THRESHOLD_AUTO if threshold == "auto" else GMOTION_THRESHOLD_FIXED
    gp.model, gp.passes, gp.threshold_mode = int(model), int(passes), int(threshold)
    gp.inlier_px, gp.scale2, gp.min_thr2 = inlier_px, scale2, min_thr2
    levels = [int(x) for x in values]
    if len(levels) != 4 or any(not 0 <= x <= 255 for x in levels):
        raise ValueError("values must be 4 levels of 0 .. 255")
    for k, x in enumerate(levels):
        gp.value[k] = x
    return gp


def _gmotion_call(height, width, device_index, state, mask, residual, result, params, device):
    """What the global-motion fits share from the state plane on.  state: None or the u8 plane; mask: False / None, True
    (allocated here) or the u8 plane; residual: False / None, True or the pair (res_u, res_v) of float32 planes of one row
    stride; result: True or False.  Returns (the C call's arguments, record, mask, res_u, res_v)."""
    def fresh(dtype):
        if device:
            import torch
            return torch.empty((height, width), dtype=getattr(torch, dtype), device="cuda:%d" % device_index)
        return np.empty((height, width), dtype)
    sp, ss = _plane(state, height, width, "uint8", "state", device) if state is not None else (None, 0)
    mask = fresh("uint8") if mask is True else (None if mask is None or mask is False else mask)
    mp, ms = _plane(mask, height, width, "uint8", "mask", device) if mask is not None else (None, 0)
    ru = rv = up = vp = None
    rs = 0
    if residual is True:
        ru, rv = fresh("float32"), fresh("float32")
    elif residual is not None and residual is not False:
        ru, rv = residual
    if ru is not None:
        (up, rs), (vp, vs) = [_plane(x, height, width, "float32", "residual", device) for x in (ru, rv)]
        if rs != vs:
            raise ValueError("the two residual planes share one row stride")
    gp = params if params is not None else make_gmotion_params()
    rec, rref = _stats_record(HsflowGmotionResult, result, device, device_index)
    return (sp, ss, ctypes.byref(gp), mp, ms, up, vp, rs, rref), rec, mask, ru, rv


def _gmotion_model(model):
    """Six floats of a model -- a sequence, an array or an `HsflowGmotionResult` -- as a ctypes array."""
    if isinstance(model, HsflowGmotionResult):
        model = list(model.p)
    vals = [float(x) for x in np.asarray(model, np.float32).reshape(-1)]
    if len(vals) != 6:
        raise ValueError("a model has six parameters")
    return (ctypes.c_float * 6)(*vals)


def make_regions_params(connectivity=8, min_area=1, join_px=0.0, fg=(1, 255)):
    """hsflow_regions_params of a labelling: `connectivity` 4 or 8; regions of fewer than `min_area` pixels are dropped;
    `join_px` 0 joins every two adjacent foreground pixels, above 0 only those whose flows differ by at most that many
    pixels (needs flow); `fg`: the range (lo, hi) of mask bytes that are foreground.  include/hsflow.h has the rule."""
    rp = HsflowRegionsParams()
    _lib.load().hsflow_default_regions_params(ctypes.byref(rp))
    rp.connectivity, rp.min_area, rp.join_px = int(connectivity), int(min_area), join_px
    rp.fg_lo, rp.fg_hi = int(fg[0]), int(fg[1])
    return rp


def _regions_call(height, width, device_index, mask, labels, records, capacity, result, params, device):
    """What the labelling entries share from the mask on.  mask: None or the u8 plane; labels: False / None, True
    (allocated here) or the int32 plane; records: False / None, True (`capacity` of them allocated here: on the host a
    ctypes array of `HsflowRegionsRecord`, on the device a CUDA uint8 tensor of capacity * 64 bytes) or such an array;
    result: True or False.  Returns (the C call's arguments, result, labels, records)."""
    capacity = int(capacity)
    mp, ms = _plane(mask, height, width, "uint8", "mask", device) if mask is not None else (None, 0)
    if labels is True:
        if device:
            import torch
            labels = torch.empty((height, width), dtype=torch.int32, device="cuda:%d" % device_index)
        else:
            labels = np.empty((height, width), np.int32)
    elif labels is None or labels is False:
        labels = None
    lp, ls = (None, 0)
    if labels is not None:
        if device != _is_device_tensor(labels) or str(labels.dtype) not in ("int32", "torch.int32") or tuple(labels.shape) != (height, width):
            raise ValueError("labels must be int32 of shape (height, width), %s" % ("a CUDA tensor" if device else "a NumPy array"))
        strides = tuple(st * 4 for st in labels.stride()) if device else labels.strides
        if strides[1] != 4:
            raise ValueError("labels must have packed elements")
        lp, ls = _ptr(labels), strides[0]
    rp_ = None
    if records is True:
        if device:
            import torch
            records = torch.empty(max(capacity, 1) * 64, dtype=torch.uint8, device="cuda:%d" % device_index)
        else:
            records = (HsflowRegionsRecord * max(capacity, 1))()
    elif records is None or records is False:
        records = None
    if records is not None:
        if device:
            if not _is_device_tensor(records) or str(records.dtype) != "torch.uint8" or not records.is_contiguous() or records.numel() < capacity * 64:
                raise ValueError("records must be a contiguous CUDA uint8 tensor of at least capacity * 64 bytes")
            rp_ = _ptr(records)
        else:
            if ctypes.sizeof(records) < capacity * 64:
                raise ValueError("records must hold at least capacity records")
            rp_ = ctypes.cast(records, ctypes.c_void_p)
    prm = params if params is not None else make_regions_params()
    rec, rref = _stats_record(HsflowRegionsResult, result, device, device_index)
    return (mp, ms, ctypes.byref(prm), lp, ls, rp_, capacity, rref), rec, labels, records


def make_corners_params(kind="min_eigen", block_r=1, nms_r=3, quality_q16=655, border=0, fg=(1, 255), max_candidates=_lib.CORNERS_MAX_CANDIDATES, min_score=1):
    """hsflow_corners_params of a corner detection: `kind` "min_eigen" or "harris" (or the constant); the structure tensor
    is summed over (2 block_r + 1)^2 pixels; a corner beats every pixel within `nms_r`; a corner's score is at least
    `quality_q16` / 65536 of the frame's best and at least `min_score`; `border`: pixels closer to a frame edge are no
    corners; `fg`: the range (lo, hi) of mask bytes that may be corners.  include/hsflow.h has the rule."""
    cp = HsflowCornersParams()
    _lib.load().hsflow_default_corners_params(ctypes.byref(cp))
    kinds = {"min_eigen": _lib.CORNERS_MIN_EIGEN, "harris": _lib.CORNERS_HARRIS}
    cp.kind = kinds[kind] if isinstance(kind, str) else int(kind)
    cp.block_r, cp.nms_r, cp.quality_q16, cp.border = int(block_r), int(nms_r), int(quality_q16), int(border)
    cp.fg_lo, cp.fg_hi = int(fg[0]), int(fg[1])
    cp.max_candidates, cp.min_score = int(max_candidates), int(min_score)
    return cp


def _corners_xy(xy, capacity, device, device_index):
    """The xy array of the corner entries: False / None (absent), True (`capacity` pairs allocated here) or a float32 array
    (capacity, 2), contiguous.  Returns (array, pointer)."""
    if xy is None or xy is False:
        return None, None
    if xy is True:
        if device:
            import torch
            xy = torch.empty((max(capacity, 1), 2), dtype=torch.float32, device="cuda:%d" % device_index)
        else:
            xy = np.empty((max(capacity, 1), 2), np.float32)
    if device != _is_device_tensor(xy) or (not device and not isinstance(xy, np.ndarray)):
        raise ValueError("xy must be %s" % ("a CUDA tensor" if device else "a NumPy array"))
    packed = xy.is_contiguous() if device else xy.flags["C_CONTIGUOUS"]
    if str(xy.dtype) not in ("float32", "torch.float32") or xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] < capacity or not packed:
        raise ValueError("xy must be contiguous float32 of shape (at least capacity, 2)")
    return xy, _ptr(xy)


def _corners_call(height, width, device_index, mask, records, capacity, xy, result, params, device):
    """What the corner entries share from the mask on.  mask: None or the u8 plane; records: False / None, True
    (`capacity` of them allocated here: on the host a ctypes array of `HsflowCornersRecord`, on the device a CUDA uint8
    tensor of capacity * 16 bytes) or such an array; xy: False / None, True or the float32 array (capacity, 2); result:
    True or False.  Returns (the C call's arguments, result, records, xy)."""
    capacity = int(capacity)
    mp, ms = _plane(mask, height, width, "uint8", "mask", device) if mask is not None else (None, 0)
    records, rp_ = _link_records(records, capacity, HsflowCornersRecord, "records", device, device_index)
    xy, xp = _corners_xy(xy, capacity, device, device_index)
    prm = params if params is not None else make_corners_params()
    rec, rref = _stats_record(HsflowCornersResult, result, device, device_index)
    return (mp, ms, ctypes.byref(prm), rp_, capacity, xp, rref), rec, records, xy


def make_link_params(cap_a=64, cap_b=None):
    """hsflow_link_params of a linking step: labels of frame k above `cap_a` only count into over_a_px, labels of frame
    k + 1 above `cap_b` (None: cap_a) are unmatched; cap_a * cap_b is at most 2^24.  include/hsflow.h has the rule."""
    lp = HsflowLinkParams()
    _lib.load().hsflow_default_link_params(ctypes.byref(lp))
    lp.cap_a, lp.cap_b = int(cap_a), int(cap_a if cap_b is None else cap_b)
    return lp


def _link_records(x, count, cls, what, device, device_index):
    """One record array of the linking entries: x False / None (absent), True (`count` records of `cls` allocated here: on
    the host a ctypes array, on the device a CUDA uint8 tensor) or such an array.  Returns (array, pointer)."""
    size = ctypes.sizeof(cls)
    if x is None or x is False:
        return None, None
    if x is True:
        if device:
            import torch
            x = torch.empty(max(count, 1) * size, dtype=torch.uint8, device="cuda:%d" % device_index)
        else:
            x = (cls * max(count, 1))()
    if device:
        if not _is_device_tensor(x) or str(x.dtype) != "torch.uint8" or not x.is_contiguous() or x.numel() < count * size:
            raise ValueError("%s must be a contiguous CUDA uint8 tensor of at least %d bytes" % (what, count * size))
        return x, _ptr(x)
    if ctypes.sizeof(x) < count * size:
        raise ValueError("%s must hold at least %d records" % (what, count))
    return x, ctypes.cast(x, ctypes.c_void_p)


def _link_call(device_index, links, link_capacity, side_a, side_b, result, params, device):
    """What the linking entries share from the params on: (the C call's arguments, result, links, side_a, side_b)."""
    prm = params if params is not None else make_link_params()
    link_capacity = int(link_capacity)
    links, kp = _link_records(links, link_capacity, HsflowLinkRecord, "links", device, device_index)
    side_a, ap = _link_records(side_a, prm.cap_a, HsflowLinkSide, "side_a", device, device_index)
    side_b, bp = _link_records(side_b, prm.cap_b, HsflowLinkSide, "side_b", device, device_index)
    rec, rref = _stats_record(HsflowLinkResult, result, device, device_index)
    return (ctypes.byref(prm), kp, link_capacity, ap, bp, rref), rec, links, side_a, side_b


def _link_list(items, n, count, cls, what):
    """One list of record arrays of a device batch: None, or n entries, each None or a CUDA uint8 tensor."""
    if items is None:
        return None
    if len(items) != n:
        raise ValueError("%s must hold one entry per step" % what)
    return (ctypes.c_void_p * n)(*[_link_records(x, count, cls, what, True, 0)[1].value if x is not None else None for x in items])


def make_chain_params(values=(255, 0, 0, 0)):
    """hsflow_chain_params of a chain: `values` is the status byte for the classes alive, left, untrusted, unknown."""
    cp = HsflowChainParams()
    _lib.load().hsflow_default_chain_params(ctypes.byref(cp))
    levels = [int(x) for x in values]
    if len(levels) != 4 or any(not 0 <= x <= 255 for x in levels):
        raise ValueError("values must be 4 levels of 0 .. 255")
    for k, x in enumerate(levels):
        cp.value[k] = x
    return cp


def _chain_list(planes, n, height, width, dtype, what, device, holes=False):
    """(pointer array, the one row stride) of the n planes of a chain, (None, 0) for None; holes: entries may be None."""
    if planes is None:
        return None, 0
    if len(planes) != n:
        raise ValueError("%s must hold one plane per pair of the chain" % what)
    got = [(None, 0) if (x is None and holes) else _plane(x, height, width, dtype, what, device) for x in planes]
    strides = set(g[1] for g, x in zip(got, planes) if x is not None)
    if len(strides) > 1:
        raise ValueError("the planes of %s share one row stride" % what)
    return (ctypes.c_void_p * n)(*[g[0].value if g[0] is not None else None for g in got]), (strides.pop() if strides else 0)


def _chain_device(device, *groups):
    """device=True, or any plane in `groups` (planes, None / True / False, or sequences of them) is a CUDA tensor."""
    def walk(x):
        if isinstance(x, (list, tuple)):
            return any(walk(y) for y in x)
        return _is_device_tensor(x)
    return bool(device) or walk(groups)


def _chain_call(height, width, device_index, n, state, start, flow, status, age, stats, params, device):
    """What the dense chain entries share from the state list on: (the C call's arguments, U, V, status, age, stats)."""
    def fresh(dtype):
        if device:
            import torch
            return torch.empty((height, width), dtype=getattr(torch, dtype), device="cuda:%d" % device_index)
        return np.empty((height, width), dtype)
    sl, ss = _chain_list(state, n, height, width, "uint8", "state", device, holes=True)
    U0p = V0p = None
    s0s = 0
    if start is not None:
        (U0p, s0s), (V0p, vs) = [_plane(x, height, width, "float32", "start", device) for x in start]
        if s0s != vs:
            raise ValueError("the two start planes share one row stride")
    U = V = Up = Vp = None
    os_ = 0
    if flow is True:
        U, V = fresh("float32"), fresh("float32")
    elif flow:
        U, V = flow
    if U is not None:
        (Up, os_), (Vp, vs) = [_plane(x, height, width, "float32", "flow output", device) for x in (U, V)]
        if os_ != vs:
            raise ValueError("the two flow outputs share one row stride")
    outs = []
    for x, what in ((status, "status"), (age, "age")):
        x = fresh("uint8") if x is True else (None if x is None or x is False else x)
        outs.append((x,) + (_plane(x, height, width, "uint8", what, device) if x is not None else (None, 0)))
    (status, stp, sts), (age, agp, ags) = outs
    cp = params if params is not None else make_chain_params()
    rec, sref = _stats_record(HsflowChainStats, stats, device, device_index)
    return (sl, ss, U0p, V0p, s0s, ctypes.byref(cp), Up, Vp, os_, stp, sts, agp, ags, sref), U, V, status, age, rec


def make_median_params(radius=1, mode="filter", min_votes=1):
    """hsflow_median_params: radius 1 (3x3) or 2 (5x5); mode "filter" (every pixel becomes its window's median) or "fill"
    (only pixels whose state is 0 are replaced), or the MEDIAN_* constant; min_votes 1 .. (2 radius + 1)^2, the voters a
    window needs.  include/hsflow.h has the rule."""
    mp = HsflowMedianParams()
    _lib.load().hsflow_default_median_params(ctypes.byref(mp))
    if isinstance(mode, str):
        if mode not in ("filter", "fill"):
            raise ValueError("mode must be 'filter' or 'fill'")
        mode = MEDIAN_FILL if mode == "fill" else MEDIAN_FILTER
    mp.radius, mp.mode, mp.min_votes = int(radius), int(mode), int(min_votes)
    return mp


def make_pyramid_params(levels=0, min_size=32, warps=1, median_radius=0):
    """hsflow_pyramid_params: levels 0 ("auto": as many as keep the smaller side >= min_size, at most 8) or 1 .. 8 as given;
    warps 1 .. 8 steps per level; median_radius 0 (none), 1 or 2: a 3x3 / 5x5 median of every total.  include/hsflow.h has
    the scheme."""
    pp = HsflowPyramidParams()
    _lib.load().hsflow_default_pyramid_params(ctypes.byref(pp))
    if levels == "auto":
        levels = 0
    pp.levels, pp.min_size, pp.warps, pp.median_radius = int(levels), int(min_size), int(warps), int(median_radius)
    return pp


def _median_call(height, width, device_index, state, flow, state_out, stats, params, radius, mode, min_votes, device):
    """What the median entries share.  state: None or the u8 plane (H, W); flow: False / None (absent), True (allocated
    here) or the pair (u_out, v_out) of float32 planes of one row stride; state_out: False / None, True or the u8 plane;
    stats: True or False.  Returns (mp, (state pointer, stride), (u pointer, v pointer, stride), (state_out pointer,
    stride), record pointer, u_out, v_out, state_out, record)."""
    def fresh(dtype):
        if device:
            import torch
            return torch.empty((height, width), dtype=getattr(torch, dtype), device="cuda:%d" % device_index)
        return np.empty((height, width), dtype)
    sp, ss = _plane(state, height, width, "uint8", "state", device) if state is not None else (None, 0)
    u_out = v_out = None
    up = vp = None
    os_ = 0
    if flow is True:
        u_out, v_out = fresh("float32"), fresh("float32")
    elif flow is not None and flow is not False:
        u_out, v_out = flow
    if u_out is not None:
        (up, os_), (vp, vs) = _plane(u_out, height, width, "float32", "u_out", device), _plane(v_out, height, width, "float32", "v_out", device)
        if vs != os_:
            raise ValueError("u_out and v_out must have one row stride")
    if state_out is True:
        state_out = fresh("uint8")
    elif state_out is False:
        state_out = None
    sop, sos = _plane(state_out, height, width, "uint8", "state_out", device) if state_out is not None else (None, 0)
    mp = params if params is not None else make_median_params(radius, mode, min_votes)
    rec, sref = _stats_record(HsflowMedianStats, stats, device, device_index)
    return mp, (sp, ss), (up, vp, os_), (sop, sos), sref, u_out, v_out, state_out, rec


def _render_target(out, height, width):
    """(pointer, row stride in bytes) of a CUDA uint8 tensor of shape (height, width, 3) with packed pixels."""
    if str(out.dtype) != "torch.uint8" or tuple(out.shape) != (height, width, 3) or out.stride(2) != 1 or out.stride(1) != 3:
        raise ValueError("out must be a CUDA uint8 tensor of shape (height, width, 3) with packed pixels")
    return ctypes.c_void_p(out.data_ptr()), out.stride(0)


def _render_host(out, height, width):
    """The host picture to draw into: `out` if given (uint8, (height, width, 3), packed pixels), else a new array."""
    if out is None:
        return np.empty((height, width, 3), np.uint8)
    if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.shape != (height, width, 3) or out.strides[2] != 1 or out.strides[1] != 3 \
            or not out.flags.writeable:
        raise ValueError("out must be a writeable uint8 array of shape (height, width, 3) with packed pixels")
    return out


class HSFlow(object):
    """A solver context holding `n_pairs` image pairs of one size resident on one GPU."""

    def __init__(self, width, height, n_pairs=1, device=0, stream=None, own_stream=False):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        self.width, self.height, self.n_pairs, self.device = int(width), int(height), int(n_pairs), int(device)
        sp = ctypes.c_void_p(int(stream)) if stream else ctypes.c_void_p()
        st = self._lib.hsflow_create(ctypes.byref(self._h), self.device, self.width, self.height,
                                     self.n_pairs, sp, 1 if own_stream else 0)
        if st != _lib.OK:
            msg = self._lib.hsflow_last_error(None).decode()
            self._h = ctypes.c_void_p()
            raise HsflowError(st, msg)

    # -- helpers -------------------------------------------------------------------------
    def _check(self, st):
        if st != _lib.OK:
            raise HsflowError(st, self._lib.hsflow_last_error(self._h).decode())

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.hsflow_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_row_origin(self, first_row):
        """The context holds rows [first_row, first_row + height) of a larger frame (row slabs): keeps the
        checkerboard phase of the update's summation order that of the whole frame (bit-identical results)."""
        self._check(self._lib.hsflow_set_row_origin(self._h, int(first_row)))

    # -- frames in -----------------------------------------------------------------------
    def set_frames(self, prev, curr, pair=0):
        """u8 single-channel frames: host numpy arrays (H, W) or CUDA tensors (H, W)."""
        if _is_device_tensor(prev):
            if str(prev.dtype) != "torch.uint8" or str(curr.dtype) != "torch.uint8":
                raise TypeError("Source images must have 8uC1 type")
            if tuple(prev.shape) != (self.height, self.width) or tuple(curr.shape) != (self.height, self.width):
                raise ValueError("frame shape must be (height, width)")
            self._check(self._lib.hsflow_set_frames_u8_device(
                self._h, pair, _ptr(prev), prev.stride(0), _ptr(curr), curr.stride(0)))
            return
        prev = np.asarray(prev)
        curr = np.asarray(curr)
        if prev.dtype != np.uint8 or curr.dtype != np.uint8:
            raise TypeError("Source images must have 8uC1 type")
        if prev.shape != (self.height, self.width) or curr.shape != (self.height, self.width):
            raise ValueError("frame shape must be (height, width)")
        if prev.strides[1] != 1:
            prev = np.ascontiguousarray(prev)
        if curr.strides[1] != 1:
            curr = np.ascontiguousarray(curr)
        self._check(self._lib.hsflow_set_frames_u8(self._h, pair, _ptr(prev), prev.strides[0],
                                                   _ptr(curr), curr.strides[0]))

    def set_frames_bgr(self, prev_bgr, curr_bgr, blur=True, pair=0):
        prev_bgr = np.ascontiguousarray(prev_bgr, dtype=np.uint8)
        curr_bgr = np.ascontiguousarray(curr_bgr, dtype=np.uint8)
        if prev_bgr.shape != (self.height, self.width, 3) or curr_bgr.shape != prev_bgr.shape:
            raise ValueError("colour frame shape must be (height, width, 3)")
        self._check(self._lib.hsflow_set_frames_bgr8(self._h, pair, _ptr(prev_bgr), prev_bgr.strides[0],
                                                     _ptr(curr_bgr), curr_bgr.strides[0], 1 if blur else 0))

    def set_frames_gray_blur(self, prev, curr, pair=0):
        """u8 gray frames, 3x3 box blur on the GPU first (the reference CPU route's cvSmooth)."""
        prev = np.ascontiguousarray(prev, dtype=np.uint8)
        curr = np.ascontiguousarray(curr, dtype=np.uint8)
        if prev.shape != (self.height, self.width) or curr.shape != prev.shape:
            raise ValueError("frame shape must be (height, width)")
        self._check(self._lib.hsflow_set_frames_gray8_blur(self._h, pair, _ptr(prev), prev.strides[0],
                                                           _ptr(curr), curr.strides[0]))

    def push_frame(self, nxt, pair=0):
        nxt = np.ascontiguousarray(nxt, dtype=np.uint8)
        if nxt.shape != (self.height, self.width):
            raise ValueError("frame shape must be (height, width)")
        self._check(self._lib.hsflow_push_frame_u8(self._h, pair, _ptr(nxt), nxt.strides[0]))

    def _device_frame(self, t, colour):
        """(pointer, row stride in bytes) of a CUDA uint8 tensor of shape (H, W) or (H, W, 3) with unit innermost stride."""
        want = (self.height, self.width, 3) if colour else (self.height, self.width)
        if not _is_device_tensor(t) or str(t.dtype) != "torch.uint8" or tuple(t.shape) != want or t.stride(-1) != 1 or (colour and t.stride(1) != 3):
            raise ValueError("device frames must be CUDA uint8 tensors of shape %r with packed pixels" % (want,))
        return _ptr(t), t.stride(0)

    def set_frames_device(self, prev, curr, frames="gray", pair=0):
        """Frames that already lie in device memory, in any layout: CUDA uint8 tensors of shape (H, W) ("gray",
        "gray_blur") or (H, W, 3) ("bgr", "bgr_blur") with unit innermost stride and any row stride.  The pre-processing
        of the pair is one launch on the context's stream (`hsflow_set_frames_device_ex`); only enqueued."""
        fmt = _lib.FRAME_FORMATS[frames]
        (pa, sa), (pb, sb) = (self._device_frame(t, fmt >= _lib.FRAMES_BGR8) for t in (prev, curr))
        self._check(self._lib.hsflow_set_frames_device_ex(self._h, pair, fmt, pa, sa, pb, sb))

    def set_sequence_device(self, frames_list, frames="gray", reblur=False, reblur_first=False, first_pair=0):
        """len(frames_list) >= 2 consecutive frames that lie in device memory (CUDA uint8 tensors as for
        `set_frames_device`, one row stride for all) into the pairs first_pair .. first_pair + len - 2: pair k holds
        (pre(frame k), pre(frame k + 1)); with reblur its previous frame is blurred once more -- the reference's camera
        loop, which blurs old and new in place -- for every pair but the first, and with reblur_first for the first too
        (the loop continued: frame 0 was the new frame of an earlier batch).  Every frame is read once, by one launch per
        `PRE_SEQ_MAX` frames (`hsflow_set_sequence_device_ex`); only enqueued."""
        fmt = _lib.FRAME_FORMATS[frames]
        targets = [self._device_frame(t, fmt >= _lib.FRAMES_BGR8) for t in frames_list]
        if len(set(s for _, s in targets)) > 1:
            raise ValueError("the frames of a sequence share one row stride")
        n = len(targets)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[p for p, _ in targets])
        self._check(self._lib.hsflow_set_sequence_device_ex(self._h, int(first_pair), fmt, ptrs, n, targets[0][1] if n else 0,
                                                            _seq_flags(reblur, reblur_first)))

    def push_frame_ex(self, nxt, frames="gray", reblur_prev=False, pair=0):
        """The camera sequence: the current frame becomes the previous one -- blurred once more with reblur_prev, which
        with a "*_blur" layout is the reference's loop -- and `nxt` is pre-processed into the current one.  nxt: a numpy
        array (uploaded; complete on return) or a CUDA tensor (only enqueued), shaped as for `set_frames_device`."""
        fmt = _lib.FRAME_FORMATS[frames]
        colour = fmt >= _lib.FRAMES_BGR8
        if _is_device_tensor(nxt):
            ptr, stride = self._device_frame(nxt, colour)
            self._check(self._lib.hsflow_push_frame_device_ex(self._h, pair, fmt, ptr, stride, 1 if reblur_prev else 0))
            return
        nxt = np.ascontiguousarray(nxt, dtype=np.uint8)
        if nxt.shape != ((self.height, self.width, 3) if colour else (self.height, self.width)):
            raise ValueError("frame shape must be (height, width) or, for colour, (height, width, 3)")
        self._check(self._lib.hsflow_push_frame_ex(self._h, pair, fmt, _ptr(nxt), nxt.strides[0], 1 if reblur_prev else 0))

    # -- solve ---------------------------------------------------------------------------
    def make_params(self, **kw):
        """hsflow_params with the defaults of hsflow_default_params; see `make_params` (module)."""
        return make_params(**kw)

    def solve(self, params=None, **kw):
        p = params if params is not None else self.make_params(**kw)
        self._check(self._lib.hsflow_solve(self._h, ctypes.byref(p)))
        return self.info()

    def solve_async(self, params=None, **kw):
        p = params if params is not None else self.make_params(**kw)
        self._check(self._lib.hsflow_solve_async(self._h, ctypes.byref(p)))

    def solve_pyramid(self, params=None, levels=0, min_size=32, warps=1, median_radius=0, pyramid=None, **kw):
        """The coarse-to-fine solve of every pair (`hsflow_solve_pyramid`): the frames halved level by level, the coarsest
        level solved from zero, and at every further step the second frame warped by the flow so far and the increment
        solved for, every solve with `params` (or make_params(**kw)).  levels, min_size, warps, median_radius as
        `make_pyramid_params` takes them (or pyramid: an HsflowPyramidParams).  The flow of level 0 is then the context's
        flow.  With ITER termination only enqueued.  Returns `pyramid_info()`."""
        p = params if params is not None else self.make_params(**kw)
        pp = pyramid if pyramid is not None else make_pyramid_params(levels, min_size, warps, median_radius)
        self._check(self._lib.hsflow_solve_pyramid(self._h, ctypes.byref(p), ctypes.byref(pp)))
        return self.pyramid_info()

    def pyramid_info(self):
        """What the last pyramid solve did: levels, warps, median_radius, sizes [(width, height)] per level, sweeps
        [level][step], solves, and the launches of the pyramid's kernels."""
        i = HsflowPyramidInfo()
        i.struct_size = ctypes.sizeof(HsflowPyramidInfo)
        self._check(self._lib.hsflow_get_pyramid_info(self._h, ctypes.byref(i)))
        n = i.levels
        return {"levels": n, "warps": i.warps, "median_radius": i.median_radius, "sizes": [(i.width[l], i.height[l]) for l in range(n)],
                "sweeps": [[i.sweeps[l][k] for k in range(i.warps)] for l in range(n)], "solves": i.solves, "down_launches": i.down_launches,
                "step_launches": i.step_launches, "total_launches": i.total_launches, "median_launches": i.median_launches}

    def pyramid_level(self, level, pair=0):
        """One level after the last pyramid solve: (prev, curr, u, v) of that level's size -- its frames (curr as `down` made
        it, not the warped one) and its total flow.  Complete on return."""
        i = HsflowPyramidInfo()
        i.struct_size = ctypes.sizeof(HsflowPyramidInfo)
        self._check(self._lib.hsflow_get_pyramid_info(self._h, ctypes.byref(i)))
        if not 0 <= level < i.levels:
            raise ValueError("level out of range")
        w, h = i.width[level], i.height[level]
        a, b = np.empty((h, w), np.uint8), np.empty((h, w), np.uint8)
        u, v = np.empty((h, w), np.float32), np.empty((h, w), np.float32)
        self._check(self._lib.hsflow_pyramid_get_level(self._h, int(level), int(pair), _ptr(a), a.strides[0], _ptr(b), b.strides[0], _ptr(u), u.strides[0],
                                                       _ptr(v), v.strides[0]))
        return a, b, u, v

    def set_eps_rows(self, first_row, rows):
        """Only the changes of rows [first_row, first_row + rows) count for Eps / the witness (rows <= 0: the whole frame)."""
        self._check(self._lib.hsflow_set_eps_rows(self._h, int(first_row), int(rows)))

    def solve_probe(self, params=None, **kw):
        """Exactly max_iter sweeps, nothing stops them; returns the Eps of every sweep (fp32 array)."""
        p = params if params is not None else self.make_params(**kw)
        out = np.empty(int(p.max_iter), np.float32)
        self._check(self._lib.hsflow_solve_probe(self._h, ctypes.byref(p), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out

    def solve_probe_pairs(self, params=None, **kw):
        """`solve_probe` with the Eps of every sweep per pair: an fp32 array of shape (max_iter, n_pairs).  Column i is what a
        one-pair context's `solve_probe` returns for pair i; the maximum of a row is what `solve_probe` returns."""
        p = params if params is not None else self.make_params(**kw)
        out = np.empty((int(p.max_iter), self.n_pairs), np.float32)
        self._check(self._lib.hsflow_solve_probe_pairs(self._h, ctypes.byref(p), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float))))
        return out

    def set_pair_termination(self, on):
        """on: under EPS termination every pair of the context stops on its own Eps, as cvCalcOpticalFlowHS called pair by
        pair does; off (the default): the batch stops as one, on the maximum of its pairs' Eps."""
        self._check(self._lib.hsflow_set_pair_termination(self._h, 1 if on else 0))

    def pair_results(self):
        """What the last solve did pair by pair: a list of dicts (pair, status, iterations_done, last_eps, eps_rerun,
        sweeps_executed).  While the batch stops as one, every pair reports the batch's values."""
        out = []
        for i in range(self.n_pairs):
            r = HsflowPairResult()
            r.struct_size = ctypes.sizeof(HsflowPairResult)
            self._check(self._lib.hsflow_get_pair_result(self._h, i, ctypes.byref(r)))
            out.append(r.as_dict())
        return out

    def take_verdict(self):
        """The early-stop check an asynchronous ITER|EPS solve owes, without acting on it: True = "no early stop" proven."""
        v = ctypes.c_int(0)
        self._check(self._lib.hsflow_take_verdict(self._h, ctypes.byref(v)))
        return bool(v.value)

    def synchronize(self):
        self._check(self._lib.hsflow_synchronize(self._h))

    # -- results out ---------------------------------------------------------------------
    def flow(self, pair=0):
        u = np.empty((self.height, self.width), np.float32)
        v = np.empty((self.height, self.width), np.float32)
        self._check(self._lib.hsflow_get_flow(self._h, pair, _ptr(u), u.strides[0], _ptr(v), v.strides[0]))
        return u, v

    def flow_rows_to(self, u_dev, v_dev, row0, nrows, pair=0):
        """Copy flow rows [row0, row0+nrows) into CUDA tensors of shape (nrows, width)."""
        self._check(self._lib.hsflow_get_flow_device(self._h, pair, row0, nrows, _ptr(u_dev),
                                                     u_dev.stride(0) * 4, _ptr(v_dev), v_dev.stride(0) * 4))

    def set_flow_rows_from(self, u_dev, v_dev, row0, nrows, pair=0, solver_made=False):
        """solver_made: the rows are flow a CV solve made (a neighbour slab's halo rows, this context's own saved flow):
        HSFLOW_FLOW_SOLVER_MADE, the next warm solve does not measure the planes."""
        self._check(self._lib.hsflow_set_flow_device_ex(self._h, pair, row0, nrows, _ptr(u_dev), u_dev.stride(0) * 4, _ptr(v_dev),
                                                        v_dev.stride(0) * 4, 1 if solver_made else 0))

    def render(self, route="cv", out=None, pair=0, params=None, **kw):
        """The reference's picture of the current flow of `pair`, drawn on the device (`make_render_params`: route, step,
        threshold, scale, dot_rgb, line_rgb).  out=None or a host array: returns an (H, W, 3) uint8 NumPy array, complete
        on return -- the flow itself is never downloaded.  out = a CUDA uint8 tensor of shape (H, W, 3): only enqueued on
        the context's stream (complete after `synchronize()`), returns `out`."""
        rp = params if params is not None else make_render_params(route, **kw)
        if _is_device_tensor(out):
            ptr, stride = _render_target(out, self.height, self.width)
            self._check(self._lib.hsflow_render_flow_device(self._h, pair, ctypes.byref(rp), ptr, stride))
            return out
        img = _render_host(out, self.height, self.width)
        self._check(self._lib.hsflow_render_flow(self._h, pair, ctypes.byref(rp), _ptr(img), img.strides[0]))
        return img

    def render_jpeg(self, route="cv", quality=95, pair=0, params=None, **kw):
        """The JPEG file of the picture `render` draws, as `bytes`: drawn and encoded on the device
        (`hsflow_render_flow_jpeg`), only the file crosses to the host.  quality 95 is what the reference's cvSaveImage
        uses: the bytes are then the reference's own output file.  Complete on return."""
        rp = params if params is not None else make_render_params(route, **kw)
        buf = np.empty(jpeg_bound(self.width, self.height), np.uint8)
        n = ctypes.c_size_t()
        self._check(self._lib.hsflow_render_flow_jpeg(self._h, pair, ctypes.byref(rp), int(quality), _ptr(buf), buf.size, ctypes.byref(n)))
        return buf[:n.value].tobytes()

    def color(self, max_flow=None, out=None, pair=0, params=None, return_scale=False):
        """The dense colour picture of the current flow of `pair` (the Middlebury wheel: hue is direction, saturation
        magnitude, zero flow white, unknown flow black), drawn on the device (`make_color_params`: max_flow=None scales by
        the picture's own largest flow).  out=None or a host array: returns an (H, W, 3) uint8 NumPy array, complete on
        return -- with return_scale=True the pair (picture, scale used).  out = a CUDA uint8 tensor of shape (H, W, 3):
        only enqueued on the context's stream (complete after `synchronize()`), returns `out`."""
        cp = params if params is not None else make_color_params(max_flow)
        if _is_device_tensor(out):
            ptr, stride = _render_target(out, self.height, self.width)
            self._check(self._lib.hsflow_color_flow_device(self._h, pair, ctypes.byref(cp), ptr, stride))
            return out
        img = _render_host(out, self.height, self.width)
        m = ctypes.c_float()
        self._check(self._lib.hsflow_color_flow(self._h, pair, ctypes.byref(cp), _ptr(img), img.strides[0], ctypes.byref(m)))
        return (img, m.value) if return_scale else img

    def color_jpeg(self, max_flow=None, quality=95, pair=0, params=None):
        """The JPEG file of the picture `color` draws, as `bytes`: drawn and encoded on the device
        (`hsflow_color_flow_jpeg`), only the file crosses to the host.  Complete on return."""
        cp = params if params is not None else make_color_params(max_flow)
        buf = np.empty(jpeg_bound(self.width, self.height), np.uint8)
        n = ctypes.c_size_t()
        self._check(self._lib.hsflow_color_flow_jpeg(self._h, pair, ctypes.byref(cp), int(quality), _ptr(buf), buf.size, ctypes.byref(n)))
        return buf[:n.value].tobytes()

    def color_jpeg_batch(self, max_flow=None, quality=95, first_pair=0, n=None, params=None):
        """`color_jpeg` for the pairs first_pair .. first_pair + n - 1 (n=None: all pairs from first_pair) by one set of
        launches per `JPEG_BATCH_MAX` pairs (`hsflow_color_flow_jpeg_batch`).  Returns the list of the files as `bytes`,
        each byte for byte what `color_jpeg(pair=i)` gives.  Complete on return."""
        cp = params if params is not None else make_color_params(max_flow)
        first_pair, n = self._batch_range(first_pair, n)
        bound = jpeg_bound(self.width, self.height)
        buf = np.empty((max(n, 1), bound), np.uint8)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[buf[i].ctypes.data for i in range(max(n, 1))])
        sizes = (ctypes.c_size_t * max(n, 1))()
        self._check(self._lib.hsflow_color_flow_jpeg_batch(self._h, first_pair, n, ctypes.byref(cp), int(quality), ptrs, bound, sizes))
        return [buf[i, :sizes[i]].tobytes() for i in range(n)]

    def color_batch_device(self, out, max_flow=None, first_pair=0, n=None, params=None):
        """`color` into caller tensors for the pairs first_pair .. first_pair + n - 1 (n=None: all pairs from first_pair)
        (`hsflow_color_flow_batch_device`).  out: a CUDA uint8 tensor (n, H, W, 3) or a list of n tensors (H, W, 3), packed
        pixels, one row stride for all.  Only enqueued on the context's stream (complete after `synchronize()`); returns
        `out`."""
        cp = params if params is not None else make_color_params(max_flow)
        first_pair, n = self._batch_range(first_pair, n)
        pictures = [out[i] for i in range(len(out))]
        if len(pictures) != n or not all(_is_device_tensor(t) for t in pictures):
            raise ValueError("out must hold one CUDA uint8 tensor of shape (height, width, 3) per pair")
        targets = [_render_target(t, self.height, self.width) for t in pictures]
        if len(set(s for _, s in targets)) > 1:
            raise ValueError("the pictures of a batch share one row stride")
        ptrs = (ctypes.c_void_p * max(n, 1))(*[p.value for p, _ in targets])
        self._check(self._lib.hsflow_color_flow_batch_device(self._h, first_pair, n, ctypes.byref(cp), ptrs, targets[0][1] if targets else 0))
        return out

    def warp(self, src=None, ref=None, out=None, pair=0, t=1.0, border="constant", fill=0, return_stats=False, params=None, picture=True):
        """`src` warped backwards by the current flow of `pair` (`make_warp_params`; include/hsflow.h has the rule): with
        t=1 the second frame of a pair onto the first.  src=None: the context's own pre-processed second frame, and ref=None
        then means its first.  `ref`: the picture the residual is taken against.  Host pictures (NumPy uint8 (H, W) or
        (H, W, 3)): synchronous, returns the warped picture, or with return_stats=True the pair (picture,
        `HsflowWarpStats`).  CUDA tensors (src, ref, out all on the device, or src=None and `out` on the device): only
        enqueued on the context's stream (complete after `synchronize()`); returns `out`, or with return_stats=True the
        pair (out, a CUDA uint8 tensor of 64 bytes that `warp_stats_from` reads).  picture=False: statistics only, no
        picture is written (returns None in its place)."""
        device, args, out, stats = _warp_call(self.height, self.width, self.device, src, ref, out, params, t, border, fill, return_stats, picture)
        self._check((self._lib.hsflow_warp_device if device else self._lib.hsflow_warp)(self._h, pair, *args))
        return (out, stats) if return_stats else out

    def warp_batch_device(self, out=None, src=None, ref=None, stats=None, first_pair=0, n=None, t=1.0, border="constant", fill=0, params=None):
        """`warp` on the device for the pairs first_pair .. first_pair + n - 1 (n=None: all pairs from first_pair) by one
        launch per `JPEG_BATCH_MAX` pairs (`hsflow_warp_batch_device`).  out, src, ref: each None, a CUDA uint8 tensor
        (n, H, W[, C]) or a list of n tensors (H, W[, C]); one row stride per list.  src=None: the context's own second
        frames (and ref=None then its first).  out=None: statistics only.  stats: None, or a CUDA uint8 tensor of n * 64
        bytes that receives record i of pair first_pair + i (`warp_stats_from`).  Only enqueued on the context's stream
        (complete after `synchronize()`); returns `out`."""
        first_pair, n = self._batch_range(first_pair, n)
        (sl, ss, s_), (rl, rs, r_), (ol, os_, o_) = [
            _plane_lists(x, n, what, "picture per pair", lambda img, what=what: _warp_image(img, self.height, self.width, what, True))
            for x, what in ((src, "src"), (ref, "ref"), (out, "out"))]
        channels = set(c for _, _, c in s_ + r_ + o_)
        if len(channels) > 1:
            raise ValueError("src, ref and out must have the same number of channels")
        wp = params if params is not None else make_warp_params(channels.pop() if channels else 1, t, border, fill)
        sref = _check_stats_tensor(stats, n, HsflowWarpStats)
        self._check(self._lib.hsflow_warp_batch_device(self._h, first_pair, n, ctypes.byref(wp), sl, ss, rl, rs, ol, os_, sref))
        return out

    def interp(self, t=0.5, prev=None, curr=None, vis_prev=None, vis_curr=None, ref=None, out=True, classes=False, stats=False, pair=0, params=None):
        """The frame at time `t` (0 .. 1) between the two frames of `pair` from its current flow (`make_interp_params`;
        include/hsflow.h has the rule).  prev, curr: the two pictures, uint8 (H, W) or (H, W, 3); both None: the context's
        own pre-processed frames.  vis_prev, vis_curr: optional uint8 (H, W) visibility planes (the masks of `fb`).  ref:
        the true frame, for the record's sad.  out, classes: False, True (allocated) or the array to fill; stats: bool.
        Host arrays: synchronous.  CUDA tensors: only enqueued on the context's stream (complete after `synchronize()`),
        the record then a CUDA uint8 tensor of 64 bytes that `interp_stats_from` reads.  Returns (out, classes, stats)."""
        device, args, out, classes, rec = _interp_call(self.height, self.width, self.device, prev, curr, vis_prev, vis_curr, ref, out, classes, stats, params, False)
        self._check((self._lib.hsflow_interp_device if device else self._lib.hsflow_interp)(self._h, pair, float(t), *args))
        return out, classes, rec

    def interp_batch_device(self, times, out=None, prev=None, curr=None, vis_prev=None, vis_curr=None, ref=None, classes=None, stats=None, pair=0, params=None):
        """`interp` on the device for the n = len(times) times of ONE pair by one set of launches per `INTERP_BATCH_MAX`
        times (`hsflow_interp_batch_device`).  out, ref: None, a CUDA uint8 tensor (n, H, W[, C]) or a list of n; classes:
        None or (n, H, W); prev, curr, vis_prev, vis_curr: as `interp` takes them, on the device; stats: None or a CUDA
        uint8 tensor of n * 64 bytes (`interp_stats_from`).  Only enqueued; returns `out`."""
        tt = [float(x) for x in times]
        n = len(tt)
        (rl, rs, r_), (ol, os_, o_) = [
            _plane_lists(x, n, what, "picture per time", lambda img, what=what: _warp_image(img, self.height, self.width, what, True))
            for x, what in ((ref, "ref"), (out, "out"))]
        kl, ks, _ = _plane_lists(classes, n, "classes", "plane per time", lambda x: _plane(x, self.height, self.width, "uint8", "classes", True))
        pics = [(_warp_image(x, self.height, self.width, what, True) if x is not None else (None, 0, None)) for x, what in ((prev, "prev"), (curr, "curr"))]
        channels = set(c for _, _, c in r_ + o_) | set(c for _, _, c in pics if c is not None)
        if len(channels) > 1:
            raise ValueError("prev, curr, ref and out must have the same number of channels")
        ip = params if params is not None else make_interp_params(channels.pop() if channels else 1)
        (vpp, vps), (vcp, vcs) = [(_plane(x, self.height, self.width, "uint8", what, True) if x is not None else (None, 0))
                                  for x, what in ((vis_prev, "vis_prev"), (vis_curr, "vis_curr"))]
        sref = _check_stats_tensor(stats, n, HsflowInterpStats)
        (pp, ps, _), (cp, cs, _) = pics
        self._check(self._lib.hsflow_interp_batch_device(self._h, pair, n, (ctypes.c_float * max(n, 1))(*tt), ctypes.byref(ip), pp, ps, cp, cs, vpp, vps, vcp, vcs,
                                                         rl, rs, ol, os_, kl, ks, sref))
        return out

    def project_flow(self, t=1.0, prev=None, curr=None, flow=True, state=False, stats=False, pair=0, params=None):
        """The flow of `pair` projected to time `t` and hole-filled, on the device (`hsflow_project_flow_device`): with
        t=1 the flow on the second frame's grid, what a camera loop hands to the next pair (`set_flow`, use_previous).
        prev, curr: CUDA uint8 pictures, or both None: the context's own frames.  flow: True (two CUDA float32 (H, W)
        tensors are allocated), False, or a pair of them; state: True, False or a CUDA uint8 (H, W) tensor (0 unfilled,
        1 hit, 2 filled); stats: bool (a CUDA uint8 tensor of 64 bytes, `interp_stats_from`).  Only enqueued on the
        context's stream.  Returns (u, v, state, stats)."""
        args, u, v, state, rec = _project_call(self.height, self.width, self.device, prev, curr, flow, state, stats, params, True)
        self._check(self._lib.hsflow_project_flow_device(self._h, pair, float(t), *args))
        return u, v, state, rec

    def set_frames_reversed(self, dst_pair, src_pair):
        """Pair `dst_pair` receives the pre-processed frames of `src_pair`, swapped (`hsflow_set_frames_reversed`): the
        reversed pair of a bidirectional solve, by device copies on the context's stream."""
        self._check(self._lib.hsflow_set_frames_reversed(self._h, int(dst_pair), int(src_pair)))

    def fb(self, fwd_pair=0, bwd_pair=1, mask=True, err2=False, stats=False, alpha=0.01, beta=0.5, values=(255, 0, 0, 0), params=None, device=False):
        """The forward-backward check of the flow of `fwd_pair` against that of `bwd_pair` (`make_fb_params`;
        include/hsflow.h has the rule).  mask, err2: False (not wanted), True (allocated here) or the plane to fill -- uint8
        and float32 of shape (H, W), any row stride; stats: True for the statistics.  Host planes: synchronous.  CUDA
        tensors (or device=True for planes allocated here): only enqueued on the context's stream (complete after
        `synchronize()`), the statistics then a CUDA uint8 tensor of 64 bytes that `fb_stats_from` reads.  Returns (mask,
        err2, stats), None for what was not asked for."""
        device, args, mask, err2, rec = _fb_call(self.height, self.width, self.device, mask, err2, stats, params, alpha, beta, values, device)
        self._check((self._lib.hsflow_fb_device if device else self._lib.hsflow_fb)(self._h, int(fwd_pair), int(bwd_pair), *args))
        return mask, err2, rec

    def fb_planes(self, ub, vb, fwd_pair=0, mask=True, err2=False, stats=False, alpha=0.01, beta=0.5, values=(255, 0, 0, 0), params=None, device=False):
        """`fb` with the backward flow from CUDA float32 tensors (H, W) of one row stride (`hsflow_fb_planes_device`,
        `hsflow_fb_planes`): another context's flow, or a flow from elsewhere, ordered before this context's stream by the
        caller."""
        strides = set(tuple(x.stride()) for x in (ub, vb))
        if (not all(_is_device_tensor(x) and str(x.dtype) == "torch.float32" and tuple(x.shape) == (self.height, self.width) for x in (ub, vb))
                or len(strides) != 1 or ub.stride(1) != 1):
            raise ValueError("ub and vb must be CUDA float32 tensors (height, width) of one row stride")
        device, args, mask, err2, rec = _fb_call(self.height, self.width, self.device, mask, err2, stats, params, alpha, beta, values, device)
        self._check((self._lib.hsflow_fb_planes_device if device else self._lib.hsflow_fb_planes)(self._h, int(fwd_pair), _ptr(ub), _ptr(vb),
                                                                                                 ub.stride(0) * 4, *args))
        return mask, err2, rec

    def fb_batch_device(self, fwd_pairs, bwd_pairs, mask=None, err2=None, stats=None, alpha=0.01, beta=0.5, values=(255, 0, 0, 0), params=None):
        """`fb` on the device for the checks (fwd_pairs[i], bwd_pairs[i]) by one launch per `JPEG_BATCH_MAX` checks
        (`hsflow_fb_batch_device`).  mask, err2: each None, a CUDA tensor (n, H, W) or a list of n tensors (H, W), uint8 and
        float32; one row stride per list.  stats: None, or a CUDA uint8 tensor of n * 64 bytes that receives record i of
        check i (`fb_stats_from`).  Only enqueued on the context's stream (complete after `synchronize()`)."""
        n = len(fwd_pairs)
        if len(bwd_pairs) != n:
            raise ValueError("fwd_pairs and bwd_pairs must have one length")
        (ml, ms, _), (el, es, _) = [
            _plane_lists(x, n, what, "plane per check", lambda p, dtype=dtype, what=what: _plane(p, self.height, self.width, dtype, what, True))
            for x, dtype, what in ((mask, "uint8", "mask"), (err2, "float32", "err2"))]
        fp = params if params is not None else make_fb_params(alpha, beta, values)
        sref = _check_stats_tensor(stats, n, HsflowFbStats)
        ints = ctypes.c_int * max(n, 1)
        self._check(self._lib.hsflow_fb_batch_device(self._h, n, ints(*[int(p) for p in fwd_pairs]), ints(*[int(p) for p in bwd_pairs]), ctypes.byref(fp),
                                                     ml, ms, el, es, sref))
        return mask, err2, stats

    def global_motion(self, pair=0, state=None, mask=False, residual=False, result=True, params=None, device=False):
        """The global motion that explains the current flow of `pair` -- the camera's -- by `hsflow_gmotion_fit[_device]`
        (`make_gmotion_params`; include/hsflow.h has the rule).  state: None or a u8 plane (H, W), non-zero = trusted (the
        mask of `fb`); mask: False, True (allocated here) or the u8 plane to fill with the class bytes; residual: False, True
        or the pair (res_u, res_v): the flow relative to the model.  Host planes: synchronous, the result an
        `HsflowGmotionResult`.  CUDA tensors (or device=True): only enqueued on the context's stream, the result then a
        CUDA uint8 tensor of 64 bytes that `gmotion_result_from` reads.  Returns (result, mask, res_u, res_v), None for
        what was not asked for."""
        device = _chain_device(device, state, mask, residual)
        args, rec, mask, ru, rv = _gmotion_call(self.height, self.width, self.device, state, mask, residual, result, params, device)
        self._check((self._lib.hsflow_gmotion_fit_device if device else self._lib.hsflow_gmotion_fit)(self._h, int(pair), *args))
        return rec, mask, ru, rv

    def global_motion_planes_device(self, u, v, state=None, mask=False, residual=False, result=True, params=None):
        """`global_motion` on the device of caller planes u, v (CUDA float32 (H, W), one row stride) -- the U and V of
        `chain_flow(device=True)`, another context's `flow_view_device` (`hsflow_gmotion_fit_planes_device`).  Only enqueued."""
        (up, us), (vp, vs) = [_plane(x, self.height, self.width, "float32", "flow", True) for x in (u, v)]
        if us != vs:
            raise ValueError("the two flow planes share one row stride")
        args, rec, mask, ru, rv = _gmotion_call(self.height, self.width, self.device, state, mask, residual, result, params, True)
        self._check(self._lib.hsflow_gmotion_fit_planes_device(self._h, up, vp, us, *args))
        return rec, mask, ru, rv

    def global_motion_batch_device(self, first_pair=0, n=None, state=None, mask=None, res_u=None, res_v=None, results=None, params=None):
        """`global_motion` on the device for the pairs first_pair .. first_pair + n - 1 (n=None: all pairs from first_pair)
        by one set of launches (`hsflow_gmotion_fit_batch_device`).  state, mask, res_u, res_v: None, or lists of n entries,
        each None or a CUDA plane (H, W); one row stride per list.  results: None, or a CUDA uint8 tensor of n * 64 bytes
        (`gmotion_result_from`).  Only enqueued."""
        first_pair, n = self._batch_range(first_pair, n)
        H, W = self.height, self.width
        (sl, ss), (ml, ms) = [_chain_list(x, n, H, W, "uint8", what, True, holes=True) for x, what in ((state, "state"), (mask, "mask"))]
        (ul, us), (vl, vs) = [_chain_list(x, n, H, W, "float32", "residual", True, holes=True) for x in (res_u, res_v)]
        if us != vs:
            raise ValueError("the residual planes share one row stride")
        gp = params if params is not None else make_gmotion_params()
        self._check(self._lib.hsflow_gmotion_fit_batch_device(self._h, first_pair, n, sl, ss, ctypes.byref(gp), ml, ms, ul, vl, us,
                                                               _check_stats_tensor(results, n, HsflowGmotionResult)))
        return results

    def regions(self, pair=0, mask=None, labels=False, records=True, capacity=64, result=True, params=None, device=False):
        """The moving objects of `pair`: the connected regions of the foreground `mask` (None: every pixel; a u8 plane (H,
        W), e.g. the mask of `global_motion` with values (0, 255, 0, 0)) with the pair's current flow, by
        `hsflow_regions[_device]` (`make_regions_params`; include/hsflow.h has the rule).  labels: False, True or the int32
        plane to fill; records: False, True (`capacity` records allocated here) or the array; result: True or False.  Host
        planes: synchronous, the result an `HsflowRegionsResult`, the records a ctypes array of `HsflowRegionsRecord` of
        which the first `n_written` are valid.  CUDA tensors (or device=True): only enqueued on the context's stream, result
        and records then CUDA uint8 tensors that `regions_result_from` / `regions_records_from` read.  Returns (result,
        labels, records), None for what was not asked for."""
        device = _chain_device(device, mask, labels, records if not isinstance(records, ctypes.Array) else None)
        args, rec, labels, records = _regions_call(self.height, self.width, self.device, mask, labels, records, capacity, result, params, device)
        self._check((self._lib.hsflow_regions_device if device else self._lib.hsflow_regions)(self._h, int(pair), *args))
        return rec, labels, records

    def regions_planes_device(self, mask=None, u=None, v=None, labels=False, records=True, capacity=64, result=True, params=None):
        """`regions` on the device of caller planes: mask None or a CUDA u8 plane, u, v None or CUDA float32 planes (H, W)
        of one row stride (`hsflow_regions_planes_device`).  Only enqueued."""
        if (u is None) != (v is None):
            raise ValueError("u and v are given together or not at all")
        up = vp = None
        us = 0
        if u is not None:
            (up, us), (vp, vs) = [_plane(x, self.height, self.width, "float32", "flow", True) for x in (u, v)]
            if us != vs:
                raise ValueError("the two flow planes share one row stride")
        args, rec, labels, records = _regions_call(self.height, self.width, self.device, mask, labels, records, capacity, result, params, True)
        self._check(self._lib.hsflow_regions_planes_device(self._h, args[0], args[1], up, vp, us, *args[2:]))
        return rec, labels, records

    def regions_batch_device(self, first_pair=0, n=None, mask=None, labels=None, records=None, capacity=64, results=None, params=None):
        """`regions` on the device for the pairs first_pair .. first_pair + n - 1 (n=None: all pairs from first_pair) by
        one set of launches (`hsflow_regions_batch_device`), each with its own flow.  mask, labels: None, or lists of n
        entries, each None or a CUDA plane (H, W); one row stride per list.  records: None, or a list of n entries, each
        None or a contiguous CUDA uint8 tensor of capacity * 64 bytes.  results: None, or a CUDA uint8 tensor of n * 64
        bytes (`regions_result_from`).  Only enqueued."""
        first_pair, n = self._batch_range(first_pair, n)
        H, W = self.height, self.width
        ml, ms = _chain_list(mask, n, H, W, "uint8", "mask", True, holes=True)
        ll, ls = _chain_list(labels, n, H, W, "int32", "labels", True, holes=True)
        rl = None
        if records is not None:
            if len(records) != n:
                raise ValueError("records must hold one entry per pair")
            for r in records:
                if r is not None and (not _is_device_tensor(r) or str(r.dtype) != "torch.uint8" or not r.is_contiguous() or r.numel() < int(capacity) * 64):
                    raise ValueError("a record array must be a contiguous CUDA uint8 tensor of at least capacity * 64 bytes")
            rl = (ctypes.c_void_p * n)(*[r.data_ptr() if r is not None else None for r in records])
        prm = params if params is not None else make_regions_params()
        self._check(self._lib.hsflow_regions_batch_device(self._h, first_pair, n, ml, ms, ctypes.byref(prm), ll, ls, rl, int(capacity),
                                                           _check_stats_tensor(results, n, HsflowRegionsResult)))
        return results

    def corners(self, pair=0, which=0, mask=None, capacity=1024, records=True, xy=False, result=True, params=None, device=False):
        """The points of a frame worth following: the corners of the context's own pre-processed gray plane of `pair`
        (`which` 0: the prev frame, 1: the curr frame), by `hsflow_corners[_device]` (`make_corners_params`;
        include/hsflow.h has the rule).  mask: None or a u8 plane (H, W) of the pixels that may be corners; records: False,
        True (`capacity` records allocated here) or the array; xy: False, True or a float32 array (capacity, 2), whose slots
        from n_written on come back NaN -- what `track_points` takes as it is; result: True or False.  Host arrays:
        synchronous, the result an `HsflowCornersResult`, the records a ctypes array of `HsflowCornersRecord` of which the
        first `n_written` are valid.  CUDA tensors (or device=True): only enqueued on the context's stream, result and
        records then CUDA uint8 tensors that `corners_result_from` / `corners_records_from` read.  Returns (result, records,
        xy), None for what was not asked for."""
        device = _chain_device(device, mask, xy, records if not isinstance(records, ctypes.Array) else None)
        args, rec, records, xy = _corners_call(self.height, self.width, self.device, mask, records, capacity, xy, result, params, device)
        self._check((self._lib.hsflow_corners_device if device else self._lib.hsflow_corners)(self._h, int(pair), int(which), *args))
        return rec, records, xy

    def corners_planes_device(self, gray, mask=None, capacity=1024, records=True, xy=False, result=True, params=None):
        """`corners` on the device of a caller's plane: gray a CUDA u8 plane (H, W) of the context's size, any row stride
        (`hsflow_corners_planes_device`).  Only enqueued."""
        gp, gs = _plane(gray, self.height, self.width, "uint8", "gray", True)
        args, rec, records, xy = _corners_call(self.height, self.width, self.device, mask, records, capacity, xy, result, params, True)
        self._check(self._lib.hsflow_corners_planes_device(self._h, gp, gs, *args))
        return rec, records, xy

    def corners_batch_device(self, first_pair=0, n=None, which=0, mask=None, records=None, capacity=1024, xy=None, results=None, params=None):
        """`corners` on the device for the pairs first_pair .. first_pair + n - 1 (n=None: all pairs from first_pair) by one
        set of launches (`hsflow_corners_batch_device`).  mask: None, or a list of n entries, each None or a CUDA u8 plane
        (H, W), one row stride.  records: None, or a list of n entries, each None or a contiguous CUDA uint8 tensor of
        capacity * 16 bytes; xy: None, or a list of n entries, each None or a contiguous CUDA float32 tensor (capacity, 2).
        results: None, or a CUDA uint8 tensor of n * 64 bytes (`corners_result_from`).  Only enqueued."""
        first_pair, n = self._batch_range(first_pair, n)
        capacity = int(capacity)
        ml, ms = _chain_list(mask, n, self.height, self.width, "uint8", "mask", True, holes=True)
        rl = _link_list(records, n, capacity, HsflowCornersRecord, "records")
        xl = None
        if xy is not None:
            if len(xy) != n:
                raise ValueError("xy must hold one entry per pair")
            xl = (ctypes.c_void_p * n)(*[_corners_xy(x, capacity, True, self.device)[1].value if x is not None else None for x in xy])
        prm = params if params is not None else make_corners_params()
        self._check(self._lib.hsflow_corners_batch_device(self._h, first_pair, n, int(which), ml, ms, ctypes.byref(prm), rl, capacity, xl,
                                                           _check_stats_tensor(results, n, HsflowCornersResult)))
        return results

    def link_regions(self, pair=0, labels_a=None, labels_b=None, links=True, link_capacity=256, side_a=True, side_b=True, result=True, params=None,
                     device=False):
        """The regions of frame k (int32 label plane `labels_a`, (H, W)) linked to those of frame k + 1 (`labels_b`) by the
        current flow of `pair`: how many pixels of region a arrive in region b (`hsflow_link_regions[_device]`,
        `make_link_params`; include/hsflow.h has the rule).  links, side_a, side_b: False, True (allocated here) or the
        array; result: True or False.  Host planes: synchronous, the result an `HsflowLinkResult`, the links a ctypes array
        of `HsflowLinkRecord` of which the first `n_written` are valid, the sides ctypes arrays of `HsflowLinkSide`.  CUDA
        tensors (or device=True): only enqueued on the context's stream, everything a CUDA uint8 tensor that
        `link_result_from` / `link_records_from` / `link_sides_from` read.  Returns (result, links, side_a, side_b), None for
        what was not asked for."""
        device = _chain_device(device, labels_a, labels_b)
        (ap, as_), (bp, bs) = [_plane(x, self.height, self.width, "int32", "labels", device) for x in (labels_a, labels_b)]
        args, rec, links, side_a, side_b = _link_call(self.device, links, link_capacity, side_a, side_b, result, params, device)
        if device:
            if as_ != bs:
                raise ValueError("the two label planes share one row stride")
            self._check(self._lib.hsflow_link_regions_device(self._h, int(pair), ap, bp, as_, *args))
        else:
            self._check(self._lib.hsflow_link_regions(self._h, int(pair), ap, as_, bp, bs, *args))
        return rec, links, side_a, side_b

    def link_regions_planes_device(self, labels_a, labels_b, u, v, links=True, link_capacity=256, side_a=True, side_b=True, result=True, params=None):
        """`link_regions` on the device of caller planes: CUDA int32 label planes and CUDA float32 flow planes (H, W), u and
        v of one row stride (`hsflow_link_regions_planes_device`).  Only enqueued."""
        (ap, as_), (bp, bs) = [_plane(x, self.height, self.width, "int32", "labels", True) for x in (labels_a, labels_b)]
        (up, us), (vp, vs) = [_plane(x, self.height, self.width, "float32", "flow", True) for x in (u, v)]
        if us != vs:
            raise ValueError("the two flow planes share one row stride")
        args, rec, links, side_a, side_b = _link_call(self.device, links, link_capacity, side_a, side_b, result, params, True)
        self._check(self._lib.hsflow_link_regions_planes_device(self._h, ap, as_, bp, bs, up, vp, us, *args))
        return rec, links, side_a, side_b

    def link_regions_batch_device(self, first_pair=0, n_steps=None, labels=None, links=None, link_capacity=256, side_a=None, side_b=None, results=None,
                                  params=None):
        """`link_regions` on the device for n_steps steps (None: all pairs from first_pair): step i links labels[i] to
        labels[i + 1] -- n_steps + 1 CUDA int32 planes of one row stride -- by the flow of pair first_pair + i
        (`hsflow_link_regions_batch_device`).  links, side_a, side_b: None, or lists of n_steps entries, each None or a
        contiguous CUDA uint8 tensor of link_capacity * 16, cap_a * 32, cap_b * 32 bytes.  results: None, or a CUDA uint8
        tensor of n_steps * 64 bytes (`link_result_from`).  Only enqueued."""
        first_pair, n = self._batch_range(first_pair, n_steps)
        prm = params if params is not None else make_link_params()
        ll, ls = _chain_list(labels, n + 1, self.height, self.width, "int32", "labels", True)
        if ll is None:
            raise ValueError("labels is needed: n_steps + 1 planes")
        self._check(self._lib.hsflow_link_regions_batch_device(self._h, first_pair, n, ll, ls, ctypes.byref(prm),
                                                                _link_list(links, n, int(link_capacity), HsflowLinkRecord, "links"), int(link_capacity),
                                                                _link_list(side_a, n, prm.cap_a, HsflowLinkSide, "side_a"),
                                                                _link_list(side_b, n, prm.cap_b, HsflowLinkSide, "side_b"),
                                                                _check_stats_tensor(results, n, HsflowLinkResult)))
        return results

    def gmotion_warp(self, model, src, ref=None, out=None, t=1.0, border="constant", fill=0, return_stats=False, params=None, picture=True):
        """`src` warped backwards by the motion `model` (six floats or an `HsflowGmotionResult`) alone, no flow plane read
        (`hsflow_gmotion_warp[_device]`); everything else as `warp` takes and returns it."""
        if src is None:
            raise ValueError("src is needed")
        device, args, out, stats = _warp_call(self.height, self.width, self.device, src, ref, out, params, t, border, fill, return_stats, picture)
        self._check((self._lib.hsflow_gmotion_warp_device if device else self._lib.hsflow_gmotion_warp)(self._h, _gmotion_model(model), *args))
        return (out, stats) if return_stats else out

    def stabilize(self, src, pair=0, state=None, params=None, t=1.0, border="constant", fill=0, return_model=False):
        """`src` (the second frame of `pair`, any channels `warp` takes) warped onto the first frame by the fitted global
        motion of the pair's flow, not by the dense flow: `global_motion` for the model (64 bytes read back), then
        `gmotion_warp`.  A CUDA `src` stays on the device.  Returns the picture, or with return_model=True (picture,
        `HsflowGmotionResult`)."""
        device = _is_device_tensor(src)
        rec, _, _, _ = self.global_motion(pair=pair, state=state, params=params, device=device)
        if device:
            self.synchronize()
            rec = gmotion_result_from(rec)
        out = self.gmotion_warp(rec, src, t=t, border=border, fill=fill)
        return (out, rec) if return_model else out

    def _chain_pairs(self, pairs):
        pairs = list(range(self.n_pairs)) if pairs is None else [int(p) for p in pairs]
        if not 1 <= len(pairs) <= CHAIN_MAX_PAIRS:
            raise ValueError("a chain takes 1 .. %d pairs; a longer one continues through `start`" % CHAIN_MAX_PAIRS)
        return pairs, (ctypes.c_int * len(pairs))(*pairs)

    def chain_flow(self, pairs=None, state=None, start=None, flow=True, status=False, age=False, stats=False, params=None, device=False):
        """The flow from the first frame of the sequence to the last: every pixel followed through the flows of `pairs`
        (None: all pairs of the context in order; at most 32, repeats allowed) by `hsflow_chain_flow[_device]`;
        include/hsflow.h has the rule.  state: None or a list with one entry per pair, each None or a u8 plane (H, W), non-zero
        = trusted (the masks of `fb`); start: None or the pair (U0, V0) a call before left -- a longer chain in two calls;
        flow: False, True (allocated here) or the pair (U, V) to fill; status, age: False, True or the u8 plane; stats: True
        for the statistics.  Host planes: synchronous.  CUDA tensors (or device=True): only enqueued on the context's stream,
        the statistics then a CUDA uint8 tensor of 64 bytes that `chain_stats_from` reads.  Returns (U, V, status, age,
        stats), None for what was not asked for."""
        pairs, ints = self._chain_pairs(pairs)
        device = _chain_device(device, state, start, flow, status, age)
        args, U, V, status, age, rec = _chain_call(self.height, self.width, self.device, len(pairs), state, start, flow, status, age, stats, params, device)
        self._check((self._lib.hsflow_chain_flow_device if device else self._lib.hsflow_chain_flow)(self._h, ints, len(pairs), *args))
        return U, V, status, age, rec

    def chain_planes_device(self, u, v, state=None, start=None, flow=True, status=False, age=False, stats=False, params=None):
        """`chain_flow` on the device through caller planes (`hsflow_chain_planes_device`): u, v lists of n CUDA float32
        tensors (H, W) of one row stride -- other contexts' `flow_view_device`, or flows from elsewhere, ordered before this
        context's stream by the caller.  Only enqueued."""
        n = len(u)
        if len(v) != n or not 1 <= n <= CHAIN_MAX_PAIRS:
            raise ValueError("u and v hold one plane each per pair, 1 .. %d pairs" % CHAIN_MAX_PAIRS)
        (ul, us), (vl, vs) = [_chain_list(x, n, self.height, self.width, "float32", "flow", True) for x in (u, v)]
        if us != vs:
            raise ValueError("all flow planes share one row stride")
        args, U, V, status, age, rec = _chain_call(self.height, self.width, self.device, n, state, start, flow, status, age, stats, params, True)
        self._check(self._lib.hsflow_chain_planes_device(self._h, n, ul, vl, us, *args))
        return U, V, status, age, rec

    def track_points(self, xy, pairs=None, state=None, track=False, status=False, age=False, stats=False, device=False, params=None):
        """The points xy -- float32 (m, 2), positions (x, y) in the first frame -- followed through the flows of `pairs`
        (`hsflow_track_points[_device]`).  track: True for the positions after 0 .. n pairs as float32 (n + 1, m, 2), the NaN
        bits from the step at which a point was lost; status, age: True for the u8 arrays (m,); stats: True for the
        statistics.  A NumPy xy: synchronous; a CUDA tensor (or device=True with one): only enqueued.  Returns (last, track,
        status, age, stats) with last the float32 (m, 2) positions in the last frame, NaN for lost points."""
        pairs, ints = self._chain_pairs(pairs)
        n = len(pairs)
        device = _chain_device(device, xy, state)
        if device != _is_device_tensor(xy) or (not device and not isinstance(xy, np.ndarray)):
            raise ValueError("xy must be %s" % ("a CUDA tensor" if device else "a NumPy array"))
        if str(xy.dtype) not in ("float32", "torch.float32") or xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
            raise ValueError("xy must be float32 of shape (m, 2)")
        if not (xy.is_contiguous() if device else xy.flags.c_contiguous):
            raise ValueError("xy must be contiguous")
        m = int(xy.shape[0])

        def fresh(shape, dtype):
            if device:
                import torch
                return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda:%d" % self.device)
            return np.empty(shape, dtype)
        sl, ss = _chain_list(state, n, self.height, self.width, "uint8", "state", device, holes=True)
        last = fresh((m, 2), "float32")
        track = fresh((n + 1, m, 2), "float32") if track else None
        status = fresh((m,), "uint8") if status else None
        age = fresh((m,), "uint8") if age else None
        cp = params if params is not None else make_chain_params()
        rec, sref = _stats_record(HsflowChainStats, stats, device, self.device)
        opt = lambda x: _ptr(x) if x is not None else None
        self._check((self._lib.hsflow_track_points_device if device else self._lib.hsflow_track_points)(
            self._h, ints, n, sl, ss, ctypes.byref(cp), _ptr(xy), m, opt(track), _ptr(last), opt(status), opt(age), sref))
        return last, track, status, age, rec

    def median(self, pair=0, state=None, flow=True, state_out=False, stats=False, radius=1, mode="filter", min_votes=1, passes=1, params=None, device=False):
        """The median filter / hole filling of the flow of `pair` (`make_median_params`; include/hsflow.h has the rule); the
        context's flow is not changed.  state: None or the u8 plane (H, W) of input states (0 invalid, 2 filled, else kept:
        the default mask of `fb` as it is); flow: False, True (allocated here) or the pair (u_out, v_out) to fill;
        state_out: False, True or the plane to fill; stats: True for the record of the last pass.  Host planes:
        synchronous, `passes` passes (`hsflow_median`).  CUDA tensors (or device=True): one pass, only enqueued on the
        context's stream (`hsflow_median_device`, complete after `synchronize()`), the record then a CUDA uint8 tensor
        of 64 bytes that `median_stats_from` reads.  Returns (u_out, v_out, state_out, stats), None for what was not
        asked for."""
        planes = [state, state_out] + (list(flow) if isinstance(flow, (tuple, list)) else [])
        device = bool(device) or any(_is_device_tensor(x) for x in planes)
        mp, (sp, ss), (up, vp, os_), (sop, sos), sref, u_out, v_out, state_out, rec = _median_call(
            self.height, self.width, self.device, state, flow, state_out, stats, params, radius, mode, min_votes, device)
        if device:
            if int(passes) != 1:
                raise ValueError("the device form runs one pass: chain `median_planes_device`, or use `median_apply`")
            self._check(self._lib.hsflow_median_device(self._h, int(pair), ctypes.byref(mp), sp, ss, up, vp, os_, sop, sos, sref))
        else:
            self._check(self._lib.hsflow_median(self._h, int(pair), ctypes.byref(mp), int(passes), sp, ss, up, vp, os_, sop, sos, sref))
        return u_out, v_out, state_out, rec

    def median_apply(self, pair=0, state=None, passes=1, state_out=False, stats=False, radius=1, mode="filter", min_votes=1, params=None):
        """`passes` passes of the median whose result REPLACES the flow of `pair` in the context (`hsflow_median_apply`):
        every later picture, warp, check and `use_previous` solve reads it.  state, state_out: CUDA uint8 tensors (H, W) as
        `median` takes them; only enqueued on the context's stream.  Returns (state_out, stats) of the last pass."""
        mp, (sp, ss), _, (sop, sos), sref, _, _, state_out, rec = _median_call(
            self.height, self.width, self.device, state, None, state_out, stats, params, radius, mode, min_votes, True)
        self._check(self._lib.hsflow_median_apply(self._h, int(pair), ctypes.byref(mp), int(passes), sp, ss, sop, sos, sref))
        return state_out, rec

    def median_planes_device(self, u, v, state=None, flow=True, state_out=False, stats=False, radius=1, mode="filter", min_votes=1, params=None):
        """One pass of the median over CUDA float32 tensors (H, W) of one row stride (`hsflow_median_planes_device`), only
        enqueued on the context's stream; the output state is a valid input state, so passes are chained by calling again
        with the outputs.  Returns (u_out, v_out, state_out, stats) as `median` does."""
        strides = set(tuple(x.stride()) for x in (u, v))
        if (not all(_is_device_tensor(x) and str(x.dtype) == "torch.float32" and tuple(x.shape) == (self.height, self.width) for x in (u, v))
                or len(strides) != 1 or u.stride(1) != 1):
            raise ValueError("u and v must be CUDA float32 tensors (height, width) of one row stride")
        mp, (sp, ss), (up, vp, os_), (sop, sos), sref, u_out, v_out, state_out, rec = _median_call(
            self.height, self.width, self.device, state, flow, state_out, stats, params, radius, mode, min_votes, True)
        self._check(self._lib.hsflow_median_planes_device(self._h, ctypes.byref(mp), _ptr(u), _ptr(v), u.stride(0) * 4, sp, ss, up, vp, os_, sop, sos, sref))
        return u_out, v_out, state_out, rec

    def median_batch_device(self, first_pair, n, state=None, u_out=None, v_out=None, state_out=None, stats=None, radius=1, mode="filter", min_votes=1, params=None):
        """One pass of the median over the flows of the pairs first_pair .. first_pair + n - 1 by one launch per
        `JPEG_BATCH_MAX` fields (`hsflow_median_batch_device`).  state, u_out, v_out, state_out: each None, a CUDA tensor
        (n, H, W) or a list of n tensors (H, W), uint8 / float32; one row stride per list, u_out and v_out one between them.
        stats: None, or a CUDA uint8 tensor of n * 64 bytes that receives record i of field i (`median_stats_from`).
        Only enqueued on the context's stream (complete after `synchronize()`)."""
        (sl, ss, _), (ul, us, _), (vl, vs, _), (ol, os_, _) = [
            _plane_lists(x, n, what, "plane per field", lambda p, dtype=dtype, what=what: _plane(p, self.height, self.width, dtype, what, True))
            for x, dtype, what in ((state, "uint8", "state"), (u_out, "float32", "u_out"), (v_out, "float32", "v_out"), (state_out, "uint8", "state_out"))]
        if u_out is not None and v_out is not None and us != vs:
            raise ValueError("u_out and v_out must have one row stride")
        mp = params if params is not None else make_median_params(radius, mode, min_votes)
        sref = _check_stats_tensor(stats, n, HsflowMedianStats)
        self._check(self._lib.hsflow_median_batch_device(self._h, int(first_pair), int(n), ctypes.byref(mp), sl, ss, ul, vl, us or vs, ol, os_, sref))
        return u_out, v_out, state_out, stats

    def encode_jpeg(self, rgb, quality=95):
        """The baseline JPEG file (4:2:0, standard tables) of an RGB picture of the context's size that lies in device
        memory -- a CUDA uint8 tensor of shape (H, W, 3) with packed pixels and any row stride -- encoded on the device
        (`hsflow_jpeg_encode_device`) on the context's stream, as `bytes`.  Waits for the tensor's producer on torch's
        current stream first and for the encode afterwards; only the file crosses to the host."""
        import torch
        if not _is_device_tensor(rgb):
            raise ValueError("expected a CUDA uint8 tensor of shape (height, width, 3); for host arrays use the module's encode_jpeg")
        ptr, stride = _render_target(rgb, self.height, self.width)
        out = torch.empty(jpeg_bound(self.width, self.height), dtype=torch.uint8, device=rgb.device)
        size = torch.zeros(1, dtype=torch.int64, device=rgb.device)
        torch.cuda.current_stream(rgb.device).synchronize()
        self._check(self._lib.hsflow_jpeg_encode_device(self._h, ptr, stride, int(quality), _ptr(out), out.numel(), _ptr(size)))
        self.synchronize()
        return out[:int(size.item())].cpu().numpy().tobytes()

    def encode_jpeg_batch(self, pictures, quality=95):
        """`encode_jpeg` for a list of CUDA uint8 tensors of shape (H, W, 3) (packed pixels, one row stride for all, any
        alignment each): one set of launches per `JPEG_BATCH_MAX` pictures (`hsflow_jpeg_encode_batch_device`).  Returns
        the list of the files as `bytes`, each byte for byte what `encode_jpeg` gives for that picture."""
        import torch
        n = len(pictures)
        if n < 1 or not all(_is_device_tensor(t) for t in pictures):
            raise ValueError("expected a non-empty list of CUDA uint8 tensors of shape (height, width, 3)")
        targets = [_render_target(t, self.height, self.width) for t in pictures]
        if len(set(s for _, s in targets)) != 1:
            raise ValueError("the pictures of a batch share one row stride")
        dev = pictures[0].device
        bound = jpeg_bound(self.width, self.height)
        out = torch.empty((n, bound), dtype=torch.uint8, device=dev)
        sizes = torch.zeros(n, dtype=torch.int64, device=dev)
        src = (ctypes.c_void_p * n)(*[p.value for p, _ in targets])
        dst = (ctypes.c_void_p * n)(*[out.data_ptr() + i * bound for i in range(n)])
        torch.cuda.current_stream(dev).synchronize()
        self._check(self._lib.hsflow_jpeg_encode_batch_device(self._h, src, n, targets[0][1], int(quality), dst, bound, _ptr(sizes)))
        self.synchronize()
        host = sizes.cpu().tolist()
        return [out[i, :int(host[i])].cpu().numpy().tobytes() for i in range(n)]

    def _batch_range(self, first_pair, n):
        first_pair = int(first_pair)
        return first_pair, self.n_pairs - first_pair if n is None else int(n)

    def render_jpeg_batch(self, route="cv", quality=95, first_pair=0, n=None, params=None, **kw):
        """`render_jpeg` for the pairs first_pair .. first_pair + n - 1 (n=None: all pairs from first_pair): drawn and
        encoded on the device by one set of launches per `JPEG_BATCH_MAX` pairs (`hsflow_render_flow_jpeg_batch`); per
        chunk the size words cross in one copy, then the files.  Returns the list of the files as `bytes`, each byte for
        byte what `render_jpeg(pair=i)` gives.  Complete on return."""
        rp = params if params is not None else make_render_params(route, **kw)
        first_pair, n = self._batch_range(first_pair, n)
        bound = jpeg_bound(self.width, self.height)
        buf = np.empty((max(n, 1), bound), np.uint8)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[buf[i].ctypes.data for i in range(max(n, 1))])
        sizes = (ctypes.c_size_t * max(n, 1))()
        self._check(self._lib.hsflow_render_flow_jpeg_batch(self._h, first_pair, n, ctypes.byref(rp), int(quality), ptrs, bound, sizes))
        return [buf[i, :sizes[i]].tobytes() for i in range(n)]

    def render_batch_device(self, out, route="cv", first_pair=0, n=None, params=None, **kw):
        """`render` into caller tensors for the pairs first_pair .. first_pair + n - 1 (n=None: all pairs from first_pair)
        by two launches per `JPEG_BATCH_MAX` pairs (`hsflow_render_flow_batch_device`).  out: a CUDA uint8 tensor
        (n, H, W, 3) or a list of n tensors (H, W, 3), packed pixels, one row stride for all.  Only enqueued on the
        context's stream (complete after `synchronize()`); returns `out`."""
        rp = params if params is not None else make_render_params(route, **kw)
        first_pair, n = self._batch_range(first_pair, n)
        pictures = [out[i] for i in range(len(out))]
        if len(pictures) != n or not all(_is_device_tensor(t) for t in pictures):
            raise ValueError("out must hold one CUDA uint8 tensor of shape (height, width, 3) per pair")
        targets = [_render_target(t, self.height, self.width) for t in pictures]
        if len(set(s for _, s in targets)) > 1:
            raise ValueError("the pictures of a batch share one row stride")
        ptrs = (ctypes.c_void_p * max(n, 1))(*[p.value for p, _ in targets])
        self._check(self._lib.hsflow_render_flow_batch_device(self._h, first_pair, n, ctypes.byref(rp), ptrs, targets[0][1] if targets else 0))
        return out

    def jpeg_decode(self, data, order="rgb", out=None):
        """The picture of a baseline JPEG file (`bytes`) of the context's size, decoded on the device
        (`hsflow_jpeg_decode`): an (H, W, 3) uint8 array, R first ("rgb") or B first ("bgr").  out: a host array to decode
        into (any row stride).  Complete on return; corrupt or truncated data raise `HsflowError` with status E_DATA."""
        buf = np.frombuffer(data, np.uint8)
        img = _render_host(out, self.height, self.width)
        self._check(self._lib.hsflow_jpeg_decode(self._h, _ptr(buf), buf.size, _jpeg_order(order), _ptr(img), img.strides[0]))
        return img

    def jpeg_decode_batch(self, files, order="rgb", out=None):
        """The pictures of n baseline JPEG files (`bytes`) of the context's size, decoded on the device by one set of
        launches per `JPEGD_BATCH_MAX` files (`hsflow_jpeg_decode_batch_device`): a CUDA uint8 tensor (n, H, W, 3) -- `out`
        (packed pixels, any row stride) or a new one -- and the list of the files' status words (0 ok, 1 corrupt,
        2 truncated: that picture is then undefined, the others are not affected).  Complete on return."""
        import torch
        n = len(files)
        if out is None:
            out = torch.empty((n, self.height, self.width, 3), dtype=torch.uint8, device="cuda:%d" % self.device)
        if not _is_device_tensor(out) or out.dim() != 4 or tuple(out.shape) != (n, self.height, self.width, 3) or out.stride(3) != 1 or out.stride(2) != 3:
            raise ValueError("out must be a CUDA uint8 tensor of shape (n, height, width, 3) with packed pixels")
        status = torch.empty(max(n, 1), dtype=torch.int32, device=out.device)
        ptrs, sizes, keep = _file_lists(files)
        pix = (ctypes.c_void_p * max(n, 1))(*[out.data_ptr() + i * out.stride(0) for i in range(n)])
        torch.cuda.current_stream(out.device).synchronize()
        self._check(self._lib.hsflow_jpeg_decode_batch_device(self._h, ptrs, sizes, n, _jpeg_order(order), pix, out.stride(1), _ptr(status)))
        torch.cuda.synchronize(out.device)  # (not `synchronize`: a decode touches no solver state, an owed check stays owed)
        return out, [int(v) for v in status[:n].cpu().tolist()]

    def set_sequence_jpeg(self, files, blur=True, first_pair=0, reblur=False, reblur_first=False):
        """len(files) >= 2 consecutive frames as baseline JPEG files (`bytes`) into the pairs first_pair .. first_pair +
        len(files) - 2, pair k = (file k, file k + 1): every file decoded once, as one batch, then `set_frames_jpeg`'s
        pre-processing of every pair by one launch (`hsflow_set_sequence_jpeg_ex`).  reblur, reblur_first: the camera
        loop's double blur of the previous frame, as in `set_sequence_device`.  All or nothing: on an error no pair's
        frames change."""
        ptrs, sizes, keep = _file_lists(files)
        self._check(self._lib.hsflow_set_sequence_jpeg_ex(self._h, int(first_pair), ptrs, sizes, len(files), 1 if blur else 0,
                                                          _seq_flags(reblur, reblur_first)))

    def set_frames_jpeg(self, prev, curr, blur=True, pair=0):
        """Both frames as baseline JPEG files (`bytes`): decoded on the device, then cvCvtColor (+ cvSmooth with
        blur=True) there (`hsflow_set_frames_jpeg`) -- only the files' entropy-coded bytes cross to the device."""
        a, b = np.frombuffer(prev, np.uint8), np.frombuffer(curr, np.uint8)
        self._check(self._lib.hsflow_set_frames_jpeg(self._h, pair, _ptr(a), a.size, _ptr(b), b.size, 1 if blur else 0))

    def push_frame_jpeg(self, nxt, blur=True, reblur_prev=False, pair=0):
        """The camera sequence fed with a JPEG frame (`hsflow_push_frame_jpeg`): as `push_frame_ex` with the frame decoded on
        the device."""
        a = np.frombuffer(nxt, np.uint8)
        self._check(self._lib.hsflow_push_frame_jpeg(self._h, pair, _ptr(a), a.size, 1 if blur else 0, 1 if reblur_prev else 0))

    def verify(self, pair=-1):
        """Is the flow held now what a sweep-by-sweep solve of the frames held, with the parameters of the last solve,
        produces?  Re-solves on the device with the one-sweep kernel behind the stand-alone derivative kernel into
        scratch of its own and compares there (`hsflow_verify`); nothing is downloaded but the report, an
        `HsflowVerifyReport` (`ok`, `u`, `v`, `deriv_differing`, `iterations_ref`, ...).  pair=-1: all pairs aggregated."""
        r = HsflowVerifyReport()
        r.struct_size = ctypes.sizeof(HsflowVerifyReport)
        self._check(self._lib.hsflow_verify(self._h, int(pair), ctypes.byref(r)))
        return r

    def compare_flow(self, u_dev, v_dev, pair=0):
        """The current flow of `pair` (side a) against two CUDA fp32 tensors of shape (height, width) with unit column
        stride and any row stride (side b), compared on the device: returns two `HsflowPlaneDiff` (u, v)."""
        for t in (u_dev, v_dev):
            if not _is_device_tensor(t) or str(t.dtype) != "torch.float32" or tuple(t.shape) != (self.height, self.width) or \
                    (self.width > 1 and t.stride(1) != 1):
                raise ValueError("expected CUDA float32 tensors of shape (height, width) with unit column stride")
        du, dv = HsflowPlaneDiff(), HsflowPlaneDiff()
        self._check(self._lib.hsflow_compare_flow_device(self._h, int(pair), _ptr(u_dev), u_dev.stride(0) * 4, _ptr(v_dev),
                                                         v_dev.stride(0) * 4, ctypes.byref(du), ctypes.byref(dv)))
        return du, dv

    def derivatives(self, pair=0):
        d = [np.empty((self.height, self.width), np.float32) for _ in range(3)]
        self._check(self._lib.hsflow_get_derivatives(self._h, pair, _ptr(d[0]), _ptr(d[1]), _ptr(d[2]),
                                                     d[0].strides[0]))
        return tuple(d)

    def frames(self, pair=0):
        a = np.empty((self.height, self.width), np.uint8)
        b = np.empty((self.height, self.width), np.uint8)
        self._check(self._lib.hsflow_get_frames_u8(self._h, pair, _ptr(a), a.strides[0], _ptr(b), b.strides[0]))
        return a, b

    def info(self):
        i = HsflowInfo()
        i.struct_size = ctypes.sizeof(HsflowInfo)
        self._check(self._lib.hsflow_get_info(self._h, ctypes.byref(i)))
        return {name: getattr(i, name) for name, _ in HsflowInfo._fields_}


def color_flow_host(u, v, max_flow=None, params=None, return_scale=False):
    """The dense colour picture of a flow field by the rule on the host (`hsflow_color_flow_host`, no GPU work): u, v
    float32 arrays of one shape (H, W).  Returns an (H, W, 3) uint8 array -- byte for byte what `HSFlow.color` draws from
    the same flow -- or with return_scale=True the pair (picture, scale used)."""
    cp = params if params is not None else make_color_params(max_flow)
    u, v = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(v, np.float32)
    if u.ndim != 2 or u.shape != v.shape:
        raise ValueError("u and v must be 2-D arrays of one shape")
    img = np.empty(u.shape + (3,), np.uint8)
    m = ctypes.c_float()
    st = _lib.load().hsflow_color_flow_host(_ptr(u), u.strides[0], _ptr(v), v.strides[0], u.shape[1], u.shape[0], ctypes.byref(cp), _ptr(img),
                                            img.strides[0], ctypes.byref(m))
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return (img, m.value) if return_scale else img


def warp_stats_from(stats, n=1):
    """The `HsflowWarpStats` records a device call left in the CUDA uint8 tensor `stats` (after `synchronize()`): one
    record for n=1, else a list of n."""
    raw = stats.cpu().numpy().tobytes()
    size = ctypes.sizeof(HsflowWarpStats)
    recs = [HsflowWarpStats.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(n)]
    return recs[0] if n == 1 else recs


def warp_host(u, v, src, ref=None, out=None, t=1.0, border="constant", fill=0, return_stats=False, params=None, picture=True):
    """`src` warped backwards by the flow (u, v) by the rule on the host (`hsflow_warp_host`, no GPU work): u, v float32
    arrays of one shape (H, W), src (and ref, out) uint8 (H, W) or (H, W, 3).  Returns the warped picture -- byte for byte
    what `HSFlow.warp` gives from the same flow -- or with return_stats=True the pair (picture, `HsflowWarpStats`).
    picture=False: statistics only (None in the picture's place)."""
    u, v = (a if a.ndim == 2 and a.strides[1] == 4 and a.strides[0] % 4 == 0 else np.ascontiguousarray(a)  # (padded rows are taken as they are)
            for a in (np.asarray(u, np.float32), np.asarray(v, np.float32)))
    if u.ndim != 2 or u.shape != v.shape:
        raise ValueError("u and v must be 2-D arrays of one shape")
    if src is None:
        raise ValueError("src is needed")
    if picture and out is None:
        out = np.empty(src.shape, np.uint8)
    if not picture:
        out = None
    (sp, ss), (rp, rs), (op, os_), wp = _warp_args(u.shape[0], u.shape[1], src, ref, out, False, params, t, border, fill)
    stats = HsflowWarpStats()
    st = _lib.load().hsflow_warp_host(_ptr(u), u.strides[0], _ptr(v), v.strides[0], u.shape[1], u.shape[0], ctypes.byref(wp), sp, ss, rp, rs, op, os_,
                                      ctypes.byref(stats) if return_stats else None)
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return (out, stats) if return_stats else out


def fb_stats_from(stats, n=1):
    """The `HsflowFbStats` records a device call left in the CUDA uint8 tensor `stats` (after `synchronize()`): one record
    for n=1, else a list of n."""
    raw = stats.cpu().numpy().tobytes()
    size = ctypes.sizeof(HsflowFbStats)
    recs = [HsflowFbStats.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(n)]
    return recs[0] if n == 1 else recs


def fb_host(uf, vf, ub, vb, mask=True, err2=False, stats=False, alpha=0.01, beta=0.5, values=(255, 0, 0, 0), params=None):
    """The forward-backward check by the rule on the host (`hsflow_fb_host`, no GPU work): four float32 arrays of one shape
    (H, W), padded rows taken as they are.  mask, err2, stats as `HSFlow.fb` takes them.  Returns (mask, err2, stats) --
    bit for bit what `HSFlow.fb` gives from the same flows."""
    planes = [a if a.ndim == 2 and a.strides[1] == 4 and a.strides[0] % 4 == 0 else np.ascontiguousarray(a)
              for a in (np.asarray(x, np.float32) for x in (uf, vf, ub, vb))]
    if planes[0].ndim != 2 or any(a.shape != planes[0].shape for a in planes):
        raise ValueError("uf, vf, ub and vb must be 2-D arrays of one shape")
    H, W = planes[0].shape
    _, args, mask, err2, rec = _fb_call(H, W, 0, mask, err2, stats, params, alpha, beta, values, False)
    flows = []
    for a in planes:
        flows += [_ptr(a), a.strides[0]]
    st = _lib.load().hsflow_fb_host(*(flows + [W, H] + list(args)))
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return mask, err2, rec


def gmotion_result_from(results, n=1):
    """The `HsflowGmotionResult` records a device call left in the CUDA uint8 tensor `results` (after `synchronize()`):
    one record for n=1, else a list of n."""
    raw = results.cpu().numpy().tobytes()
    size = ctypes.sizeof(HsflowGmotionResult)
    recs = [HsflowGmotionResult.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(n)]
    return recs[0] if n == 1 else recs


def regions_result_from(results, n=1):
    """The `HsflowRegionsResult` headers a device call left in the CUDA uint8 tensor `results` (after `synchronize()`):
    one for n=1, else a list of n."""
    raw = results.cpu().numpy().tobytes()
    size = ctypes.sizeof(HsflowRegionsResult)
    recs = [HsflowRegionsResult.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(n)]
    return recs[0] if n == 1 else recs


def regions_records_from(records, n):
    """The first n `HsflowRegionsRecord` of a record array: a CUDA uint8 tensor (after `synchronize()`) or the ctypes
    array of the host forms; a list."""
    raw = records.cpu().numpy().tobytes() if _is_device_tensor(records) else bytes(records)
    return [HsflowRegionsRecord.from_buffer_copy(raw[i * 64:(i + 1) * 64]) for i in range(n)]


def regions_host(mask=None, u=None, v=None, labels=False, records=True, capacity=64, result=True, params=None, shape=None):
    """The labelling by the rule on the host (`hsflow_regions_host`, no GPU work): mask None or a u8 array (H, W), u, v
    None or float32 arrays (H, W), padded rows taken as they are; with neither mask nor flow `shape` = (H, W) is needed.
    labels, records, capacity, result as `HSFlow.regions` takes them.  Returns (result, labels, records) -- bit for bit
    what the device forms give from the same planes."""
    if (u is None) != (v is None):
        raise ValueError("u and v are given together or not at all")
    if u is not None:
        u, v = (np.asarray(a, np.float32) for a in (u, v))
        if u.ndim != 2 or u.shape != v.shape:
            raise ValueError("u and v must be 2-D arrays of one shape")
        if any(a.strides[1] != 4 or a.strides[0] % 4 for a in (u, v)) or u.strides[0] != v.strides[0]:
            u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
    if mask is not None:
        H, W = mask.shape
    elif u is not None:
        H, W = u.shape
    elif shape is not None:
        H, W = shape
    else:
        raise ValueError("with neither mask nor flow the shape is needed")
    if u is not None and u.shape != (H, W):
        raise ValueError("mask and flow must have one shape")
    args, rec, labels, records = _regions_call(H, W, 0, mask, labels, records, capacity, result, params, False)
    st = _lib.load().hsflow_regions_host(args[0], args[1], _ptr(u) if u is not None else None, _ptr(v) if v is not None else None,
                                         u.strides[0] if u is not None else 0, W, H, *args[2:])
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return rec, labels, records


def corners_result_from(results, n=1):
    """The `HsflowCornersResult` headers a device call left in the CUDA uint8 tensor `results` (after `synchronize()`):
    one for n=1, else a list of n."""
    raw = results.cpu().numpy().tobytes()
    size = ctypes.sizeof(HsflowCornersResult)
    recs = [HsflowCornersResult.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(n)]
    return recs[0] if n == 1 else recs


def corners_records_from(records, n):
    """The first n `HsflowCornersRecord` of a record array: a CUDA uint8 tensor (after `synchronize()`) or the ctypes
    array of the host forms; a list."""
    raw = records.cpu().numpy().tobytes() if _is_device_tensor(records) else bytes(records)
    return [HsflowCornersRecord.from_buffer_copy(raw[i * 16:(i + 1) * 16]) for i in range(n)]


def corners_host(gray, mask=None, capacity=1024, records=True, xy=False, result=True, params=None):
    """The corner detection by the rule on the host (`hsflow_corners_host`, no GPU work): gray a u8 array (H, W), mask
    None or such an array, padded rows taken as they are.  capacity, records, xy, result as `HSFlow.corners` takes them.
    Returns (result, records, xy) -- byte for byte what the device forms give from the same planes."""
    if not isinstance(gray, np.ndarray) or gray.dtype != np.uint8 or gray.ndim != 2:
        raise ValueError("gray must be a 2-D uint8 NumPy array")
    H, W = gray.shape
    gp, gs = _plane(gray, H, W, "uint8", "gray", False)
    args, rec, records, xy = _corners_call(H, W, 0, mask, records, capacity, xy, result, params, False)
    st = _lib.load().hsflow_corners_host(gp, gs, W, H, *args)
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return rec, records, xy


def link_result_from(results, n=1):
    """The `HsflowLinkResult` headers a device call left in the CUDA uint8 tensor `results` (after `synchronize()`): one
    for n=1, else a list of n."""
    raw = results.cpu().numpy().tobytes()
    recs = [HsflowLinkResult.from_buffer_copy(raw[i * 64:(i + 1) * 64]) for i in range(n)]
    return recs[0] if n == 1 else recs


def link_records_from(links, n):
    """The first n `HsflowLinkRecord` of a link array: a CUDA uint8 tensor (after `synchronize()`) or the ctypes array of
    the host forms; a list."""
    raw = links.cpu().numpy().tobytes() if _is_device_tensor(links) else bytes(links)
    return [HsflowLinkRecord.from_buffer_copy(raw[i * 16:(i + 1) * 16]) for i in range(n)]


def link_sides_from(sides, n):
    """The first n `HsflowLinkSide` of a side array (record k - 1 is label k): a CUDA uint8 tensor (after `synchronize()`)
    or the ctypes array of the host forms; a ctypes array, as `link_tracks` takes it."""
    raw = sides.cpu().numpy().tobytes() if _is_device_tensor(sides) else bytes(sides)
    return (HsflowLinkSide * n).from_buffer_copy(raw[:32 * n])


def link_regions_host(labels_a, labels_b, u, v, links=True, link_capacity=256, side_a=True, side_b=True, result=True, params=None):
    """A linking step by the rule on the host (`hsflow_link_regions_host`, no GPU work): int32 label arrays and float32
    flow arrays of one shape (H, W), padded rows taken as they are.  links, link_capacity, side_a, side_b, result as
    `HSFlow.link_regions` takes them.  Returns (result, links, side_a, side_b) -- byte for byte what the device forms give
    from the same planes."""
    u, v = (np.asarray(a, np.float32) for a in (u, v))
    if u.ndim != 2 or u.shape != v.shape:
        raise ValueError("u and v must be 2-D arrays of one shape")
    if any(a.strides[1] != 4 or a.strides[0] % 4 for a in (u, v)) or u.strides[0] != v.strides[0]:
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
    H, W = u.shape
    (ap, as_), (bp, bs) = [_plane(x, H, W, "int32", "labels", False) for x in (labels_a, labels_b)]
    args, rec, links, side_a, side_b = _link_call(0, links, link_capacity, side_a, side_b, result, params, False)
    st = _lib.load().hsflow_link_regions_host(ap, as_, bp, bs, _ptr(u), _ptr(v), u.strides[0], W, H, *args)
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return rec, links, side_a, side_b


def link_tracks(side_a, side_b, n_regions, cap, min_share_256=128):
    """Object ids over a chain of steps (`hsflow_link_tracks_host`): side_a, side_b lists of n_steps ctypes arrays of `cap`
    `HsflowLinkSide` each (`link_sides_from`), n_regions the n_steps + 1 region counts of the frames.  A region continues
    the id of its best sender when that is mutual and the sender gives it at least min_share_256 / 256 of its pixels; else
    it starts a fresh id.  Returns (ids, n_tracks): ids a uint32 array (n_steps + 1, cap), ids[k, label - 1], 0 for slots
    that hold no region."""
    n_steps = len(side_a)
    if len(side_b) != n_steps or len(n_regions) != n_steps + 1:
        raise ValueError("side_a and side_b hold one array per step, n_regions one count per frame")
    for x in list(side_a) + list(side_b):
        if not isinstance(x, ctypes.Array) or ctypes.sizeof(x) < 32 * int(cap):
            raise ValueError("a side array must be a ctypes array of at least cap HsflowLinkSide")
    pa = (ctypes.c_void_p * max(n_steps, 1))(*[ctypes.addressof(x) for x in side_a])
    pb = (ctypes.c_void_p * max(n_steps, 1))(*[ctypes.addressof(x) for x in side_b])
    counts = (ctypes.c_uint32 * (n_steps + 1))(*[int(x) for x in n_regions])
    ids = np.zeros((n_steps + 1, max(int(cap), 1)), np.uint32)
    n_tracks = ctypes.c_uint32(0)
    st = _lib.load().hsflow_link_tracks_host(pa, pb, counts, n_steps, int(cap), int(min_share_256), _ptr(ids), ctypes.byref(n_tracks))
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return ids, int(n_tracks.value)


def global_motion_host(u, v, state=None, mask=False, residual=False, result=True, params=None):
    """The global-motion fit by the rule on the host (`hsflow_gmotion_fit_host`, no GPU work): u, v float32 arrays of one
    shape (H, W), padded rows taken as they are; state, mask, residual, result as `HSFlow.global_motion` takes them.
    Returns (result, mask, res_u, res_v) -- bit for bit what `HSFlow.global_motion` gives from the same flow."""
    u, v = (np.asarray(a, np.float32) for a in (u, v))
    if u.ndim != 2 or u.shape != v.shape:
        raise ValueError("u and v must be 2-D arrays of one shape")
    if any(a.strides[1] != 4 or a.strides[0] % 4 for a in (u, v)) or u.strides[0] != v.strides[0]:
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
    H, W = u.shape
    args, rec, mask, ru, rv = _gmotion_call(H, W, 0, state, mask, residual, result, params, False)
    st = _lib.load().hsflow_gmotion_fit_host(_ptr(u), _ptr(v), u.strides[0], args[0], args[1], W, H, *args[2:])
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return rec, mask, ru, rv


def gmotion_warp_host(model, src, ref=None, out=None, t=1.0, border="constant", fill=0, return_stats=False, params=None, picture=True):
    """`src` warped backwards by the motion `model` by the rule on the host (`hsflow_gmotion_warp_host`, no GPU work); the
    pictures and the result as `warp_host`."""
    if src is None:
        raise ValueError("src is needed")
    if picture and out is None:
        out = np.empty(src.shape, np.uint8)
    if not picture:
        out = None
    H, W = src.shape[:2]
    (sp, ss), (rp, rs), (op, os_), wp = _warp_args(H, W, src, ref, out, False, params, t, border, fill)
    stats = HsflowWarpStats()
    st = _lib.load().hsflow_gmotion_warp_host(_gmotion_model(model), W, H, ctypes.byref(wp), sp, ss, rp, rs, op, os_, ctypes.byref(stats) if return_stats else None)
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return (out, stats) if return_stats else out


def gmotion_compose(m1, m2):
    """The model of "first m1, then m2" on positions (`hsflow_gmotion_compose_host`): float32 (6,)."""
    out = (ctypes.c_float * 6)()
    st = _lib.load().hsflow_gmotion_compose_host(_gmotion_model(m1), _gmotion_model(m2), out)
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return np.array(out[:], np.float32)


def gmotion_invert(m):
    """The model of the inverse map (`hsflow_gmotion_invert_host`): float32 (6,); a singular linear part raises."""
    out = (ctypes.c_float * 6)()
    st = _lib.load().hsflow_gmotion_invert_host(_gmotion_model(m), out)
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return np.array(out[:], np.float32)


def chain_stats_from(stats):
    """The `HsflowChainStats` record a device call left in the CUDA uint8 tensor `stats` (after `synchronize()`)."""
    return HsflowChainStats.from_buffer_copy(stats.cpu().numpy().tobytes()[:ctypes.sizeof(HsflowChainStats)])


def _chain_host_planes(u, v):
    """The flow planes of a host chain as float32 arrays of one shape and ONE row stride (copied where they are not)."""
    if len(u) != len(v) or not 1 <= len(u) <= CHAIN_MAX_PAIRS:
        raise ValueError("u and v hold one plane each per pair, 1 .. %d pairs" % CHAIN_MAX_PAIRS)
    planes = [np.asarray(x, np.float32) for x in list(u) + list(v)]
    if planes[0].ndim != 2 or any(a.shape != planes[0].shape for a in planes):
        raise ValueError("the flow planes must be 2-D arrays of one shape")
    if any(a.strides[1] != 4 or a.strides[0] % 4 or a.strides[0] != planes[0].strides[0] for a in planes):
        planes = [np.ascontiguousarray(a) for a in planes]
    n = len(u)
    ptrs = lambda part: (ctypes.c_void_p * n)(*[a.ctypes.data for a in part])
    return planes, n, ptrs(planes[:n]), ptrs(planes[n:]), planes[0].strides[0]


def chain_flow_host(u, v, state=None, start=None, flow=True, status=False, age=False, stats=False, params=None):
    """The dense chain by the rule on the host (`hsflow_chain_flow_host`, no GPU work): u, v lists of n float32 arrays of
    one shape (H, W); state, start, flow, status, age, stats as `HSFlow.chain_flow` takes them.  Returns (U, V, status, age,
    stats) -- bit for bit what `HSFlow.chain_flow` gives from the same flows."""
    planes, n, ul, vl, fs = _chain_host_planes(u, v)
    H, W = planes[0].shape
    args, U, V, status, age, rec = _chain_call(H, W, 0, n, state, start, flow, status, age, stats, params, False)
    st = _lib.load().hsflow_chain_flow_host(n, ul, vl, fs, args[0], args[1], W, H, *args[2:])
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return U, V, status, age, rec


def track_points_host(u, v, xy, state=None, track=False, status=False, age=False, stats=False, params=None):
    """Points by the rule on the host (`hsflow_track_points_host`, no GPU work); arguments and result as
    `HSFlow.track_points`: (last, track, status, age, stats)."""
    planes, n, ul, vl, fs = _chain_host_planes(u, v)
    H, W = planes[0].shape
    xy = np.ascontiguousarray(xy, np.float32)
    if xy.ndim != 2 or xy.shape[1] != 2 or xy.shape[0] < 1:
        raise ValueError("xy must be float32 of shape (m, 2)")
    m = xy.shape[0]
    sl, ss = _chain_list(state, n, H, W, "uint8", "state", False, holes=True)
    last = np.empty((m, 2), np.float32)
    track = np.empty((n + 1, m, 2), np.float32) if track else None
    status = np.empty((m,), np.uint8) if status else None
    age = np.empty((m,), np.uint8) if age else None
    cp = params if params is not None else make_chain_params()
    rec, sref = _stats_record(HsflowChainStats, stats, False, 0)
    opt = lambda x: _ptr(x) if x is not None else None
    st = _lib.load().hsflow_track_points_host(n, ul, vl, fs, sl, ss, W, H, ctypes.byref(cp), _ptr(xy), m, opt(track), _ptr(last), opt(status), opt(age), sref)
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return last, track, status, age, rec


def median_stats_from(stats, n=1):
    """The `HsflowMedianStats` records a device call left in the CUDA uint8 tensor `stats` (after `synchronize()`): one
    record for n=1, else a list of n."""
    raw = stats.cpu().numpy().tobytes()
    size = ctypes.sizeof(HsflowMedianStats)
    recs = [HsflowMedianStats.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(n)]
    return recs[0] if n == 1 else recs


def median_host(u, v, state=None, flow=True, state_out=False, stats=False, radius=1, mode="filter", min_votes=1, passes=1, params=None):
    """The median filter / hole filling by the rule on the host (`hsflow_median_host`, no GPU work): two float32 arrays of
    one shape (H, W), padded rows taken as they are; state, flow, state_out, stats as `HSFlow.median` takes them.
    Returns (u_out, v_out, state_out, stats) -- bit for bit what the device forms give from the same planes."""
    planes = [a if a.ndim == 2 and a.strides[1] == 4 and a.strides[0] % 4 == 0 else np.ascontiguousarray(a)
              for a in (np.asarray(x, np.float32) for x in (u, v))]
    if planes[0].ndim != 2 or planes[1].shape != planes[0].shape:
        raise ValueError("u and v must be 2-D arrays of one shape")
    H, W = planes[0].shape
    mp, (sp, ss), (up, vp, os_), (sop, sos), sref, u_out, v_out, state_out, rec = _median_call(
        H, W, 0, state, flow, state_out, stats, params, radius, mode, min_votes, False)
    st = _lib.load().hsflow_median_host(_ptr(planes[0]), planes[0].strides[0], _ptr(planes[1]), planes[1].strides[0], sp, ss, W, H, ctypes.byref(mp),
                                        int(passes), up, vp, os_, sop, sos, sref)
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return u_out, v_out, state_out, rec


def _host_check(st):
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())


def pyramid_plan(width, height, levels=0, min_size=32, warps=1, median_radius=0, params=None):
    """The level sizes `HSFlow.solve_pyramid` would use for a width x height context (`hsflow_pyramid_plan`, no GPU work): a
    list of (width, height), level 0 first."""
    pp = params if params is not None else make_pyramid_params(levels, min_size, warps, median_radius)
    n = ctypes.c_int(0)
    ws, hs_ = (ctypes.c_int * _lib.PYRAMID_MAX_LEVELS)(), (ctypes.c_int * _lib.PYRAMID_MAX_LEVELS)()
    _host_check(_lib.load().hsflow_pyramid_plan(int(width), int(height), ctypes.byref(pp), ctypes.byref(n), ws, hs_))
    return [(ws[l], hs_[l]) for l in range(n.value)]


def _rows_as_they_are(a, dtype):
    a = np.asarray(a, dtype)
    item = np.dtype(dtype).itemsize
    return a if a.ndim == 2 and a.strides[1] == item and a.strides[0] % item == 0 and a.strides[0] >= a.shape[1] * item else np.ascontiguousarray(a)


def pyramid_down_host(img, out=None):
    """A uint8 frame (H, W) at half the size, (ceil(H/2), ceil(W/2)), by the pyramid's rule on the host
    (`hsflow_pyramid_down_host`, no GPU work); padded rows are taken as they are.  out: a uint8 array of that shape (its
    row stride is used), else a new one."""
    img = _rows_as_they_are(img, np.uint8)
    if img.ndim != 2:
        raise ValueError("img must be a 2-D uint8 array")
    H, W = img.shape
    if out is None:
        out = np.empty(((H + 1) // 2, (W + 1) // 2), np.uint8)
    if out.dtype != np.uint8 or out.shape != ((H + 1) // 2, (W + 1) // 2) or (out.shape[1] > 1 and out.strides[1] != 1):
        raise ValueError("out must be a uint8 array of shape (ceil(H/2), ceil(W/2)) with dense rows")
    _host_check(_lib.load().hsflow_pyramid_down_host(_ptr(img), img.strides[0] if H > 1 else max(img.strides[0], W), W, H, _ptr(out),
                                                     out.strides[0] if out.shape[0] > 1 else max(out.strides[0], out.shape[1])))
    return out


def pyramid_prolong_host(coarse, width, height, out=None):
    """A coarse float32 plane (ceil(height/2), ceil(width/2)) at the fine size (height, width), doubled, by the pyramid's
    rule on the host (`hsflow_pyramid_prolong_host`, no GPU work); padded rows are taken as they are."""
    coarse = _rows_as_they_are(coarse, np.float32)
    width, height = int(width), int(height)
    if coarse.ndim != 2 or coarse.shape != ((height + 1) // 2, (width + 1) // 2):
        raise ValueError("coarse must be a 2-D float32 array of shape (ceil(height/2), ceil(width/2))")
    if out is None:
        out = np.empty((height, width), np.float32)
    if out.dtype != np.float32 or out.shape != (height, width) or (width > 1 and out.strides[1] != 4):
        raise ValueError("out must be a float32 array of shape (height, width) with dense rows")
    _host_check(_lib.load().hsflow_pyramid_prolong_host(_ptr(coarse), coarse.strides[0] if coarse.shape[0] > 1 else max(coarse.strides[0], 4 * coarse.shape[1]),
                                                        width, height, _ptr(out), out.strides[0] if height > 1 else max(out.strides[0], 4 * width)))
    return out


def interp_stats_from(stats, n=1):
    """The `HsflowInterpStats` records a device call left in the CUDA uint8 tensor `stats` (after `synchronize()`): one
    record for n=1, else a list of n."""
    raw = stats.cpu().numpy().tobytes()
    size = ctypes.sizeof(HsflowInterpStats)
    recs = [HsflowInterpStats.from_buffer_copy(raw[i * size:(i + 1) * size]) for i in range(n)]
    return recs[0] if n == 1 else recs


def _host_flow(u, v):
    u, v = (a if a.ndim == 2 and a.strides[1] == 4 and a.strides[0] % 4 == 0 else np.ascontiguousarray(a)  # (padded rows are taken as they are)
            for a in (np.asarray(u, np.float32), np.asarray(v, np.float32)))
    if u.ndim != 2 or u.shape != v.shape:
        raise ValueError("u and v must be 2-D arrays of one shape")
    return u, v


def interp_host(u, v, prev, curr, t=0.5, vis_prev=None, vis_curr=None, ref=None, out=True, classes=False, stats=False, params=None):
    """The frame at time `t` between `prev` and `curr` from the forward flow (u, v) by the rule on the host
    (`hsflow_interp_host`, no GPU work); arguments as `HSFlow.interp` takes them.  Returns (out, classes, stats) -- bit for
    bit what the device forms give from the same flow."""
    u, v = _host_flow(u, v)
    H, W = u.shape
    _, args, out, classes, rec = _interp_call(H, W, 0, prev, curr, vis_prev, vis_curr, ref, out, classes, stats, params, False)
    st = _lib.load().hsflow_interp_host(_ptr(u), u.strides[0], _ptr(v), v.strides[0], W, H, float(t), *args)
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return out, classes, rec


def project_flow_host(u, v, prev, curr, t=1.0, flow=True, state=False, stats=False, params=None):
    """The forward flow (u, v) projected to time `t` and hole-filled by the rule on the host (`hsflow_project_flow_host`);
    arguments as `HSFlow.project_flow` takes them, NumPy arrays.  Returns (u, v, state, stats)."""
    u, v = _host_flow(u, v)
    H, W = u.shape
    args, uo, vo, state, rec = _project_call(H, W, 0, prev, curr, flow, state, stats, params, False)
    st = _lib.load().hsflow_project_flow_host(_ptr(u), u.strides[0], _ptr(v), v.strides[0], W, H, float(t), *args)
    if st != _lib.OK:
        raise HsflowError(st, (_lib.load().hsflow_last_error(None) or b"").decode())
    return uo, vo, state, rec


def compare_planes(a, b):
    """The comparison rule of `HSFlow.verify` over two host fp32 arrays of one 2-D shape (a: the side under test,
    b: the reference side), on the host -- the same header the device kernel is compiled from; no device needed.
    Returns an `HsflowPlaneDiff` (differing, failing, nonfinite, first_failing, max_abs_diff, max_ulp)."""
    lib = _lib.load()
    a = np.asarray(a)
    b = np.asarray(b)
    if a.dtype != np.float32 or b.dtype != np.float32 or a.ndim != 2 or a.shape != b.shape:
        raise ValueError("expected two float32 arrays of the same 2-D shape")
    if a.shape[1] > 1 and a.strides[1] != 4:
        a = np.ascontiguousarray(a)
    if b.shape[1] > 1 and b.strides[1] != 4:
        b = np.ascontiguousarray(b)
    d = HsflowPlaneDiff()
    st = lib.hsflow_compare_planes_host(_ptr(a), a.strides[0], _ptr(b), b.strides[0], a.shape[1], a.shape[0], ctypes.byref(d))
    if st:
        raise HsflowError(st, (lib.hsflow_last_error(None) or b"").decode())
    return d


def preprocess_frame(img, frames):
    """The pre-processing rule on the host (`hsflow_preprocess_frame_host`; no device needed): the (H, W) uint8 frame the
    solver sees for `img` given as layout `frames` -- "gray", "gray_blur" ((H, W) uint8) or "bgr", "bgr_blur" ((H, W, 3))."""
    lib = _lib.load()
    fmt = _lib.FRAME_FORMATS[frames]
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim != (3 if fmt >= _lib.FRAMES_BGR8 else 2) or (img.ndim == 3 and img.shape[2] != 3):
        raise ValueError("expected a uint8 array of shape (H, W), or (H, W, 3) for colour")
    if img.strides[-1] != 1 or (img.ndim == 3 and img.strides[1] != 3):
        img = np.ascontiguousarray(img)
    out = np.empty(img.shape[:2], np.uint8)
    st = lib.hsflow_preprocess_frame_host(fmt, _ptr(img), img.strides[0], img.shape[1], img.shape[0], _ptr(out), out.strides[0])
    if st:
        raise HsflowError(st, (lib.hsflow_last_error(None) or b"").decode())
    return out


def _seq_flags(reblur, reblur_first):
    """HSFLOW_SEQ_* of the two keywords (reblur_first alone is passed on as it is: the library refuses it)."""
    return (_lib.SEQ_REBLUR if reblur else 0) | (_lib.SEQ_REBLUR_FIRST if reblur_first else 0)


def preprocess_sequence(frames_list, fmt, reblur=False, reblur_first=False):
    """The sequence rule on the host (`hsflow_preprocess_sequence_host`; no device needed): for n >= 2 frames given in
    layout `fmt` ("gray", "gray_blur": (H, W) uint8; "bgr", "bgr_blur": (H, W, 3)) the list of the n - 1 pairs'
    (prev, curr) planes, what `HSFlow.set_sequence_device` leaves in `HSFlow.frames(k)`."""
    lib = _lib.load()
    f = _lib.FRAME_FORMATS[fmt]
    colour = f >= _lib.FRAMES_BGR8
    imgs = [np.asarray(a) for a in frames_list]
    for a in imgs:
        if a.dtype != np.uint8 or a.ndim != (3 if colour else 2) or (colour and a.shape[2] != 3) or a.shape != imgs[0].shape:
            raise ValueError("expected uint8 arrays of one shape (H, W), or (H, W, 3) for colour")
    if imgs and (len(set(a.strides for a in imgs)) > 1 or imgs[0].strides[-1] != 1 or (colour and imgs[0].strides[1] != 3)):
        imgs = [np.ascontiguousarray(a) for a in imgs]
    n = len(imgs)
    H, W = imgs[0].shape[:2] if n else (0, 0)
    prev = np.empty((max(n - 1, 1), H, W), np.uint8)
    curr = np.empty((max(n - 1, 1), H, W), np.uint8)
    src = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data for a in imgs])
    pp = (ctypes.c_void_p * max(n - 1, 1))(*[prev[k].ctypes.data for k in range(max(n - 1, 1))])
    pc = (ctypes.c_void_p * max(n - 1, 1))(*[curr[k].ctypes.data for k in range(max(n - 1, 1))])
    st = lib.hsflow_preprocess_sequence_host(f, _seq_flags(reblur, reblur_first), src, n, imgs[0].strides[0] if n else 0, W, H, pp, pc, W)
    if st:
        raise HsflowError(st, (lib.hsflow_last_error(None) or b"").decode())
    return [(prev[k], curr[k]) for k in range(n - 1)]


def jpeg_bound(width, height):
    """Bytes that always suffice for the JPEG file of a width x height picture (`hsflow_jpeg_bound`); 0 for a non-positive size."""
    return int(_lib.load().hsflow_jpeg_bound(int(width), int(height)))


def encode_jpeg(rgb, quality=95):
    """The JPEG rule on the host (`hsflow_jpeg_encode_host`; no device needed): the file of an (H, W, 3) uint8 RGB array as
    `bytes` -- baseline, 4:2:0, standard tables, byte for byte what the device encoder and the drop-in CLI write."""
    lib = _lib.load()
    rgb = np.asarray(rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError("expected a uint8 array of shape (H, W, 3)")
    if rgb.strides[2] != 1 or rgb.strides[1] != 3 or rgb.strides[0] < 3 * rgb.shape[1]:
        rgb = np.ascontiguousarray(rgb)
    buf = np.empty(jpeg_bound(rgb.shape[1], rgb.shape[0]), np.uint8)
    n = ctypes.c_size_t()
    st = lib.hsflow_jpeg_encode_host(_ptr(rgb), rgb.strides[0], rgb.shape[1], rgb.shape[0], int(quality), _ptr(buf), buf.size, ctypes.byref(n))
    if st:
        raise HsflowError(st, (lib.hsflow_last_error(None) or b"").decode())
    return buf[:n.value].tobytes()


def _file_lists(files):
    """(pointer array, size array, what keeps them alive) for a list of `bytes`-like files."""
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    n = max(len(bufs), 1)
    ptrs = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    return ptrs, sizes, bufs


def _jpeg_order(order):
    if order not in ("rgb", "bgr"):
        raise ValueError('order must be "rgb" or "bgr"')
    return _lib.JPEG_ORDER_RGB if order == "rgb" else _lib.JPEG_ORDER_BGR


def jpeg_read_header(data):
    """What the header of a baseline JPEG file (`bytes`) says (`hsflow_jpeg_read_header`; no device needed): a dict of
    width, height, components, h_samp, v_samp, restart_interval, subseq_bits, blocks, scan_offset, scan_bytes."""
    lib = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    info = _lib.HsflowJpegInfo()
    info.struct_size = ctypes.sizeof(info)
    st = lib.hsflow_jpeg_read_header(_ptr(buf), buf.size, ctypes.byref(info))
    if st:
        raise HsflowError(st, (lib.hsflow_last_error(None) or b"").decode())
    return info.as_dict()


def jpeg_decode_host(data, order="rgb"):
    """The JPEG decoding rule on the host (`hsflow_jpeg_decode_host`; no device needed): the (H, W, 3) uint8 picture of a
    baseline JPEG file given as `bytes`, R first ("rgb") or B first ("bgr") -- pixel for pixel what the device decoder,
    the drop-in CLI's reader and libjpeg give.  A one-component file gives three equal channels."""
    info = jpeg_read_header(data)
    lib = _lib.load()
    buf = np.frombuffer(data, np.uint8)
    img = np.empty((info["height"], info["width"], 3), np.uint8)
    st = lib.hsflow_jpeg_decode_host(_ptr(buf), buf.size, _jpeg_order(order), _ptr(img), img.strides[0], None)
    if st:
        raise HsflowError(st, (lib.hsflow_last_error(None) or b"").decode())
    return img


def plan_query(width, height, n_pairs=1, params=None, **kw):
    """The launch plan hsflow_solve would use for this size and these parameters (no device needed)."""
    lib = _lib.load()
    p = params if params is not None else make_params(**kw)
    i = HsflowInfo()
    i.struct_size = ctypes.sizeof(HsflowInfo)
    st = lib.hsflow_plan_query(int(width), int(height), int(n_pairs), ctypes.byref(p), ctypes.byref(i))
    if st:
        raise HsflowError(st, (lib.hsflow_last_error(None) or b"").decode())
    return {name: getattr(i, name) for name, _ in HsflowInfo._fields_}


def calc_optical_flow_hs(prev, curr, use_previous, velx, vely, lam, criteria, device=0, **tuning):
    """cvCalcOpticalFlowHS(prev, curr, use_previous, velx, vely, lambda, criteria) on the GPU.

    prev/curr: (H, W) uint8; velx/vely: (H, W) float32, written in place (read first when
    use_previous).  criteria: TermCriteria / (type, max_iter, epsilon).  Raises TypeError /
    ValueError for what the original rejects with "Source images must have 8uC1 type and
    destination images must have 32fC1 type" and for mismatched sizes.
    """
    prev = np.asarray(prev)
    curr = np.asarray(curr)
    if prev.dtype != np.uint8 or curr.dtype != np.uint8 or prev.ndim != 2 or curr.ndim != 2:
        raise TypeError("Source images must have 8uC1 type and destination images must have 32fC1 type")
    if not (isinstance(velx, np.ndarray) and isinstance(vely, np.ndarray)) or \
            velx.dtype != np.float32 or vely.dtype != np.float32 or velx.ndim != 2 or vely.ndim != 2:
        raise TypeError("Source images must have 8uC1 type and destination images must have 32fC1 type")
    if prev.shape != curr.shape or velx.shape != prev.shape or vely.shape != prev.shape:
        raise ValueError("images and velocity fields must have equal sizes")
    ctype, max_iter, eps = criteria
    H, W = prev.shape
    with HSFlow(W, H, 1, device=device, own_stream=True) as ctx:
        ctx.set_frames(prev, curr)
        if use_previous:
            import torch  # device staging only
            ud = torch.from_numpy(np.ascontiguousarray(velx)).to("cuda:%d" % device)
            vd = torch.from_numpy(np.ascontiguousarray(vely)).to("cuda:%d" % device)
            torch.cuda.synchronize(device)
            ctx.set_flow_rows_from(ud, vd, 0, H)
            ctx.synchronize()
        info = ctx.solve(lam=lam, max_iter=max_iter, epsilon=eps, term_type=ctype,
                         use_previous=bool(use_previous), **tuning)
        u, v = ctx.flow()
    velx[...] = u
    vely[...] = v
    return info
