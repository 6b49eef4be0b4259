"""Independent pairs streamed through one GPU: host frames in, host flow out (BASELINE config C4).

Mirror of `hsflow_pipeline_*` (include/hsflow.h).  The reference handles a pair as blocking write ->
derivatives -> iterations -> blocking read (HSOpticalFlowOpenCL.cpp:744-767); the pipeline keeps
`depth` pairs in flight on separate streams so that the PCIe copies of the neighbouring pairs run
beside the solve of the current one.  Host buffers should be page-locked (`pinned_empty`).
"""
import ctypes
import weakref

import numpy as np

from . import _lib
from ._lib import HsflowError, HsflowInfo, HsflowVerifyReport, TERM_ITER
from .solver import _is_device_tensor, _render_host, _render_target, _warp_call, _fb_call, _median_call, _interp_call, jpeg_bound, make_color_params, make_params, make_render_params


def pinned_empty(shape, dtype):
    """numpy array over page-locked host memory (hsflow_host_alloc); freed with the array."""
    lib = _lib.load()
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    p = ctypes.c_void_p()
    st = lib.hsflow_host_alloc(ctypes.byref(p), max(n, 1))
    if st:
        raise HsflowError(st, (lib.hsflow_last_error(None) or b"").decode())
    buf = (ctypes.c_ubyte * max(n, 1)).from_address(p.value)
    weakref.finalize(buf, lib.hsflow_host_free, ctypes.c_void_p(p.value))  # runs when the last view is gone
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


class _DeviceView(object):
    """fp32 device memory described for torch.as_tensor (zero copy)."""

    def __init__(self, ptr, shape, strides):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<f4", "data": (int(ptr), False), "strides": tuple(strides), "version": 2}


class PairPipeline(object):
    """`depth` single-pair contexts used round-robin.  Termination: ITER (default) or ITER|EPS.
    With lanes >= 3 a pair that leaves the launch shape to the planner gets the pipeline's own (strip kernel, up to 20 sweeps
    per launch, 5 rows per lane) on frames of 256 x 80 .. 1.5 Mpixel: same flow bits (include/hsflow.h, hsflow_pipeline_create_lanes)."""

    def __init__(self, width, height, depth=4, device=0, lanes=None):
        """lanes: streams the slots are spread over (default: one per slot -- host-memory pairs; device-resident streams
        want 2 lanes with 4 - 8 slots, hsflow_pipeline_create_lanes)."""
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        self.width, self.height, self.device = int(width), int(height), int(device)
        st = self._lib.hsflow_pipeline_create_lanes(ctypes.byref(self._h), int(device), self.width, self.height, int(depth),
                                                    int(depth if lanes is None else lanes))
        if st:
            self._h = None
            raise HsflowError(st, (self._lib.hsflow_pipeline_last_error(None) or b"").decode())
        self.depth = self._lib.hsflow_pipeline_depth(self._h)
        self._held = {}  # ticket -> arrays kept alive while the device may touch them

    def _check(self, st):
        if st:
            raise HsflowError(st, (self._lib.hsflow_pipeline_last_error(self._h) or b"").decode())

    def submit(self, prev, curr, u_out, v_out, params=None, frames="gray", **kw):
        """Enqueues upload -> [pre-processing] -> solve -> download of one pair; returns its ticket.  The four
        arrays belong to the pipeline until `wait(ticket)` (or `drain()`) returned.
        frames: "gray" (u8, as is), "gray_blur" (3x3 box blur on the device), "bgr" / "bgr_blur" ((H, W, 3) u8)."""
        fmt = _lib.FRAME_FORMATS[frames]
        colour = fmt >= _lib.FRAMES_BGR8
        for a in (prev, curr):
            want = (self.height, self.width, 3) if colour else (self.height, self.width)
            if not isinstance(a, np.ndarray) or a.dtype != np.uint8 or a.shape != want or a.strides[-1] != 1 or (colour and a.strides[1] != 3):
                raise ValueError("frames must be u8 arrays of shape %r with packed pixels" % (want,))
        for a, dt in ((u_out, np.float32), (v_out, np.float32)):
            if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != (self.height, self.width) or a.strides[1] != a.itemsize:
                raise ValueError("pipeline buffers must be (height, width) arrays: u8 frames, fp32 flow, unit column stride")
        if not (u_out.flags.writeable and v_out.flags.writeable):
            raise ValueError("flow outputs must be writeable")
        if params is None:
            kw.setdefault("term_type", TERM_ITER)
            params = make_params(**kw)
        t = ctypes.c_uint64()
        self._check(self._lib.hsflow_pipeline_submit_ex(
            self._h, fmt, ctypes.c_void_p(prev.ctypes.data), prev.strides[0], ctypes.c_void_p(curr.ctypes.data), curr.strides[0],
            ctypes.c_void_p(u_out.ctypes.data), u_out.strides[0], ctypes.c_void_p(v_out.ctypes.data), v_out.strides[0],
            ctypes.byref(params), ctypes.byref(t)))
        self._held.pop(t.value - self.depth, None)  # that slot was waited for inside submit
        self._held[t.value] = (prev, curr, u_out, v_out)
        return t.value

    def submit_device(self, prev, curr, params=None, frames="gray", **kw):
        """A pair that already lies in device memory (CUDA uint8 tensors of shape (height, width), unit column stride):
        the slot gets its own copy of the frames (from the solve's first launch where that can read the tensors in place,
        `copies_elided`) -> solve; the flow stays in the slot (`flow_device`).  The tensors are held
        until the ticket has been waited for.
        frames: "gray" (as is), or "gray_blur", "bgr" / "bgr_blur" ((height, width, 3), packed pixels): the pre-processing
        is then one launch ahead of the solve (`hsflow_pipeline_submit_device_ex`) and the slot holds its result."""
        fmt = _lib.FRAME_FORMATS[frames]
        colour = fmt >= _lib.FRAMES_BGR8
        want = (self.height, self.width, 3) if colour else (self.height, self.width)
        for a in (prev, curr):
            if not (hasattr(a, "is_cuda") and a.is_cuda) or str(a.dtype) != "torch.uint8" or tuple(a.shape) != want or a.stride(-1) != 1 or \
                    (colour and a.stride(1) != 3):
                raise ValueError("device frames must be CUDA uint8 tensors of shape %r with unit column stride (packed pixels)" % (want,))
        if params is None:
            kw.setdefault("term_type", TERM_ITER)
            params = make_params(**kw)
        t = ctypes.c_uint64()
        if fmt == _lib.FRAMES_GRAY8:
            self._check(self._lib.hsflow_pipeline_submit_device(self._h, ctypes.c_void_p(prev.data_ptr()), prev.stride(0), ctypes.c_void_p(curr.data_ptr()),
                                                                curr.stride(0), ctypes.byref(params), ctypes.byref(t)))
        else:
            self._check(self._lib.hsflow_pipeline_submit_device_ex(self._h, fmt, ctypes.c_void_p(prev.data_ptr()), prev.stride(0),
                                                                   ctypes.c_void_p(curr.data_ptr()), curr.stride(0), ctypes.byref(params), ctypes.byref(t)))
        self._held.pop(t.value - self.depth, None)
        self._held[t.value] = (prev, curr)
        return t.value

    def submit_jpeg(self, prev, curr, blur=True, params=None, **kw):
        """A pair of baseline JPEG files (`bytes`) of the pipeline's size: both decoded as a batch of two on the slot's
        stream, cvCvtColor (+ cvSmooth with blur=True) and the solve behind them (`hsflow_pipeline_submit_jpeg`); the flow
        stays in the slot (`flow_device`, `render_jpeg`).  Returns the ticket.  What the headers show raises at once
        (no ticket); corrupt or truncated entropy-coded data raise E_DATA when the ticket is waited for."""
        a, b = np.frombuffer(prev, np.uint8), np.frombuffer(curr, np.uint8)
        if params is None:
            kw.setdefault("term_type", TERM_ITER)
            params = make_params(**kw)
        t = ctypes.c_uint64()
        self._check(self._lib.hsflow_pipeline_submit_jpeg(self._h, ctypes.c_void_p(a.ctypes.data), a.size, ctypes.c_void_p(b.ctypes.data), b.size,
                                                          1 if blur else 0, ctypes.byref(params), ctypes.byref(t)))
        self._held.pop(t.value - self.depth, None)
        return t.value

    def flow_device(self, ticket, copy=True):
        """wait(ticket) + that pair's flow as two CUDA tensors of shape (height, width).  copy=False: views of the slot's
        own planes (row stride = the context's pitch), valid until `depth` more pairs have been submitted."""
        import torch
        pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        self._check(self._lib.hsflow_pipeline_flow_device(self._h, int(ticket), ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)))
        self._held.pop(int(ticket), None)
        out = []
        for p in (pu, pv):
            view = torch.as_tensor(_DeviceView(p.value, (self.height, self.width), (sb.value, 4)), device="cuda")
            out.append(view.clone() if copy else view)
        return tuple(out)

    def render(self, ticket, route="cv", out=None, params=None, **kw):
        """wait(ticket) + the reference's picture of that pair's flow, drawn on the device on the slot's stream
        (`HSFlow.render`): an (H, W, 3) uint8 NumPy array, or into the CUDA uint8 tensor `out`; complete on return
        either way.  Raises HsflowError (E_STATE) once `depth` more pairs have been submitted."""
        rp = params if params is not None else make_render_params(route, **kw)
        if _is_device_tensor(out):
            ptr, stride = _render_target(out, self.height, self.width)
            self._check(self._lib.hsflow_pipeline_render_device(self._h, int(ticket), ctypes.byref(rp), ptr, stride))
            self._held.pop(int(ticket), None)
            return out
        img = _render_host(out, self.height, self.width)
        self._check(self._lib.hsflow_pipeline_render(self._h, int(ticket), ctypes.byref(rp), ctypes.c_void_p(img.ctypes.data), img.strides[0]))
        self._held.pop(int(ticket), None)
        return img

    def render_jpeg(self, ticket, route="cv", quality=95, params=None, **kw):
        """wait(ticket) + the JPEG file of that pair's picture as `bytes` (`HSFlow.render_jpeg` on the slot's stream):
        drawn and encoded on the device, complete on return.  Raises HsflowError (E_STATE) once `depth` more pairs have
        been submitted."""
        rp = params if params is not None else make_render_params(route, **kw)
        buf = np.empty(jpeg_bound(self.width, self.height), np.uint8)
        n = ctypes.c_size_t()
        self._check(self._lib.hsflow_pipeline_render_jpeg(self._h, int(ticket), ctypes.byref(rp), int(quality), ctypes.c_void_p(buf.ctypes.data),
                                                          buf.size, ctypes.byref(n)))
        self._held.pop(int(ticket), None)
        return buf[:n.value].tobytes()

    def color(self, ticket, max_flow=None, out=None, params=None):
        """wait(ticket) + the dense colour picture of that pair's flow, drawn on the device on the slot's stream
        (`HSFlow.color`): an (H, W, 3) uint8 NumPy array, or into the CUDA uint8 tensor `out` (`color_device`); complete on
        return either way.  Raises HsflowError (E_STATE) once `depth` more pairs have been submitted."""
        if _is_device_tensor(out):
            return self.color_device(ticket, out, max_flow=max_flow, params=params)
        cp = params if params is not None else make_color_params(max_flow)
        img = _render_host(out, self.height, self.width)
        self._check(self._lib.hsflow_pipeline_color(self._h, int(ticket), ctypes.byref(cp), ctypes.c_void_p(img.ctypes.data), img.strides[0], None))
        self._held.pop(int(ticket), None)
        return img

    def color_device(self, ticket, out, max_flow=None, params=None):
        """`color` into the CUDA uint8 tensor `out` of shape (H, W, 3) (`hsflow_pipeline_color_device`); returns `out`."""
        cp = params if params is not None else make_color_params(max_flow)
        ptr, stride = _render_target(out, self.height, self.width)
        self._check(self._lib.hsflow_pipeline_color_device(self._h, int(ticket), ctypes.byref(cp), ptr, stride))
        self._held.pop(int(ticket), None)
        return out

    def color_jpeg(self, ticket, max_flow=None, quality=95, params=None):
        """wait(ticket) + the JPEG file of that pair's colour picture as `bytes` (`HSFlow.color_jpeg` on the slot's
        stream): drawn and encoded on the device, complete on return.  Raises HsflowError (E_STATE) once `depth` more
        pairs have been submitted."""
        cp = params if params is not None else make_color_params(max_flow)
        buf = np.empty(jpeg_bound(self.width, self.height), np.uint8)
        n = ctypes.c_size_t()
        self._check(self._lib.hsflow_pipeline_color_jpeg(self._h, int(ticket), ctypes.byref(cp), int(quality), ctypes.c_void_p(buf.ctypes.data),
                                                         buf.size, ctypes.byref(n)))
        self._held.pop(int(ticket), None)
        return buf[:n.value].tobytes()

    def warp(self, ticket, src=None, ref=None, out=None, t=1.0, border="constant", fill=0, return_stats=False, params=None, picture=True):
        """wait(ticket) + `HSFlow.warp` of that pair on its slot, on the slot's stream: `src` (None: the pair's own second
        frame, and ref=None then its first) warped backwards by the pair's flow; host pictures or CUDA tensors as there,
        but complete on return either way.  Raises HsflowError (E_STATE) once `depth` more pairs have been submitted."""
        device, args, out, stats = _warp_call(self.height, self.width, self.device, src, ref, out, params, t, border, fill, return_stats, picture)
        self._check((self._lib.hsflow_pipeline_warp_device if device else self._lib.hsflow_pipeline_warp)(self._h, int(ticket), *args))
        self._held.pop(int(ticket), None)
        return (out, stats) if return_stats else out

    def interp(self, ticket, t=0.5, prev=None, curr=None, vis_prev=None, vis_curr=None, ref=None, out=True, classes=False, stats=False, params=None):
        """wait(ticket) + `HSFlow.interp` of that pair on its slot: the frame at time `t` between the pair's two frames
        (prev, curr both None: the slot's own pre-processed frames) from the pair's flow; host pictures or CUDA tensors as
        there, but complete on return either way.  Returns (out, classes, stats).  Raises HsflowError (E_STATE) once the
        slot has been reused by a later pair."""
        device, args, out, classes, rec = _interp_call(self.height, self.width, self.device, prev, curr, vis_prev, vis_curr, ref, out, classes, stats, params, False)
        self._check((self._lib.hsflow_pipeline_interp_device if device else self._lib.hsflow_pipeline_interp)(self._h, int(ticket), float(t), *args))
        self._held.pop(int(ticket), None)
        return out, classes, rec

    def fb(self, ticket_fwd, ticket_bwd, mask=True, err2=False, stats=False, alpha=0.01, beta=0.5, values=(255, 0, 0, 0), params=None, device=False):
        """wait(both tickets) + `HSFlow.fb` of ticket_fwd's flow against ticket_bwd's on the forward pair's slot: host planes
        or CUDA tensors as there, but complete on return either way.  Returns (mask, err2, stats).  Raises HsflowError
        (E_STATE) once either slot has been reused by a later pair."""
        device, args, mask, err2, rec = _fb_call(self.height, self.width, self.device, mask, err2, stats, params, alpha, beta, values, device)
        self._check((self._lib.hsflow_pipeline_fb_device if device else self._lib.hsflow_pipeline_fb)(self._h, int(ticket_fwd), int(ticket_bwd), *args))
        self._held.pop(int(ticket_fwd), None)
        self._held.pop(int(ticket_bwd), None)
        return mask, err2, rec

    def median(self, ticket, state=None, flow=True, state_out=False, stats=False, radius=1, mode="filter", min_votes=1, passes=1, params=None):
        """wait(ticket) + the host form of `HSFlow.median` of that pair's flow on its slot (NumPy planes, the slot's flow
        unchanged): complete on return.  Returns (u_out, v_out, state_out, stats).  Raises HsflowError (E_STATE) once the
        slot has been reused by a later pair."""
        mp, (sp, ss), (up, vp, os_), (sop, sos), sref, u_out, v_out, state_out, rec = _median_call(
            self.height, self.width, self.device, state, flow, state_out, stats, params, radius, mode, min_votes, False)
        self._check(self._lib.hsflow_pipeline_median(self._h, int(ticket), ctypes.byref(mp), int(passes), sp, ss, up, vp, os_, sop, sos, sref))
        self._held.pop(int(ticket), None)
        return u_out, v_out, state_out, rec

    def median_apply(self, ticket, state=None, passes=1, state_out=False, stats=False, radius=1, mode="filter", min_votes=1, params=None):
        """wait(ticket) + `HSFlow.median_apply` on that pair's slot: the slot's flow is replaced (CUDA tensors as there),
        complete on return.  Returns (state_out, stats)."""
        mp, (sp, ss), _, (sop, sos), sref, _, _, state_out, rec = _median_call(
            self.height, self.width, self.device, state, None, state_out, stats, params, radius, mode, min_votes, True)
        self._check(self._lib.hsflow_pipeline_median_apply(self._h, int(ticket), ctypes.byref(mp), int(passes), sp, ss, sop, sos, sref))
        self._held.pop(int(ticket), None)
        return state_out, rec

    def verify(self, ticket):
        """wait(ticket) + `HSFlow.verify` of that pair on its slot (what the slot actually ran, the pipeline's own launch
        shape included): an `HsflowVerifyReport`.  Raises HsflowError (E_STATE) once `depth` more pairs have been submitted."""
        r = HsflowVerifyReport()
        r.struct_size = ctypes.sizeof(HsflowVerifyReport)
        self._check(self._lib.hsflow_pipeline_verify(self._h, int(ticket), ctypes.byref(r)))
        self._held.pop(int(ticket), None)
        return r

    def frames(self, ticket):
        """wait(ticket) + the slot's own copy of that pair's frames as two (H, W) uint8 NumPy arrays."""
        a = np.empty((self.height, self.width), np.uint8)
        b = np.empty((self.height, self.width), np.uint8)
        self._check(self._lib.hsflow_pipeline_frames_u8(self._h, int(ticket), ctypes.c_void_p(a.ctypes.data), a.strides[0],
                                                        ctypes.c_void_p(b.ctypes.data), b.strides[0]))
        self._held.pop(int(ticket), None)
        return a, b

    def copies_elided(self):
        """Submissions so far whose frame copy rode in the solve's first launch (hsflow_pipeline_copies_elided)."""
        n = ctypes.c_uint64()
        self._check(self._lib.hsflow_pipeline_copies_elided(self._h, ctypes.byref(n)))
        return n.value

    def wait(self, ticket):
        self._check(self._lib.hsflow_pipeline_wait(self._h, int(ticket)))
        self._held.pop(int(ticket), None)

    def info(self, ticket):
        """wait(ticket) + the solver's report for that pair (iterations_done, last_eps, eps_rerun, ...)."""
        i = HsflowInfo()
        i.struct_size = ctypes.sizeof(HsflowInfo)
        self._check(self._lib.hsflow_pipeline_info(self._h, int(ticket), ctypes.byref(i)))
        self._held.pop(int(ticket), None)
        return {name: getattr(i, name) for name, _ in HsflowInfo._fields_}

    def drain(self):
        self._check(self._lib.hsflow_pipeline_drain(self._h))
        self._held.clear()

    def close(self):
        if self._h is not None:
            self._lib.hsflow_pipeline_destroy(self._h)
            self._h = None
            self._held.clear()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
