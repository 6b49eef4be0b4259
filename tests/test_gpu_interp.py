"""The frame between the two frames of a pair on the GPU (include/hsflow.h, ABI 0.20: hsflow_interp*, hsflow_project_flow_device,
hsflow_pipeline_interp*; kernels in opticalflowhs_amd/csrc/hs_kernels_interp.hip.h) against the rule on the host
(hsflow_interp_host / hsflow_project_flow_host, which tests/test_interp_host.py holds to a NumPy restatement).  Planes and
pictures are compared bit for bit, records exactly."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
OK, E_ARG, E_SIZE, E_STATE = 0, 1, 2, 5
FILL = 0xA5
ENV_MAX = "HSFLOW_INTERP_BATCH_MAX"
BIG = np.nextafter(np.float32(1e9), np.float32(np.inf))
SPECIAL = [(np.nan, 1.0), (1.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (BIG, 0.0), (0.0, -BIG), (1e9, 0.0), (0.0, -1e9), (0.0, 0.0), (-0.0, -0.0),
           (1e-42, -1e-42), (2.0, -0.0), (0.5, 0.5), (-1e9, 1e9)]
STAT_FIELDS = ("blended", "prev_only", "curr_only", "clamped", "sad", "holes", "unfilled", "collisions", "left", "unknown", "max_diff")


def field(W, H, seed, sigma=6.0):
    """A Gaussian flow with the special values scattered over it (as many as fit)."""
    rng = np.random.default_rng(seed)
    u, v = (rng.standard_normal((H, W)) * sigma).astype(np.float32), (rng.standard_normal((H, W)) * sigma).astype(np.float32)
    spots = rng.permutation(W * H)
    for k, (a, b) in zip(spots, SPECIAL[:max(0, W * H // 8)]):
        u.flat[k], v.flat[k] = a, b
    return u, v


def pictures(W, H, C, seed):
    """Two pictures with structure (the costs differ) and noise, a reference, and two visibility planes."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(xs / 5.0) + 50 * np.cos(ys / 3.0)
    prev, curr = (np.clip(base[..., None] + rng.integers(-20, 21, (H, W, C)), 0, 255).astype(np.uint8) for _ in range(2))
    ref = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    vis = [((rng.random((H, W)) < 0.8) * 255).astype(np.uint8) for _ in range(2)]
    return prev, curr, ref, vis[0], vis[1]


def put_flow(ctx, u, v, pair=0):
    import torch
    ud, vd = torch.from_numpy(np.ascontiguousarray(u, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    torch.cuda.synchronize()
    ctx.set_flow_rows_from(ud, vd, 0, u.shape[0], pair=pair)
    ctx.synchronize()


def stat_tuple(s):
    return tuple(int(getattr(s, k)) for k in STAT_FIELDS)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


class DevImage(object):
    """H rows of `rowb` bytes in device memory, `stride` apart, the first `off` bytes behind a 256-byte multiple; FILL all
    around."""

    def __init__(self, H, rowb, off, stride, rows=None):
        import torch
        host = np.full(256 + off + H * stride + 16, FILL, np.uint8)
        self.buf = torch.from_numpy(host).cuda()
        self.base = (-self.buf.data_ptr()) % 256 + off
        self.H, self.rowb, self.stride = H, rowb, stride
        if rows is not None:
            host = np.full(self.buf.numel(), FILL, np.uint8)
            view = host[self.base:self.base + H * stride].reshape(H, stride)
            view[:, :rowb] = np.ascontiguousarray(rows).view(np.uint8).reshape(H, rowb)
            self.buf.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.base)

    def rows_and_rest(self):
        """(the picture's rows, True if every byte around them is still FILL)."""
        host = self.buf.cpu().numpy()
        rows = host[self.base:self.base + self.H * self.stride].reshape(self.H, self.stride)
        last = self.base + (self.H - 1) * self.stride + self.rowb
        clean = (rows[:-1, self.rowb:] == FILL).all() and (host[last:] == FILL).all() and (host[:self.base] == FILL).all()
        return np.ascontiguousarray(rows[:, :self.rowb]), bool(clean)


def dev_stats(n=1):
    import torch
    t = torch.full((64 * n + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def cuda(*arrays):
    import torch
    out = [torch.from_numpy(np.ascontiguousarray(a)).cuda() if a is not None else None for a in arrays]
    torch.cuda.synchronize()
    return out


def flow_unchanged(ctx, u, v, pair=0):
    u2, v2 = ctx.flow(pair)
    return np.array_equal(bits(u2), bits(u)) and np.array_equal(bits(v2), bits(v))


# ---- 1. device against host ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("W,H", [(13, 7), (260, 37), (1027, 9), (96, 64)])
def test_device_equals_host_written_flow(hs, gpu_ok, W, H, C):
    """A written Gaussian flow with special values: projected planes, state, class plane, picture and record, in unaligned
    device memory with FILL all around."""
    L = hs._lib.load()
    prev, curr, ref, vp, vc = pictures(W, H, C, W + C)
    u, v = field(W, H, 7 * W + H)
    rowb = W * C
    layouts = [(0, (rowb + 3) // 4 * 4), (1, rowb + 1), (2, rowb), (3, rowb + 5)]   # (offset from a 256-byte multiple, stride)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for k, (t, passes, radius, with_vis) in enumerate(((0.5, 4, 1, True), (0.25, 1, 2, False), (1.0, 0, 1, True), (0.0, 4, 1, False))):
            ip = hs.make_interp_params(C, radius, 1, passes)
            hvp, hvc = (vp, vc) if with_vis else (None, None)
            want, wcls, ws = hs.interp_host(u, v, prev, curr, t=t, vis_prev=hvp, vis_curr=hvc, ref=ref, classes=True, stats=True, params=ip)
            wu, wv, wstate, wps = hs.project_flow_host(u, v, prev, curr, t=t, state=True, stats=True, params=ip)
            assert ws.unknown >= 6 or W * H < 100
            got, gcls, gs = ctx.interp(t, prev, curr, hvp, hvc, ref, classes=True, stats=True, params=ip)       # host memory in and out
            assert np.array_equal(got, want) and np.array_equal(gcls, wcls), (t, int((got != want).sum()))
            assert stat_tuple(gs) == stat_tuple(ws)
            off, stride = layouts[k]
            p_off, p_stride = layouts[(k + 1) % 4]
            c_off, c_stride = layouts[(k + 2) % 4]
            dprev, dcurr, dref = DevImage(H, rowb, p_off, p_stride, prev), DevImage(H, rowb, c_off, c_stride, curr), DevImage(H, rowb, off, stride, ref)
            dvp, dvc = DevImage(H, W, 1, W + 3, vp), DevImage(H, W, 0, W, vc)
            ddst, dcls, dst = DevImage(H, rowb, off, stride), DevImage(H, W, (k + 1) % 4, W + k), dev_stats()
            assert L.hsflow_interp_device(ctx._h, 0, t, ctypes.byref(ip), dprev.ptr, p_stride, dcurr.ptr, c_stride, dvp.ptr if with_vis else None, W + 3,
                                          dvc.ptr if with_vis else None, W, dref.ptr, stride, ddst.ptr, stride, dcls.ptr, W + k,
                                          ctypes.c_void_p(dst.data_ptr())) == OK
            ctx.synchronize()
            rows, clean = ddst.rows_and_rest()
            assert np.array_equal(rows.reshape(H, W, C), want) and clean, (t, off, stride)
            rows, clean = dcls.rows_and_rest()
            assert np.array_equal(rows, wcls) and clean, t
            assert stat_tuple(hs.interp_stats_from(dst)) == stat_tuple(ws)
            assert bool((dst[64:] == FILL).all().item())
            assert all(d.rows_and_rest()[1] for d in (dprev, dcurr, dref, dvp, dvc))
            # the projection alone, into padded planes
            du, dv, dstate, dst = DevImage(H, 4 * W, 4 * (k % 2), 4 * W + 4 * k), DevImage(H, 4 * W, 0, 4 * W + 4 * k), DevImage(H, W, k, W + 2), dev_stats()
            assert L.hsflow_project_flow_device(ctx._h, 0, t, ctypes.byref(ip), dprev.ptr, p_stride, dcurr.ptr, c_stride, du.ptr, dv.ptr, 4 * W + 4 * k,
                                                dstate.ptr, W + 2, ctypes.c_void_p(dst.data_ptr())) == OK
            ctx.synchronize()
            for d, w in ((du, wu), (dv, wv)):
                rows, clean = d.rows_and_rest()
                assert np.array_equal(rows.view(np.uint32), bits(wu if d is du else wv)) and clean, t
            rows, clean = dstate.rows_and_rest()
            assert np.array_equal(rows, wstate) and clean
            assert stat_tuple(hs.interp_stats_from(dst)) == stat_tuple(wps)
            assert flow_unchanged(ctx, u, v)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("W,H", [(13, 7), (260, 37), (1027, 9), (96, 64)])
def test_device_equals_host_solved_flow(hs, gpu_ok, W, H, C):
    """A solved flow, read where the solver left it (c->cur, the pitched planes): projected planes, state, class plane,
    picture and record.  C = 1: the context's own frames (d_prev == NULL); C = 3: the caller's pictures.  At the two shapes
    where a translation of (2, -1.5) leaves an interior, the interpolated frame beats the cross-fade on the device too."""
    L = hs._lib.load()
    prev, curr = synth.translating_pair(W, H, seed=1, dx=2.0, dy=-1.5)
    tint = np.array([1.0, 0.8, 0.6])
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        ctx.set_frames(prev, curr)
        ctx.solve(lam=0.1, max_iter=99, term_type=ITER)             # (an odd count: the flow ends in the other buffer than at 100)
        u, v = ctx.flow()
        A, B = ctx.frames()
        if C == 3:
            A, B = (np.clip(np.rint(g[..., None] * tint), 0, 255).astype(np.uint8) for g in (A, B))
        for t in (0.25, 0.5, 0.75):
            true = synth.translating_pair(W, H, seed=1, dx=2.0 * t, dy=-1.5 * t)[1]
            if C == 3:
                true = np.clip(np.rint(true[..., None] * tint), 0, 255).astype(np.uint8)
            want, wcls, ws = hs.interp_host(u, v, A, B, t=t, ref=true, classes=True, stats=True)
            if C == 3:
                got, gcls, gs = ctx.interp(t, A, B, ref=true, classes=True, stats=True)
            else:
                got, gcls, gs = ctx.interp(t, ref=true, classes=True, stats=True)      # d_prev == NULL: the context's own frames
            assert np.array_equal(got, want) and np.array_equal(gcls, wcls) and stat_tuple(gs) == stat_tuple(ws), t
            # the projection alone, on the device, into padded planes
            wu, wv, wstate, wps = hs.project_flow_host(u, v, A, B, t=t, state=True, stats=True, params=hs.make_interp_params(C))
            du, dv, dstate, dst = DevImage(H, 4 * W, 4, 4 * W + 8), DevImage(H, 4 * W, 0, 4 * W + 8), DevImage(H, W, 1, W + 2), dev_stats()
            dA, dB = cuda(A, B) if C == 3 else (None, None)
            ip = hs.make_interp_params(C)
            assert L.hsflow_project_flow_device(ctx._h, 0, t, ctypes.byref(ip), ctypes.c_void_p(dA.data_ptr()) if C == 3 else None, W * C,
                                                ctypes.c_void_p(dB.data_ptr()) if C == 3 else None, W * C, du.ptr, dv.ptr, 4 * W + 8, dstate.ptr, W + 2,
                                                ctypes.c_void_p(dst.data_ptr())) == OK
            ctx.synchronize()
            for d, w in ((du, wu), (dv, wv)):
                rows, clean = d.rows_and_rest()
                assert np.array_equal(rows.view(np.uint32), bits(w)) and clean, t
            rows, clean = dstate.rows_and_rest()
            assert np.array_equal(rows, wstate) and clean
            assert stat_tuple(hs.interp_stats_from(dst)) == stat_tuple(wps)
            if (W, H) in ((96, 64), (260, 37)):
                zero = np.zeros_like(u)
                _, _, cross = hs.interp_host(zero, zero, A, B, t=t, ref=true, stats=True)
                print("%dx%d C=%d t=%.2f: interp %d, cross-fade %d" % (W, H, C, t, gs.sad, cross.sad))
                assert 3 * gs.sad < 2 * cross.sad
        assert flow_unchanged(ctx, u, v)


# ---- 2. batch --------------------------------------------------------------------------------------------------------

def _with_batch_max(value):
    class Guard(object):
        def __enter__(self):
            self.saved = os.environ.get(ENV_MAX)
            if value is None:
                os.environ.pop(ENV_MAX, None)
            else:
                os.environ[ENV_MAX] = value

        def __exit__(self, *a):
            os.environ.pop(ENV_MAX, None)
            if self.saved is not None:
                os.environ[ENV_MAX] = self.saved
    return Guard()


@pytest.mark.parametrize("chunk", [None, "3"])
def test_batch_of_eleven_times(hs, gpu_ok, chunk):
    """11 times are two chunks of at most 8, or four of at most 3: picture i is that of the single call."""
    import torch
    W, H, C, N = 70, 21, 3, 11
    prev, curr, _, vp, vc = pictures(W, H, C, 9)
    refs = np.random.default_rng(1).integers(0, 256, (N, H, W, C), dtype=np.uint8)
    u, v = field(W, H, 4, sigma=4.0)
    times = [k / (N - 1) for k in range(N)]
    ip = hs.make_interp_params(C, fill_passes=3)
    wants = [hs.interp_host(u, v, prev, curr, t=t, vis_prev=vp, vis_curr=vc, ref=refs[k], classes=True, stats=True, params=ip) for k, t in enumerate(times)]
    dprev, dcurr, dvp, dvc, drefs = cuda(prev, curr, vp, vc, refs)
    with _with_batch_max(chunk), hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        out = torch.full((N, H, W, C), FILL, dtype=torch.uint8, device="cuda")
        cls = torch.full((N, H, W), FILL, dtype=torch.uint8, device="cuda")
        st = dev_stats(N)
        assert ctx.interp_batch_device(times, out, dprev, dcurr, dvp, dvc, drefs, cls, st, params=ip) is out
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), np.stack([w[0] for w in wants]))
        assert np.array_equal(cls.cpu().numpy(), np.stack([w[1] for w in wants]))
        assert [stat_tuple(g) for g in hs.interp_stats_from(st, N)] == [stat_tuple(w[2]) for w in wants]
        assert bool((st[64 * N:] == FILL).all().item())
        for k in (0, 4, 10):                                       # the single call through the same scratch
            one, _, s1 = ctx.interp(times[k], dprev, dcurr, dvp, dvc, drefs[k], stats=True, params=ip)
            ctx.synchronize()
            assert np.array_equal(one.cpu().numpy(), wants[k][0]) and stat_tuple(hs.interp_stats_from(s1)) == stat_tuple(wants[k][2])
        st = dev_stats(N)
        ctx.interp_batch_device(times, None, dprev, dcurr, dvp, dvc, drefs, None, st, params=ip)                 # statistics only
        ctx.synchronize()
        assert [stat_tuple(g) for g in hs.interp_stats_from(st, N)] == [stat_tuple(w[2]) for w in wants]
        out.fill_(FILL)
        ctx.interp_batch_device(times, out, dprev, dcurr, dvp, dvc, params=ip)                                   # pictures only
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), np.stack([w[0] for w in wants]))
        assert flow_unchanged(ctx, u, v)
        os.environ[ENV_MAX] = "9"
        with pytest.raises(hs.HsflowError) as e:
            ctx.interp_batch_device(times, out, dprev, dcurr, params=ip)
        assert e.value.status == E_ARG and ENV_MAX in str(e.value)


# ---- 3. ordering -----------------------------------------------------------------------------------------------------

def _patch_pair(W, H):
    """A flat frame with a patch one grey level brighter; with lambda 1e-3 / epsilon 1e-4 its early stop fires."""
    a = np.full((H, W), 90, np.uint8)
    b = a.copy()
    rows, cols = slice(H // 4, H // 4 + min(80, H // 2)), slice(W // 5, W // 5 + min(300, W // 2))
    a[rows, cols], b[rows, cols] = 120, 121
    return a, b


def test_own_frames_behind_an_asynchronous_solve(hs, gpu_ok):
    """d_prev == NULL behind an asynchronous ITER|EPS solve whose check is still owed."""
    import torch
    L = hs._lib.load()
    W, H = 300, 70
    kw = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)
    A, B = _patch_pair(W, H)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        info = ctx.solve(**kw)
        assert 1 < info["iterations_done"] < 400, info             # its early stop fires
        u, v = ctx.flow()
        fa, fb = ctx.frames()
    want, wcls, ws = hs.interp_host(u, v, fa, fb, t=0.5, ref=fa, classes=True, stats=True)
    for async_reduce in (0, 1):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with hs.HSFlow(W, H, stream=s.cuda_stream) as ctx:
            assert L.hsflow_set_async_reduce(ctx._h, async_reduce) == OK
            ctx.set_frames(A, B)
            out = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
            dref = cuda(fa)[0]
            ctx.solve_async(**kw)
            _, cls, st = ctx.interp(0.5, ref=dref, out=out, classes=True, stats=True)   # at once: the owed ITER|EPS check is settled first
            assert L.hsflow_wait_solve(ctx._h) == OK
            assert s.query(), "wait_solve returned while an interpolation was still in flight"
            assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(cls.cpu().numpy(), wcls), async_reduce
            assert stat_tuple(hs.interp_stats_from(st)) == stat_tuple(ws)
            assert ctx.info()["iterations_done"] == info["iterations_done"]
            ctx.solve_async(**kw)
            got, _, gs = ctx.interp(0.5, ref=fa, stats=True)       # the synchronous form behind an asynchronous solve
            assert np.array_equal(got, want) and stat_tuple(gs) == stat_tuple(ws)
            assert flow_unchanged(ctx, u, v)


def test_per_pair_stop(hs, gpu_ok):
    """A context with hsflow_set_pair_termination: every pair is interpolated by its own final flow."""
    W, H = 300, 70
    kw = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)
    still = np.full((H, W), 77, np.uint8)
    pairs = [synth.translating_pair(W, H, seed=2, dx=1.5, dy=-1.0), _patch_pair(W, H), (still, still.copy())]
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        ctx.set_pair_termination(True)
        for p, (A, B) in enumerate(pairs):
            ctx.set_frames(A, B, pair=p)
        ctx.solve(**kw)
        assert len(set(r["iterations_done"] for r in ctx.pair_results())) == 3
        for p in range(3):
            u, v = ctx.flow(p)
            A, B = ctx.frames(p)
            want, _, ws = hs.interp_host(u, v, A, B, t=0.5, ref=A, stats=True)
            got, _, gs = ctx.interp(0.5, ref=A, stats=True, pair=p)
            assert np.array_equal(got, want) and stat_tuple(gs) == stat_tuple(ws), p


# ---- 4. with the other operators -------------------------------------------------------------------------------------

def test_visibility_from_the_forward_backward_check(hs, gpu_ok):
    """The vis planes are the masks of hsflow_fb_device of a two-pair context made with hsflow_set_frames_reversed."""
    import torch
    W, H = 96, 64
    prev, curr = synth.translating_pair(W, H, seed=3, dx=3.0, dy=1.0)
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        ctx.set_frames(prev, curr, pair=0)
        ctx.set_frames_reversed(1, 0)
        ctx.solve(lam=0.1, max_iter=100, term_type=ITER)
        vis_prev = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        vis_curr = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        ctx.fb(0, 1, mask=vis_prev)
        ctx.fb(1, 0, mask=vis_curr)
        out, cls, st = ctx.interp(0.5, vis_prev=vis_prev, vis_curr=vis_curr, out=torch.zeros((H, W), dtype=torch.uint8, device="cuda"), classes=True, stats=True)
        ctx.synchronize()
        u, v = ctx.flow(0)
        A, B = ctx.frames(0)
        hp, hc = vis_prev.cpu().numpy(), vis_curr.cpu().numpy()
        assert 0 < int((hp == 0).sum()) < W * H and 0 < int((hc == 0).sum()) < W * H
        want, wcls, ws = hs.interp_host(u, v, A, B, t=0.5, vis_prev=hp, vis_curr=hc, classes=True, stats=True)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(cls.cpu().numpy(), wcls)
        gs = hs.interp_stats_from(st)
        assert stat_tuple(gs) == stat_tuple(ws) and gs.prev_only > 0 and gs.curr_only > 0


def test_projected_flow_starts_the_next_solve(hs, gpu_ok):
    """hsflow_project_flow_device at t = 1 written back with hsflow_set_flow_device, followed by a warm solve that runs."""
    W, H = 96, 64
    prev, curr = synth.translating_pair(W, H, seed=1, dx=2.0, dy=-1.5)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        ctx.set_frames(prev, curr)
        ctx.solve(lam=0.1, max_iter=100, term_type=ITER)
        u, v = ctx.flow()
        A, B = ctx.frames()
        du, dv, dstate, st = ctx.project_flow(1.0, state=True, stats=True)
        ctx.synchronize()
        wu, wv, wstate, ws = hs.project_flow_host(u, v, A, B, t=1.0, state=True, stats=True)
        assert np.array_equal(bits(du.cpu().numpy()), bits(wu)) and np.array_equal(bits(dv.cpu().numpy()), bits(wv))
        assert np.array_equal(dstate.cpu().numpy(), wstate) and stat_tuple(hs.interp_stats_from(st)) == stat_tuple(ws)
        assert flow_unchanged(ctx, u, v)
        ctx.set_flow_rows_from(du, dv, 0, H)
        u1, v1 = ctx.flow()
        assert np.array_equal(bits(u1), bits(wu)) and np.array_equal(bits(v1), bits(wv))
        info = ctx.solve(lam=0.1, max_iter=10, term_type=ITER, use_previous=True)
        assert info["iterations_done"] == 10
        u2, v2 = ctx.flow()
        assert np.isfinite(u2).all() and not np.array_equal(u2, u1)
        # ten warm sweeps from the projected flow stay closer to the converged flow than ten cold ones
        cold = ctx.solve(lam=0.1, max_iter=10, term_type=ITER) and ctx.flow()
        assert np.abs(u2 - u).mean() < np.abs(cold[0] - u).mean()


def test_pipeline(hs, gpu_ok):
    import torch
    W, H, depth = 64, 48, 3
    kw = dict(lam=0.1, max_iter=60, term_type=ITER)
    pairs = [synth.translating_pair(W, H, seed=s, dx=dx, dy=dy) for s, dx, dy in ((1, 0.75, -0.5), (2, -1.0, 1.0), (3, 0.25, 0.5), (4, 1.25, 0.0))]
    cp, cc, cref, _, _ = pictures(W, H, 3, 4)
    want = []
    for A, B in pairs:
        with hs.HSFlow(W, H, own_stream=True) as ctx:
            ctx.set_frames(A, B)
            ctx.solve(**kw)
            want.append((ctx.interp(0.5, stats=True), ctx.interp(0.25, cp, cc, ref=cref, classes=True, stats=True)))
    dev = [tuple(torch.from_numpy(f).cuda() for f in AB) for AB in pairs]
    dcp, dcc, dcref = cuda(cp, cc, cref)

    def check_ticket(pl, t):
        (own_pic, _, own_stats), (col_pic, col_cls, col_stats) = want[t]
        pic, _, st = pl.interp(t, 0.5, stats=True)
        assert np.array_equal(pic, own_pic) and stat_tuple(st) == stat_tuple(own_stats), t
        pic, cls, st = pl.interp(t, 0.25, cp, cc, ref=cref, classes=True, stats=True)
        assert np.array_equal(pic, col_pic) and np.array_equal(cls, col_cls) and stat_tuple(st) == stat_tuple(col_stats), t
        out = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pic, _, st = pl.interp(t, 0.25, dcp, dcc, ref=dcref, out=out, stats=True)          # complete on return
        assert pic is out and np.array_equal(out.cpu().numpy(), col_pic) and stat_tuple(hs.interp_stats_from(st)) == stat_tuple(col_stats), t

    with hs.PairPipeline(W, H, depth=depth, lanes=2) as pl:
        for t in range(len(pairs)):
            if t >= depth:
                check_ticket(pl, t - depth)                        # the oldest pair, before its slot is taken again
            assert pl.submit_device(dev[t][0], dev[t][1], **kw) == t
        for t in range(len(pairs) - depth, len(pairs)):
            check_ticket(pl, t)
        for call in (lambda: pl.interp(0), lambda: pl.interp(0, 0.5, dcp, dcc)):   # its slot has been reused since
            with pytest.raises(hs.HsflowError) as e:
                call()
            assert e.value.status == E_STATE
        check_ticket(pl, len(pairs) - 1)                           # the pipeline still works


# ---- 5. command line -------------------------------------------------------------------------------------------------

def _cli(args, extra_env=None, ok=True):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for name in ("HSFLOW_RENDER_DEVICE", "HSFLOW_JPEG_DEVICE", "HSFLOW_PICTURE", "HSFLOW_COLOR_MAX", "HSFLOW_WARP_T", "HSFLOW_INTERP_T", "HSFLOW_INTERP_FB"):
        env.pop(name, None)
    env.update(extra_env or {})
    r = subprocess.run([cli] + args, env=env, capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_cli_intermediate_frame(hs, gpu_ok, tmp_path):
    W, H = 96, 64
    A, B = synth.translating_pair(W, H, seed=1, dx=2.0, dy=-1.5)
    tint = np.array([1.0, 0.8, 0.6])
    frames = [np.clip(np.rint(g[..., None] * tint), 0, 255).astype(np.uint8) for g in (A, B)]   # a small colour pair
    names = [str(tmp_path / ("frame%d.ppm" % k)) for k in range(2)]
    for name, f in zip(names, frames):
        with open(name, "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (W, H) + f.tobytes())
    head = len(b"P6\n%d %d\n255\n" % (W, H))
    fields = ["blended", "prev_only", "curr_only", "clamped", "holes", "unfilled", "collisions", "left", "unknown"]
    for args in (["-cv", "-hd", names[0], names[1], None, ".1", "100"], ["-cl", "-hd", names[0], names[1], None, "3", "50", "1", "GPU"]):
        for extra in ({}, {"HSFLOW_INTERP_T": "0.25"}, {"HSFLOW_INTERP_FB": "1"}):
            files, lines = {}, {}
            for route, env in (("host", {}), ("device", {"HSFLOW_RENDER_DEVICE": "1"})):
                out = str(tmp_path / ("%s_%s_%s.ppm" % (args[0][1:], route, "_".join(extra) or "plain")))
                r = _cli([out if a is None else a for a in args], dict(env, HSFLOW_PICTURE="interp", **extra))
                files[route] = open(out, "rb").read()
                lines[route] = [ln for ln in r.stdout.splitlines() if ln.startswith("interp:")]
                assert len(lines[route]) == 1
            assert files["host"] == files["device"] and lines["host"] == lines["device"]
            pic = np.frombuffer(files["host"][head:], np.uint8).reshape(H, W, 3)
            words = lines["host"][0].split()
            assert words[1] == "t" and words[3::2] == fields
            t = float(words[2])
            counts = dict(zip(fields, (int(x) for x in words[4::2])))
            assert t == float(extra.get("HSFLOW_INTERP_T", 0.5))
            assert counts["blended"] + counts["prev_only"] + counts["curr_only"] + counts["clamped"] == W * H and counts["unknown"] == 0
            if args[0] == "-cv" and "HSFLOW_INTERP_FB" not in extra:   # the library's own solve of the same frames, by the host rule
                with hs.HSFlow(W, H, own_stream=True) as ctx:
                    ctx.set_frames_bgr(np.ascontiguousarray(frames[0][..., ::-1]), np.ascontiguousarray(frames[1][..., ::-1]), blur=True)
                    ctx.solve(lam=0.1, max_iter=100)
                    u, v = ctx.flow()
                want, _, ws = hs.interp_host(u, v, frames[0], frames[1], t=t, stats=True)
                assert np.array_equal(pic, want)
                assert counts == {k: int(getattr(ws, k)) for k in fields}
            if "HSFLOW_INTERP_FB" in extra:
                assert counts["prev_only"] + counts["curr_only"] > 0
    for bad in ({"HSFLOW_PICTURE": "interp", "HSFLOW_INTERP_T": "1x"}, {"HSFLOW_PICTURE": "interp", "HSFLOW_INTERP_T": "nan"},
                {"HSFLOW_PICTURE": "interp", "HSFLOW_INTERP_T": "1.5"}, {"HSFLOW_PICTURE": "interpolate"}):
        r = _cli(["-cv", "-hd", names[0], names[1], str(tmp_path / "bad.ppm"), ".1", "10"], bad, ok=False)
        assert r.returncode == 1 and "HSFLOW_" in r.stdout
    r = _cli(["-cv", "-hd", names[0], names[1], str(tmp_path / "bad.ppm"), ".1", "10"], {"HSFLOW_PICTURE": "bogus"}, ok=False)
    assert "interp" in r.stdout
    r = _cli(["-cv", "-cam"], {"HSFLOW_PICTURE": "interp"}, ok=False)
    assert r.returncode == 1 and "HSFLOW_PICTURE=interp" in r.stdout


# ---- 6. errors -------------------------------------------------------------------------------------------------------

def test_argument_errors(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, C, N = 64, 4, 3, 2
    u, v = field(W, H, 1)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        prev = torch.full((H, W, C), 50, dtype=torch.uint8, device="cuda")
        curr = torch.full((H, W, C), 60, dtype=torch.uint8, device="cuda")
        vis = torch.full((H, W), 255, dtype=torch.uint8, device="cuda")
        out = torch.full((N, H, W, C), FILL, dtype=torch.uint8, device="cuda")
        cls = torch.full((N, H, W), FILL, dtype=torch.uint8, device="cuda")
        fu = torch.full((2, H, W), 7.0, dtype=torch.float32, device="cuda")
        stats = dev_stats(N)
        lst = lambda t: (ctypes.c_void_p * N)(*[t[i].data_ptr() for i in range(N)])
        outs, clss = lst(out), lst(cls)
        holed = (ctypes.c_void_p * N)(outs[0], None)
        pp, cp, vp = (ctypes.c_void_p(x.data_ptr()) for x in (prev, curr, vis))
        sp = ctypes.c_void_p(stats.data_ptr())
        rb = W * C
        times = (ctypes.c_float * N)(0.25, 0.75)
        host_prev, host_curr, host_out = np.full((H, rb), 50, np.uint8), np.full((H, rb), 60, np.uint8), np.full((H, rb), FILL, np.uint8)
        hstats = hs.HsflowInterpStats()
        ctypes.memset(ctypes.byref(hstats), FILL, 64)
        torch.cuda.synchronize()

        def dev(ip, t=0.5, pair=0, p=pp, ps=rb, c=cp, cs=rb, v1=None, v1s=0, d=outs[0], ds=rb, k=clss[0], ks=W, s=sp, h=ctx._h):
            return L.hsflow_interp_device(h, pair, t, ip, p, ps, c, cs, v1, v1s, None, 0, None, 0, d, ds, k, ks, s)

        def bat(ip, n=N, tt=times, p=pp, ps=rb, c=cp, cs=rb, d=outs, ds=rb, k=clss, ks=W, s=sp):
            return L.hsflow_interp_batch_device(ctx._h, 0, n, tt, ip, p, ps, c, cs, None, 0, None, 0, None, 0, d, ds, k, ks, s)

        def syn(ip, t=0.5, pair=0, p=host_prev.ctypes.data, ps=rb, c=host_curr.ctypes.data, cs=rb, d=host_out.ctypes.data, ds=rb):
            return L.hsflow_interp(ctx._h, pair, t, ip, p, ps, c, cs, None, 0, None, 0, None, 0, d, ds, None, 0, ctypes.byref(hstats))

        def prj(ip, t=1.0, a=ctypes.c_void_p(fu[0].data_ptr()), b=ctypes.c_void_p(fu[1].data_ptr()), os_=4 * W, s=sp, p=pp, c=cp):
            return L.hsflow_project_flow_device(ctx._h, 0, t, ip, p, rb, c, rb, a, b, os_, None, 0, s)
        bad = []
        for change in (dict(struct_size=16), dict(channels=2), dict(channels=0), dict(fill_radius=3), dict(fill_radius=0), dict(fill_min_votes=0),
                       dict(fill_min_votes=10), dict(fill_passes=-1), dict(fill_passes=65)):
            b = hs.make_interp_params(C)
            for key, val in change.items():
                setattr(b, key, val)
            bad.append(ctypes.byref(b))
        for b in bad + [None]:
            assert dev(b) == E_ARG and bat(b) == E_ARG and syn(b) == E_ARG and prj(b) == E_ARG
        r = ctypes.byref(hs.make_interp_params(C))
        r1 = ctypes.byref(hs.make_interp_params(1))
        for t in (float("nan"), float("inf"), -0.001, 1.001):
            assert dev(r, t=t) == E_ARG and syn(r, t=t) == E_ARG and prj(r, t=t) == E_ARG
            assert bat(r, tt=(ctypes.c_float * N)(0.5, t)) == E_ARG
        assert bat(r, tt=None) == E_ARG and bat(r, n=0) == E_ARG
        assert dev(r, pair=1) == E_ARG and dev(r, pair=-1) == E_ARG and dev(r, h=None) == E_ARG and syn(r, pair=1) == E_ARG
        assert bat(r, d=holed) == E_ARG and bat(r, k=holed) == E_ARG
        assert dev(r, p=None, c=None) == E_ARG and syn(r, p=None, c=None) == E_ARG and prj(r, p=None, c=None) == E_ARG   # 3 channels of the own frames
        assert dev(r, p=None) == E_ARG and dev(r, c=None) == E_ARG                                  # one frame of the two
        assert dev(r, d=pp) == E_ARG and dev(r, d=cp) == E_ARG and dev(r, v1=vp, v1s=W, k=vp) == E_ARG   # onto an input
        assert bat(r, d=(ctypes.c_void_p * N)(outs[0], pp.value)) == E_ARG
        assert syn(r, d=host_prev.ctypes.data) == E_ARG
        assert dev(r, d=None, k=None, s=None) == E_ARG and bat(r, d=None, k=None, s=None) == E_ARG   # nothing asked for
        assert prj(r, a=None, b=None, s=None) == E_ARG and prj(r, b=None) == E_ARG
        assert dev(r, ps=rb - 1) == E_SIZE and dev(r, cs=rb - 1) == E_SIZE and dev(r, ds=rb - 1) == E_SIZE and dev(r, ks=W - 1) == E_SIZE
        assert dev(r, v1=vp, v1s=W - 1) == E_SIZE
        assert bat(r, ps=rb - 1) == E_SIZE and bat(r, ds=rb - 1) == E_SIZE and bat(r, ks=W - 1) == E_SIZE
        assert syn(r, ps=rb - 1) == E_SIZE and syn(r, ds=rb - 1) == E_SIZE
        assert prj(r, os_=4 * W - 4) == E_SIZE and prj(r, os_=4 * W + 2) == E_SIZE
        assert prj(r, a=ctypes.c_void_p(fu[0].data_ptr() + 2)) == E_ARG                             # a misaligned flow plane
        assert dev(r1, p=None, c=None, ds=W - 1) == E_SIZE
        for odd in (1, 4):                                        # the records are 64-bit counters: 8-byte aligned or refused
            off = ctypes.c_void_p(stats.data_ptr() + odd)
            assert dev(r, s=off) == E_ARG and bat(r, s=off) == E_ARG and prj(r, s=off) == E_ARG
        ctx.synchronize()
        assert bool((out == FILL).all().item()) and bool((cls == FILL).all().item()) and bool((stats == FILL).all().item())   # nothing was written
        assert bool((fu == 7.0).all().item()) and (host_out == FILL).all() and bytes(hstats) == bytes([FILL]) * 64
        assert syn(r) == OK
        want, _, ws = hs.interp_host(u, v, host_prev.reshape(H, W, C), host_curr.reshape(H, W, C), t=0.5, stats=True)
        assert np.array_equal(host_out.reshape(H, W, C), want) and stat_tuple(hstats) == stat_tuple(ws)
        assert flow_unchanged(ctx, u, v)
