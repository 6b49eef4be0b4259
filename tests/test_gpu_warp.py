"""A picture warped by the flow on the GPU, and the residual (include/hsflow.h, ABI 0.17: hsflow_warp*, hsflow_pipeline_warp*;
kernel in opticalflowhs_amd/csrc/hs_kernels_warp.hip.h) against the rule on the host (hsflow_warp_host, which
tests/test_warp_host.py holds to a NumPy restatement).  Pictures are compared byte for byte, statistics exactly."""
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
ENV_MAX = "HSFLOW_JPEG_BATCH_MAX"
BIG = np.nextafter(np.float32(1e9), np.float32(np.inf))
SPECIAL = [(np.nan, 1.0), (1.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (BIG, 0.0), (0.0, -BIG), (1e9, 0.0), (0.0, -1e9), (0.0, 0.0), (-0.0, -0.0),
           (1e-42, -1e-42), (2.0, -0.0), (0.5, 0.5), (-1e9, 1e9)]
STAT_FIELDS = ("inside", "outside", "unknown", "sad_warped", "sad_plain", "max_warped", "max_plain")


def field(W, H, seed, sigma=6.0):
    """A Gaussian flow with the special values scattered over it (as many as fit), and pixels that sample the last column
    and the last row exactly."""
    rng = np.random.default_rng(seed)
    u, v = (rng.standard_normal((H, W)) * sigma).astype(np.float32), (rng.standard_normal((H, W)) * sigma).astype(np.float32)
    spots = rng.permutation(W * H)
    vals = SPECIAL[:max(0, W * H // 2)]
    for k, (a, b) in zip(spots, vals):
        u.flat[k], v.flat[k] = a, b
    for k in spots[len(vals):len(vals) + 4]:                      # fx == W-1, fy == H-1, fx == 0, fy == 0, exactly
        y, x = divmod(int(k), W)
        u[y, x], v[y, x] = ((W - 1 - x, 0.0), (0.0, H - 1 - y), (-x, 0.0), (0.0, -y))[int(k) % 4]
    return u, v


def put_flow(ctx, u, v, pair=0):
    import torch
    ud, vd = torch.from_numpy(np.ascontiguousarray(u, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    torch.cuda.synchronize()
    ctx.set_flow_rows_from(ud, vd, 0, u.shape[0], pair=pair)
    ctx.synchronize()


def stat_tuple(s):
    return tuple(int(getattr(s, k)) for k in STAT_FIELDS)


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
            view[:, :rowb] = rows.reshape(H, rowb)
            self.buf.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.base)

    def rows_and_rest(self):
        """(the picture's rows, True if every byte around them is still FILL)."""
        host = self.buf.cpu().numpy()
        rows = host[self.base:self.base + self.H * self.stride].reshape(self.H, self.stride)
        last = self.base + (self.H - 1) * self.stride + self.rowb
        clean = (rows[:-1, self.rowb:] == FILL).all() and (host[last:] == FILL).all() and (host[:self.base] == FILL).all()
        return rows[:, :self.rowb], bool(clean)


def dev_stats(n=1):
    import torch
    t = torch.full((64 * n + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


# ---- 1. device against host ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("W,H", [(13, 7), (260, 37), (1027, 9), (96, 64)])
def test_device_equals_host(hs, gpu_ok, W, H, C):
    L = hs._lib.load()
    rng = np.random.default_rng(W + C)
    src = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    ref = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    u, v = field(W, H, 7 * W + H)
    rowb = W * C
    aligned = (rowb + 3) // 4 * 4
    layouts = [(0, aligned), (1, rowb + 1), (2, rowb), (3, rowb + 5)]   # (offset from a 256-byte multiple, stride)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for border in ("constant", "replicate"):
            for t in (1.0, -0.5):
                wp = hs.make_warp_params(C, t, border, (7, 200, 33))
                want, ws = hs.warp_host(u, v, src, ref=ref, params=wp, return_stats=True)
                assert ws.unknown >= 6 or W * H < 40
                got, gs = ctx.warp(src, ref=ref, params=wp, return_stats=True)            # host pictures in and out
                assert np.array_equal(got, want), (border, t, int((got != want).sum()))
                assert stat_tuple(gs) == stat_tuple(ws)
                for k, (off, stride) in enumerate(layouts):
                    s_off, s_stride = layouts[(k + 1) % 4]
                    r_off, r_stride = layouts[(k + 2) % 4]
                    dsrc, dref = DevImage(H, rowb, s_off, s_stride, src), DevImage(H, rowb, r_off, r_stride, ref)
                    ddst, dst = DevImage(H, rowb, off, stride), dev_stats()
                    assert L.hsflow_warp_device(ctx._h, 0, ctypes.byref(wp), dsrc.ptr, s_stride, dref.ptr, r_stride, ddst.ptr, stride,
                                                ctypes.c_void_p(dst.data_ptr())) == OK
                    ctx.synchronize()
                    rows, clean = ddst.rows_and_rest()
                    assert np.array_equal(rows.reshape(H, W, C), want), (border, t, off, stride)
                    assert clean, (off, stride)                                              # nothing beyond C*W of a row
                    assert stat_tuple(hs.warp_stats_from(dst)) == stat_tuple(ws)
                    assert bool((dst[64:] == FILL).all().item())
                    assert dsrc.rows_and_rest()[1] and dref.rows_and_rest()[1]


def test_statistics_only_and_no_reference(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, C = 260, 37, 3
    rng = np.random.default_rng(2)
    src = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    ref = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    u, v = field(W, H, 3)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        want, ws = hs.warp_host(u, v, src, ref=ref, return_stats=True)
        _, ws_noref = hs.warp_host(u, v, src, return_stats=True)
        assert stat_tuple(ws_noref)[3:] == (0, 0, 0, 0) and stat_tuple(ws)[3] > 0
        dsrc, dref = torch.from_numpy(src).cuda(), torch.from_numpy(ref).cuda()
        torch.cuda.synchronize()
        none, st = ctx.warp(dsrc, ref=dref, return_stats=True, picture=False)             # d_dst == NULL
        ctx.synchronize()
        assert none is None and stat_tuple(hs.warp_stats_from(st)) == stat_tuple(ws)
        out, st = ctx.warp(dsrc, return_stats=True)                                        # d_ref == NULL
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), want) and stat_tuple(hs.warp_stats_from(st)) == stat_tuple(ws_noref)
        out = ctx.warp(dsrc)                                                               # no statistics
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), want)
        none, hs_only = ctx.warp(src, ref=ref, return_stats=True, picture=False)           # the host form, statistics only
        assert none is None and stat_tuple(hs_only) == stat_tuple(ws)
        # another kind of picture through the same context's staging
        gray = np.ascontiguousarray(src[..., 0])
        assert np.array_equal(ctx.warp(gray), hs.warp_host(u, v, gray))
        assert np.array_equal(ctx.warp(src), want)
        assert L.hsflow_warp_device(ctx._h, 0, ctypes.byref(hs.make_warp_params(C)), ctypes.c_void_p(dsrc.data_ptr()), W * C, None, 0, None, 0, None) == E_ARG


# ---- 2. batch --------------------------------------------------------------------------------------------------------

def _with_batch_max(value):
    class Guard(object):
        def __enter__(self):
            self.saved = os.environ.get(ENV_MAX)
            os.environ[ENV_MAX] = value

        def __exit__(self, *a):
            os.environ.pop(ENV_MAX, None)
            if self.saved is not None:
                os.environ[ENV_MAX] = self.saved
    return Guard()


def test_batch_in_three_chunks(hs, gpu_ok):
    import torch
    W, H, N, C = 40, 12, 5, 3
    rng = np.random.default_rng(9)
    flows = [field(W, H, 40 + p, sigma=1.0 + 2.0 * p) for p in range(N)]
    flows[2] = (np.full((H, W), np.nan, np.float32), np.full((H, W), np.nan, np.float32))
    srcs = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
    refs = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
    frames = [synth.translating_pair(W, H, seed=20 + p, dx=0.5 * p, dy=-0.25 * p) for p in range(N)]
    with _with_batch_max("2"), hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p, (u, v) in enumerate(flows):
            ctx.set_frames(frames[p][0], frames[p][1], pair=p)
            put_flow(ctx, u, v, pair=p)
        wp = hs.make_warp_params(C, 1.0, "replicate", (1, 2, 3))
        wants = [hs.warp_host(u, v, srcs[p], ref=refs[p], params=wp, return_stats=True) for p, (u, v) in enumerate(flows)]
        assert stat_tuple(wants[2][1])[:3] == (0, 0, W * H) and (wants[2][0] == np.array([1, 2, 3], np.uint8)).all()
        dsrc, dref = torch.from_numpy(srcs).cuda(), torch.from_numpy(refs).cuda()
        for first, n in ((0, N), (1, 3), (4, 1), (2, 2)):
            out = torch.full((n, H, W, C), FILL, dtype=torch.uint8, device="cuda")
            st = dev_stats(n)
            assert ctx.warp_batch_device(out, dsrc[first:first + n], dref[first:first + n], stats=st, first_pair=first, n=n, params=wp) is out
            ctx.synchronize()
            assert np.array_equal(out.cpu().numpy(), np.stack([w for w, _ in wants[first:first + n]])), (first, n)
            got = hs.warp_stats_from(st, n)
            got = got if n > 1 else [got]
            assert [stat_tuple(g) for g in got] == [stat_tuple(s) for _, s in wants[first:first + n]], (first, n)
            assert bool((st[64 * n:] == FILL).all().item())
        # the context's own frames: pair i's second frame onto its first, by pair i's flow
        own = [hs.warp_host(u, v, frames[p][1], ref=frames[p][0], return_stats=True) for p, (u, v) in enumerate(flows)]
        out = torch.full((N, H, W), FILL, dtype=torch.uint8, device="cuda")
        st = dev_stats(N)
        ctx.warp_batch_device(out, stats=st)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), np.stack([w for w, _ in own]))
        assert [stat_tuple(g) for g in hs.warp_stats_from(st, N)] == [stat_tuple(s) for _, s in own]
        st = dev_stats(N)
        ctx.warp_batch_device(None, stats=st)                                              # statistics only
        ctx.synchronize()
        assert [stat_tuple(g) for g in hs.warp_stats_from(st, N)] == [stat_tuple(s) for _, s in own]
        for p in (0, 3):
            one, s1 = ctx.warp(pair=p, return_stats=True)                                  # the synchronous form on its own frames
            assert np.array_equal(one, own[p][0]) and stat_tuple(s1) == stat_tuple(own[p][1])
        os.environ[ENV_MAX] = "0"
        with pytest.raises(hs.HsflowError) as e:
            ctx.warp_batch_device(out)
        assert e.value.status == E_ARG and ENV_MAX in str(e.value)


def _patch_pair(W, H):
    """A flat frame with a patch one grey level brighter; with lambda 1e-3 / epsilon 1e-4 its early stop fires."""
    a = np.full((H, W), 90, np.uint8)
    b = a.copy()
    rows, cols = slice(H // 4, H // 4 + min(80, H // 2)), slice(W // 5, W // 5 + min(300, W // 2))
    a[rows, cols], b[rows, cols] = 120, 121
    return a, b


def test_per_pair_stop(hs, gpu_ok):
    import torch
    W, H = 300, 70
    kw = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)
    still = np.full((H, W), 77, np.uint8)                         # nothing moves: its first sweep changes nothing, it stops there
    pairs = [synth.translating_pair(W, H, seed=2, dx=1.5, dy=-1.0), _patch_pair(W, H), (still, still.copy())]
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        ctx.set_pair_termination(True)
        for p, (A, B) in enumerate(pairs):
            ctx.set_frames(A, B, pair=p)
        ctx.solve(**kw)
        iters = [r["iterations_done"] for r in ctx.pair_results()]
        print("iterations per pair:", iters)
        assert len(set(iters)) == 3                               # three pairs, each stopping at a sweep of its own
        out = torch.full((3, H, W), FILL, dtype=torch.uint8, device="cuda")
        st = dev_stats(3)
        ctx.warp_batch_device(out, stats=st)
        ctx.synchronize()
        got = hs.warp_stats_from(st, 3)
        for p in range(3):
            u, v = ctx.flow(p)
            A, B = ctx.frames(p)
            want, ws = hs.warp_host(u, v, B, ref=A, return_stats=True)
            assert np.array_equal(out[p].cpu().numpy(), want), p
            assert stat_tuple(got[p]) == stat_tuple(ws), p


# ---- 3. the context's own frames: the physics -------------------------------------------------------------------------

def test_own_frames_and_direction(hs, gpu_ok):
    W, H = 96, 64
    prev, curr = synth.translating_pair(W, H, seed=1)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        ctx.set_frames(prev, curr)
        ctx.solve(lam=0.1, max_iter=100, term_type=ITER)
        u, v = ctx.flow()
        A, B = ctx.frames()
        fwd_pic, fwd = ctx.warp(return_stats=True)
        want, ws = hs.warp_host(u, v, B, ref=A, return_stats=True)
        assert np.array_equal(fwd_pic, want) and stat_tuple(fwd) == stat_tuple(ws)
        _, back = ctx.warp(t=-1.0, return_stats=True)
        assert stat_tuple(back) == stat_tuple(hs.warp_host(u, v, B, ref=A, t=-1.0, return_stats=True)[1])
        print("t=1: %d vs %d; t=-1: %d vs %d" % (fwd.sad_warped, fwd.sad_plain, back.sad_warped, back.sad_plain))
        assert fwd.sad_warped * 2 < fwd.sad_plain                 # the warped second frame approximates the FIRST
        assert back.sad_warped > back.sad_plain
        same = ctx.warp(t=0.0)
        assert np.array_equal(same, B)
        # the caller's reference with the context's own second frame
        other = np.random.default_rng(1).integers(0, 256, (H, W), dtype=np.uint8)
        _, s2 = ctx.warp(ref=other, return_stats=True)
        assert stat_tuple(s2) == stat_tuple(hs.warp_host(u, v, B, ref=other, return_stats=True)[1])


# ---- 4. ordering -----------------------------------------------------------------------------------------------------

def test_behind_an_asynchronous_solve(hs, gpu_ok):
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
    want, ws = hs.warp_host(u, v, fb, ref=fa, t=40.0, return_stats=True)   # (a flow of hundredths of a pixel, made visible)
    assert not np.array_equal(want, fb)
    for async_reduce in (0, 1):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with hs.HSFlow(W, H, stream=s.cuda_stream) as ctx:
            assert L.hsflow_set_async_reduce(ctx._h, async_reduce) == OK
            ctx.set_frames(A, B)
            out = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.solve_async(**kw)
            _, st = ctx.warp(out=out, t=40.0, return_stats=True)   # at once: the owed ITER|EPS check is settled first
            assert L.hsflow_wait_solve(ctx._h) == OK
            assert s.query(), "wait_solve returned while a warp was still in flight"
            assert np.array_equal(out.cpu().numpy(), want), async_reduce
            assert stat_tuple(hs.warp_stats_from(st)) == stat_tuple(ws)
            assert ctx.info()["iterations_done"] == info["iterations_done"]
            ctx.solve_async(**kw)
            got, gs = ctx.warp(t=40.0, return_stats=True)          # the synchronous form behind an asynchronous solve
            assert np.array_equal(got, want) and stat_tuple(gs) == stat_tuple(ws)
            u2, v2 = ctx.flow()
            assert np.array_equal(u2, u) and np.array_equal(v2, v)  # the flow is read and never changed


# ---- 5. pipeline -----------------------------------------------------------------------------------------------------

def test_pipeline(hs, gpu_ok):
    import torch
    W, H, depth = 64, 48, 3
    kw = dict(lam=0.1, max_iter=60, term_type=ITER)
    pairs = [synth.translating_pair(W, H, seed=s, dx=dx, dy=dy) for s, dx, dy in ((1, 0.75, -0.5), (2, -1.0, 1.0), (3, 0.25, 0.5), (4, 1.25, 0.0))]
    colour = np.random.default_rng(4).integers(0, 256, (H, W, 3), dtype=np.uint8)
    want = []
    for A, B in pairs:
        with hs.HSFlow(W, H, own_stream=True) as ctx:
            ctx.set_frames(A, B)
            ctx.solve(**kw)
            want.append((ctx.warp(return_stats=True), ctx.warp(colour, ref=colour, return_stats=True, border="replicate")))
    dev = [tuple(torch.from_numpy(f).cuda() for f in AB) for AB in pairs]
    dcolour = torch.from_numpy(colour).cuda()
    torch.cuda.synchronize()

    def check_ticket(pl, t):
        (own_pic, own_stats), (col_pic, col_stats) = want[t]
        pic, st = pl.warp(t, return_stats=True)
        assert np.array_equal(pic, own_pic) and stat_tuple(st) == stat_tuple(own_stats), t
        pic, st = pl.warp(t, colour, ref=colour, return_stats=True, border="replicate")
        assert np.array_equal(pic, col_pic) and stat_tuple(st) == stat_tuple(col_stats), t
        out = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        pic, st = pl.warp(t, dcolour, ref=dcolour, out=out, return_stats=True, border="replicate")   # complete on return
        assert pic is out and np.array_equal(out.cpu().numpy(), col_pic) and stat_tuple(hs.warp_stats_from(st)) == stat_tuple(col_stats), t

    with hs.PairPipeline(W, H, depth=depth, lanes=2) as pl:
        for t in range(len(pairs)):
            if t >= depth:
                check_ticket(pl, t - depth)                        # the oldest pair, before its slot is taken again
            assert pl.submit_device(dev[t][0], dev[t][1], **kw) == t
        for t in range(len(pairs) - depth, len(pairs)):
            check_ticket(pl, t)
        for call in (lambda: pl.warp(0), lambda: pl.warp(0, dcolour)):   # its slot has been reused since
            with pytest.raises(hs.HsflowError) as e:
                call()
            assert e.value.status == E_STATE
        check_ticket(pl, len(pairs) - 1)                           # the pipeline still works


# ---- 6. command line -------------------------------------------------------------------------------------------------

def _cli(args, extra_env=None, ok=True):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for name in ("HSFLOW_RENDER_DEVICE", "HSFLOW_JPEG_DEVICE", "HSFLOW_PICTURE", "HSFLOW_COLOR_MAX", "HSFLOW_WARP_T"):
        env.pop(name, None)
    env.update(extra_env or {})
    r = subprocess.run([cli] + args, env=env, capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_cli_warped_frame(hs, gpu_ok, tmp_path):
    W, H = 96, 64
    A, B = synth.translating_pair(W, H, seed=1)
    tint = np.array([1.0, 0.8, 0.6])
    frames = [np.clip(np.rint(g[..., None] * tint), 0, 255).astype(np.uint8) for g in (A, B)]   # a small colour pair
    names = [str(tmp_path / ("frame%d.ppm" % k)) for k in range(2)]
    for name, f in zip(names, frames):
        with open(name, "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (W, H) + f.tobytes())
    head = len(b"P6\n%d %d\n255\n" % (W, H))
    for args in (["-cv", "-hd", names[0], names[1], None, ".1", "100"], ["-cl", "-hd", names[0], names[1], None, "3", "50", "1", "GPU"]):
        for extra in ({}, {"HSFLOW_WARP_T": "-0.5"}):
            files, lines = {}, {}
            for route, env in (("host", {}), ("device", {"HSFLOW_RENDER_DEVICE": "1"})):
                out = str(tmp_path / ("%s_%s_%d.ppm" % (args[0][1:], route, len(extra))))
                r = _cli([out if a is None else a for a in args], dict(env, HSFLOW_PICTURE="warp", **extra))
                files[route] = open(out, "rb").read()
                lines[route] = [ln for ln in r.stdout.splitlines() if ln.startswith("warp:")]
                assert len(lines[route]) == 1
            assert files["host"] == files["device"] and lines["host"] == lines["device"]
            pic = np.frombuffer(files["host"][head:], np.uint8).reshape(H, W, 3)
            words = lines["host"][0].split()
            assert words[1::2] == ["inside", "outside", "unknown", "sad_warped", "sad_plain"]
            inside, outside, unknown, sad_warped, sad_plain = (int(x) for x in words[2::2])
            assert inside + outside + unknown == W * H and unknown == 0
            if args[0] == "-cv" and not extra:                     # the library's own solve of the same frames, by the host rule
                with hs.HSFlow(W, H, own_stream=True) as ctx:
                    ctx.set_frames_bgr(np.ascontiguousarray(frames[0][..., ::-1]), np.ascontiguousarray(frames[1][..., ::-1]), blur=True)
                    ctx.solve(lam=0.1, max_iter=100)
                    u, v = ctx.flow()
                want, ws = hs.warp_host(u, v, frames[1], ref=frames[0], return_stats=True)
                assert np.array_equal(pic, want)
                assert (inside, outside, unknown, sad_warped, sad_plain) == stat_tuple(ws)[:5]
                assert sad_warped * 2 < sad_plain
            if args[0] == "-cv" and extra:
                assert sad_warped > sad_plain                      # half the flow, the wrong way
    for bad in ({"HSFLOW_PICTURE": "warp", "HSFLOW_WARP_T": "1x"}, {"HSFLOW_WARP_T": "nan"}, {"HSFLOW_PICTURE": "warp", "HSFLOW_WARP_T": "2e6"},
                {"HSFLOW_PICTURE": "warped"}):
        r = _cli(["-cv", "-hd", names[0], names[1], str(tmp_path / "bad.ppm"), ".1", "10"], bad, ok=False)
        assert r.returncode == 1 and "HSFLOW_" in r.stdout


# ---- 7. errors -------------------------------------------------------------------------------------------------------

def test_argument_errors(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, N, C = 64, 4, 2, 3
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, *field(W, H, p), pair=p)
        src = torch.full((N, H, W, C), 50, dtype=torch.uint8, device="cuda")
        out = torch.full((N, H, W, C), FILL, dtype=torch.uint8, device="cuda")
        stats = dev_stats(N)
        lst = lambda t: (ctypes.c_void_p * N)(*[t[i].data_ptr() for i in range(N)])
        srcs, outs = lst(src), lst(out)
        holed = (ctypes.c_void_p * N)(outs[0], None)
        host_src, host_out = np.full((H, W * C), 50, np.uint8), np.full((H, W * C), FILL, np.uint8)
        hstats = hs.HsflowWarpStats()
        ctypes.memset(ctypes.byref(hstats), FILL, 64)
        torch.cuda.synchronize()
        rb = W * C
        sp = ctypes.c_void_p(stats.data_ptr())
        dev = lambda wp, pair=0, s=srcs[0], ss=rb, d=outs[0], ds=rb, h=ctx._h: L.hsflow_warp_device(h, pair, wp, s, ss, None, 0, d, ds, sp)
        bat = lambda wp, first=0, n=N, s=srcs, ss=rb, d=outs, ds=rb: L.hsflow_warp_batch_device(ctx._h, first, n, wp, s, ss, None, 0, d, ds, sp)
        syn = lambda wp, pair=0, s=host_src.ctypes.data, ss=rb, d=host_out.ctypes.data, ds=rb: L.hsflow_warp(ctx._h, pair, wp, s, ss, None, 0, d, ds,
                                                                                                             ctypes.byref(hstats))
        bad = []
        for change in (dict(struct_size=16), dict(channels=2), dict(channels=0), dict(border=2), dict(border=-1), dict(t=float("nan")),
                       dict(t=float("inf")), dict(t=1.5e6)):
            b = hs.make_warp_params(C)
            for k, val in change.items():
                setattr(b, k, val)
            bad.append(ctypes.byref(b))
        for b in bad + [None]:
            assert dev(b) == E_ARG and bat(b) == E_ARG and syn(b) == E_ARG
        r = ctypes.byref(hs.make_warp_params(C))
        r1 = ctypes.byref(hs.make_warp_params(1))
        assert dev(r, pair=N) == E_ARG and dev(r, pair=-1) == E_ARG and dev(r, h=None) == E_ARG and syn(r, pair=N) == E_ARG
        assert bat(r, n=0) == E_ARG and bat(r, first=1) == E_ARG and bat(r, first=-1, n=1) == E_ARG
        assert bat(r, s=holed) == E_ARG and bat(r, d=holed) == E_ARG
        assert dev(r, s=None) == E_ARG and bat(r, s=None) == E_ARG and syn(r, s=None) == E_ARG     # 3 channels of the context's own frames
        assert dev(r, d=srcs[0]) == E_ARG and bat(r, d=srcs) == E_ARG                                # onto the source
        assert syn(r, d=host_src.ctypes.data) == E_ARG
        assert L.hsflow_warp_device(ctx._h, 0, r, srcs[0], rb, outs[0], rb, outs[0], rb, None) == E_ARG   # onto the reference
        assert L.hsflow_warp_device(ctx._h, 0, r, srcs[0], rb, None, 0, None, 0, None) == E_ARG      # nothing asked for
        assert dev(r, ss=rb - 1) == E_SIZE and dev(r, ds=rb - 1) == E_SIZE and bat(r, ss=rb - 1) == E_SIZE and bat(r, ds=rb - 1) == E_SIZE
        assert syn(r, ss=rb - 1) == E_SIZE and syn(r, ds=rb - 1) == E_SIZE
        assert L.hsflow_warp_device(ctx._h, 0, r, srcs[0], rb, srcs[1], rb - 1, outs[0], rb, None) == E_SIZE
        assert dev(r1, s=None, ds=W - 1) == E_SIZE
        for odd in (1, 4):                                        # the records are 64-bit counters: 8-byte aligned or refused
            off = ctypes.c_void_p(stats.data_ptr() + odd)
            assert L.hsflow_warp_device(ctx._h, 0, r, srcs[0], rb, None, 0, outs[0], rb, off) == E_ARG
            assert L.hsflow_warp_batch_device(ctx._h, 0, N, r, srcs, rb, None, 0, outs, rb, off) == E_ARG
        ctx.synchronize()
        assert bool((out == FILL).all().item()) and bool((stats == FILL).all().item()) and (host_out == FILL).all()   # nothing was written
        assert bytes(hstats) == bytes([FILL]) * 64
        assert syn(r, pair=1) == OK
        assert np.array_equal(host_out.reshape(H, W, C), hs.warp_host(*field(W, H, 1), host_src.reshape(H, W, C)))
