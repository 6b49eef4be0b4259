"""The forward-backward consistency of two flows on the GPU (include/hsflow.h, ABI 0.18: hsflow_fb*, hsflow_set_frames_reversed,
hsflow_pipeline_fb*; kernel in opticalflowhs_amd/csrc/hs_kernels_fb.hip.h) against the rule on the host (hsflow_fb_host,
which tests/test_fb_host.py holds to a NumPy restatement).  Masks are compared byte for byte, err2 bit for bit, statistics
exactly."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from opticalflowhs_amd import synth
from test_fb_host import PARAM_SETS, fields, stat_tuple

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
OK, E_ARG, E_SIZE, E_STATE = 0, 1, 2, 5
FILL = 0xA5
ENV_MAX = "HSFLOW_JPEG_BATCH_MAX"
SHAPES = [(13, 7), (260, 37), (1027, 9), (96, 64)]


def put_flow(ctx, u, v, pair=0):
    import torch
    ud, vd = torch.from_numpy(np.ascontiguousarray(u, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    torch.cuda.synchronize()
    ctx.set_flow_rows_from(ud, vd, 0, u.shape[0], pair=pair)
    ctx.synchronize()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


class DevPlane(object):
    """H rows of `rowb` bytes in device memory, `stride` apart, the first `off` bytes behind a 256-byte multiple; FILL all
    around."""

    def __init__(self, H, rowb, off, stride):
        import torch
        self.buf = torch.full((256 + off + H * stride + 16,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.base = (-self.buf.data_ptr()) % 256 + off
        self.H, self.rowb, self.stride = H, rowb, stride
        self.ptr = ctypes.c_void_p(self.buf.data_ptr() + self.base)

    def rows_and_rest(self):
        """(the plane's rows as bytes, True if every byte around them is still FILL)."""
        host = self.buf.cpu().numpy()
        last = self.base + (self.H - 1) * self.stride + self.rowb
        body = host[self.base:self.base + self.H * self.stride].reshape(self.H, self.stride)
        clean = (body[:-1, self.rowb:] == FILL).all() and (host[last:] == FILL).all() and (host[:self.base] == FILL).all()
        rows = np.stack([host[self.base + y * self.stride:self.base + y * self.stride + self.rowb] for y in range(self.H)])
        return rows, bool(clean)


def dev_stats(n=1):
    import torch
    t = torch.full((64 * n + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def host_want(hs, fwd, bwd, **kw):
    """(mask, err2 bits, statistics tuple) of the host rule."""
    mask, err2, s = hs.fb_host(fwd[0], fwd[1], bwd[0], bwd[1], mask=True, err2=True, stats=True, **kw)
    return mask, err2.view(np.uint32), stat_tuple(s)


def two_fields(W, H, seed):
    uf, vf, ub, vb = fields(W, H, seed)
    return (uf, vf), (ub, vb)


# ---- 1. device against host ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SHAPES)
def test_device_equals_host(hs, gpu_ok, W, H):
    L = hs._lib.load()
    flows = two_fields(W, H, 7 * W + H)
    aligned = (W + 3) // 4 * 4
    mask_layouts = [(0, aligned), (1, W + 1), (2, W), (3, W + 5)]     # (offset from a 256-byte multiple, stride)
    err2_layouts = [(0, (4 * W + 15) // 16 * 16), (4, 4 * W + 4)]
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        for p in range(2):
            put_flow(ctx, *flows[p], pair=p)
        for kw in PARAM_SETS:
            fp = hs.make_fb_params(**kw)
            for fwd, bwd in ((0, 1), (1, 0)):
                mask, bits, st = host_want(hs, flows[fwd], flows[bwd], params=fp)
                if not kw:
                    assert all(n > 0 for n in st[:4]), st
                gm, ge, gs = ctx.fb(fwd, bwd, mask=True, err2=True, stats=True, params=fp)       # host memory, synchronous
                assert np.array_equal(gm, mask) and np.array_equal(ge.view(np.uint32), bits) and stat_tuple(gs) == st, (kw, fwd)
                for k, (off, stride) in enumerate(mask_layouts):
                    eoff, estride = err2_layouts[k % 2]
                    dm, de, ds = DevPlane(H, W, off, stride), DevPlane(H, 4 * W, eoff, estride), dev_stats()
                    assert L.hsflow_fb_device(ctx._h, fwd, bwd, ctypes.byref(fp), dm.ptr, stride, de.ptr, estride, ctypes.c_void_p(ds.data_ptr())) == OK
                    ctx.synchronize()
                    rows, clean = dm.rows_and_rest()
                    assert np.array_equal(rows, mask), (kw, fwd, off, stride, int((rows != mask).sum()))
                    assert clean, (off, stride)                                                # nothing beyond W bytes of a row
                    rows, clean = de.rows_and_rest()
                    assert np.array_equal(np.ascontiguousarray(rows).view(np.uint32), bits), (kw, fwd, eoff, estride)
                    assert clean, (eoff, estride)                                              # nothing beyond W floats of a row
                    assert stat_tuple(hs.fb_stats_from(ds)) == st
                    assert bool((ds[64:] == FILL).all().item()) and bytes(ds[44:64].cpu().numpy()) == b"\0" * 20
        for p in range(2):                                            # the flow is read and never changed
            u, v = ctx.flow(p)
            assert same_bits(u, flows[p][0]) and same_bits(v, flows[p][1])


# ---- 2. each output alone, and all three together ----------------------------------------------------------------------

def test_each_output_alone(hs, gpu_ok):
    W, H = 260, 37
    flows = two_fields(W, H, 5)
    mask, bits, st = host_want(hs, flows[0], flows[1])
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        for p in range(2):
            put_flow(ctx, *flows[p], pair=p)
        for device in (False, True):
            for want_mask, want_err2, want_stats in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
                gm, ge, gs = ctx.fb(0, 1, mask=bool(want_mask), err2=bool(want_err2), stats=bool(want_stats), device=device)
                ctx.synchronize()
                assert (gm is None) == (not want_mask) and (ge is None) == (not want_err2) and (gs is None) == (not want_stats)
                if want_mask:
                    assert np.array_equal(gm.cpu().numpy() if device else gm, mask), (device, want_mask, want_err2, want_stats)
                if want_err2:
                    assert np.array_equal((ge.cpu().numpy() if device else ge).view(np.uint32), bits), (device, want_mask, want_err2, want_stats)
                if want_stats:
                    assert stat_tuple(hs.fb_stats_from(gs) if device else gs) == st, (device, want_mask, want_err2, want_stats)


# ---- 3. batch and chunking ------------------------------------------------------------------------------------------------

class _batch_max(object):
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.saved = os.environ.get(ENV_MAX)
        os.environ.pop(ENV_MAX, None)
        if self.value is not None:
            os.environ[ENV_MAX] = self.value

    def __exit__(self, *a):
        os.environ.pop(ENV_MAX, None)
        if self.saved is not None:
            os.environ[ENV_MAX] = self.saved


def test_batch_and_chunking(hs, gpu_ok):
    import torch
    W, H, N = 96, 64, 5
    fwd, bwd = [0, 1, 2, 3, 4, 1], [1, 0, 4, 2, 3, 1]
    n = len(fwd)
    flows = []
    for p in range(N):
        a, b = two_fields(W, H, 60 + p)
        flows.append(a if p % 2 == 0 else b)
    fp = hs.make_fb_params(values=(200, 100, 50, 25))
    wants = [host_want(hs, flows[f], flows[b], params=fp) for f, b in zip(fwd, bwd)]
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, *flows[p], pair=p)
        for value in (None, "1", "4"):
            with _batch_max(value):
                masks = torch.full((n, H, W), FILL, dtype=torch.uint8, device="cuda")
                err2 = torch.full((n, H, W), -7.0, dtype=torch.float32, device="cuda")
                st = dev_stats(n)
                ctx.fb_batch_device(fwd, bwd, mask=masks, err2=err2, stats=st, params=fp)
                ctx.synchronize()
                got = hs.fb_stats_from(st, n)
                for i in range(n):
                    assert np.array_equal(masks[i].cpu().numpy(), wants[i][0]), (value, i)
                    assert np.array_equal(err2[i].cpu().numpy().view(np.uint32), wants[i][1]), (value, i)
                    assert stat_tuple(got[i]) == wants[i][2], (value, i)
                assert bool((st[64 * n:] == FILL).all().item())         # records 64 bytes apart, nothing behind the last
                st = dev_stats(n)
                ctx.fb_batch_device(fwd, bwd, stats=st, params=fp)      # statistics only
                ctx.synchronize()
                assert [stat_tuple(g) for g in hs.fb_stats_from(st, n)] == [w[2] for w in wants], value
        with _batch_max("0"):
            with pytest.raises(hs.HsflowError) as e:
                ctx.fb_batch_device(fwd, bwd, stats=dev_stats(n), params=fp)
            assert e.value.status == E_ARG and ENV_MAX in str(e.value)


# ---- 4. backward planes from the caller -----------------------------------------------------------------------------------

def test_planes_device(hs, gpu_ok):
    import torch
    W, H = 260, 37
    flows = two_fields(W, H, 11)
    mask, bits, st = host_want(hs, flows[0], flows[1])
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, *flows[0])
        wide = torch.full((2, H, W + 3), float("nan"), dtype=torch.float32, device="cuda")   # stride 4 * W + 12
        wide[0, :, :W] = torch.from_numpy(flows[1][0]).cuda()
        wide[1, :, :W] = torch.from_numpy(flows[1][1]).cuda()
        torch.cuda.synchronize()
        ub, vb = wide[0, :, :W], wide[1, :, :W]
        assert ub.stride(0) * 4 == 4 * W + 12
        gm, ge, gs = ctx.fb_planes(ub, vb, mask=True, err2=True, stats=True, device=True)
        ctx.synchronize()
        assert np.array_equal(gm.cpu().numpy(), mask) and np.array_equal(ge.cpu().numpy().view(np.uint32), bits)
        assert stat_tuple(hs.fb_stats_from(gs)) == st
        gm, ge, gs = ctx.fb_planes(ub, vb, mask=True, err2=True, stats=True)                 # results to host memory
        assert np.array_equal(gm, mask) and np.array_equal(ge.view(np.uint32), bits) and stat_tuple(gs) == st


# ---- 5. after real solves ---------------------------------------------------------------------------------------------------

def test_after_real_solves(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H = 96, 64
    A, B = synth.translating_pair(W, H, seed=1)
    bgr = [np.ascontiguousarray(np.repeat(g[..., None], 3, axis=2)) for g in (A, B)]
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        with pytest.raises(hs.HsflowError) as e:
            ctx.set_frames_reversed(1, 0)                              # before frames are set
        assert e.value.status == E_STATE
        ctx.set_frames_bgr(bgr[0], bgr[1], blur=True, pair=0)
        for dst, src in ((0, 0), (1, 1), (2, 0), (1, -1)):
            with pytest.raises(hs.HsflowError) as e:
                ctx.set_frames_reversed(dst, src)
            assert e.value.status == E_ARG
        ctx.set_frames_reversed(1, 0)
        p0, c0 = ctx.frames(0)
        p1, c1 = ctx.frames(1)
        assert np.array_equal(p1, c0) and np.array_equal(c1, p0) and not np.array_equal(p0, c0)

        def check(solved_flows=None):
            fl = [ctx.flow(p) for p in range(2)]
            for fwd, bwd in ((0, 1), (1, 0)):
                mask, bits, st = host_want(hs, fl[fwd], fl[bwd])
                gm, ge, gs = ctx.fb(fwd, bwd, mask=True, err2=True, stats=True)
                assert np.array_equal(gm, mask) and np.array_equal(ge.view(np.uint32), bits) and stat_tuple(gs) == st
                share = st[0] / float(st[0] + st[1])
                print("direction (%d, %d): evaluated %d consistent %d share %.3f" % (fwd, bwd, st[0] + st[1], st[0], share))
                assert share >= 0.85
            return fl

        ctx.solve(lam=0.1, max_iter=100, term_type=ITER)
        first = check()
        ctx.solve(lam=0.1, max_iter=100, term_type=ITER)               # the graph is cached by now: bit-identical flow
        again = [ctx.flow(p) for p in range(2)]
        assert all(same_bits(a, b) for p in range(2) for a, b in zip(first[p], again[p]))

    # ITER|EPS with every pair's own stop: epsilon 1e-2 stops the two directions at sweeps of their own (the CPU oracle: 54
    # and 44); the owed check is settled by the call
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    kw = dict(lam=0.1, max_iter=100, term_type=ITER | EPS, epsilon=1e-2)
    with hs.HSFlow(W, H, 2, stream=s.cuda_stream) as ctx:
        ctx.set_pair_termination(True)
        ctx.set_frames(A, B, pair=0)
        ctx.set_frames_reversed(1, 0)
        ctx.solve(**kw)
        iters = [r["iterations_done"] for r in ctx.pair_results()]
        want_flows = [ctx.flow(p) for p in range(2)]
        wants = {d: host_want(hs, want_flows[d[0]], want_flows[d[1]]) for d in ((0, 1), (1, 0))}
        print("iterations per pair:", iters)
        assert iters[0] != iters[1] and max(iters) < 100
        ctx.solve_async(**kw)
        dm = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
        gm, ge, gs = ctx.fb(0, 1, mask=dm, err2=True, stats=True)      # at once: the owed ITER|EPS check is settled first
        assert L.hsflow_wait_solve(ctx._h) == OK
        ctx.synchronize()
        assert np.array_equal(dm.cpu().numpy(), wants[(0, 1)][0]) and np.array_equal(ge.cpu().numpy().view(np.uint32), wants[(0, 1)][1])
        assert stat_tuple(hs.fb_stats_from(gs)) == wants[(0, 1)][2]
        assert [r["iterations_done"] for r in ctx.pair_results()] == iters
        ctx.solve_async(**kw)
        gm, ge, gs = ctx.fb(1, 0, mask=True, err2=True, stats=True)    # the synchronous form behind an asynchronous solve
        assert np.array_equal(gm, wants[(1, 0)][0]) and np.array_equal(ge.view(np.uint32), wants[(1, 0)][1]) and stat_tuple(gs) == wants[(1, 0)][2]
        assert wants[(0, 1)][2][0] >= 0.85 * (wants[(0, 1)][2][0] + wants[(0, 1)][2][1])


def test_synchronous_form_behind_an_early_stop_without_pair_termination(hs, gpu_ok):
    """Two pairs, no hsflow_set_pair_termination, hsflow_solve_async under ITER|EPS with epsilons that fire early: the owed
    check re-runs the solve, which may end in the other buffer of the flow's two; hsflow_fb settles first and only then
    names the planes of BOTH pairs.  Several epsilons, so that the re-run ends after odd and even numbers of launches."""
    import torch
    L = hs._lib.load()
    W, H = 96, 64
    A, B = synth.translating_pair(W, H, seed=1)
    for async_reduce in (0, 1):
        for eps in (3e-2, 1e-2, 5e-3):
            kw = dict(lam=0.1, max_iter=100, term_type=ITER | EPS, epsilon=eps)
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            with hs.HSFlow(W, H, 2, stream=s.cuda_stream) as ctx:
                assert L.hsflow_set_async_reduce(ctx._h, async_reduce) == OK
                ctx.set_frames(A, B, pair=0)
                ctx.set_frames_reversed(1, 0)
                info = ctx.solve(**kw)
                assert 1 < info["iterations_done"] < 100, info         # its early stop fires
                want_flows = [ctx.flow(p) for p in range(2)]
                wants = {d: host_want(hs, want_flows[d[0]], want_flows[d[1]]) for d in ((0, 1), (1, 0))}
                for d in ((0, 1), (1, 0)):
                    ctx.solve_async(**kw)
                    gm, ge, gs = ctx.fb(d[0], d[1], mask=True, err2=True, stats=True)   # at once: the owed check is settled first
                    assert np.array_equal(gm, wants[d][0]) and np.array_equal(ge.view(np.uint32), wants[d][1]), (async_reduce, eps, d)
                    assert stat_tuple(gs) == wants[d][2], (async_reduce, eps, d)
                    assert ctx.info()["iterations_done"] == info["iterations_done"]
                    after = [ctx.flow(p) for p in range(2)]
                    assert all(same_bits(a, b) for p in range(2) for a, b in zip(after[p], want_flows[p]))
                    ctx.solve_async(**kw)
                    dm = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    ctx.fb(d[0], d[1], mask=dm, err2=False, stats=False)    # the device form behind the same
                    ctx.synchronize()
                    assert np.array_equal(dm.cpu().numpy(), wants[d][0]), (async_reduce, eps, d)


def test_pairs_stop_at_sweeps_of_their_own(hs, gpu_ok):
    """hsflow_set_pair_termination: an epsilon that stops the two pairs at different sweeps; both directions read every
    pair's own final flow."""
    W, H = 300, 70
    kw = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)
    a = np.full((H, W), 90, np.uint8)
    b = a.copy()
    a[17:52, 60:210], b[17:52, 60:210] = 120, 121                     # (its early stop fires after a few sweeps)
    still = np.full((H, W), 77, np.uint8)
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        ctx.set_pair_termination(True)
        ctx.set_frames(a, b, pair=0)
        ctx.set_frames_reversed(1, 0)
        ctx.set_frames(still, still.copy(), pair=2)
        ctx.solve_async(**kw)
        gm, ge, gs = ctx.fb(0, 1, mask=True, err2=True, stats=True)    # the owed check is settled by the call
        iters = [r["iterations_done"] for r in ctx.pair_results()]
        print("iterations per pair:", iters)
        assert iters[2] < iters[0] < 400 and iters[2] < iters[1] < 400
        fl = [ctx.flow(p) for p in range(3)]
        for fwd, bwd in ((0, 1), (1, 0), (0, 2), (2, 1)):
            mask, bits, st = host_want(hs, fl[fwd], fl[bwd])
            if (fwd, bwd) == (0, 1):
                assert np.array_equal(gm, mask) and np.array_equal(ge.view(np.uint32), bits) and stat_tuple(gs) == st
            m2, e2, s2 = ctx.fb(fwd, bwd, mask=True, err2=True, stats=True)
            assert np.array_equal(m2, mask) and np.array_equal(e2.view(np.uint32), bits) and stat_tuple(s2) == st, (fwd, bwd)


# ---- 6. pipeline ------------------------------------------------------------------------------------------------------------

def test_pipeline(hs, gpu_ok):
    import torch
    W, H = 96, 64
    kw = dict(lam=0.1, max_iter=60, term_type=ITER)
    A, B = synth.translating_pair(W, H, seed=1)
    flows = []
    for prev, curr in ((A, B), (B, A)):
        with hs.HSFlow(W, H, own_stream=True) as ctx:
            ctx.set_frames(prev, curr)
            ctx.solve(**kw)
            flows.append(ctx.flow())
    wants = {d: host_want(hs, flows[d[0]], flows[d[1]]) for d in ((0, 1), (1, 0))}
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    torch.cuda.synchronize()
    with hs.PairPipeline(W, H, depth=2, lanes=2) as pl:
        tf = pl.submit_device(dA, dB, **kw)
        tb = pl.submit_device(dB, dA, **kw)
        for (f, b), d in (((tf, tb), (0, 1)), ((tb, tf), (1, 0))):
            gm, ge, gs = pl.fb(f, b, mask=True, err2=True, stats=True)                       # host outputs
            assert np.array_equal(gm, wants[d][0]) and np.array_equal(ge.view(np.uint32), wants[d][1]) and stat_tuple(gs) == wants[d][2], d
            dm = torch.full((H, W), 7, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            gm, ge, gs = pl.fb(f, b, mask=dm, err2=True, stats=True)                         # device outputs, complete on return
            assert gm is dm and np.array_equal(dm.cpu().numpy(), wants[d][0]) and np.array_equal(ge.cpu().numpy().view(np.uint32), wants[d][1])
            assert stat_tuple(hs.fb_stats_from(gs)) == wants[d][2], d
        t2 = pl.submit_device(dA, dB, **kw)
        t3 = pl.submit_device(dB, dA, **kw)
        for call in (lambda: pl.fb(tf, tb), lambda: pl.fb(tf, t3), lambda: pl.fb(t2, tb, device=True)):   # a slot has been reused since
            with pytest.raises(hs.HsflowError) as e:
                call()
            assert e.value.status == E_STATE
        gm, _, gs = pl.fb(t2, t3, stats=True)                          # the pipeline still works
        assert np.array_equal(gm, wants[(0, 1)][0]) and stat_tuple(gs) == wants[(0, 1)][2]


# ---- 7. command line ----------------------------------------------------------------------------------------------------------

def _cli(args, extra_env=None, ok=True):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for name in ("HSFLOW_RENDER_DEVICE", "HSFLOW_JPEG_DEVICE", "HSFLOW_PICTURE", "HSFLOW_COLOR_MAX", "HSFLOW_WARP_T", "HSFLOW_FB_ALPHA", "HSFLOW_FB_BETA"):
        env.pop(name, None)
    env.update(extra_env or {})
    r = subprocess.run([cli] + args, env=env, capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_cli_mask(hs, gpu_ok, tmp_path):
    W, H = 96, 64
    A, B = synth.translating_pair(W, H, seed=1)
    tint = np.array([1.0, 0.8, 0.6])
    frames = [np.clip(np.rint(g[..., None] * tint), 0, 255).astype(np.uint8) for g in (A, B)]   # a small colour pair
    names = [str(tmp_path / ("frame%d.ppm" % k)) for k in range(2)]
    for name, f in zip(names, frames):
        with open(name, "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (W, H) + f.tobytes())
    head = len(b"P5\n%d %d\n255\n" % (W, H))
    for args in (["-cv", "-hd", names[0], names[1], None, ".1", "100"], ["-cl", "-hd", names[0], names[1], None, "3", "50", "1", "GPU"]):
        for extra in ({}, {"HSFLOW_FB_ALPHA": "0.05", "HSFLOW_FB_BETA": "0.125"}):
            files, lines = {}, {}
            for route, env in (("host", {}), ("device", {"HSFLOW_RENDER_DEVICE": "1"})):
                out = str(tmp_path / ("%s_%s_%d.pgm" % (args[0][1:], route, len(extra))))
                r = _cli([out if a is None else a for a in args], dict(env, HSFLOW_PICTURE="fb", **extra))
                files[route] = open(out, "rb").read()
                lines[route] = [ln for ln in r.stdout.splitlines() if ln.startswith("fb:")]
                assert len(lines[route]) == 1
            assert files["host"] == files["device"] and lines["host"] == lines["device"]
            assert files["host"].startswith(b"P5\n%d %d\n255\n" % (W, H))
            pic = np.frombuffer(files["host"][head:], np.uint8).reshape(H, W)
            words = lines["host"][0].split()
            assert words[1::2] == ["consistent", "inconsistent", "outside", "unknown", "mse"]
            counts = [int(x) for x in words[2:9:2]]
            assert sum(counts) == W * H and int((pic == 255).sum()) == counts[0] and int((pic == 0).sum()) == W * H - counts[0]
            if args[0] == "-cv":                                       # the library's own two-pair solve, by the host rule
                with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
                    ctx.set_frames_bgr(np.ascontiguousarray(frames[0][..., ::-1]), np.ascontiguousarray(frames[1][..., ::-1]), blur=True)
                    ctx.set_frames_reversed(1, 0)
                    ctx.solve(lam=0.1, max_iter=100)
                    (uf, vf), (ub, vb) = ctx.flow(0), ctx.flow(1)
                kw = dict(alpha=0.05, beta=0.125) if extra else {}
                mask, _, s = hs.fb_host(uf, vf, ub, vb, stats=True, **kw)
                assert np.array_equal(pic, mask)
                assert counts == list(stat_tuple(s)[:4])
                assert words[10] == "%.6f" % (s.sum_err2_q / (256.0 * (s.consistent + s.inconsistent)))
                assert counts[0] > 0 and counts[1] > 0
    for bad in ({"HSFLOW_PICTURE": "fb", "HSFLOW_FB_ALPHA": "-1"}, {"HSFLOW_PICTURE": "fb", "HSFLOW_FB_BETA": "1x"}, {"HSFLOW_PICTURE": "fbb"}):
        r = _cli(["-cv", "-hd", names[0], names[1], str(tmp_path / "bad.pgm"), ".1", "10"], bad, ok=False)
        assert r.returncode == 1 and "HSFLOW_" in r.stdout
    for route in (["-cv", "-cam"], ["-cl", "-cam", "x", "3", "5", "1", "GPU"]):
        r = _cli(route, {"HSFLOW_PICTURE": "fb"}, ok=False)
        assert r.returncode == 1 and "HSFLOW_PICTURE=fb" in r.stdout


# ---- 8. errors ----------------------------------------------------------------------------------------------------------------

def test_argument_errors(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, N = 64, 4, 2
    flows = two_fields(W, H, 3)
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, *flows[p], pair=p)
        masks = torch.full((N, H, W), FILL, dtype=torch.uint8, device="cuda")
        err2 = torch.full((N, H, W + 1), -7.0, dtype=torch.float32, device="cuda")
        planes = torch.zeros((2, H, W), dtype=torch.float32, device="cuda")
        stats = dev_stats(N)
        lst = lambda ptrs: (ctypes.c_void_p * N)(*ptrs)
        ml, el = lst([masks[i].data_ptr() for i in range(N)]), lst([err2[i].data_ptr() for i in range(N)])
        holed = (ctypes.c_void_p * N)(ml[0], None)
        ints = lambda *v: (ctypes.c_int * len(v))(*v)
        host_mask, host_err2 = np.full((H, W), FILL, np.uint8), np.full((H, W), -7.0, np.float32)
        hstats = hs.HsflowFbStats()
        ctypes.memset(ctypes.byref(hstats), FILL, 64)
        torch.cuda.synchronize()
        sp = ctypes.c_void_p(stats.data_ptr())
        es = (W + 1) * 4
        ub, vb = ctypes.c_void_p(planes[0].data_ptr()), ctypes.c_void_p(planes[1].data_ptr())
        dev = lambda fp, f=0, b=1, m=ml[0], ms=W, e=el[0], es_=es, s=sp, h=ctx._h: L.hsflow_fb_device(h, f, b, fp, m, ms, e, es_, s)
        bat = lambda fp, n=N, f=ints(0, 1), b=ints(1, 0), m=ml, ms=W, e=el, es_=es, s=sp: L.hsflow_fb_batch_device(ctx._h, n, f, b, fp, m, ms, e, es_, s)
        pln = lambda fp, f=0, u=ub, v=vb, bs=W * 4, m=ml[0], ms=W, e=el[0], es_=es, s=sp: L.hsflow_fb_planes_device(ctx._h, f, u, v, bs, fp, m, ms, e, es_, s)
        syn = lambda fp, f=0, b=1, m=host_mask.ctypes.data, ms=W, e=host_err2.ctypes.data, es_=W * 4: L.hsflow_fb(ctx._h, f, b, fp, m, ms, e, es_,
                                                                                                                 ctypes.byref(hstats))
        bad = []
        for change in (dict(struct_size=12), dict(alpha=float("nan")), dict(alpha=-1.0), dict(alpha=2e6), dict(beta=float("inf")), dict(beta=-0.5),
                       dict(beta=2e30)):
            b = hs.make_fb_params()
            for k, val in change.items():
                setattr(b, k, val)
            bad.append(ctypes.byref(b))
        for b in bad + [None]:
            assert dev(b) == E_ARG and bat(b) == E_ARG and pln(b) == E_ARG and syn(b) == E_ARG
        r = ctypes.byref(hs.make_fb_params())
        assert dev(r, f=N) == E_ARG and dev(r, f=-1) == E_ARG and dev(r, b=N) == E_ARG and dev(r, b=-1) == E_ARG and dev(r, h=None) == E_ARG
        assert syn(r, f=N) == E_ARG and syn(r, b=-1) == E_ARG and pln(r, f=N) == E_ARG
        assert bat(r, n=0) == E_ARG and bat(r, n=-1) == E_ARG and bat(r, f=None) == E_ARG and bat(r, b=None) == E_ARG
        assert bat(r, f=ints(0, N)) == E_ARG and bat(r, b=ints(-1, 0)) == E_ARG
        assert bat(r, m=holed) == E_ARG and bat(r, e=holed) == E_ARG
        assert pln(r, u=None) == E_ARG and pln(r, v=None) == E_ARG and pln(r, u=ctypes.c_void_p(planes[0].data_ptr() + 2)) == E_ARG
        assert pln(r, bs=W * 4 - 4) == E_SIZE and pln(r, bs=W * 4 + 2) == E_SIZE
        assert dev(r, m=None, e=None, s=None) == E_ARG and bat(r, m=None, e=None, s=None) == E_ARG and pln(r, m=None, e=None, s=None) == E_ARG   # nothing asked for
        assert L.hsflow_fb(ctx._h, 0, 1, r, None, 0, None, 0, None) == E_ARG
        for odd in (1, 4):                                            # the records are 64-bit counters: 8-byte aligned or refused
            off = ctypes.c_void_p(stats.data_ptr() + odd)
            assert dev(r, s=off) == E_ARG and bat(r, s=off) == E_ARG and pln(r, s=off) == E_ARG
        for odd in (1, 2):                                            # err2 is written as floats
            off = ctypes.c_void_p(err2.data_ptr() + odd)
            assert dev(r, e=off) == E_ARG and pln(r, e=off) == E_ARG and bat(r, e=lst([el[0], off.value])) == E_ARG
        assert dev(r, ms=W - 1) == E_SIZE and bat(r, ms=W - 1) == E_SIZE and pln(r, ms=W - 1) == E_SIZE and syn(r, ms=W - 1) == E_SIZE
        for short in (W * 4 - 4, W * 4 + 2):
            assert dev(r, es_=short) == E_SIZE and bat(r, es_=short) == E_SIZE and pln(r, es_=short) == E_SIZE and syn(r, es_=short) == E_SIZE
        with _batch_max("33"):
            assert bat(r) == E_ARG and dev(r) == E_ARG and ENV_MAX in ctx._lib.hsflow_last_error(ctx._h).decode()
        ctx.synchronize()
        assert bool((masks == FILL).all().item()) and bool((err2 == -7.0).all().item()) and bool((stats == FILL).all().item())   # nothing was written
        assert (host_mask == FILL).all() and (host_err2 == -7.0).all() and bytes(hstats) == bytes([FILL]) * 64
        assert syn(r, f=1, b=0) == OK                                 # the context still works
        mask, bits, st = host_want(hs, flows[1], flows[0])
        assert np.array_equal(host_mask, mask) and np.array_equal(host_err2.view(np.uint32), bits) and stat_tuple(hstats) == st
        assert bat(r) == OK
        ctx.synchronize()
        assert np.array_equal(masks[1].cpu().numpy(), mask) and np.array_equal(err2[1, :, :W].cpu().numpy().view(np.uint32), bits)
