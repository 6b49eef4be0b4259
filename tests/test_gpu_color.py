"""The dense colour picture drawn on the GPU (include/hsflow.h, ABI 0.16: hsflow_color_flow*, hsflow_pipeline_color*;
kernels in opticalflowhs_amd/csrc/hs_kernels_color.hip.h) against the rule on the host (hsflow_color_flow_host, which
tests/test_color_host.py holds to a float64 statement).  Pictures and files are compared byte for byte."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))
OK, E_ARG, E_SIZE, E_STATE = 0, 1, 2, 5
FILL = 0xA5
ENV_MAX = "HSFLOW_JPEG_BATCH_MAX"
BIG = np.float32(1e9) * (np.float32(1) + np.float32(2.0 ** -23))
SPECIAL = [(np.nan, 1.0), (1.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (BIG, 0.0), (0.0, -BIG), (1e9, 0.0), (0.0, 0.0), (-0.0, 0.0), (1e-42, -1e-42),
           (2.0, -0.0), (2.0, 0.0), (-2.0, 0.0), (0.0, 2.0), (0.0, -2.0), (1.5, 1.5), (1e-20, 3e-20)]


def field(W, H, seed, last_max=False, scale=3.0):
    """A random flow with the CPU test's special values scattered over it (as many as fit); last_max: the largest radius
    sits in the last column of the last row (and 1e9 is left out, so that it is)."""
    rng = np.random.default_rng(seed)
    u, v = (rng.standard_normal((H, W)) * scale).astype(np.float32), (rng.standard_normal((H, W)) * scale).astype(np.float32)
    vals = [s for s in SPECIAL if not (last_max and s[0] == 1e9)]
    spots = rng.permutation(W * H)[:len(vals)]
    for k, (a, b) in zip(spots, vals):
        u.flat[k], v.flat[k] = a, b
    if last_max:
        u[H - 1, W - 1], v[H - 1, W - 1] = 60.0, -80.0
    return u, v


def put_flow(ctx, u, v, pair=0):
    import torch
    ud, vd = torch.from_numpy(np.ascontiguousarray(u, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    torch.cuda.synchronize()
    ctx.set_flow_rows_from(ud, vd, 0, u.shape[0], pair=pair)
    ctx.synchronize()


def view_pointers(hs, ctx, pair=0):
    pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    assert hs._lib.load().hsflow_flow_view_device(ctx._h, pair, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == OK
    return pu.value, pv.value, sb.value


def fixed_scale(hs, u, v):
    """A third of the AUTO scale: a good share of the pixels takes the 0.75 branch."""
    return float(np.float32(hs.color_flow_host(u, v, return_scale=True)[1] / 3))


# ---- 1. device against host ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(1, 1), (3, 2), (5, 7), (64, 4), (257, 9), (300, 70)])
def test_device_equals_host(hs, gpu_ok, W, H):
    import torch
    L = hs._lib.load()
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        for last_max in (False, True):
            u, v = field(W, H, 11 * W + H, last_max=last_max)
            put_flow(ctx, u, v)
            for mf in (None, fixed_scale(hs, u, v)):
                want, m = hs.color_flow_host(u, v, max_flow=mf, return_scale=True)
                if last_max and mf is None:
                    assert m == 100.0
                got, m_dev = ctx.color(max_flow=mf, return_scale=True)
                assert np.array_equal(got, want), (W, H, last_max, mf, int((got != want).any(axis=2).sum()))
                assert m_dev == m
                cp = hs.make_color_params(mf)
                for off in range(4):
                    for stride in (3 * W, 3 * W + 1, 3 * W + 5):
                        buf = torch.full((256 + off + H * stride + 16,), FILL, dtype=torch.uint8, device="cuda")
                        base = (-buf.data_ptr()) % 256 + off
                        torch.cuda.synchronize()
                        assert L.hsflow_color_flow_device(ctx._h, 0, ctypes.byref(cp), ctypes.c_void_p(buf.data_ptr() + base), stride) == OK
                        ctx.synchronize()
                        host = buf.cpu().numpy()
                        rows = host[base:base + H * stride].reshape(H, stride)
                        assert np.array_equal(rows[:, :3 * W].reshape(H, W, 3), want), (off, stride, mf)
                        last = base + (H - 1) * stride + 3 * W        # behind the last pixel: padding and everything after
                        assert (rows[:-1, 3 * W:] == FILL).all() and (host[last:] == FILL).all() and (host[:base] == FILL).all(), (off, stride)


# ---- 2. batch --------------------------------------------------------------------------------------------------------

def _patch_pair(W, H):
    """tests/test_gpu_render.py::_patch_pair: a flat frame with a patch one grey level brighter; with lambda 1e-3 / epsilon
    1e-4 its early stop fires."""
    a = np.full((H, W), 90, np.uint8)
    b = a.copy()
    rows, cols = slice(H // 4, H // 4 + min(80, H // 2)), slice(W // 5, W // 5 + min(300, W // 2))
    a[rows, cols], b[rows, cols] = 120, 121
    return a, b


def test_batch_in_three_chunks(hs, gpu_ok):
    import torch
    W, H, N = 300, 70, 5
    flows = [field(W, H, 40 + p, last_max=(p == 3), scale=1.0 + 2.0 * p) for p in range(N)]
    flows[2] = (np.full((H, W), np.nan, np.float32), np.full((H, W), np.nan, np.float32))
    saved = os.environ.get(ENV_MAX)
    os.environ[ENV_MAX] = "2"
    try:
        with hs.HSFlow(W, H, N, own_stream=True) as ctx:
            for p, (u, v) in enumerate(flows):
                put_flow(ctx, u, v, pair=p)
            for mf in (None, 4.0):
                wants = [hs.color_flow_host(u, v, max_flow=mf) for u, v in flows]
                assert not wants[2].any() and all(w.any() for i, w in enumerate(wants) if i != 2)
                singles = [ctx.color(max_flow=mf, pair=p) for p in range(N)]
                for p in range(N):
                    assert np.array_equal(singles[p], wants[p]), (p, mf)
                out = torch.full((N, H, W, 3), FILL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.color_batch_device(out, max_flow=mf)
                ctx.synchronize()
                assert np.array_equal(out.cpu().numpy(), np.stack(wants)), mf
                part = torch.full((3, H, W, 3), FILL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.color_batch_device(part, max_flow=mf, first_pair=1, n=3)
                ctx.synchronize()
                assert np.array_equal(part.cpu().numpy(), np.stack(wants[1:4])), mf
                files = ctx.color_jpeg_batch(max_flow=mf)
                assert files == [hs.encode_jpeg(w, 95) for w in wants]
                assert [ctx.color_jpeg(max_flow=mf, pair=p) for p in (0, 4)] == [files[0], files[4]]
            os.environ[ENV_MAX] = "0"
            with pytest.raises(hs.HsflowError) as e:
                ctx.color_batch_device(out)
            assert e.value.status == E_ARG and ENV_MAX in str(e.value)
    finally:
        os.environ.pop(ENV_MAX, None)
        if saved is not None:
            os.environ[ENV_MAX] = saved


def test_per_pair_stop(hs, gpu_ok):
    W, H = 300, 70
    kw = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)
    pairs = [synth.translating_pair(W, H, seed=2, dx=1.5, dy=-1.0), _patch_pair(W, H), synth.translating_pair(W, H, seed=5, dx=-2.0, dy=0.5)]
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        ctx.set_pair_termination(True)
        for p, (A, B) in enumerate(pairs):
            ctx.set_frames(A, B, pair=p)
        ctx.solve(**kw)
        iters = [r["iterations_done"] for r in ctx.pair_results()]
        print("iterations per pair:", iters)
        assert len(set(iters)) > 1                                # pairs stopping at different sweeps
        files = ctx.color_jpeg_batch()
        for p in range(3):
            u, v = ctx.flow(p)
            want = hs.color_flow_host(u, v)
            assert want.min() < 255
            assert np.array_equal(ctx.color(pair=p), want), p
            assert files[p] == hs.encode_jpeg(want, 95), p


# ---- 3. ordering -----------------------------------------------------------------------------------------------------

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
    want, m = hs.color_flow_host(u, v, return_scale=True)
    assert want.min() < 255
    for async_reduce in (0, 1):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with hs.HSFlow(W, H, stream=s.cuda_stream) as ctx:
            assert L.hsflow_set_async_reduce(ctx._h, async_reduce) == OK
            ctx.set_frames(A, B)
            ctx.solve_async(**kw)
            got, m_dev = ctx.color(return_scale=True)             # the owed ITER|EPS check is settled first
            assert np.array_equal(got, want) and m_dev == m
            assert ctx.info()["iterations_done"] == info["iterations_done"]
            # the device form right behind the solve: only enqueued, and wait_solve returns only when the picture is through
            out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.solve_async(**kw)
            for _ in range(4):
                ctx.color(out=out, max_flow=m)
            assert L.hsflow_wait_solve(ctx._h) == OK
            assert s.query(), "wait_solve returned while a colour picture was still in flight"
            assert np.array_equal(out.cpu().numpy(), want)
            # the flow's pointers and planes are what they were, and so must flow_view wait
            before = view_pointers(hs, ctx)
            out.zero_()
            torch.cuda.synchronize()
            for _ in range(4):
                ctx.color(out=out)
            assert view_pointers(hs, ctx) == before
            assert s.query(), "flow_view returned while a colour picture was still in flight"
            assert np.array_equal(out.cpu().numpy(), want)
            u2, v2 = ctx.flow()
            assert np.array_equal(u2, u) and np.array_equal(v2, v)


# ---- 4. files --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(33, 17), (300, 70)])
def test_files(hs, gpu_ok, W, H):
    L = hs._lib.load()
    flows = [field(W, H, 90 + p, last_max=bool(p)) for p in range(2)]
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        for p, (u, v) in enumerate(flows):
            put_flow(ctx, u, v, pair=p)
        for mf in (None, 2.5):
            for quality in (95, 30):
                wants = [hs.encode_jpeg(hs.color_flow_host(u, v, max_flow=mf), quality) for u, v in flows]
                assert [ctx.color_jpeg(max_flow=mf, quality=quality, pair=p) for p in range(2)] == wants
                assert ctx.color_jpeg_batch(max_flow=mf, quality=quality) == wants
        # a capacity that is too small: HSFLOW_E_SIZE, the size needed, the buffer left alone
        want = hs.encode_jpeg(hs.color_flow_host(*flows[1]), 95)
        cp = hs.make_color_params()
        cap = len(want) - 1
        buf = np.full(cap + 16, FILL, np.uint8)
        n = ctypes.c_size_t(7)
        assert L.hsflow_color_flow_jpeg(ctx._h, 1, ctypes.byref(cp), 95, buf.ctypes.data, cap, ctypes.byref(n)) == E_SIZE
        assert n.value == len(want) and (buf == FILL).all()
        n = ctypes.c_size_t(7)
        assert L.hsflow_color_flow_jpeg(ctx._h, 1, ctypes.byref(cp), 95, buf.ctypes.data, cap + 1, ctypes.byref(n)) == OK
        assert n.value == len(want) and buf[:cap + 1].tobytes() == want and (buf[cap + 1:] == FILL).all()
        assert len(want) <= hs.jpeg_bound(W, H)


def test_device_file_forms(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, N = 33, 17, 3
    flows = [field(W, H, 70 + p) for p in range(N)]
    wants = [hs.encode_jpeg(hs.color_flow_host(u, v), 95) for u, v in flows]
    bound = hs.jpeg_bound(W, H)
    cp = hs.make_color_params()
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p, (u, v) in enumerate(flows):
            put_flow(ctx, u, v, pair=p)
        out = torch.full((N + 1, bound + 16), FILL, dtype=torch.uint8, device="cuda")
        words = torch.full((N + 1,), 77, dtype=torch.int64, device="cuda")
        ptrs = (ctypes.c_void_p * N)(*[out[i].data_ptr() for i in range(N)])
        torch.cuda.synchronize()
        assert L.hsflow_color_flow_jpeg_batch_device(ctx._h, 0, N, ctypes.byref(cp), 95, ptrs, bound, ctypes.c_void_p(words.data_ptr())) == OK
        assert L.hsflow_color_flow_jpeg_device(ctx._h, 1, ctypes.byref(cp), 95, ctypes.c_void_p(out[N].data_ptr()), bound,
                                               ctypes.c_void_p(words.data_ptr() + 8 * N)) == OK
        ctx.synchronize()
        host, sizes = out.cpu().numpy(), words.cpu().tolist()
        for i, want in enumerate(wants + [wants[1]]):
            assert sizes[i] == len(want) and host[i, :len(want)].tobytes() == want and (host[i, len(want):] == FILL).all(), i


# ---- 5. pipeline -----------------------------------------------------------------------------------------------------

def test_pipeline(hs, gpu_ok):
    import torch
    W, H, depth = 300, 70, 3
    P1 = dict(lam=1.0, max_iter=60, term_type=ITER | EPS, epsilon=EPS6)
    P3 = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)
    pairs = {"t1": (synth.translating_pair(W, H, seed=1), P1), "t2": (synth.translating_pair(W, H, seed=2, dx=-1.0, dy=2.0), P1),
             "patch": (_patch_pair(W, H), P3)}
    want = {}
    for k, ((A, B), kw) in pairs.items():
        with hs.HSFlow(W, H, own_stream=True) as ctx:
            ctx.set_frames(A, B)
            ctx.solve(**kw)
            u, v = ctx.flow()
            want[k] = {mf: hs.color_flow_host(u, v, max_flow=mf) for mf in (None, 0.5)}
            assert np.array_equal(ctx.color(), want[k][None])
    dev = {k: tuple(torch.from_numpy(f).cuda() for f in AB) for k, (AB, _) in pairs.items()}
    torch.cuda.synchronize()
    order = ["t1", "t2", "patch", "t2", "t1", "patch", "t1"]
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")

    def check_ticket(pl, t):
        k = order[t]
        mf = None if t % 2 else 0.5
        assert np.array_equal(pl.color(t, max_flow=mf), want[k][mf]), (t, k)
        out.fill_(7)
        torch.cuda.synchronize()
        assert pl.color_device(t, out, max_flow=mf) is out         # complete on return
        assert np.array_equal(out.cpu().numpy(), want[k][mf]), (t, k)
        assert pl.color_jpeg(t, max_flow=mf) == hs.encode_jpeg(want[k][mf], 95), (t, k)

    with hs.PairPipeline(W, H, depth=depth, lanes=2) as pl:
        for t, k in enumerate(order):
            if t >= depth:
                check_ticket(pl, t - depth)                        # the oldest pair, before its slot is taken again
            assert pl.submit_device(dev[k][0], dev[k][1], **pairs[k][1]) == t
        for t in range(len(order) - depth, len(order)):
            check_ticket(pl, t)
        for call in (lambda: pl.color(0), lambda: pl.color_device(1, out), lambda: pl.color_jpeg(2)):   # slots reused since
            with pytest.raises(hs.HsflowError) as e:
                call()
            assert e.value.status == E_STATE
        check_ticket(pl, len(order) - 1)                           # the pipeline still works


# ---- 6. command line -------------------------------------------------------------------------------------------------

def _cli(args, extra_env=None, ok=True):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for name in ("HSFLOW_RENDER_DEVICE", "HSFLOW_JPEG_DEVICE", "HSFLOW_PICTURE", "HSFLOW_COLOR_MAX"):
        env.pop(name, None)
    env.update(extra_env or {})
    r = subprocess.run([cli] + args, env=env, capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_cli_colour_picture_on_three_routes(hs, gpu_ok, tmp_path):
    a, b = os.path.join(GOLDEN, "ref_city_1.jpg"), os.path.join(GOLDEN, "ref_city_2.jpg")
    routes = {"host": {}, "device": {"HSFLOW_RENDER_DEVICE": "1"}, "file": {"HSFLOW_RENDER_DEVICE": "1", "HSFLOW_JPEG_DEVICE": "1"}}
    for args in (["-cv", "-hd", a, b, None, ".1", "10"], ["-cl", "-hd", a, b, None, "15", "10", "1", "GPU"]):
        files = {}
        for colour in ({"HSFLOW_PICTURE": "color"}, {"HSFLOW_PICTURE": "color", "HSFLOW_COLOR_MAX": "0.75"}):
            for name, env in routes.items():
                out = str(tmp_path / ("%s_%s_%d.jpg" % (args[0][1:], name, len(colour))))
                _cli([out if t is None else t for t in args], dict(env, **colour))
                files[name, len(colour)] = open(out, "rb").read()
            assert files["host", len(colour)] == files["device", len(colour)] == files["file", len(colour)]
        assert files["host", 1] != files["host", 2]
        assert files["host", 1] != open(os.path.join(GOLDEN, "ref_city_%s_out.jpg" % args[0][1:]), "rb").read()
    # without the variable the file is still the reference's arrow picture
    out = str(tmp_path / "arrows.jpg")
    _cli(["-cv", "-hd", a, b, out, ".1", "10"], {"HSFLOW_RENDER_DEVICE": "1", "HSFLOW_COLOR_MAX": "3"})
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "ref_city_cv_out.jpg"), "rb").read()
    for bad in ({"HSFLOW_PICTURE": "colour"}, {"HSFLOW_PICTURE": "color", "HSFLOW_COLOR_MAX": "0"}, {"HSFLOW_COLOR_MAX": "1x"}):
        r = _cli(["-cv", "-hd", a, b, out, ".1", "10"], bad, ok=False)
        assert r.returncode == 1 and "HSFLOW_" in r.stdout


def test_cli_camera_loop_colour(hs, gpu_ok, tmp_path):
    W, H, n = 160, 96, 4
    cam = tmp_path / "cam"
    cam.mkdir()
    for i in range(n):
        _, moved = synth.translating_pair(W, H, seed=77, dx=1.5 * i, dy=-0.75 * i)
        with open(str(cam / ("frame_%04d.pgm" % i)), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (W, H) + moved.tobytes())
    for args in (["-cv", "-cam", ".1", "12"], ["-cl", "-cam", "3", "12", "1", "GPU"]):
        files = {}
        modes = {"host": {}, "device": {"HSFLOW_RENDER_DEVICE": "1"}}
        if args[0] == "-cv":
            modes["batch_host"] = {"HSFLOW_CAMERA_BATCH": "2"}
            modes["batch_device"] = {"HSFLOW_CAMERA_BATCH": "2", "HSFLOW_RENDER_DEVICE": "1"}
        for mode, extra in modes.items():
            out = tmp_path / (args[0][1:] + mode)
            out.mkdir()
            env = dict(extra, HSFLOW_CAMERA_DIR=str(cam), HSFLOW_CAMERA_OUT=str(out), HSFLOW_PICTURE="color")
            assert "Avg time" in _cli(args, env).stdout
            files[mode] = {p: open(str(out / p), "rb").read() for p in sorted(os.listdir(str(out)))}
        assert sorted(files["host"]) == ["flow_%04d.ppm" % i for i in range(1, n)]
        for mode in modes:
            assert files[mode] == files["host"], mode
        body = np.frombuffer(files["host"]["flow_0001.ppm"][15:], np.uint8)
        assert (body != 0).mean() > 0.9                            # dense: hardly a black byte


# ---- 7. errors -------------------------------------------------------------------------------------------------------

def test_argument_errors(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, N = 64, 4, 2
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, *field(W, H, p), pair=p)
        out = torch.full((N, H, W, 3), FILL, dtype=torch.uint8, device="cuda")
        ptrs = (ctypes.c_void_p * N)(*[out[i].data_ptr() for i in range(N)])
        holed = (ctypes.c_void_p * N)(ptrs[0], None)
        cp = hs.make_color_params()
        host = np.full((H, 3 * W), FILL, np.uint8)
        m = ctypes.c_float(-1.0)
        torch.cuda.synchronize()
        dev, bat, syn = L.hsflow_color_flow_device, L.hsflow_color_flow_batch_device, L.hsflow_color_flow
        bad = []
        for change in (dict(struct_size=12), dict(scale_mode=2), dict(scale_mode=1, max_flow=0.0), dict(scale_mode=1, max_flow=float("inf")),
                       dict(scale_mode=1, max_flow=float("nan")), dict(scale_mode=1, max_flow=-2.0)):
            b = hs.make_color_params()
            for k, val in change.items():
                setattr(b, k, val)
            bad.append(b)
        for b in bad + [None]:
            ref = ctypes.byref(b) if b is not None else None
            assert dev(ctx._h, 0, ref, ptrs[0], 3 * W) == E_ARG
            assert bat(ctx._h, 0, N, ref, ptrs, 3 * W) == E_ARG
            assert syn(ctx._h, 0, ref, host.ctypes.data, 3 * W, ctypes.byref(m)) == E_ARG
        r = ctypes.byref(cp)
        assert dev(ctx._h, N, r, ptrs[0], 3 * W) == E_ARG and dev(ctx._h, -1, r, ptrs[0], 3 * W) == E_ARG
        assert dev(ctx._h, 0, r, None, 3 * W) == E_ARG and dev(None, 0, r, ptrs[0], 3 * W) == E_ARG
        assert dev(ctx._h, 0, r, ptrs[0], 3 * W - 1) == E_SIZE
        assert bat(ctx._h, 0, 0, r, ptrs, 3 * W) == E_ARG and bat(ctx._h, 1, N, r, ptrs, 3 * W) == E_ARG and bat(ctx._h, -1, 1, r, ptrs, 3 * W) == E_ARG
        assert bat(ctx._h, 0, N, r, None, 3 * W) == E_ARG and bat(ctx._h, 0, N, r, holed, 3 * W) == E_ARG
        assert bat(ctx._h, 0, N, r, ptrs, 3 * W - 1) == E_SIZE
        assert syn(ctx._h, 0, r, None, 3 * W, None) == E_ARG and syn(ctx._h, 0, r, host.ctypes.data, 3 * W - 1, None) == E_SIZE
        n = ctypes.c_size_t(5)
        jp = L.hsflow_color_flow_jpeg
        assert jp(ctx._h, 0, r, 0, host.ctypes.data, host.size, ctypes.byref(n)) == E_ARG
        assert jp(ctx._h, 0, r, 95, None, host.size, ctypes.byref(n)) == E_ARG
        assert jp(ctx._h, 0, r, 95, host.ctypes.data, host.size, None) == E_ARG
        assert jp(ctx._h, N, r, 95, host.ctypes.data, host.size, ctypes.byref(n)) == E_ARG
        ctx.synchronize()
        assert bool((out == FILL).all().item()) and (host == FILL).all() and m.value == -1.0 and n.value == 5   # nothing was written
        assert syn(ctx._h, 1, r, host.ctypes.data, 3 * W, None) == OK                                                 # scale_used may be null
        assert np.array_equal(host.reshape(H, W, 3), hs.color_flow_host(*field(W, H, 1)))
