"""The flow picture drawn on the GPU (include/hsflow.h: hsflow_render_flow[_device], hsflow_pipeline_render[_device];
kernels in opticalflowhs_amd/csrc/hs_kernels_render.hip.h) against the host drawing rule.

The yardstick is `refpics.render` (the rule of OpticalFlowOpenCV.cpp:33-46 / HSOpticalFlowOpenCL.cpp:759-769 restated
on the CPU; it draws the reference's own pictures), and `yardstick` below, its generalisation to other steps,
thresholds, scales and colours, built on `refpics.cv_line` and shown equal to `refpics.render` for both presets before
it is used.  Pictures are compared with np.array_equal: every byte of every pixel."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import refpics
from conftest import GOLDEN, ROOT
from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))
OK, E_ARG, E_SIZE, E_STATE = 0, 1, 2, 5
PRESETS = {"cv": (1.0, 0.5), "cl": (0.5, 1.0)}
DISC = [(dx, dy) for dy in range(-2, 3) for dx in range(-2, 3) if dx * dx + dy * dy <= 4]


def yardstick(u, v, route="cv", step=4, threshold=None, scale=None, dot_rgb=(0, 0, 255), line_rgb=(255, 0, 0), with_line_mask=False):
    """refpics.render for any step / threshold / scale / colours, plus the feature's own out-of-range rule
    (include/hsflow.h): where an end-point coordinate is not finite or its magnitude is >= 2^20 -- where the host's int
    conversion is undefined and refpics.render raises -- the dot is drawn and no line.
    with_line_mask: also returns which pixels ANY line reached, whatever lies over them in the end."""
    t = np.float32(PRESETS[route][0] if threshold is None else threshold)
    s = np.float32(PRESETS[route][1] if scale is None else scale)
    H, W = u.shape
    img = np.zeros((H, W, 3), np.uint8)
    reached = np.zeros((H, W, 3), np.uint8)
    with np.errstate(all="ignore"):
        for y in range(0, H, step):
            for x in range(0, W, step):
                a, b = np.float32(u[y, x]), np.float32(v[y, x])
                if not (a > t or b > t or a < -t or b < -t):
                    continue
                for dx, dy in DISC:
                    if 0 <= x + dx < W and 0 <= y + dy < H:
                        img[y + dy, x + dx] = dot_rgb
                fx, fy = np.float32(x) + a * s, np.float32(y) + b * s   # fp32, as the int + float of the host
                if not (np.isfinite(fx) and np.isfinite(fy) and abs(fx) < 2.0 ** 20 and abs(fy) < 2.0 ** 20):
                    continue
                refpics.cv_line(img, x, y, int(fx), int(fy), line_rgb)
                if with_line_mask:
                    refpics.cv_line(reached, x, y, int(fx), int(fy), (1, 1, 1))
    return (img, reached[:, :, 0].astype(bool)) if with_line_mask else img


def put_flow(ctx, u, v, pair=0):
    """Writes a flow into the context's planes from torch tensors (hsflow_set_flow_device)."""
    import torch
    ud, vd = torch.from_numpy(np.ascontiguousarray(u, np.float32)).cuda(), torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    torch.cuda.synchronize()
    ctx.set_flow_rows_from(ud, vd, 0, u.shape[0], pair=pair)
    ctx.synchronize()


def check(ctx, u, v, route="cv", pair=0, **kw):
    """Host form and device form of the render against the yardstick; returns the expected picture."""
    import torch
    want = yardstick(u, v, route, **kw)
    got = ctx.render(route, pair=pair, **kw)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), ("host form", route, kw, int((got != want).any(axis=2).sum()))
    out = torch.full(want.shape, 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()   # (the context draws on a stream of its own)
    assert ctx.render(route, out=out, pair=pair, **kw) is out
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), want), ("device form", route, kw)
    return want


def solved_reference_pair(hs, ctx, name, route):
    """The solve behind the reference's pictures (refpics: lambda 0.1 / alpha 15 as shipped, 10 sweeps, blur for cv)."""
    A, B = refpics.gray_pair(name)
    if route == "cv":
        ctx.set_frames_gray_blur(A, B)
        ctx.solve(lam=refpics.LAMBDA, max_iter=refpics.ITERATIONS, epsilon=refpics.EPSILON, term_type=ITER | EPS)
    else:
        ctx.set_frames(A, B)
        ctx.solve(mode=hs.MODE_CLASSIC_AS_SHIPPED, alpha=refpics.ALPHA, max_iter=refpics.ITERATIONS, term_type=ITER)


# ---- 1. the reference's pictures -------------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["cv", "cl"])
@pytest.mark.parametrize("name", ["city", "bunny"])
def test_reference_pictures(hs, gpu_ok, name, route):
    pytest.importorskip("PIL")
    H, W = refpics.gray_pair(name)[0].shape
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        solved_reference_pair(hs, ctx, name, route)
        picture = ctx.render(route)
        u, v = ctx.flow()
    assert np.array_equal(picture, refpics.render(u, v, route))
    assert (picture != 0).any()
    wrong, quality = refpics.picture_difference(picture, name, route)
    assert wrong == 0, (wrong, quality)


# ---- 2. rendering apart from solving ---------------------------------------------------------------------------------

SIZES = [(600, 480), (203, 117)]   # the reference's default size; one that is no multiple of 4 either way


def test_yardstick_is_refpics_render():
    rng = np.random.default_rng(5)
    u, v = (rng.uniform(-9, 9, (61, 83)).astype(np.float32) for _ in range(2))
    for route in ("cv", "cl"):
        assert np.array_equal(yardstick(u, v, route), refpics.render(u, v, route))


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("route", ["cv", "cl"])
def test_order_rule_dense_long_arrows(hs, gpu_ok, W, H, route):
    """(a) Uniform random arrows in [-40, 40]^2 at every grid point: thousands of lines cross earlier and later dots."""
    rng = np.random.default_rng(7)
    u, v = (rng.uniform(-40, 40, (H, W)).astype(np.float32) for _ in range(2))
    want, reached = yardstick(u, v, route, with_line_mask=True)
    if (W, H) == (600, 480):
        assert np.array_equal(want, refpics.render(u, v, route))
    # the case must show the order: pixels a line reached whose final colour is a dot (a LATER one: a point's own dot lies under its line)
    later_dot = int((reached & (want == (0, 0, 255)).all(axis=2)).sum())
    print("order rule %dx%d %s: %d line pixels under a later dot" % (W, H, route, later_dot))
    # at least 10 000 on the 18 000 grid points of 600 x 480, and the same share of the grid points on the smaller size
    grid_points = -(-W // 4) * -(-H // 4)
    assert later_dot >= 10000 * grid_points // 18000, later_dot
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        got = ctx.render(route)
    assert np.array_equal(got, want), int((got != want).any(axis=2).sum())


@pytest.mark.parametrize("W,H", SIZES)
def test_arrows_leaving_the_image(hs, gpu_ok, W, H):
    """(b) Arrows of length up to 5000 across all four edges and out of all four corners, among short ones."""
    rng = np.random.default_rng(8)
    u, v = (rng.uniform(-3, 3, (H, W)).astype(np.float32) for _ in range(2))
    ys, xs = rng.integers(0, (H + 3) // 4, 240) * 4, rng.integers(0, (W + 3) // 4, 240) * 4
    ang, length = rng.uniform(0, 2 * np.pi, 240), rng.uniform(50, 5000, 240)
    u[ys, xs], v[ys, xs] = (length * np.cos(ang)).astype(np.float32), (length * np.sin(ang)).astype(np.float32)
    gx, gy = (W - 1) // 4 * 4, (H - 1) // 4 * 4
    for x, y in ((0, 0), (gx, 0), (0, gy), (gx, gy), (8, 8), (gx - 8, gy - 8)):   # out of the corners, diagonally, and straight out
        sx, sy = (-1 if x < W // 2 else 1), (-1 if y < H // 2 else 1)
        u[y, x], v[y, x] = 4000.0 * sx, 4000.0 * sy
        u[y, x + 4 if x < W // 2 else x - 4], v[y, x + 4 if x < W // 2 else x - 4] = 0.0, 3000.0 * sy
        u[y + 4 if y < H // 2 else y - 4, x], v[y + 4 if y < H // 2 else y - 4, x] = 3000.0 * sx, 0.0
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for route in ("cv", "cl"):
            want = check(ctx, u, v, route)
            edges = (want[0] != 0).any(), (want[-1] != 0).any(), (want[:, 0] != 0).any(), (want[:, -1] != 0).any()
            assert all(edges), edges


@pytest.mark.parametrize("W,H", SIZES)
def test_threshold_truncation_and_zero_flow(hs, gpu_ok, W, H):
    """(c) the threshold exactly, (d) end points in (-1, 0) that truncate to 0, (e) an all-zero flow."""
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        black = ctx.render("cv")                                  # (e): the planes of a fresh context are zero
        assert black.shape == (H, W, 3) and not black.any()
        for route, (t, s) in PRESETS.items():
            t32 = np.float32(t)
            up, dn = np.nextafter(t32, np.float32(np.inf)), np.nextafter(t32, np.float32(0))
            specials = [t32, up, dn, -t32, -up, -dn, np.float32(-0.0), np.float32(0.0)]
            u, v = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
            k = 0
            for y in range(8, H - 8, 8):                          # every pairing of the special values, apart from each other
                for x in range(8, W - 8, 8):
                    u[y, x], v[y, x] = specials[k % 8], specials[(k // 8) % 8]
                    k += 1
            assert k >= 64
            put_flow(ctx, u, v)
            want = check(ctx, u, v, route)
            assert (want != 0).any() and not want[8, 8].any()     # u = v = t exactly: not drawn
            # (d): at x = 0 / y = 0 an end point in (-1, 0) truncates to 0 -- toward zero, not to -1
            u[:], v[:] = 0, 0
            for i, y in enumerate(range(0, H, 4)):
                u[y, 0], v[y, 0] = np.float32(-(0.05 + 0.9 * (i % 10) / 10) / s), np.float32(2.0 / s)
            for i, x in enumerate(range(4, W, 4)):
                u[0, x], v[0, x] = np.float32(2.0 / s), np.float32(-(0.05 + 0.9 * (i % 10) / 10) / s)
            u[0, 0], v[0, 0] = np.float32(-0.999 / s), np.float32(-0.999 / s)
            put_flow(ctx, u, v)
            want = check(ctx, u, v, route)
            assert tuple(want[0, 0]) == (255, 0, 0)               # the line's one pixel over the dot
        u[:], v[:] = 0, 0
        put_flow(ctx, u, v)
        assert not ctx.render("cl").any()                         # (e) again, on a plane that has been drawn on


@pytest.mark.parametrize("W,H", SIZES)
def test_other_steps_scales_colours(hs, gpu_ok, W, H):
    """(f) step 1, 3, 8; scale 2.0 and -1.0; other colours and thresholds."""
    rng = np.random.default_rng(9)
    u, v = (rng.uniform(-6, 6, (H, W)).astype(np.float32) for _ in range(2))
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        check(ctx, u, v, "cv", step=1, threshold=5.5, scale=2.0)
        check(ctx, u, v, "cl", step=3, scale=-1.0, dot_rgb=(9, 200, 17), line_rgb=(1, 2, 3))
        check(ctx, u, v, "cv", step=8, threshold=0.0, scale=2.0, dot_rgb=(255, 255, 255), line_rgb=(0, 0, 1))
        check(ctx, u, v, "cl", step=max(W, H) + 5, threshold=0.0)   # one grid point


# ---- 3. out of range ---------------------------------------------------------------------------------------------------

def test_out_of_range_end_points(hs, gpu_ok):
    """inf, -inf, 1e9 and NaN in one component: the dot and no line, status OK -- and at once: the work of a lane is bounded
    by the image.  refpics.render cannot take such values; the yardstick of this file applies the rule of the header."""
    W, H = 600, 480
    rng = np.random.default_rng(10)
    u, v = (rng.uniform(-5, 5, (H, W)).astype(np.float32) for _ in range(2))
    assert np.array_equal(yardstick(u, v, "cv"), refpics.render(u, v, "cv"))       # in range: the yardstick is refpics.render
    odd = [np.inf, -np.inf, 1e9, -1e9, np.nan, 3e38, 2.0 ** 21, -2.0 ** 21, 2.0 ** 20 - 700, -(2.0 ** 20) + 700]
    points = []
    for i, val in enumerate(odd):
        for j, comp in enumerate("uv"):
            y, x = 40 + 40 * i + 20 * j, 60 + 200 * j + 12 * i   # no two in one row or column: the long in-range lines run along them
            u[y - 8:y + 9, x - 8:x + 9], v[y - 8:y + 9, x - 8:x + 9] = 0, 0   # no neighbour's line over this dot
            (u if comp == "u" else v)[y, x] = val
            (v if comp == "u" else u)[y, x] = 2.5
            points.append((y, x, val))
    u[440, 440], v[440, 440] = np.nan, np.nan                                     # NaN in both: nothing at all
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        want = check(ctx, u, v, "cl")                                              # one input, rendered once per form
    for y, x, val in points:
        if not abs(val) < 2.0 ** 20:                                               # (NaN included): the whole dot, no line over it
            assert all(tuple(want[y + dy, x + dx]) == (0, 0, 255) for dx, dy in DISC), (y, x, val)
            assert int((want[y - 3:y + 4, x - 3:x + 4] != 0).any(axis=2).sum()) == 13


# ---- 4. buffers ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,pad", [(600, 480, 8), (600, 480, 5), (203, 117, 7), (203, 117, 3)])
def test_pitched_destination_and_repeat(hs, gpu_ok, W, H, pad):
    """A pitched device destination with a sentinel in the padding and in a row before and after stays untouched there
    (pad 8 / 7: rows on 4-byte boundaries, the wide stores; 5 / 3: not); rendering twice gives the same bytes."""
    import torch
    rng = np.random.default_rng(12)
    u, v = (rng.uniform(-12, 12, (H, W)).astype(np.float32) for _ in range(2))
    want = yardstick(u, v, "cl")
    stride = 3 * W + pad
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for offset in (0, 1):   # (1: the picture itself off the 4-byte boundary)
            buf = torch.full(((H + 2) * stride + 4,), 0xA5, dtype=torch.uint8, device="cuda")
            out = torch.as_strided(buf, (H, W, 3), (stride, 3, 1), storage_offset=stride + offset)
            torch.cuda.synchronize()
            for _ in range(2):
                ctx.render("cl", out=out)
                ctx.synchronize()
                host = buf.cpu().numpy()
                rows = host[offset:offset + (H + 2) * stride].reshape(H + 2, stride)
                assert np.array_equal(rows[1:H + 1, :3 * W].reshape(H, W, 3), want)
                assert (rows[1:H + 1, 3 * W:] == 0xA5).all() and (rows[0] == 0xA5).all() and (rows[H + 1] == 0xA5).all()
                assert (host[:offset] == 0xA5).all() and (host[offset + (H + 2) * stride:] == 0xA5).all()
        first = ctx.render("cl")
        assert np.array_equal(first, ctx.render("cl")) and np.array_equal(first, want)
        # a host destination with a pitch
        big = np.full((H, stride), 0xA5, np.uint8)
        view = np.lib.stride_tricks.as_strided(big, (H, W, 3), (stride, 3, 1))
        assert ctx.render("cl", out=view) is view
        assert np.array_equal(view, want) and (big[:, 3 * W:] == 0xA5).all()


def test_second_pair_renders_its_own_flow(hs, gpu_ok):
    W, H = 203, 117
    rng = np.random.default_rng(13)
    flows = [tuple(rng.uniform(-8, 8, (H, W)).astype(np.float32) for _ in range(2)) for _ in range(3)]
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        for p, (u, v) in enumerate(flows):
            put_flow(ctx, u, v, pair=p)
        pictures = [check(ctx, u, v, "cv", pair=p) for p, (u, v) in enumerate(flows)]
        assert not np.array_equal(pictures[0], pictures[1]) and not np.array_equal(pictures[1], pictures[2])
        assert np.array_equal(ctx.render("cv", pair=1), pictures[1])


# ---- 5. ordering with asynchronous solves ---------------------------------------------------------------------------

def _view(hs, ctx, W, H):
    import torch
    from opticalflowhs_amd.pipeline import _DeviceView
    pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    assert hs._lib.load().hsflow_flow_view_device(ctx._h, 0, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == OK
    return tuple(torch.as_tensor(_DeviceView(p.value, (H, W), (sb.value, 4)), device="cuda") for p in (pu, pv))


def test_render_behind_an_asynchronous_solve(hs, gpu_ok):
    """solve_async (ITER|EPS) and render with no call in between, on an async-reduce context: the picture of the synchronous
    solve.  The render counts as work behind the solve's marker: hsflow_wait_solve and hsflow_flow_view_device return only
    when it is through, and the flow planes are what they were."""
    import torch
    L = hs._lib.load()
    W, H = 1920, 1080
    A, B = synth.translating_pair(W, H, seed=1, dx=3.0, dy=-2.0)
    kw = dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6)
    rkw = dict(threshold=0.05, scale=4.0)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with hs.HSFlow(W, H, 1, stream=s.cuda_stream) as ctx:
        assert L.hsflow_set_async_reduce(ctx._h, 1) == OK
        ctx.set_frames(A, B)
        ctx.solve(**kw)
        u, v = ctx.flow()
        want = ctx.render("cv", **rkw)
        assert (want != 0).any() and np.array_equal(want, yardstick(u, v, "cv", **rkw))
        before = tuple(t.clone() for t in _view(hs, ctx, W, H))
        torch.cuda.synchronize()
        # host form right behind the asynchronous solve
        ctx.solve_async(**kw)
        got = ctx.render("cv", **rkw)
        assert np.array_equal(got, want)
        # device form: only enqueued; flow_view must wait for it, and hands out unchanged planes
        out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.solve_async(**kw)
        for _ in range(8):
            ctx.render("cv", out=out, **rkw)
        uv = _view(hs, ctx, W, H)
        assert s.query(), "flow_view returned while a render was still in flight"
        assert torch.equal(uv[0].clone(), before[0]) and torch.equal(uv[1].clone(), before[1])
        assert np.array_equal(out.cpu().numpy(), want)
        # ... and so must hsflow_wait_solve
        ctx.solve_async(**kw)
        for _ in range(8):
            ctx.render("cv", out=out, **rkw)
        assert L.hsflow_wait_solve(ctx._h) == OK
        assert s.query(), "wait_solve returned while a render was still in flight"
        assert np.array_equal(out.cpu().numpy(), want)
        uv = _view(hs, ctx, W, H)
        assert torch.equal(uv[0].clone(), before[0]) and torch.equal(uv[1].clone(), before[1])


# ---- 6. pipeline ----------------------------------------------------------------------------------------------------------

def _patch_pair(W, H):
    """A flat frame with a patch one grey level brighter: with lambda 1e-3 / epsilon 1e-4 its early stop fires
    (tests/test_gpu_pipeline_lanes.py builds the same)."""
    a = np.full((H, W), 90, np.uint8)
    b = a.copy()
    rows, cols = slice(H // 4, H // 4 + min(80, H // 2)), slice(W // 5, W // 5 + min(300, W // 2))
    a[rows, cols], b[rows, cols] = 120, 121
    return a, b


def test_pipeline_render(hs, gpu_ok):
    import torch
    W, H, depth = 600, 480, 6
    P1 = dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6)
    P3 = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)
    rkw = dict(threshold=0.02, scale=6.0)
    pairs = {"t1": (synth.translating_pair(W, H, seed=1), P1), "t2": (synth.translating_pair(W, H, seed=2), P1), "patch": (_patch_pair(W, H), P3)}
    want, flows = {}, {}
    for k, ((A, B), kw) in pairs.items():
        with hs.HSFlow(W, H, own_stream=True) as ctx:
            ctx.set_frames(A, B)
            info = ctx.solve(**kw)
            flows[k] = ctx.flow()
        if k == "patch":
            assert 1 < info["iterations_done"] < 400, info          # its early stop fires
        want[k] = yardstick(flows[k][0], flows[k][1], "cv", **rkw)
        assert (want[k] != 0).any(), k
    dev = {k: tuple(torch.from_numpy(f).cuda() for f in AB) for k, (AB, _) in pairs.items()}
    torch.cuda.synchronize()
    order = ["t1", "t2"] * 7
    order[5] = "patch"
    out = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")

    def check_ticket(pl, t):
        if t % 2:
            got = pl.render(t, "cv", **rkw)
        else:
            out.fill_(7)
            torch.cuda.synchronize()
            assert pl.render(t, "cv", out=out, **rkw) is out      # complete on return: read on another stream at once
            got = out.cpu().numpy()
        assert np.array_equal(got, want[order[t]]), (t, order[t])
        if order[t] == "patch":
            assert pl.info(t)["eps_rerun"] == 1                   # the early-stop pair was re-solved before it was drawn

    with hs.PairPipeline(W, H, depth=depth, lanes=2) as pl:
        for t, k in enumerate(order):
            if t >= depth:
                check_ticket(pl, t - depth)                       # the oldest pair, before its slot is taken again
            assert pl.submit_device(dev[k][0], dev[k][1], **pairs[k][1]) == t
        for t in range(len(order) - depth, len(order)):
            check_ticket(pl, t)
        for t in (0, 7):                                          # slots that have been reused since
            with pytest.raises(hs.HsflowError) as e:
                pl.render(t, "cv")
            assert e.value.status == E_STATE
            with pytest.raises(hs.HsflowError) as e:
                pl.render(t, "cv", out=out)
            assert e.value.status == E_STATE
        with pytest.raises(hs.HsflowError) as e:
            pl.render(len(order), "cv")                           # never issued
        assert e.value.status == E_ARG
        check_ticket(pl, len(order) - 1)                          # the pipeline still works
        # host buffers: upload -> solve -> download, then the picture of the slot's flow
        (A, B), kw = pairs["t2"]
        bufs = [hs.pinned_empty((H, W), np.uint8) for _ in range(2)] + [hs.pinned_empty((H, W), np.float32) for _ in range(2)]
        bufs[0][:], bufs[1][:] = A, B
        t = pl.submit(bufs[0], bufs[1], bufs[2], bufs[3], **kw)
        assert np.array_equal(pl.render(t, "cv", **rkw), want["t2"])
        assert np.array_equal(bufs[2], flows["t2"][0]) and np.array_equal(bufs[3], flows["t2"][1])
        assert np.array_equal(pl.render(t, "cv", out=out, **rkw).cpu().numpy(), want["t2"])


# ---- 7. command line ------------------------------------------------------------------------------------------------------

def _cli(args, extra_env=None):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    env.pop("HSFLOW_RENDER_DEVICE", None)
    env.update(extra_env or {})
    r = subprocess.run([cli] + args, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


@pytest.mark.parametrize("name", ["city", "bunny"])
def test_cli_device_route_writes_the_reference_files(hs, gpu_ok, tmp_path, name):
    """HSFLOW_RENDER_DEVICE=1: the reference's command lines on its own JPEG inputs write its own output files, byte for byte."""
    a, b = os.path.join(GOLDEN, "ref_%s_1.jpg" % name), os.path.join(GOLDEN, "ref_%s_2.jpg" % name)
    out = str(tmp_path / "out.jpg")
    on = {"HSFLOW_RENDER_DEVICE": "1"}
    _cli(["-cv", "-hd", a, b, out, ".1", "10"], on)
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "ref_%s_cv_out.jpg" % name), "rb").read()
    os.remove(out)
    _cli(["-cl", "-hd", a, b, out, "15", "10", "1", "GPU"], dict(on, HSFLOW_CL_AS_SHIPPED="1"))
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "ref_%s_cl_out.jpg" % name), "rb").read()


@pytest.mark.parametrize("route", ["cv", "cl"])
def test_cli_camera_loop_same_pictures_on_both_routes(hs, gpu_ok, tmp_path, route):
    W, H, n = 160, 96, 4
    cam = tmp_path / "cam"
    cam.mkdir()
    for i in range(n):
        _, moved = synth.translating_pair(W, H, seed=77, dx=1.5 * i, dy=-0.75 * i)   # the texture, 1.5 pixels further every frame
        with open(str(cam / ("frame_%04d.pgm" % i)), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (W, H) + moved.tobytes())
    args = ["-cv", "-cam", ".1", "12"] if route == "cv" else ["-cl", "-cam", "3", "12", "1", "GPU"]
    files = {}
    for mode in ("host", "device"):
        out = tmp_path / mode
        out.mkdir()
        env = {"HSFLOW_CAMERA_DIR": str(cam), "HSFLOW_CAMERA_OUT": str(out)}
        if mode == "device":
            env["HSFLOW_RENDER_DEVICE"] = "1"
        assert "Avg time" in _cli(args, env).stdout
        files[mode] = {p: open(str(out / p), "rb").read() for p in sorted(os.listdir(str(out)))}
    assert sorted(files["host"]) == ["flow_%04d.ppm" % i for i in range(1, n)]
    assert files["host"] == files["device"]
    assert any(any(data[15:]) for data in files["host"].values())   # not all black


# ---- 8. errors ----------------------------------------------------------------------------------------------------------

def test_argument_errors(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H = 64, 32
    RP = hs._lib.HsflowRenderParams
    host = np.zeros(H * (3 * W + 4), np.uint8)
    dev = torch.zeros(H * (3 * W + 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hp, dp = ctypes.c_void_p(host.ctypes.data), ctypes.c_void_p(dev.data_ptr())

    def bad(**kw):
        rp = hs.make_render_params("cv")
        for k, val in kw.items():
            setattr(rp, k, val)
        return ctypes.byref(rp)

    good = bad()
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        for fn, p in ((L.hsflow_render_flow, hp), (L.hsflow_render_flow_device, dp)):
            assert fn(ctx._h, 0, good, p, 3 * W) == OK
            assert fn(ctx._h, 1, good, p, 3 * W + 1) == OK
            assert fn(ctx._h, 0, None, p, 3 * W) == E_ARG
            assert fn(ctx._h, 0, good, None, 3 * W) == E_ARG
            assert fn(ctx._h, 2, good, p, 3 * W) == E_ARG and fn(ctx._h, -1, good, p, 3 * W) == E_ARG
            assert fn(ctx._h, 0, bad(struct_size=ctypes.sizeof(RP) - 4), p, 3 * W) == E_ARG
            assert fn(ctx._h, 0, bad(step=0), p, 3 * W) == E_ARG and fn(ctx._h, 0, bad(step=-4), p, 3 * W) == E_ARG
            for t in (float("nan"), float("inf"), -0.5):
                assert fn(ctx._h, 0, bad(threshold=t), p, 3 * W) == E_ARG, t
            for s in (float("nan"), float("inf"), float("-inf")):
                assert fn(ctx._h, 0, bad(scale=s), p, 3 * W) == E_ARG, s
            assert fn(ctx._h, 0, good, p, 3 * W - 1) == E_SIZE and fn(ctx._h, 0, good, p, 0) == E_SIZE
            assert b"stride" in L.hsflow_last_error(ctx._h)
            assert fn(ctx._h, 0, bad(threshold=0.0, scale=0.0), p, 3 * W) == OK
        ctx.synchronize()
        with pytest.raises(ValueError):
            ctx.render("cv", out=np.zeros((H, W), np.uint8))
        with pytest.raises(ValueError):
            ctx.render("cv", out=torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda"))
    A, B = synth.translating_pair(W, H, seed=1)
    dA, dB = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    torch.cuda.synchronize()
    with hs.PairPipeline(W, H, depth=2, lanes=2) as pl:
        t = pl.submit_device(dA, dB, max_iter=5)
        for fn, p in ((L.hsflow_pipeline_render, hp), (L.hsflow_pipeline_render_device, dp)):
            assert fn(pl._h, t, good, p, 3 * W) == OK
            assert fn(pl._h, t, None, p, 3 * W) == E_ARG and fn(pl._h, t, good, None, 3 * W) == E_ARG
            assert fn(pl._h, t, bad(step=0), p, 3 * W) == E_ARG
            assert fn(pl._h, t, good, p, 3 * W - 1) == E_SIZE
            assert fn(pl._h, t + 1, good, p, 3 * W) == E_ARG      # never issued


# ---- 9. 1080p ------------------------------------------------------------------------------------------------------------

def test_1080p_once(hs, gpu_ok):
    """The seed-1 synthetic pair, 100 sweeps, cv preset: the whole frame against refpics.render (about 130 000 grid points)."""
    W, H = 1920, 1080
    A, B = synth.translating_pair(W, H, seed=1)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        ctx.solve(lam=1.0, max_iter=100, term_type=ITER)
        picture = ctx.render("cv")
        picture_cl = ctx.render("cl")
        u, v = ctx.flow()
    want = refpics.render(u, v, "cv")
    print("1080p: %d pixels drawn (cv)" % int((want != 0).any(axis=2).sum()))
    assert np.array_equal(picture, want)
    # the pair moves by (0.75, -0.5): under the cv threshold of 1 nearly everywhere, over the cl threshold of 0.5
    want = refpics.render(u, v, "cl")
    assert int((want != 0).any(axis=2).sum()) > 100000
    assert np.array_equal(picture_cl, want)
