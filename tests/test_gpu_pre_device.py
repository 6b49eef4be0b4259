"""Frame pre-processing on the device (ABI 0.9): the fused kernel behind hsflow_set_frames_device_ex against the CPU oracle,
and the host-pointer entries (uploads into the context's staging, then k_bgr2gray / k_box_blur3) against the oracle too; the
camera sequence of hsflow_push_frame[_device]_ex against the oracle run through the reference's loop,
hsflow_pipeline_submit_device_ex against the host-buffer pipeline, and the CLI's camera route, which pushes frames instead
of reading the blurred one back."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))
WIDTHS = [1, 2, 3, 4, 5, 7, 255, 256, 257, 260]
FORMATS = ["gray_blur", "bgr", "bgr_blur"]


def heights(hs):
    S = hs.PRE_STRIP_ROWS
    return sorted({1, 2, 3, S - 1, S, S + 1, 2 * S + 1} - {0})


def oracle_pre(oracle, img, frames):
    g = oracle.bgr2gray(np.ascontiguousarray(img)) if frames.startswith("bgr") else np.ascontiguousarray(img)
    return oracle.box_blur3(g) if frames.endswith("blur") else g


def strided_device(img, offset, stride):
    """`img` ((H, W) or (H, W, 3) uint8) as a view into a larger CUDA byte tensor: base `offset` bytes past the allocation's
    start, rows `stride` bytes apart, the bytes between rows filled with a value of their own; the tensor ends with the last row."""
    import torch
    H, rowb = img.shape[0], int(np.prod(img.shape[1:]))
    assert stride >= rowb
    host = np.full(offset + (H - 1) * stride + rowb, 0x5A, np.uint8)
    rows = np.lib.stride_tricks.as_strided(host[offset:], (H, rowb), (stride, 1))
    rows[...] = img.reshape(H, rowb)
    big = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()   # the contexts work on streams of their own
    shape, strides = ((H, img.shape[1], 3), (stride, 3, 1)) if img.ndim == 3 else ((H, img.shape[1]), (stride, 1))
    view = torch.as_strided(big, shape, strides, storage_offset=offset)
    assert view.data_ptr() % 4 == offset % 4
    return view


def host_route(ctx, a, b, frames):
    """The same pixels through the host-pointer entries (uploaded into the staging, then k_bgr2gray / k_box_blur3)."""
    if frames == "gray_blur":
        ctx.set_frames_gray_blur(a, b)
    else:
        ctx.set_frames_bgr(a, b, blur=frames == "bgr_blur")
    return ctx.frames()


def check_both_routes_against_the_oracle(hs, oracle):
    """Device sources against the oracle, then host sources of the same pixels against the oracle and against the device
    route.  Every shape of the CPU list x every format, the (alignment, stride) variant cycling through all sixteen; then
    all sixteen on one shape that has a ragged last group and a strip seam."""
    S = hs.PRE_STRIP_ROWS
    rng = np.random.default_rng(17)
    case = 0

    def one(ctx, W, H, frames, off_a, off_b, extra_a, extra_b):
        colour = frames.startswith("bgr")
        shape = (H, W, 3) if colour else (H, W)
        a, b = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
        rowb = W * (3 if colour else 1)
        da, db = strided_device(a, off_a, rowb + extra_a), strided_device(b, off_b, rowb + extra_b)
        ctx.set_frames_device(da, db, frames=frames)
        fa, fb = ctx.frames()
        tag = (W, H, frames, off_a, off_b, extra_a, extra_b)
        assert np.array_equal(fa, oracle_pre(oracle, a, frames)) and np.array_equal(fb, oracle_pre(oracle, b, frames)), tag
        ha, hb = host_route(ctx, a, b, frames)
        assert np.array_equal(ha, oracle_pre(oracle, a, frames)) and np.array_equal(hb, oracle_pre(oracle, b, frames)), tag
        assert np.array_equal(fa, ha) and np.array_equal(fb, hb), tag

    extras = [0, 1, 4, 3]   # strides 3W, 3W+1, 3W+4 (W, W+1, W+4 for gray) and +3
    for W in WIDTHS:
        for H in heights(hs):
            with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
                for frames in FORMATS:
                    one(ctx, W, H, frames, case % 4, (case // 4) % 4, extras[(case // 16) % 4], extras[(case // 3) % 4])
                    case += 1
    W, H = 257, S + 1
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for frames in FORMATS:
            for off in range(4):
                for extra in extras:
                    one(ctx, W, H, frames, off, (off + 1) % 4, extra, extras[(extras.index(extra) + 1) % 4])
    # flat frames: the ends of the rounding division
    with hs.HSFlow(260, 2 * S + 1, 1, own_stream=True) as ctx:
        for value in (0, 255):
            a = np.full((2 * S + 1, 260, 3), value, np.uint8)
            da, db = strided_device(a, 1, 781), strided_device(a, 0, 780)
            ctx.set_frames_device(da, db, frames="bgr_blur")
            fa, fb = ctx.frames()
            assert np.all(fa == value) and np.all(fb == value)


def test_fused_kernel_against_oracle_and_host_entries(hs, oracle, gpu_ok):
    check_both_routes_against_the_oracle(hs, oracle)


def strided_host(img, offset, stride):
    """`img` as a view into a larger NumPy byte array: base `offset` bytes past its start, rows `stride` bytes apart, the
    bytes between rows filled with a value of their own; the array ends with the last row.  Returns (rows, the array)."""
    H, rowb = img.shape[0], int(np.prod(img.shape[1:]))
    host = np.full(offset + (H - 1) * stride + rowb, 0xA5, np.uint8)
    rows = np.lib.stride_tricks.as_strided(host[offset:], (H, rowb), (stride, 1))
    rows[...] = img.reshape(H, rowb)
    return rows, host


@pytest.mark.parametrize("entry", ["sync", "async"])
def test_host_sources_that_are_not_dense(hs, oracle, gpu_ok, entry):
    """Host frames with padded rows and an odd base, straight through the C entries (the Python wrappers make rows dense):
    a ragged last group, a strip seam and, at 257, more than one wavefront.  Frame a and frame b are different random
    frames and each plane is compared with its own oracle frame, so a swap of the two staging areas, or a launch that
    reads area 0 twice, fails here."""
    S = hs.PRE_STRIP_ROWS
    L = hs._lib.load()
    rng = np.random.default_rng(23)
    tail = "_async" if entry == "async" else ""
    for W, H in ((5, S + 1), (257, S + 1)):
        with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
            for frames in FORMATS:
                colour = frames.startswith("bgr")
                shape = (H, W, 3) if colour else (H, W)
                rowb = W * (3 if colour else 1)
                for extra_a, extra_b, off_a, off_b in ((1, 4, 1, 3), (4, 1, 3, 1)):
                    a, b = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
                    (ra, keep_a), (rb, keep_b) = strided_host(a, off_a, rowb + extra_a), strided_host(b, off_b, rowb + extra_b)
                    pa, pb = ctypes.c_void_p(ra.ctypes.data), ctypes.c_void_p(rb.ctypes.data)
                    assert pa.value % 2 == 1 and pb.value % 2 == 1
                    if colour:
                        st = getattr(L, "hsflow_set_frames_bgr8" + tail)(ctx._h, 0, pa, rowb + extra_a, pb, rowb + extra_b, int(frames == "bgr_blur"))
                    else:
                        st = getattr(L, "hsflow_set_frames_gray8_blur" + tail)(ctx._h, 0, pa, rowb + extra_a, pb, rowb + extra_b)
                    assert st == 0, (W, frames, st)
                    ctx.synchronize()   # the asynchronous forms own keep_a / keep_b until here
                    fa, fb = ctx.frames()
                    tag = (W, H, frames, extra_a, extra_b)
                    assert np.array_equal(fa, oracle_pre(oracle, a, frames)) and np.array_equal(fb, oracle_pre(oracle, b, frames)), tag
                    del keep_a, keep_b


@pytest.mark.parametrize("frames", ["bgr_blur", "gray_blur"])
def test_staging_reused_in_stream_order(hs, oracle, gpu_ok, frames):
    """One slot, so every pair goes through the same two staging areas: three different host pairs submitted one after
    the other without a wait of the test's own (the pipeline itself waits for the slot's last job in every submit), then
    three more with the slot's frames read after each.  Every flow is bit for bit that of a plain context given the
    oracle's planes, every frames() the oracle's.  Reuse with the earlier launch still in flight: the next test."""
    W, H = 264, 96
    rng = np.random.default_rng(31)
    shape = (H, W, 3) if frames.startswith("bgr") else (H, W)
    pairs = [(rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)) for _ in range(3)]
    crit = dict(lam=0.2, max_iter=40, epsilon=EPS6, term_type=ITER | EPS)
    want = []
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for a, b in pairs:
            oa, ob = oracle_pre(oracle, a, frames), oracle_pre(oracle, b, frames)
            ctx.set_frames(oa, ob)
            ctx.solve(**crit)
            want.append((oa, ob) + ctx.flow())
    with hs.PairPipeline(W, H, depth=1) as pl:
        out = [(np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)) for _ in range(6)]
        tickets = [pl.submit(a, b, out[k][0], out[k][1], frames=frames, **crit) for k, (a, b) in enumerate(pairs)]
        fa, fb = pl.frames(tickets[2])
        assert np.array_equal(fa, want[2][0]) and np.array_equal(fb, want[2][1])
        for k, (a, b) in enumerate(pairs):
            t = pl.submit(a, b, out[3 + k][0], out[3 + k][1], frames=frames, **crit)
            fa, fb = pl.frames(t)
            assert np.array_equal(fa, want[k][0]) and np.array_equal(fb, want[k][1]), k
        pl.drain()
    for k in range(6):
        assert np.array_equal(out[k][0], want[k % 3][2]) and np.array_equal(out[k][1], want[k % 3][3]), k


def test_staging_reused_while_the_earlier_pair_is_in_flight(hs, oracle, gpu_ok):
    """Two hsflow_set_frames_*_async calls on one context with nothing waited for in between, a 1080p BGR pair and then a
    gray pair: the second pair's uploads land in the areas the first pair's launches read, behind them in stream order."""
    W, H = 1920, 1080
    L = hs._lib.load()
    rng = np.random.default_rng(43)
    a, b = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    g, h = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        ctx.set_frames_bgr(a, b, pair=1)   # (the staging has its size: nothing below waits to grow it)
        assert L.hsflow_set_frames_bgr8_async(ctx._h, 0, ptr(a), 3 * W, ptr(b), 3 * W, 1) == 0
        assert L.hsflow_set_frames_gray8_blur_async(ctx._h, 1, ptr(g), W, ptr(h), W) == 0
        ctx.synchronize()
        fa, fb = ctx.frames(pair=0)
        ga, gb = ctx.frames(pair=1)
    assert np.array_equal(fa, oracle_pre(oracle, a, "bgr_blur")) and np.array_equal(fb, oracle_pre(oracle, b, "bgr_blur"))
    assert np.array_equal(ga, oracle.box_blur3(g)) and np.array_equal(gb, oracle.box_blur3(h))


def test_staging_shared_with_the_derivative_read_back(hs, oracle, gpu_ok):
    """Frame staging and hsflow_get_derivatives use one grow-only buffer: the read-back grows it between two uploads."""
    W, H = 260, 17
    rng = np.random.default_rng(37)
    a, b = rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    g, h = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
    crit = dict(lam=0.2, max_iter=8, term_type=ITER)
    with hs.HSFlow(W, H, 1, own_stream=True) as fresh:
        fresh.set_frames(oracle_pre(oracle, a, "bgr_blur"), oracle_pre(oracle, b, "bgr_blur"))
        fresh.solve(**crit)
        want = fresh.derivatives()
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames_bgr(a, b)
        ctx.solve(**crit)
        got = ctx.derivatives()
        ctx.set_frames_gray_blur(g, h)
        fa, fb = ctx.frames()
    assert np.array_equal(fa, oracle.box_blur3(g)) and np.array_equal(fb, oracle.box_blur3(h))
    for x, y in zip(got, want):
        assert np.array_equal(x, y)


def test_push_from_host_where_every_column_is_a_border_column(hs, oracle, gpu_ok):
    W, H = 5, 3
    rng = np.random.default_rng(41)
    a, b = rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W), dtype=np.uint8)
    bgr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames_gray_blur(a, b)
        ctx.push_frame_ex(bgr, "bgr_blur", reblur_prev=True)
        fa, fb = ctx.frames()
    assert np.array_equal(fa, oracle.box_blur3(oracle.box_blur3(b))) and np.array_equal(fb, oracle.box_blur3(oracle.bgr2gray(bgr)))


def test_pair_isolation(hs, oracle, gpu_ok):
    """Three pairs in one context, pair 1 set from device memory: its planes hold the oracle's bytes, 0 and 2 keep theirs."""
    S = hs.PRE_STRIP_ROWS
    W, H = 261, 2 * S + 3
    rng = np.random.default_rng(5)
    keep = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(6)]
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        for i in range(3):
            ctx.set_frames(keep[2 * i], keep[2 * i + 1], pair=i)
        for frames in FORMATS:
            shape = (H, W, 3) if frames.startswith("bgr") else (H, W)
            a, b = rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)
            rowb = int(np.prod(shape[1:]))
            da, db = strided_device(a, 0, rowb + 3), strided_device(b, 2, rowb)
            ctx.set_frames_device(da, db, frames=frames, pair=1)
            fa, fb = ctx.frames(pair=1)
            assert np.array_equal(fa, oracle_pre(oracle, a, frames)) and np.array_equal(fb, oracle_pre(oracle, b, frames)), frames
            for i in (0, 2):
                ga, gb = ctx.frames(pair=i)
                assert np.array_equal(ga, keep[2 * i]) and np.array_equal(gb, keep[2 * i + 1]), (frames, i)


def camera_frames():
    from opticalflowhs_amd import synth
    return [synth.translating_pair(160, 96, seed=77, dx=1.5 * i, dy=-0.75 * i)[0] for i in range(4)]


@pytest.mark.parametrize("where", ["numpy", "cuda"])
def test_camera_sequence(hs, oracle, gpu_ok, where):
    """The reference's loop (OpticalFlowOpenCV.cpp:92-93,118): old = blur(blur(.)) from the second pair on.  After every
    push the planes are the oracle loop's, and the flow is bit for bit that of a fresh context given those planes."""
    import torch
    W, H = 160, 96
    frames = camera_frames()
    crit = dict(lam=0.1, max_iter=12, epsilon=EPS6, term_type=ITER | EPS)

    held = []   # device frames stay alive: a push from device memory is only enqueued

    def give(f):
        if where != "cuda":
            return f
        held.append(torch.from_numpy(f).cuda())
        torch.cuda.synchronize()   # the context works on a stream of its own
        return held[-1]

    with hs.HSFlow(W, H, 1, own_stream=True) as ctx, hs.HSFlow(W, H, 1, own_stream=True) as fresh:
        old = frames[0]
        for i in range(1, 4):
            old_b, new_b = oracle.box_blur3(old), oracle.box_blur3(frames[i])
            if i == 1:
                ctx.set_frames_gray_blur(frames[0], frames[1])
            else:
                nxt = give(frames[i])
                ctx.push_frame_ex(nxt, "gray_blur", reblur_prev=True)
                with pytest.raises(hs.HsflowError) as e:   # frames were pushed since the last solve
                    ctx.verify()
                assert e.value.status == hs._lib.E_STATE
            a, b = ctx.frames()
            assert np.array_equal(a, old_b) and np.array_equal(b, new_b), i
            info = ctx.solve(**crit)
            u, v = ctx.flow()
            fresh.set_frames(old_b, new_b)
            want = fresh.solve(**crit)
            uf, vf = fresh.flow()
            assert np.array_equal(u, uf) and np.array_equal(v, vf) and info["iterations_done"] == want["iterations_done"], i
            assert ctx.verify().ok == 1
            old = new_b                                   # already blurred; blurred again next time round
        # reblur_prev = False: the old frame is blurred once
        ctx.push_frame_ex(give(frames[0]), "gray_blur", reblur_prev=False)
        a, b = ctx.frames()
        assert np.array_equal(a, oracle.box_blur3(frames[3])) and np.array_equal(b, oracle.box_blur3(frames[0]))
        # plain gray, with and without the re-blur; and a colour frame
        ctx.push_frame_ex(give(frames[1]), "gray", reblur_prev=True)
        a, b = ctx.frames()
        assert np.array_equal(a, oracle.box_blur3(oracle.box_blur3(frames[0]))) and np.array_equal(b, frames[1])
        ctx.push_frame_ex(give(frames[2]), "gray")
        a, b = ctx.frames()
        assert np.array_equal(a, frames[1]) and np.array_equal(b, frames[2])
        bgr = np.random.default_rng(8).integers(0, 256, (H, W, 3), dtype=np.uint8)
        ctx.push_frame_ex(give(bgr), "bgr_blur", reblur_prev=True)
        a, b = ctx.frames()
        assert np.array_equal(a, oracle.box_blur3(frames[2])) and np.array_equal(b, oracle.box_blur3(oracle.bgr2gray(bgr)))


def test_push_call_order_and_arguments(hs, oracle, gpu_ok):
    W, H = 160, 96
    frames = camera_frames()
    L = hs._lib.load()
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        with pytest.raises(hs.HsflowError) as e:          # nothing to become the previous frame
            ctx.push_frame_ex(frames[0], "gray_blur", reblur_prev=True)
        assert e.value.status == hs._lib.E_STATE
        ctx.set_frames_gray_blur(frames[0], frames[1])
        p = ctypes.c_void_p(frames[2].ctypes.data)
        assert L.hsflow_push_frame_ex(ctx._h, 0, 1, None, W, 1) == hs._lib.E_ARG
        assert L.hsflow_push_frame_ex(ctx._h, 0, 7, p, W, 1) == hs._lib.E_ARG
        assert L.hsflow_push_frame_ex(ctx._h, 0, 1, p, W, 2) == hs._lib.E_ARG
        assert L.hsflow_push_frame_ex(ctx._h, 0, 1, p, W - 1, 1) == hs._lib.E_SIZE
        assert L.hsflow_push_frame_ex(ctx._h, 0, 3, p, 3 * W - 1, 1) == hs._lib.E_SIZE
        assert L.hsflow_push_frame_device_ex(ctx._h, 0, 1, None, W, 0) == hs._lib.E_ARG
        assert L.hsflow_set_frames_device_ex(ctx._h, 0, 4, p, W, p, W) == hs._lib.E_ARG
        assert L.hsflow_set_frames_device_ex(ctx._h, 0, 1, p, W, None, W) == hs._lib.E_ARG
        assert L.hsflow_set_frames_device_ex(ctx._h, 0, 2, p, 3 * W - 1, p, 3 * W) == hs._lib.E_SIZE
        a, b = ctx.frames()                                # the refusals changed nothing
        assert np.array_equal(a, oracle.box_blur3(frames[0])) and np.array_equal(b, oracle.box_blur3(frames[1]))


def test_push_settles_an_owed_check_first(hs, oracle, gpu_ok):
    """solve_async under ITER|EPS on a pair of equal frames: the early stop fires at sweep 1, which only the owed check finds
    out -- by solving again from the frames.  A push in between must settle that check BEFORE it replaces them."""
    W, H = 160, 96
    frames = camera_frames()
    crit = dict(lam=0.1, max_iter=12, epsilon=EPS6, term_type=ITER | EPS)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames_gray_blur(frames[0], frames[0])
        want = ctx.solve(**crit)
        assert want["iterations_done"] == 1 and want["eps_rerun"] == 1
        ctx.set_frames_gray_blur(frames[0], frames[0])
        ctx.solve_async(**crit)
        ctx.push_frame_ex(frames[1], "gray_blur", reblur_prev=True)
        got = ctx.info()
        assert got["iterations_done"] == 1 and got["eps_rerun"] == 1, got
        u, v = ctx.flow()
        assert not u.any() and not v.any()
        a, b = ctx.frames()
        assert np.array_equal(a, oracle.box_blur3(oracle.box_blur3(frames[0]))) and np.array_equal(b, oracle.box_blur3(frames[1]))


def clean(r):
    return r.ok == 1 and r.iterations_ref == r.iterations_done and r.u.failing == 0 and r.v.failing == 0 and r.deriv_differing == 0


@pytest.mark.parametrize("depth,lanes,frames", [(3, 3, "bgr_blur"), (4, 2, "gray_blur")])
def test_pipeline_submit_device_formats(hs, oracle, gpu_ok, depth, lanes, frames):
    """Seven resident pairs through hsflow_pipeline_submit_device_ex (every slot reused; with three lanes the pipeline's own
    launch shape): flow bit-equal to the host-buffer submit of the same pixels on a pipeline of the same shape, the slot's
    frames the oracle's, verify clean; pair 3 has equal frames and stops at sweep 1 like on a plain context."""
    import torch
    W, H, n = 264, 96, 7
    colour = frames.startswith("bgr")
    rng = np.random.default_rng(depth)
    shape = (H, W, 3) if colour else (H, W)
    pairs = [(rng.integers(0, 256, shape, dtype=np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)) for _ in range(n)]
    pairs[3] = (pairs[3][0], pairs[3][0].copy())
    crit = dict(lam=0.2, max_iter=40, epsilon=EPS6, term_type=ITER | EPS)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        host_route(ctx, pairs[3][0], pairs[3][1], frames)
        plain = ctx.solve(**crit)
    assert plain["iterations_done"] == 1
    ref = []
    with hs.PairPipeline(W, H, depth=depth, lanes=lanes) as pl:
        for a, b in pairs:
            u, v = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
            t = pl.submit(np.ascontiguousarray(a), np.ascontiguousarray(b), u, v, frames=frames, **crit)
            ref.append((u, v, t))
        pl.drain()
    rowb = W * (3 if colour else 1)
    dev = [(strided_device(a, k % 4, rowb + (k % 3)), strided_device(b, 0, rowb)) for k, (a, b) in enumerate(pairs)]
    torch.cuda.synchronize()
    p = hs.make_params(**crit)
    with hs.PairPipeline(W, H, depth=depth, lanes=lanes) as pl:
        tickets = [pl.submit_device(dev[k][0], dev[k][1], params=p, frames=frames) if k < depth else None for k in range(n)]
        for k in range(n):   # pair k is asked for while pairs k+1 .. k+depth-1 are in flight
            u, v = pl.flow_device(tickets[k])
            assert np.array_equal(u.cpu().numpy(), ref[k][0]) and np.array_equal(v.cpu().numpy(), ref[k][1]), k
            fa, fb = pl.frames(tickets[k])
            assert np.array_equal(fa, oracle_pre(oracle, pairs[k][0], frames)) and np.array_equal(fb, oracle_pre(oracle, pairs[k][1], frames)), k
            assert clean(pl.verify(tickets[k])), k
            info = pl.info(tickets[k])
            if k == 3:
                assert info["iterations_done"] == plain["iterations_done"] and info["eps_rerun"] == 1, info
                assert not u.any() and not v.any()
            else:
                assert info["iterations_done"] > 1, (k, info)
            if k + depth < n:
                tickets[k + depth] = pl.submit_device(dev[k + depth][0], dev[k + depth][1], params=p, frames=frames)
        pl.drain()
        assert pl.copies_elided() == 0   # nothing was read in place: every pair went through the pre-processing launch
        with pytest.raises(ValueError):
            pl.submit_device(dev[0][0][:, :, 0] if colour else dev[0][0][:, :-1], dev[0][1], params=p, frames=frames)


def test_gray_submissions_still_ride_in_the_first_launch(hs, gpu_ok):
    """frames="gray" is hsflow_pipeline_submit_device as before, the in-place read included: it counts in copies_elided();
    a pre-processed format never does."""
    import torch
    from opticalflowhs_amd import synth
    W, H = 600, 480
    A, B = synth.translating_pair(W, H, seed=1)
    da, db = torch.from_numpy(A).cuda(), torch.from_numpy(B).cuda()
    torch.cuda.synchronize()
    p = hs.make_params(lam=1.0, max_iter=40, term_type=ITER | EPS, epsilon=EPS6, use_graph=True)
    with hs.PairPipeline(W, H, depth=4, lanes=4) as pl:
        pl.submit_device(da, db, params=p)
        pl.submit_device(da, db, params=p, frames="gray")
        t = pl.submit_device(da, db, params=p, frames="gray_blur")
        pl.wait(t)
        pl.drain()
        assert pl.copies_elided() == 2


def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + np.ascontiguousarray(img, dtype=np.uint8).tobytes())


def read_ppm(path):
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P6"
        w, h = (int(x) for x in f.readline().split())
        assert f.readline().strip() == b"255"
        return np.frombuffer(f.read(), np.uint8).reshape(h, w, 3)


def test_cli_camera_route_writes_the_oracle_loops_pictures(hs, oracle, gpu_ok, tmp_path):
    """`-cv -cam` on four PGM frames: flow_%04d.ppm byte for byte what the oracle run through the reference's loop draws."""
    import refpics
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    frames = camera_frames()
    cam, out = tmp_path / "cam", tmp_path / "out"
    cam.mkdir()
    out.mkdir()
    for i, f in enumerate(frames):
        write_pgm(str(cam / ("frame_%04d.pgm" % i)), f)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               HSFLOW_CAMERA_DIR=str(cam), HSFLOW_CAMERA_OUT=str(out))
    for name in ("HSFLOW_RENDER_DEVICE", "HSFLOW_VERIFY"):
        env.pop(name, None)
    r = subprocess.run([cli, "-cv", "-cam", ".1", "12"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Avg time" in r.stdout, r.stdout + r.stderr
    old = frames[0]
    for i in range(1, len(frames)):
        old_b, new_b = oracle.box_blur3(old), oracle.box_blur3(frames[i])
        u, v = oracle.calc_optical_flow_hs(old_b, new_b, 0.1, 12, EPS6, ITER | EPS)
        assert np.array_equal(read_ppm(str(out / ("flow_%04d.ppm" % i))), refpics.render(u, v)), i
        old = new_b
    assert not (out / ("flow_%04d.ppm" % len(frames))).exists()

