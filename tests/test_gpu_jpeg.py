"""The JPEG encoder on the GPU (include/hsflow.h: hsflow_jpeg_encode_device, hsflow_render_flow_jpeg[_device],
hsflow_pipeline_render_jpeg; kernels in opticalflowhs_amd/csrc/hs_kernels_jpeg.hip.h) against the host rule
(hsflow_jpeg_encode_host), which tests/test_jpeg_host.py pins to the CLI's writer, to libjpeg and to the reference's own
files.  Files are compared as bytes: every one of them."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import jpeg_pictures
import refpics
from conftest import GOLDEN, ROOT
from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))
OK, E_ARG, E_SIZE, E_STATE = 0, 1, 2, 5


def device_picture(arr, odd):
    """arr on the device: packed rows (odd = False), or rows 3 W + 5 bytes apart from a base 1 byte off the allocation's
    (odd = True: nothing is aligned, the byte-wise read path).  Returns (tensor view, the allocation)."""
    import torch
    H, W = arr.shape[:2]
    if not odd:
        t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        return t, t
    stride = 3 * W + 5
    buf = torch.full((H * stride + 8,), 0x3C, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, (H, W, 3), (stride, 3, 1), storage_offset=1)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)).cuda())
    assert view.data_ptr() % 4 == 1 or view.data_ptr() % 2 == 1
    return view, buf


def stuffed_after_header(data):
    return data[623:].count(b"\xff\x00")


# ---- 1. device against host -------------------------------------------------------------------------------------------

SIZES = [(1, 1), (7, 9), (8, 8), (9, 7), (16, 16), (17, 15), (24, 40), (33, 17), (64, 48), (150, 70)]


@pytest.mark.parametrize("W,H", SIZES)
def test_device_equals_host_rule(hs, gpu_ok, W, H):
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        for kind in ("noise", "arrows"):
            arr = jpeg_pictures.picture(kind, W, H, 7 * W + H)
            for quality in (100, 95, 10):
                want = hs.encode_jpeg(arr, quality)
                assert len(want) <= hs.jpeg_bound(W, H)
                if (W, H, kind, quality) == (64, 48, "noise", 100):
                    n = stuffed_after_header(want)
                    print("64x48 noise at 100: %d stuffed FF 00 behind the header, %d bytes" % (n, len(want)))
                    assert n >= 1          # the stuffing pass cannot go untested
                for odd in (False, True):
                    t, keep = device_picture(arr, odd)
                    got = ctx.encode_jpeg(t, quality)
                    assert got == want, (W, H, kind, quality, odd, len(got), len(want))
                    del t, keep


# ---- 2. more than one scan tile ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,kind", [(600, 480, "noise"), (1920, 1080, "arrows")])
def test_large_pictures_and_repeat(hs, gpu_ok, W, H, kind):
    arr = jpeg_pictures.picture(kind, W, H, 3)
    other = jpeg_pictures.picture("arrows" if kind == "noise" else "constant", W, H, 4)
    want, want_other = hs.encode_jpeg(arr, 95), hs.encode_jpeg(other, 95)
    assert 6 * -(-W // 16) * -(-H // 16) > 4096          # more than one tile of the blocks' scan
    print("%dx%d %s: %d bytes, %d stuffed" % (W, H, kind, len(want), stuffed_after_header(want)))
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        t, _ = device_picture(arr, False)
        o, _ = device_picture(other, False)
        first = ctx.encode_jpeg(t, 95)
        assert first == want, (len(first), len(want))
        assert ctx.encode_jpeg(t, 95) == first             # the same bytes on every run
        assert ctx.encode_jpeg(o, 95) == want_other        # a shorter stream over the scratch of a longer one, and back
        assert ctx.encode_jpeg(t, 95) == want


# ---- 3. capacity on the device ----------------------------------------------------------------------------------------

def test_capacity_on_the_device(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H = 64, 48
    arr = jpeg_pictures.picture("noise", W, H, 11)
    want = hs.encode_jpeg(arr, 100)
    size, bound = len(want), hs.jpeg_bound(W, H)
    t, _ = device_picture(arr, False)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        for cap in (size - 1, size, 700, 100, bound):
            out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            n = torch.zeros(1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            assert L.hsflow_jpeg_encode_device(ctx._h, ctypes.c_void_p(t.data_ptr()), 3 * W, 100, ctypes.c_void_p(out.data_ptr()), cap,
                                               ctypes.c_void_p(n.data_ptr())) == OK
            ctx.synchronize()
            host = out.cpu().numpy()
            assert int(n.item()) == size, (cap, int(n.item()), size)           # the size needed, whatever the capacity
            assert (host[cap:] == 0xA5).all(), cap                             # the guard behind the capacity keeps its fill
            k = min(cap, size)
            assert host[:k].tobytes() == want[:k], cap
        # argument errors of the device form
        out = torch.zeros(bound + 8, dtype=torch.uint8, device="cuda")
        n = torch.zeros(2, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        f, tp, op, sp = L.hsflow_jpeg_encode_device, ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(n.data_ptr())
        assert f(ctx._h, tp, 3 * W, 0, op, bound, sp) == E_ARG and f(ctx._h, tp, 3 * W, 101, op, bound, sp) == E_ARG
        assert f(ctx._h, None, 3 * W, 95, op, bound, sp) == E_ARG and f(ctx._h, tp, 3 * W, 95, None, bound, sp) == E_ARG
        assert f(ctx._h, tp, 3 * W, 95, op, bound, None) == E_ARG
        assert f(ctx._h, tp, 3 * W, 95, op, bound, ctypes.c_void_p(n.data_ptr() + 4)) == E_ARG          # not 8-byte aligned
        assert f(ctx._h, tp, 3 * W - 1, 95, op, bound, sp) == E_SIZE and b"stride" in L.hsflow_last_error(ctx._h)
        assert b"picture 0" not in L.hsflow_last_error(ctx._h) and b"file 0" not in L.hsflow_last_error(ctx._h)
        rp = hs.make_render_params("cv")
        host = np.zeros(bound, np.uint8)
        hn = ctypes.c_size_t()
        g, hp = L.hsflow_render_flow_jpeg, ctypes.c_void_p(host.ctypes.data)
        assert g(ctx._h, 0, ctypes.byref(rp), 95, hp, bound, ctypes.byref(hn)) == OK and hn.value > 625
        need = hn.value
        assert g(ctx._h, 0, ctypes.byref(rp), 95, hp, need - 1, ctypes.byref(hn)) == E_SIZE and hn.value == need
        msg = L.hsflow_last_error(ctx._h)
        assert b"smaller than the file" in msg and b"picture 0" not in msg and b"file 0" not in msg, msg
        assert g(ctx._h, 0, ctypes.byref(rp), 95, hp, need, ctypes.byref(hn)) == OK and hn.value == need
        assert g(ctx._h, 0, ctypes.byref(rp), 0, hp, bound, ctypes.byref(hn)) == E_ARG
        assert g(ctx._h, 1, ctypes.byref(rp), 95, hp, bound, ctypes.byref(hn)) == E_ARG                  # bad pair
        assert g(ctx._h, 0, None, 95, hp, bound, ctypes.byref(hn)) == E_ARG
        assert g(ctx._h, 0, ctypes.byref(rp), 95, None, bound, ctypes.byref(hn)) == E_ARG
        rp.struct_size -= 4
        assert g(ctx._h, 0, ctypes.byref(rp), 95, hp, bound, ctypes.byref(hn)) == E_ARG
        with pytest.raises(ValueError):
            ctx.encode_jpeg(arr)                                                                           # a host array


# ---- 4. end to end on the reference's pairs ---------------------------------------------------------------------------

def solved_reference_pair(hs, ctx, name, route):
    """The solve behind the reference's pictures (refpics: lambda 0.1 / alpha 15 as shipped, 10 sweeps, blur for cv)."""
    A, B = refpics.gray_pair(name)
    if route == "cv":
        ctx.set_frames_gray_blur(A, B)
        ctx.solve(lam=refpics.LAMBDA, max_iter=refpics.ITERATIONS, epsilon=refpics.EPSILON, term_type=ITER | EPS)
    else:
        ctx.set_frames(A, B)
        ctx.solve(mode=hs.MODE_CLASSIC_AS_SHIPPED, alpha=refpics.ALPHA, max_iter=refpics.ITERATIONS, term_type=ITER)


def view_pointers(hs, ctx):
    pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    assert hs._lib.load().hsflow_flow_view_device(ctx._h, 0, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == OK
    return pu.value, pv.value, sb.value


@pytest.mark.parametrize("route", ["cv", "cl"])
@pytest.mark.parametrize("name", ["city", "bunny"])
def test_reference_files_end_to_end(hs, gpu_ok, name, route):
    H, W = refpics.gray_pair(name)[0].shape
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        solved_reference_pair(hs, ctx, name, route)
        before, info = view_pointers(hs, ctx), ctx.info()
        u0, v0 = ctx.flow()
        data = ctx.render_jpeg(route)
        assert view_pointers(hs, ctx) == before and ctx.info() == info
        u1, v1 = ctx.flow()
        assert np.array_equal(u0, u1) and np.array_equal(v0, v1)
        assert data == hs.encode_jpeg(ctx.render(route), 95)
    assert data == open(os.path.join(GOLDEN, "ref_%s_%s_out.jpg" % (name, route)), "rb").read()


# ---- 5. pipeline ------------------------------------------------------------------------------------------------------

def _patch_pair(W, H):
    """A flat frame with a patch one grey level brighter: with lambda 1e-3 / epsilon 1e-4 its early stop fires
    (tests/test_gpu_pipeline_lanes.py builds the same)."""
    a = np.full((H, W), 90, np.uint8)
    b = a.copy()
    rows, cols = slice(H // 4, H // 4 + min(80, H // 2)), slice(W // 5, W // 5 + min(300, W // 2))
    a[rows, cols], b[rows, cols] = 120, 121
    return a, b


def test_pipeline_render_jpeg(hs, gpu_ok):
    import torch
    W, H, depth = 600, 480, 3
    P1 = dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6)
    P3 = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)
    rkw = dict(threshold=0.02, scale=6.0)
    pairs = {"t1": (synth.translating_pair(W, H, seed=1), P1), "patch": (_patch_pair(W, H), P3)}
    want = {}
    for k, ((A, B), kw) in pairs.items():
        with hs.HSFlow(W, H, own_stream=True) as ctx:       # the synchronous solve: for the patch pair the re-solved flow
            ctx.set_frames(A, B)
            info = ctx.solve(**kw)
            picture = ctx.render("cv", **rkw)
        if k == "patch":
            assert 1 < info["iterations_done"] < 400, info      # its early stop fires
        assert (picture != 0).any(), k
        want[k] = hs.encode_jpeg(picture, 95)
    dev = {k: tuple(torch.from_numpy(f).cuda() for f in AB) for k, (AB, _) in pairs.items()}
    torch.cuda.synchronize()
    order = ["t1", "patch", "t1", "t1", "patch"]
    with hs.PairPipeline(W, H, depth=depth, lanes=2) as pl:

        def check_ticket(t):
            got = pl.render_jpeg(t, "cv", **rkw)
            assert got == hs.encode_jpeg(pl.render(t, "cv", **rkw), 95), t       # the host rule applied to render(ticket)
            assert got == want[order[t]], (t, order[t])
            if order[t] == "patch":
                assert pl.info(t)["eps_rerun"] == 1                             # re-solved before it was drawn and encoded

        for t, k in enumerate(order):
            if t >= depth:
                check_ticket(t - depth)                                          # the oldest pair, before its slot is taken again
            assert pl.submit_device(dev[k][0], dev[k][1], **pairs[k][1]) == t
        for t in range(len(order) - depth, len(order)):
            check_ticket(t)
        with pytest.raises(hs.HsflowError) as e:
            pl.render_jpeg(0, "cv")                                              # its slot has been reused since
        assert e.value.status == E_STATE
        with pytest.raises(hs.HsflowError) as e:
            pl.render_jpeg(len(order), "cv")                                     # never issued
        assert e.value.status == E_ARG
        check_ticket(len(order) - 1)                                             # the pipeline still works
        # host buffers: upload -> solve -> download, then the file of the slot's flow
        (A, B), kw = pairs["t1"]
        bufs = [hs.pinned_empty((H, W), np.uint8) for _ in range(2)] + [hs.pinned_empty((H, W), np.float32) for _ in range(2)]
        bufs[0][:], bufs[1][:] = A, B
        t = pl.submit(bufs[0], bufs[1], bufs[2], bufs[3], **kw)
        assert pl.render_jpeg(t, "cv", **rkw) == want["t1"]
        assert pl.render_jpeg(t, "cv", quality=40, **rkw) == hs.encode_jpeg(pl.render(t, "cv", **rkw), 40)


# ---- 6. command line --------------------------------------------------------------------------------------------------

def _cli(args, extra_env=None):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    env.pop("HSFLOW_RENDER_DEVICE", None)
    env.pop("HSFLOW_JPEG_DEVICE", None)
    env.update(extra_env or {})
    r = subprocess.run([cli] + args, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_cli_writes_the_reference_files_from_the_device(hs, gpu_ok, tmp_path):
    """HSFLOW_RENDER_DEVICE=1 HSFLOW_JPEG_DEVICE=1: the reference's command lines on its own JPEG inputs write its own
    output files, byte for byte, and the file's bytes come from the device."""
    a, b = os.path.join(GOLDEN, "ref_city_1.jpg"), os.path.join(GOLDEN, "ref_city_2.jpg")
    out = str(tmp_path / "out.jpg")
    on = {"HSFLOW_RENDER_DEVICE": "1", "HSFLOW_JPEG_DEVICE": "1"}
    _cli(["-cv", "-hd", a, b, out, ".1", "10"], on)
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "ref_city_cv_out.jpg"), "rb").read()
    os.remove(out)
    _cli(["-cl", "-hd", a, b, out, "15", "10", "1", "GPU"], dict(on, HSFLOW_CL_AS_SHIPPED="1"))
    assert open(out, "rb").read() == open(os.path.join(GOLDEN, "ref_city_cl_out.jpg"), "rb").read()
    # another extension: the switch changes nothing
    ppm = str(tmp_path / "out.ppm")
    _cli(["-cv", "-hd", a, b, ppm, ".1", "10"], on)
    assert open(ppm, "rb").read()[:2] == b"P6"


# ---- 7. async-reduce context ------------------------------------------------------------------------------------------

def _view(hs, ctx, W, H):
    import torch
    from opticalflowhs_amd.pipeline import _DeviceView
    pu, pv, sb = view_pointers(hs, ctx)
    return tuple(torch.as_tensor(_DeviceView(p, (H, W), (sb, 4)), device="cuda") for p in (pu, pv))


def test_render_jpeg_behind_an_asynchronous_solve(hs, gpu_ok):
    """solve_async (ITER|EPS) and render_jpeg with no call in between, on an async-reduce context: the file of the
    synchronous solve.  The work counts as work behind the solve's marker, as a render does: hsflow_wait_solve and
    hsflow_flow_view_device return only when it is through, and the flow planes are what they were."""
    import torch
    L = hs._lib.load()
    W, H = 1920, 1080
    A, B = synth.translating_pair(W, H, seed=1, dx=3.0, dy=-2.0)
    kw = dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6)
    rkw = dict(threshold=0.05, scale=4.0)
    rp = hs.make_render_params("cv", **rkw)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with hs.HSFlow(W, H, 1, stream=s.cuda_stream) as ctx:
        assert L.hsflow_set_async_reduce(ctx._h, 1) == OK
        ctx.set_frames(A, B)
        ctx.solve(**kw)
        picture = ctx.render("cv", **rkw)
        assert (picture != 0).any()
        want = hs.encode_jpeg(picture, 95)
        before = tuple(t.clone() for t in _view(hs, ctx, W, H))
        torch.cuda.synchronize()
        # host form right behind the asynchronous solve
        ctx.solve_async(**kw)
        assert ctx.render_jpeg("cv", **rkw) == want
        assert L.hsflow_wait_solve(ctx._h) == OK
        uv = _view(hs, ctx, W, H)
        assert torch.equal(uv[0].clone(), before[0]) and torch.equal(uv[1].clone(), before[1])
        # device form: only enqueued; flow_view and wait_solve must wait for it, and the planes are unchanged
        out = torch.zeros(hs.jpeg_bound(W, H), dtype=torch.uint8, device="cuda")
        n = torch.zeros(1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def enqueue():
            for _ in range(4):
                assert L.hsflow_render_flow_jpeg_device(ctx._h, 0, ctypes.byref(rp), 95, ctypes.c_void_p(out.data_ptr()), out.numel(),
                                                        ctypes.c_void_p(n.data_ptr())) == OK

        ctx.solve_async(**kw)
        enqueue()
        uv = _view(hs, ctx, W, H)
        assert s.query(), "flow_view returned while an encode was still in flight"
        assert torch.equal(uv[0].clone(), before[0]) and torch.equal(uv[1].clone(), before[1])
        assert out[:int(n.item())].cpu().numpy().tobytes() == want
        ctx.solve_async(**kw)
        enqueue()
        assert L.hsflow_wait_solve(ctx._h) == OK
        assert s.query(), "wait_solve returned while an encode was still in flight"
        assert out[:int(n.item())].cpu().numpy().tobytes() == want


# ---- 8. the single entries and the batch maximum ------------------------------------------------------------------------

def test_single_entries_ignore_the_batch_maximum(hs, gpu_ok, monkeypatch):
    """A single picture is never cut into chunks: an unusable HSFLOW_JPEG_BATCH_MAX in the environment stops the batch
    entries (E_ARG, naming the variable) and nothing else."""
    import torch
    L = hs._lib.load()
    W, H = 17, 15
    ENV_MAX = "HSFLOW_JPEG_BATCH_MAX"
    arr = jpeg_pictures.picture("noise", W, H, 7 * W + H)
    rng = np.random.default_rng(17)
    u, v = (rng.uniform(-6, 6, (H, W)).astype(np.float32) for _ in range(2))
    drawn = refpics.render(u, v, "cv")
    assert (drawn != 0).any()
    want_pic, want_drawn = hs.encode_jpeg(arr, 95), hs.encode_jpeg(drawn, 95)
    bound = hs.jpeg_bound(W, H)
    rp = hs.make_render_params("cv")
    monkeypatch.setenv(ENV_MAX, "0")
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        ud, vd = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
        t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
        out = torch.full((2, bound), 0xA5, dtype=torch.uint8, device="cuda")
        n = torch.zeros(2, dtype=torch.int64, device="cuda")
        pic = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.set_flow_rows_from(ud, vd, 0, H)
        assert L.hsflow_jpeg_encode_device(ctx._h, ctypes.c_void_p(t.data_ptr()), 3 * W, 95, ctypes.c_void_p(out[0].data_ptr()), bound,
                                           ctypes.c_void_p(n.data_ptr())) == OK
        assert L.hsflow_render_flow_jpeg_device(ctx._h, 0, ctypes.byref(rp), 95, ctypes.c_void_p(out[1].data_ptr()), bound,
                                                ctypes.c_void_p(n.data_ptr() + 8)) == OK
        ctx.synchronize()
        sizes = n.cpu().tolist()
        assert out[0, :sizes[0]].cpu().numpy().tobytes() == want_pic and out[1, :sizes[1]].cpu().numpy().tobytes() == want_drawn
        assert ctx.render_jpeg("cv") == want_drawn                                   # hsflow_render_flow_jpeg
        assert np.array_equal(ctx.render("cv"), drawn)                               # hsflow_render_flow
        # the batch entries: stopped by the variable, before anything is enqueued
        src, dst = (ctypes.c_void_p * 1)(t.data_ptr()), (ctypes.c_void_p * 1)(out[0].data_ptr())
        words, pics = ctypes.c_void_p(n.data_ptr()), (ctypes.c_void_p * 1)(pic.data_ptr())
        host = np.zeros(bound, np.uint8)
        hp, hn = (ctypes.c_void_p * 1)(host.ctypes.data), (ctypes.c_size_t * 1)()
        for call in (lambda: L.hsflow_jpeg_encode_batch_device(ctx._h, src, 1, 3 * W, 95, dst, bound, words),
                     lambda: L.hsflow_render_flow_batch_device(ctx._h, 0, 1, ctypes.byref(rp), pics, 3 * W),
                     lambda: L.hsflow_render_flow_jpeg_batch_device(ctx._h, 0, 1, ctypes.byref(rp), 95, dst, bound, words),
                     lambda: L.hsflow_render_flow_jpeg_batch(ctx._h, 0, 1, ctypes.byref(rp), 95, hp, bound, hn)):
            assert call() == E_ARG
            assert ENV_MAX.encode() in L.hsflow_last_error(ctx._h)
