"""The JPEG decoder on the GPU (include/hsflow.h: hsflow_jpeg_decode[_device], hsflow_set_frames_jpeg,
hsflow_push_frame_jpeg; kernels in opticalflowhs_amd/csrc/hs_kernels_jpegd.hip.h) against the host rule
(hsflow_jpeg_decode_host), which tests/test_jpegd_host.py pins to PIL's pixels, to the CLI's reader and to the committed
gray planes.  Pictures are compared as bytes: every one of them."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest

import jpegd_cases as jc
import refpics
from conftest import GOLDEN, ROOT
from jpegd_cases import BGR, E_DATA, E_SIZE, OK, RGB
from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))
ENV = "HSFLOW_JPEGD_SUBSEQ_BITS"


@contextlib.contextmanager
def subseq_bits(S):
    old = os.environ.pop(ENV, None)
    if S:
        os.environ[ENV] = str(S)
    try:
        yield
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old


def host_pixels(hs, blob, order):
    return hs.jpeg_decode_host(blob, "rgb" if order == RGB else "bgr")


def decode_sync(hs, ctx, blob, order, pad=0, shift=0):
    """hsflow_jpeg_decode into host rows `pad` bytes longer than tight from a base `shift` bytes off: (status, rows)."""
    buf = np.frombuffer(blob, np.uint8)
    flat = np.full(ctx.height * (3 * ctx.width + pad) + 8, 0xA5, np.uint8)
    rows = np.lib.stride_tricks.as_strided(flat[shift:], (ctx.height, 3 * ctx.width + pad), (3 * ctx.width + pad, 1))
    st = ctx._lib.hsflow_jpeg_decode(ctx._h, ctypes.c_void_p(buf.ctypes.data), buf.size, order, ctypes.c_void_p(rows.ctypes.data), rows.strides[0])
    return st, rows, flat


def decode_device(hs, ctx, blob, order, pad=0, shift=0):
    """hsflow_jpeg_decode_device into a device buffer of 0xA5: (call status, status word, rows, everything)."""
    import torch
    buf = np.frombuffer(blob, np.uint8)
    stride = 3 * ctx.width + pad
    flat = torch.full((ctx.height * stride + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    word = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = ctx._lib.hsflow_jpeg_decode_device(ctx._h, ctypes.c_void_p(buf.ctypes.data), buf.size, order, ctypes.c_void_p(flat.data_ptr() + shift), stride,
                                            ctypes.c_void_p(word.data_ptr()))
    torch.cuda.synchronize()      # (not hsflow_synchronize: nothing of the context's state is to be touched)
    host = flat.cpu().numpy()
    rows = np.lib.stride_tricks.as_strided(host[shift:], (ctx.height, stride), (stride, 1))
    return st, int(word.item()), rows, host


# ---- 1. device against host -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", jc.names())
def test_device_equals_host_rule(hs, gpu_ok, name):
    blob = jc.data(name)
    want_rgb = jc.pil_pixels(name)
    H, W = want_rgb.shape[:2]
    rst = "rst" in name
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        for S in (32, 256, 0):
            with subseq_bits(S):
                assert jc.header(hs, blob)[1].subseq_bits == (0 if rst else (S or hs._lib.JPEGD_SUBSEQ_BITS))     # what runs
                for order in (RGB, BGR):
                    want = host_pixels(hs, blob, order).reshape(H, 3 * W)
                    assert np.array_equal(want.reshape(H, W, 3), want_rgb if order == RGB else want_rgb[:, :, ::-1])
                    for pad, shift in ((0, 0), (8, 0), (5, 1), (0, 3)):         # tight, padded words, nothing aligned, odd base
                        st, rows, flat = decode_sync(hs, ctx, blob, order, pad, shift)
                        assert st == OK, (name, S, order, pad, shift, ctx._lib.hsflow_last_error(ctx._h))
                        assert np.array_equal(rows[:, :3 * W], want), (name, S, order, pad, shift)
                        assert (rows[:, 3 * W:] == 0xA5).all() and (flat[:shift] == 0xA5).all() and (flat[shift + H * (3 * W + pad):] == 0xA5).all()
                    for pad, shift in ((0, 0), (5, 1)):                          # the device form, word and byte stores
                        st, word, rows, flat = decode_device(hs, ctx, blob, order, pad, shift)
                        assert st == OK and word == 0, (name, S, order, pad, shift, word)
                        assert np.array_equal(rows[:, :3 * W], want), (name, S, order, pad, shift, "device")
                        assert (rows[:-1, 3 * W:] == 0xA5).all() and (flat[:shift] == 0xA5).all() and (flat[shift + (H - 1) * (3 * W + pad) + 3 * W:] == 0xA5).all()
        assert np.array_equal(ctx.jpeg_decode(blob), want_rgb) and np.array_equal(ctx.jpeg_decode(blob, "bgr"), want_rgb[:, :, ::-1])


def test_many_groups_and_repair_rounds(hs, gpu_ok):
    """S = 32 cuts the 64x48 noise file into more subsequences than one workgroup holds: the hand-over between groups."""
    blob = jc.data("c64x48_420_q95_noise")
    _, info = jc.header(hs, blob)
    assert info.scan_bytes * 8 // 32 > 3 * 256
    with hs.HSFlow(64, 48, own_stream=True) as ctx:
        with subseq_bits(32):
            assert np.array_equal(ctx.jpeg_decode(blob), jc.pil_pixels("c64x48_420_q95_noise"))
        with subseq_bits(31):
            with pytest.raises(hs.HsflowError) as e:
                ctx.jpeg_decode(blob)
            assert e.value.status == 1
        with subseq_bits(8192):
            with pytest.raises(hs.HsflowError):
                ctx.jpeg_decode(blob)


@pytest.mark.parametrize("value", ["0", "99"])
def test_single_entries_ignore_the_batch_maximum(hs, gpu_ok, monkeypatch, value):
    """A single file is never cut into chunks: an unusable HSFLOW_JPEGD_BATCH_MAX in the environment stops the batch
    entry (E_ARG) and nothing else."""
    import torch
    name = "c17x9_420_q75_noise"
    blob = jc.data(name)
    W, H = 17, 9
    monkeypatch.setenv("HSFLOW_JPEGD_BATCH_MAX", value)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        for order in (RGB, BGR):
            want = host_pixels(hs, blob, order).reshape(H, 3 * W)
            st, rows, _ = decode_sync(hs, ctx, blob, order)
            assert st == OK and np.array_equal(rows, want), (order, ctx._lib.hsflow_last_error(ctx._h))
            st, word, rows, _ = decode_device(hs, ctx, blob, order)
            assert st == OK and word == 0 and np.array_equal(rows, want), order
        ctx.set_frames_jpeg(blob, blob, blur=False)
        gray = hs.preprocess_frame(hs.jpeg_decode_host(blob, "bgr"), "bgr")
        a, b = ctx.frames()
        assert np.array_equal(a, gray) and np.array_equal(b, gray)
        buf = np.frombuffer(blob, np.uint8)
        pic = torch.full((H, 3 * W), 0xA5, dtype=torch.uint8, device="cuda")
        word = torch.full((1,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        files, sizes, pix = (ctypes.c_void_p * 1)(buf.ctypes.data), (ctypes.c_size_t * 1)(buf.size), (ctypes.c_void_p * 1)(pic.data_ptr())
        assert ctx._lib.hsflow_jpeg_decode_batch_device(ctx._h, files, sizes, 1, RGB, pix, 3 * W, ctypes.c_void_p(word.data_ptr())) == jc.E_ARG
        assert b"HSFLOW_JPEGD_BATCH_MAX" in ctx._lib.hsflow_last_error(ctx._h)
        torch.cuda.synchronize()
        assert int(word.item()) == 77 and bool((pic == 0xA5).all().item())


# ---- 2. the reference's inputs ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pic", ["city", "bunny"])
def test_reference_inputs(hs, gpu_ok, pic):
    blobs = [jc.golden("ref_%s_%d.jpg" % (pic, k)) for k in (1, 2)]
    gray = [refpics.read_pgm(os.path.join(GOLDEN, "%s_%d_gray.pgm" % (pic, k))) for k in (1, 2)]
    H, W = gray[0].shape
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        for blob in blobs:
            assert np.array_equal(ctx.jpeg_decode(blob, "bgr"), hs.jpeg_decode_host(blob, "bgr"))
        ctx.set_frames_jpeg(blobs[0], blobs[1], blur=False)
        a, b = ctx.frames()
        assert np.array_equal(a, gray[0]) and np.array_equal(b, gray[1])
        ctx.set_frames_jpeg(blobs[0], blobs[1], blur=True)
        a, b = ctx.frames()
        assert np.array_equal(a, hs.preprocess_frame(gray[0], "gray_blur")) and np.array_equal(b, hs.preprocess_frame(gray[1], "gray_blur"))
        assert np.array_equal(a, hs.preprocess_frame(hs.jpeg_decode_host(blobs[0], "bgr"), "bgr_blur"))
        # end to end: the reference's own output file
        ctx.solve(lam=refpics.LAMBDA, max_iter=refpics.ITERATIONS, epsilon=refpics.EPSILON, term_type=ITER | EPS)
        assert ctx.render_jpeg("cv", 95) == jc.golden("ref_%s_cv_out.jpg" % pic)


def test_1080p_twice_over_the_scratch_of_a_longer_file(hs, gpu_ok):
    W, H = 1920, 1080
    A, _ = synth.translating_pair(W, H, seed=3)
    rng = np.random.default_rng(4)
    smooth = np.repeat(A[:, :, None], 3, axis=2)
    busy = smooth.copy()
    busy[::2, ::3, 1] = rng.integers(0, 256, size=busy[::2, ::3, 1].shape, dtype=np.uint8)
    short, longer = hs.encode_jpeg(smooth, 75), hs.encode_jpeg(busy, 95)
    assert len(longer) > len(short)
    want = hs.jpeg_decode_host(short)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        first = ctx.jpeg_decode(short)
        assert np.array_equal(ctx.jpeg_decode(longer), hs.jpeg_decode_host(longer))
        second = ctx.jpeg_decode(short)
        assert np.array_equal(first, want) and np.array_equal(second, want)


# ---- 3. broken streams ----------------------------------------------------------------------------------------------------

def no_index(ctx):
    """The single entries' messages name no position in a list."""
    msg = ctx._lib.hsflow_last_error(ctx._h)
    return b"file 0" not in msg and b"picture 0" not in msg

def test_broken_streams(hs, gpu_ok):
    name = "c64x48_420_q95_noise"
    blob = jc.data(name)
    off, n = jc.scan_range(hs, blob)
    cut = jc.cut_scan(hs, blob, n // 2)
    A, B = synth.translating_pair(64, 48, seed=2)
    with hs.HSFlow(64, 48, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        ctx.solve(lam=1.0, max_iter=30, term_type=ITER)
        u0, v0 = ctx.flow()
        for S in (32, 0):
            with subseq_bits(S):
                st, word, rows, flat = decode_device(hs, ctx, cut, RGB, 5, 1)
                assert st == OK and word == 2, (S, word)
                assert (rows[:-1, 192:] == 0xA5).all() and (flat[:1] == 0xA5).all() and (flat[1 + 47 * 197 + 192:] == 0xA5).all()
                st, rows, flat = decode_sync(hs, ctx, cut, RGB)
                assert st == E_DATA and (flat == 0xA5).all() and b"truncated" in ctx._lib.hsflow_last_error(ctx._h)
                assert no_index(ctx)
        with pytest.raises(hs.HsflowError) as e:
            ctx.set_frames_jpeg(blob, cut)
        assert e.value.status == E_DATA and no_index(ctx)
        with pytest.raises(hs.HsflowError) as e:
            ctx.set_frames_jpeg(blob[:off // 2], blob)
        assert e.value.status == E_DATA and no_index(ctx)
        with pytest.raises(hs.HsflowError) as e:
            ctx.push_frame_jpeg(cut)
        assert e.value.status == E_DATA and no_index(ctx)
        a, b = ctx.frames()
        assert np.array_equal(a, A) and np.array_equal(b, B)
        ctx.solve(lam=1.0, max_iter=30, term_type=ITER)
        u1, v1 = ctx.flow()
        assert np.array_equal(u0, u1) and np.array_equal(v0, v1)
        # a file with restart intervals, cut: its later intervals are missing
        with pytest.raises(hs.HsflowError) as e:
            ctx.jpeg_decode(jc.cut_scan(hs, jc.data("c64x48_444_q30_smooth_rst1"), 300))
        assert e.value.status == E_DATA
        # a picture of another size
        with pytest.raises(hs.HsflowError) as e:
            ctx.jpeg_decode(jc.data("c48x40_420_q95_noise_opt"))
        assert e.value.status == E_SIZE
        with pytest.raises(hs.HsflowError) as e:
            ctx.set_frames_jpeg(blob, jc.data("c48x40_420_q95_noise_opt"))
        assert e.value.status == E_SIZE
    bad = jc.run_past_63(hs, jc.data("g8x8_q75_smooth"))
    with hs.HSFlow(8, 8, own_stream=True) as ctx:
        st, word, rows, flat = decode_device(hs, ctx, bad, BGR)
        assert st == OK and word == 1
        assert (flat[8 * 24:] == 0xA5).all()
        st, rows, flat = decode_sync(hs, ctx, bad, BGR)
        assert st == E_DATA and (flat == 0xA5).all() and b"corrupt" in ctx._lib.hsflow_last_error(ctx._h) and no_index(ctx)
        assert np.array_equal(ctx.jpeg_decode(jc.data("g8x8_q75_smooth")), jc.pil_pixels("g8x8_q75_smooth"))     # and the context still decodes


# ---- 4. the camera sequence -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("reblur", [0, 1])
def test_push_frame_jpeg(hs, gpu_ok, reblur):
    W, H = 150, 70
    rng = np.random.default_rng(8)
    files = []
    for k in range(4):
        A, _ = synth.translating_pair(W, H, seed=10 + k)
        rgb = np.stack([A, np.roll(A, k, axis=1), 255 - A], axis=2)
        rgb[::5, ::7] = rng.integers(0, 256, size=rgb[::5, ::7].shape, dtype=np.uint8)
        files.append(hs.encode_jpeg(np.ascontiguousarray(rgb), 90))
    bgr = [hs.jpeg_decode_host(f, "bgr") for f in files]
    with hs.HSFlow(W, H, own_stream=True) as got, hs.HSFlow(W, H, own_stream=True) as want:
        got.set_frames_jpeg(files[0], files[1], blur=True)
        want.set_frames_bgr(bgr[0], bgr[1], blur=True)
        for k in (2, 3):
            got.push_frame_jpeg(files[k], blur=True, reblur_prev=bool(reblur))
            want.push_frame_ex(bgr[k], frames="bgr_blur", reblur_prev=bool(reblur))
            got.synchronize()
            for x, y in zip(got.frames(), want.frames()):
                assert np.array_equal(x, y), (k, reblur)
            i1 = got.solve(lam=1.0, max_iter=20, term_type=ITER)
            want.solve(lam=1.0, max_iter=20, term_type=ITER)
            for x, y in zip(got.flow(), want.flow()):
                assert np.array_equal(x, y), (k, reblur)
            assert i1["iterations_done"] == 20


# ---- 5. command line ----------------------------------------------------------------------------------------------------------

def _cli(args, extra_env):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for k in ("HSFLOW_RENDER_DEVICE", "HSFLOW_JPEG_DEVICE", "HSFLOW_JPEG_IN_DEVICE", ENV):
        env.pop(k, None)
    env.update(extra_env)
    r = subprocess.run([cli] + args, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_cli_reads_and_writes_on_the_device(hs, gpu_ok, tmp_path):
    """HSFLOW_JPEG_IN_DEVICE=1 HSFLOW_RENDER_DEVICE=1 HSFLOW_JPEG_DEVICE=1: the reference's command lines on its own
    JPEG inputs write its own output files, byte for byte; only files cross to and from the device."""
    on = {"HSFLOW_JPEG_IN_DEVICE": "1", "HSFLOW_RENDER_DEVICE": "1", "HSFLOW_JPEG_DEVICE": "1"}
    out = str(tmp_path / "out.jpg")
    for pic in ("city", "bunny"):
        a, b = os.path.join(GOLDEN, "ref_%s_1.jpg" % pic), os.path.join(GOLDEN, "ref_%s_2.jpg" % pic)
        _cli(["-cv", "-hd", a, b, out, ".1", "10"], on)
        assert open(out, "rb").read() == jc.golden("ref_%s_cv_out.jpg" % pic), pic
        os.remove(out)
        _cli(["-cl", "-hd", a, b, out, "15", "10", "1", "GPU"], dict(on, HSFLOW_CL_AS_SHIPPED="1"))
        assert open(out, "rb").read() == jc.golden("ref_%s_cl_out.jpg" % pic), pic
        os.remove(out)


# ---- 6. behind an asynchronous solve --------------------------------------------------------------------------------------------

def test_decode_behind_an_asynchronous_solve(hs, gpu_ok):
    """hsflow_jpeg_decode_device touches no solver state: the ITER|EPS check hsflow_solve_async owes stays owed, and the
    flow view's pointers stay what they were."""
    import torch
    W, H = 250, 130
    name = "c250x130_420_q75_smooth"
    A, B = synth.translating_pair(W, H, seed=5)
    kw = dict(lam=1.0, max_iter=60, term_type=ITER | EPS, epsilon=EPS6)
    with hs.HSFlow(W, H, own_stream=True) as ref:
        ref.set_frames(A, B)
        ref.solve(lam=1.0, max_iter=60, term_type=ITER)
        want = ref.flow()                                                           # the whole budget: what stands behind take_verdict
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        L = ctx._lib

        def view():
            pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
            assert L.hsflow_flow_view_device(ctx._h, 0, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == OK
            return pu.value, pv.value, sb.value

        ctx.set_frames(A, B)
        ctx.solve_async(**kw)
        st, word, rows, _ = decode_device(hs, ctx, jc.data(name), RGB)
        assert st == OK and word == 0 and np.array_equal(rows.reshape(H, W, 3), jc.pil_pixels(name))
        ctx.take_verdict()                                                          # E_STATE had the decode settled the check
        pu, pv, sb = view()
        from opticalflowhs_amd.pipeline import _DeviceView
        for p, w in zip((pu, pv), want):
            got = torch.as_tensor(_DeviceView(p, (H, W), (sb, 4)), device="cuda").cpu().numpy()
            assert np.array_equal(got, w)
        st, word, rows, _ = decode_device(hs, ctx, jc.data(name), BGR)             # ... and the view's pointers stay valid behind another
        assert st == OK and word == 0 and view() == (pu, pv, sb)
        for x, y in zip(ctx.flow(), want):
            assert np.array_equal(x, y)
