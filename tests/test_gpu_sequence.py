"""A sequence of frames into a context of N pairs by one launch per chunk (include/hsflow.h, ABI 0.14:
hsflow_set_sequence_device_ex, hsflow_set_sequence_jpeg_ex; the kernel k_pre_sequence of csrc/hs_kernels_pre.hip.h) and
the batched `-cv -cam` route of the drop-in CLI built on it.  Two yardsticks for every plane: the host rule
(hsflow_preprocess_sequence_host, which tests/test_sequence_host.py pins to compositions of the one-frame rule) and a
one-pair context filled by the calls that existed before -- set_frames_device_ex, then push_frame_device_ex(..., 1) for a
pair whose previous frame is blurred twice.  Everything is compared as bytes."""
import contextlib
import ctypes
import os
import subprocess

import numpy as np
import pytest

import jpegd_cases as jc
from conftest import ROOT
from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))
E_ARG, E_SIZE, E_DATA = 1, 2, 7
ENV = "HSFLOW_PRE_SEQ_MAX"
FORMATS = ["gray", "gray_blur", "bgr", "bgr_blur"]
FLAGS = [0, 1, 3]
COUNTS = [2, 3, 5]
# W x H: the host list, then several wavefronts across, strips that end inside, at and beyond the frame, a ragged last word
SHAPES = [(1, 1), (2, 1), (1, 2), (3, 3), (5, 2), (4, 7), (7, 9), (8, 8), (9, 16), (13, 17), (255, 8), (257, 10), (256, 9), (260, 23), (515, 19)]


@contextlib.contextmanager
def seq_max(value):
    old = os.environ.pop(ENV, None)
    if value is not None:
        os.environ[ENV] = str(value)
    try:
        yield
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old


def reblurred(flags, k):
    return bool(flags & 1) and (k > 0 or bool(flags & 2))


def on_device(img, offset, stride):
    """`img` ((H, W) or (H, W, 3) uint8) as a view into a CUDA byte tensor that ends with the frame's last row: base `offset`
    bytes past the allocation's start, rows `stride` bytes apart, 0x5A between the rows."""
    import torch
    H, rowb = img.shape[0], int(np.prod(img.shape[1:]))
    assert stride >= rowb
    host = np.full(offset + (H - 1) * stride + rowb, 0x5A, np.uint8)
    np.lib.stride_tricks.as_strided(host[offset:], (H, rowb), (stride, 1))[...] = img.reshape(H, rowb)
    big = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()   # the contexts work on streams of their own
    shape, strides = ((H, img.shape[1], 3), (stride, 3, 1)) if img.ndim == 3 else ((H, img.shape[1]), (stride, 1))
    view = torch.as_strided(big, shape, strides, storage_offset=offset)
    assert view.data_ptr() % 4 == offset % 4
    return view


def noise(rng, W, H, fmt, n):
    return [rng.integers(0, 256, (H, W, 3) if fmt.startswith("bgr") else (H, W), dtype=np.uint8) for _ in range(n)]


def planes_equal(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---- 1. planes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FORMATS)
def test_planes_against_the_host_rule_and_the_one_pair_calls(hs, gpu_ok, fmt):
    """Every shape x flag set x frame count, from sources with an aligned base and stride (word loads) and from a base + 1
    with an odd stride (byte loads).  The one-pair yardstick of (frame k, reblurred or not) is computed once per shape."""
    ch = 3 if fmt.startswith("bgr") else 1
    rng = np.random.default_rng(40 + FORMATS.index(fmt))
    for W, H in SHAPES:
        frames = noise(rng, W, H, fmt, 5)
        rowb = W * ch
        aligned = [on_device(f, 0, (rowb + 3) // 4 * 4 + 4) for f in frames]
        ragged = [on_device(f, 1, rowb + 1 + rowb % 2) for f in frames]      # an odd stride
        assert aligned[0].stride(0) % 4 == 0 and ragged[0].stride(0) % 2 == 1
        with hs.HSFlow(W, H, 4, own_stream=True) as ctx, hs.HSFlow(W, H, 1, own_stream=True) as one:
            yard = {}
            for k in range(4):
                one.set_frames_device(aligned[k], aligned[k + 1], fmt)
                yard[(k, False)] = one.frames()
                one.set_frames_device(ragged[k], ragged[k], fmt)
                one.push_frame_ex(ragged[k + 1], fmt, reblur_prev=True)
                yard[(k, True)] = one.frames()
            for flags in FLAGS:
                for n in COUNTS:
                    want = hs.preprocess_sequence(frames[:n], fmt, reblur=bool(flags & 1), reblur_first=bool(flags & 2))
                    for name, src in (("aligned", aligned), ("ragged", ragged)):
                        ctx.set_sequence_device(src[:n], fmt, reblur=bool(flags & 1), reblur_first=bool(flags & 2))
                        for k in range(n - 1):
                            got = ctx.frames(k)
                            assert planes_equal(got, want[k]), (W, H, flags, n, name, k, "host rule")
                            assert planes_equal(got, yard[(k, reblurred(flags, k))]), (W, H, flags, n, name, k, "one-pair calls")


# ---- 2. chunking -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["bgr_blur", "gray"])
def test_chunks_of_one_two_and_all_give_the_same_bytes(hs, gpu_ok, fmt):
    W, H = 260, 23
    rng = np.random.default_rng(7)
    frames = noise(rng, W, H, fmt, 5)
    dev = [on_device(f, 0, f.shape[1] * (3 if f.ndim == 3 else 1)) for f in frames]
    want = hs.preprocess_sequence(frames, fmt, reblur=True, reblur_first=True)
    with hs.HSFlow(W, H, 4, own_stream=True) as ctx:
        for value in (1, 2, None, hs.PRE_SEQ_MAX):
            zero = np.zeros((H, W), np.uint8)
            for k in range(4):
                ctx.set_frames(zero, zero, pair=k)
            with seq_max(value):
                ctx.set_sequence_device(dev, fmt, reblur=True, reblur_first=True)
            for k in range(4):
                assert planes_equal(ctx.frames(k), want[k]), (value, k)
        before = [ctx.frames(k) for k in range(4)]
        for value in ("0", "x", "2x", str(hs.PRE_SEQ_MAX + 1), "-1"):
            with seq_max(value):
                with pytest.raises(hs.HsflowError) as e:
                    ctx.set_sequence_device(dev[::-1], fmt)
            assert e.value.status == E_ARG and ENV in str(e.value), value
        assert all(planes_equal(ctx.frames(k), before[k]) for k in range(4))


# ---- 3. placement, errors, an owed check ----------------------------------------------------------------------------------------------

def test_first_pair_and_errors_leave_the_other_planes_alone(hs, gpu_ok):
    W, H = 13, 17
    rng = np.random.default_rng(11)
    frames = noise(rng, W, H, "bgr_blur", 5)
    dev = [on_device(f, 0, 3 * W) for f in frames]
    sentinel = [(np.full((H, W), 10 + k, np.uint8), np.full((H, W), 20 + k, np.uint8)) for k in range(4)]
    with hs.HSFlow(W, H, 4, own_stream=True) as ctx:
        for k in range(4):
            ctx.set_frames(*sentinel[k], pair=k)
        ctx.set_sequence_device(dev[:3], "bgr_blur", reblur=True, first_pair=1)
        want = hs.preprocess_sequence(frames[:3], "bgr_blur", reblur=True)
        assert planes_equal(ctx.frames(0), sentinel[0]) and planes_equal(ctx.frames(3), sentinel[3])
        assert planes_equal(ctx.frames(1), want[0]) and planes_equal(ctx.frames(2), want[1])
        ctx.set_sequence_device(dev[3:], "bgr_blur", reblur=True, reblur_first=True, first_pair=3)      # the last pair alone
        assert planes_equal(ctx.frames(3), hs.preprocess_sequence(frames[3:], "bgr_blur", reblur=True, reblur_first=True)[0])
        assert planes_equal(ctx.frames(0), sentinel[0]) and planes_equal(ctx.frames(2), want[1])
        before = [ctx.frames(k) for k in range(4)]
        L, h = ctx._lib, ctx._h
        ptrs = (ctypes.c_void_p * 5)(*[t.data_ptr() for t in dev])
        holed = (ctypes.c_void_p * 5)(dev[0].data_ptr(), dev[1].data_ptr(), None, dev[3].data_ptr(), dev[4].data_ptr())
        stride = 3 * W
        cases = [("null list", (0, 3, None, 5, stride, 0), E_ARG), ("null entry", (0, 3, holed, 5, stride, 0), E_ARG),
                 ("format 4", (0, 4, ptrs, 5, stride, 0), E_ARG), ("format -1", (0, -1, ptrs, 5, stride, 0), E_ARG),
                 ("one frame", (0, 3, ptrs, 1, stride, 0), E_ARG), ("no frame", (0, 3, ptrs, 0, stride, 0), E_ARG),
                 ("first_pair -1", (-1, 3, ptrs, 3, stride, 0), E_ARG), ("beyond the context", (1, 3, ptrs, 5, stride, 0), E_ARG),
                 ("first_pair 4", (4, 3, ptrs, 2, stride, 0), E_ARG), ("flags 2", (0, 3, ptrs, 5, stride, 2), E_ARG),
                 ("flags 4", (0, 3, ptrs, 5, stride, 4), E_ARG), ("flags -1", (0, 3, ptrs, 5, stride, -1), E_ARG),
                 ("colour stride", (0, 3, ptrs, 5, stride - 1, 0), E_SIZE), ("gray stride", (0, 1, ptrs, 5, W - 1, 1), E_SIZE)]
        for what, (first, fmt, lst, n, st, flags), code in cases:
            assert L.hsflow_set_sequence_device_ex(h, first, fmt, lst, n, st, flags) == code, what
            assert L.hsflow_last_error(h), what
        with seq_max("0"):
            assert L.hsflow_set_sequence_device_ex(h, 0, 3, ptrs, 5, stride, 0) == E_ARG
        ctx.synchronize()
        assert all(planes_equal(ctx.frames(k), before[k]) for k in range(4))
        ctx.set_sequence_device(dev, "bgr_blur")                                                    # and the context still works
        assert all(planes_equal(ctx.frames(k), w) for k, w in enumerate(hs.preprocess_sequence(frames, "bgr_blur")))


def test_a_sequence_settles_an_owed_check_first(hs, gpu_ok):
    """solve_async under ITER|EPS on pairs of equal frames: the early stop fires at sweep 1, which only the owed check
    finds out -- by solving again from the frames.  A sequence call in between must settle it BEFORE it replaces them."""
    W, H = 160, 96
    frames = [synth.translating_pair(W, H, seed=5, dx=1.25 * i, dy=-0.5 * i)[1] for i in range(3)]
    dev = [on_device(f, 0, W) for f in frames]
    crit = dict(lam=0.1, max_iter=12, epsilon=EPS6, term_type=ITER | EPS)
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        ctx.set_sequence_device([dev[0], dev[0], dev[0]], "gray_blur")
        want = ctx.solve(**crit)
        assert want["iterations_done"] == 1 and want["eps_rerun"] == 1
        ctx.set_sequence_device([dev[0], dev[0], dev[0]], "gray_blur")
        ctx.solve_async(**crit)
        ctx.set_sequence_device(dev, "gray_blur", reblur=True)
        got = ctx.info()
        assert got["iterations_done"] == 1 and got["eps_rerun"] == 1, got
        for k in range(2):
            u, v = ctx.flow(k)
            assert not u.any() and not v.any()
        want = hs.preprocess_sequence(frames, "gray_blur", reblur=True)
        assert all(planes_equal(ctx.frames(k), want[k]) for k in range(2))


# ---- 4. solve: the camera loop in one context -----------------------------------------------------------------------------------------

def test_solve_equals_the_loop_frame_by_frame(hs, gpu_ok):
    """Five translating frames, HSFLOW_SEQ_REBLUR, per-pair termination, ITER|EPS on the strip kernel: flow, iterations_done
    and last_eps of pair k bit for bit those of a one-pair context driven through the reference's loop by the existing
    calls.  A second sequence call and solve replay the cached graph on new frames."""
    W, H = 250, 130
    kw = dict(lam=0.1, max_iter=12, term_type=ITER | EPS, epsilon=EPS6, kernel=hs.KERNEL_STRIP)
    assert hs.plan_query(W, H, 4, **kw)["kernel"] == hs.KERNEL_STRIP and hs.plan_query(W, H, 1, **kw)["kernel"] == hs.KERNEL_STRIP
    frames = [synth.translating_pair(W, H, seed=31, dx=1.5 * i, dy=-0.75 * i)[1] for i in range(5)]
    dev = [on_device(f, 0, W + 2) for f in frames]

    def loop(order):
        out = []
        with hs.HSFlow(W, H, 1, own_stream=True) as one:
            for i in range(1, 5):
                if i == 1:
                    one.set_frames_device(order[0], order[1], "gray_blur")
                else:
                    one.push_frame_ex(order[i], "gray_blur", reblur_prev=True)
                info = one.solve(**kw)
                out.append((one.flow(), info["iterations_done"], info["last_eps"], one.frames()))
        return out

    with hs.HSFlow(W, H, 4, own_stream=True) as ctx:
        ctx.set_pair_termination(True)
        for order in (dev, dev[::-1]):
            want = loop(order)
            ctx.set_sequence_device(order, "gray_blur", reblur=True)
            ctx.solve(**kw)
            res = ctx.pair_results()
            for k in range(4):
                flow, iters, eps, planes = want[k]
                assert planes_equal(ctx.frames(k), planes), k
                print("pair", k, "iterations", res[k]["iterations_done"], iters, "last_eps", res[k]["last_eps"], eps)
                assert res[k]["status"] == 0 and res[k]["iterations_done"] == iters and res[k]["last_eps"] == eps, (k, res[k], iters, eps)
                got = ctx.flow(k)
                assert np.array_equal(got[0], flow[0]) and np.array_equal(got[1], flow[1]), k
                assert got[0].any() and got[1].any()


# ---- 5. JPEG files ----------------------------------------------------------------------------------------------------------------

GROUPS = {"250x130": ["c250x130_420_q75_smooth", "c250x130_422_q30_noise", "g250x130_q30_noise_opt"],
          "33x31": ["c33x31_420_q95_noise_rst3_opt", "c33x31_422_q30_smooth", "g33x31_q95_noise_rst3"]}


@pytest.mark.parametrize("group", ["250x130", "33x31"])
def test_jpeg_sequence_with_the_loops_double_blur(hs, gpu_ok, group):
    blobs = [jc.data(n) for n in GROUPS[group]]
    st, info = jc.header(hs, blobs[0])
    assert st == 0
    W, H = info.width, info.height
    with hs.HSFlow(W, H, 2, own_stream=True) as got, hs.HSFlow(W, H, 1, own_stream=True) as one:
        for blur in (True, False):
            # the loop from its start: pair 0 as set_frames_jpeg leaves it, pair 1 after one push
            got.set_sequence_jpeg(blobs, blur=blur, reblur=True)
            one.set_frames_jpeg(blobs[0], blobs[1], blur=blur)
            assert planes_equal(got.frames(0), one.frames()), (blur, 0)
            one.push_frame_jpeg(blobs[2], blur=blur, reblur_prev=True)
            assert planes_equal(got.frames(1), one.frames()), (blur, 1)
            # the loop continued: file 0 was a new frame before
            got.set_sequence_jpeg(blobs, blur=blur, reblur=True, reblur_first=True)
            one.set_frames_jpeg(blobs[0], blobs[0], blur=blur)
            for k in (0, 1):
                one.push_frame_jpeg(blobs[k + 1], blur=blur, reblur_prev=True)
                assert planes_equal(got.frames(k), one.frames()), (blur, "first", k)
        # the defaults are the entry as it was
        got.set_sequence_jpeg(blobs)
        for k in (0, 1):
            one.set_frames_jpeg(blobs[k], blobs[k + 1])
            assert planes_equal(got.frames(k), one.frames()), k
        # all or nothing
        before = [got.frames(k) for k in (0, 1)]
        half = jc.scan_range(hs, blobs[1])[1] // 2
        with pytest.raises(hs.HsflowError) as e:
            got.set_sequence_jpeg([blobs[2], jc.cut_scan(hs, blobs[1], half), blobs[0]], reblur=True)
        assert e.value.status == E_DATA
        with pytest.raises(hs.HsflowError) as e:
            got.set_sequence_jpeg(blobs, reblur=False, reblur_first=True)
        assert e.value.status == E_ARG
        with seq_max("0"):
            with pytest.raises(hs.HsflowError) as e:
                got.set_sequence_jpeg(blobs[::-1], reblur=True)
        assert e.value.status == E_ARG
        assert all(planes_equal(got.frames(k), before[k]) for k in (0, 1))


# ---- 6. the drop-in CLI: `-cv -cam` in batches ----------------------------------------------------------------------------------------

def write_pgm(path, img):
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + np.ascontiguousarray(img, dtype=np.uint8).tobytes())


def run_cli(cam, out, extra):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    out.mkdir()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               HSFLOW_CAMERA_DIR=str(cam), HSFLOW_CAMERA_OUT=str(out))
    for name in ("HSFLOW_RENDER_DEVICE", "HSFLOW_VERIFY", "HSFLOW_CAMERA_BATCH", "HSFLOW_JPEG_IN_DEVICE", "HSFLOW_JPEG_DEVICE", ENV):
        env.pop(name, None)
    env.update(extra)
    r = subprocess.run([cli, "-cv", "-cam", ".1", "12"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "Avg time" in r.stdout, (extra, r.stdout + r.stderr)
    return {name: open(str(out / name), "rb").read() for name in sorted(os.listdir(str(out)))}, r.stdout


def camera_clip():
    return [synth.translating_pair(160, 96, seed=77, dx=1.5 * i, dy=-0.75 * i)[1] for i in range(6)]


def test_cli_camera_batches_write_the_loops_files(hs, gpu_ok, tmp_path):
    """Six PGM frames: batches of 1, 2, 4 (a ragged tail of one pair) and 8 (larger than the clip) write the files of the
    loop byte for byte, and no other file; once more with the pictures drawn on the device, and once with every pair
    verified there."""
    cam = tmp_path / "cam"
    cam.mkdir()
    for i, f in enumerate(camera_clip()):
        write_pgm(str(cam / ("frame_%04d.pgm" % i)), f)
    want, _ = run_cli(cam, tmp_path / "plain", {})
    assert sorted(want) == ["flow_%04d.ppm" % i for i in range(1, 6)]
    assert len(set(want.values())) > 1 and all(np.frombuffer(v, np.uint8)[15:].any() for v in want.values())
    for n in (1, 2, 4, 8):
        got, _ = run_cli(cam, tmp_path / ("batch%d" % n), {"HSFLOW_CAMERA_BATCH": str(n)})
        assert sorted(got) == sorted(want), n
        for name in want:
            assert got[name] == want[name], (n, name)
    want_dev, _ = run_cli(cam, tmp_path / "plain_dev", {"HSFLOW_RENDER_DEVICE": "1"})
    got, _ = run_cli(cam, tmp_path / "batch_dev", {"HSFLOW_CAMERA_BATCH": "4", "HSFLOW_RENDER_DEVICE": "1"})
    assert got == want_dev and sorted(got) == sorted(want)
    got, text = run_cli(cam, tmp_path / "batch_verify", {"HSFLOW_CAMERA_BATCH": "2", "HSFLOW_VERIFY": "1"})
    assert got == want and text.count("Passed!") == 5 and "Failed" not in text, text


def test_cli_camera_batches_of_jpeg_files_decoded_on_the_device(hs, gpu_ok, tmp_path):
    cam = tmp_path / "cam"
    cam.mkdir()
    for i, f in enumerate(camera_clip()):
        with open(str(cam / ("frame_%04d.jpg" % i)), "wb") as out:
            out.write(hs.encode_jpeg(np.ascontiguousarray(np.repeat(f[:, :, None], 3, 2)), 95))
    want, _ = run_cli(cam, tmp_path / "plain", {})
    assert sorted(want) == ["flow_%04d.ppm" % i for i in range(1, 6)] and len(set(want.values())) > 1
    for n in (2, 8):
        got, _ = run_cli(cam, tmp_path / ("batch%d" % n), {"HSFLOW_CAMERA_BATCH": str(n), "HSFLOW_JPEG_IN_DEVICE": "1"})
        assert got == want, n
