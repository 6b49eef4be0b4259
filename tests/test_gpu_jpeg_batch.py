"""A batch of pictures encoded (and drawn) by one set of launches (include/hsflow.h, ABI 0.13:
hsflow_jpeg_encode_batch_device, hsflow_render_flow_batch_device, hsflow_render_flow_jpeg_batch[_device]; kernels in
opticalflowhs_amd/csrc/hs_kernels_jpeg.hip.h and hs_kernels_render.hip.h).  The want side is always the host rule
(hs.encode_jpeg, which tests/test_jpeg_host.py pins to libjpeg and to the reference's own files); the single device
encode of the same picture is checked too.  Files are compared as bytes: every one of them."""
import ctypes
import os

import numpy as np
import pytest

import jpeg_pictures
import refpics
from conftest import GOLDEN
from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))
OK, E_ARG, E_SIZE = 0, 1, 2
GUARD, FILL, WORD0 = 16, 0xA5, 77
KINDS = ("noise", "constant", "arrows", "two_level")   # neighbouring streams two orders of magnitude apart in length
ENV_MAX = "HSFLOW_JPEG_BATCH_MAX"
RKW = dict(threshold=0.02, scale=6.0)


def vp(x):
    return ctypes.c_void_p(x)


def pictures(W, H, n, seed0=None):
    """n pictures of mixed kinds; the first is the noise picture tests/test_gpu_jpeg.py uses at this size."""
    seed0 = 7 * W + H if seed0 is None else seed0
    return [jpeg_pictures.picture(KINDS[i % 4], W, H, seed0 + i) for i in range(n)]


def device_picture_at(arr, base_off, stride):
    """arr on the device, rows `stride` bytes apart, its first byte base_off bytes behind a 256-byte aligned address."""
    import torch
    H, W = arr.shape[:2]
    buf = torch.full((H * stride + 264,), 0x3C, dtype=torch.uint8, device="cuda")
    off = (-buf.data_ptr()) % 256 + base_off
    view = torch.as_strided(buf, (H, W, 3), (stride, 3, 1), storage_offset=off)
    view.copy_(torch.from_numpy(np.ascontiguousarray(arr)).cuda())
    assert view.data_ptr() % 256 == base_off
    return view, buf


class Slots(object):
    """n output slots of `cap` bytes in ONE buffer of 0xA5, 16 guard bytes in front, between and behind; size words at 77."""

    def __init__(self, n, cap):
        import torch
        self.n, self.cap, self.pitch = n, cap, cap + GUARD
        self.buf = torch.full((GUARD + n * self.pitch,), FILL, dtype=torch.uint8, device="cuda")
        self.words = torch.full((n,), WORD0, dtype=torch.int64, device="cuda")
        self.ptrs = (ctypes.c_void_p * n)(*[self.buf.data_ptr() + GUARD + i * self.pitch for i in range(n)])
        torch.cuda.synchronize()

    def untouched(self):
        return bool((self.buf == FILL).all().item()) and self.words.cpu().tolist() == [WORD0] * self.n

    def check(self, wants):
        """Slot i holds the first min(cap, size) bytes of wants[i] and 0xA5 everywhere else; its word the whole size."""
        host, sizes = self.buf.cpu().numpy(), self.words.cpu().tolist()
        assert (host[:GUARD] == FILL).all()
        for i, want in enumerate(wants):
            o = GUARD + i * self.pitch
            k = min(self.cap, len(want))
            assert sizes[i] == len(want), (i, sizes[i], len(want))
            assert host[o:o + k].tobytes() == want[:k], i
            assert (host[o + k:o + self.pitch] == FILL).all(), i     # behind the file, at and beyond capacity, the guard


def encode_batch(L, ctx, views, stride, quality, slots, n=None):
    n = len(views) if n is None else n
    src = (ctypes.c_void_p * len(views))(*[v.data_ptr() for v in views])
    return L.hsflow_jpeg_encode_batch_device(ctx._h, src, n, stride, quality, slots.ptrs, slots.cap, vp(slots.words.data_ptr()))


# ---- 1. batch equals host rule and singles ----------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(17, 15), (64, 48), (150, 70)])
def test_batch_equals_host_rule_and_singles(hs, gpu_ok, W, H):
    L = hs._lib.load()
    arrs = pictures(W, H, 5)
    dev = [device_picture_at(a, 0, 3 * W) for a in arrs]
    bound = hs.jpeg_bound(W, H)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        for quality in (100, 95, 10):
            wants = [hs.encode_jpeg(a, quality) for a in arrs]
            if (W, H, quality) == (64, 48, 100):
                assert wants[0][623:].count(b"\xff\x00") >= 1      # the batched stuffing pass cannot go untested
            print("%dx%d at %d: file sizes %s" % (W, H, quality, [len(w) for w in wants]))
            for i, a in enumerate(arrs):
                assert ctx.encode_jpeg(dev[i][0], quality) == wants[i], (i, quality)
            for n in (1, 2, 3, 5):
                slots = Slots(n, bound)
                assert encode_batch(L, ctx, [v for v, _ in dev[:n]], 3 * W, quality, slots) == OK
                ctx.synchronize()
                slots.check(wants[:n])
            assert ctx.encode_jpeg_batch([v for v, _ in dev], quality) == wants


# ---- 2. mixed alignment in one batch ----------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,stride", [(64, 48, 192), (64, 48, 197), (150, 70, 452), (150, 70, 455), (17, 15, 52)])
def test_mixed_alignment_in_one_batch(hs, gpu_ok, W, H, stride):
    """A batch has one row stride, so what can differ from picture to picture is the base: pictures alternate an aligned
    base and the base 1 byte off of tests/test_gpu_jpeg.py::device_picture.  With a stride that is a multiple of 4 the
    `wide` flag then differs between neighbours; with 3 W + 5 (that test's odd stride) every picture takes the byte-wise path."""
    L = hs._lib.load()
    arrs = pictures(W, H, 4, seed0=900 + W)
    dev = [device_picture_at(a, (0, 1, 0, 3)[i], stride) for i, a in enumerate(arrs)]
    wants = [hs.encode_jpeg(a, 95) for a in arrs]
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        slots = Slots(4, hs.jpeg_bound(W, H))
        assert encode_batch(L, ctx, [v for v, _ in dev], stride, 95, slots) == OK
        ctx.synchronize()
        slots.check(wants)


# ---- 3. capacity ------------------------------------------------------------------------------------------------------

def test_capacity(hs, gpu_ok):
    L = hs._lib.load()
    W, H = 64, 48
    arrs = [jpeg_pictures.picture(k, W, H, s) for k, s in (("arrows", 5), ("noise", 11), ("constant", 6))]
    wants = [hs.encode_jpeg(a, 95) for a in arrs]
    cap = len(wants[1]) - 1
    assert len(wants[0]) <= cap and len(wants[2]) <= cap           # the neighbours fit
    dev = [device_picture_at(a, 0, 3 * W) for a in arrs]
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        slots = Slots(3, cap)
        assert encode_batch(L, ctx, [v for v, _ in dev], 3 * W, 95, slots) == OK
        ctx.synchronize()
        slots.check(wants)          # the middle word: the size needed; its first `cap` bytes; nothing at or beyond cap
    # host form: a busy pair between two pairs of identical frames (black pictures, the shortest files)
    A, B = synth.translating_pair(W, H, seed=3, dx=1.5, dy=-1.0)
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        for p, (a, b) in enumerate(((A, A), (A, B), (B, B))):
            ctx.set_frames(a, b, pair=p)
        ctx.solve(lam=1.0, max_iter=60, term_type=ITER)
        files = ctx.render_jpeg_batch("cv", **RKW)
        assert files == [hs.encode_jpeg(ctx.render("cv", pair=p, **RKW), 95) for p in range(3)]
        assert len(files[1]) > len(files[0]) and len(files[1]) > len(files[2])
        cap = len(files[1]) - 1
        host = np.full((3, cap + GUARD), FILL, np.uint8)
        ptrs = (ctypes.c_void_p * 3)(*[host[i].ctypes.data for i in range(3)])
        sizes = (ctypes.c_size_t * 3)(WORD0, WORD0, WORD0)
        rp = hs.make_render_params("cv", **RKW)
        assert L.hsflow_render_flow_jpeg_batch(ctx._h, 0, 3, ctypes.byref(rp), 95, ptrs, cap, sizes) == E_SIZE
        assert list(sizes) == [len(f) for f in files]              # the size needed, for every picture
        assert (host[1] == FILL).all()                             # the too-small buffer is left alone
        for i in (0, 2):
            assert host[i, :len(files[i])].tobytes() == files[i] and (host[i, len(files[i]):] == FILL).all()


# ---- 4. more than one scan tile per picture ---------------------------------------------------------------------------

def test_more_than_one_scan_tile_and_repeat(hs, gpu_ok):
    L = hs._lib.load()
    W, H = 600, 480
    assert 6 * -(-W // 16) * -(-H // 16) > 4096
    long_ = [jpeg_pictures.picture(k, W, H, 3 + i) for i, k in enumerate(("noise", "arrows", "constant"))]
    short = [jpeg_pictures.picture(k, W, H, 9 + i) for i, k in enumerate(("constant", "constant", "arrows"))]
    wl, ws = [hs.encode_jpeg(a, 95) for a in long_], [hs.encode_jpeg(a, 95) for a in short]
    dl, ds = [device_picture_at(a, 0, 3 * W) for a in long_], [device_picture_at(a, 0, 3 * W) for a in short]
    bound = hs.jpeg_bound(W, H)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        for dev, wants in ((dl, wl), (dl, wl), (ds, ws), (dl, wl)):   # repeated; shorter streams over the same scratch; back
            slots = Slots(3, bound)
            assert encode_batch(L, ctx, [v for v, _ in dev], 3 * W, 95, slots) == OK
            ctx.synchronize()
            slots.check(wants)
        assert ctx.encode_jpeg(dl[0][0], 95) == wl[0]


# ---- 5. chunking ------------------------------------------------------------------------------------------------------

def test_chunking(hs, gpu_ok):
    L = hs._lib.load()
    W, H, n = 64, 48, 5
    arrs = pictures(W, H, n, seed0=50)
    wants = [hs.encode_jpeg(a, 95) for a in arrs]
    dev = [device_picture_at(a, 0, 3 * W) for a in arrs]
    saved = os.environ.pop(ENV_MAX, None)
    try:
        with hs.HSFlow(W, H, own_stream=True) as ctx:
            for value in ("1", "2", None, "2"):
                if value is None:
                    os.environ.pop(ENV_MAX, None)
                else:
                    os.environ[ENV_MAX] = value
                slots = Slots(n, hs.jpeg_bound(W, H))
                assert encode_batch(L, ctx, [v for v, _ in dev], 3 * W, 95, slots) == OK, value
                ctx.synchronize()
                slots.check(wants)
            for value in ("0", str(hs.JPEG_BATCH_MAX + 1), "x", "-1"):
                os.environ[ENV_MAX] = value
                slots = Slots(n, hs.jpeg_bound(W, H))
                assert encode_batch(L, ctx, [v for v, _ in dev], 3 * W, 95, slots) == E_ARG, value
                assert ENV_MAX.encode() in L.hsflow_last_error(ctx._h)
                ctx.synchronize()
                assert slots.untouched()
        # one picture more than the header's maximum, nothing in the environment: two chunks, the second of one picture
        W, H, n = 17, 15, hs.JPEG_BATCH_MAX + 1
        os.environ.pop(ENV_MAX, None)
        arrs = pictures(W, H, n, seed0=300)
        dev = [device_picture_at(a, 0, 3 * W) for a in arrs]
        with hs.HSFlow(W, H, own_stream=True) as ctx:
            slots = Slots(n, hs.jpeg_bound(W, H))
            assert encode_batch(L, ctx, [v for v, _ in dev], 3 * W, 95, slots) == OK
            ctx.synchronize()
            slots.check([hs.encode_jpeg(a, 95) for a in arrs])
    finally:
        os.environ.pop(ENV_MAX, None)
        if saved is not None:
            os.environ[ENV_MAX] = saved


# ---- 6. back to back --------------------------------------------------------------------------------------------------

def test_back_to_back_without_synchronisation(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H = 150, 70
    a1, a2 = pictures(W, H, 3, seed0=70), pictures(W, H, 2, seed0=80)
    one = jpeg_pictures.picture("noise", W, H, 99)
    d1, d2 = [device_picture_at(a, 0, 3 * W) for a in a1], [device_picture_at(a, 0, 3 * W) for a in a2]
    done, _ = device_picture_at(one, 0, 3 * W)
    bound = hs.jpeg_bound(W, H)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        assert ctx.encode_jpeg(done, 95) == hs.encode_jpeg(one, 95)     # the single encode's scratch exists
        s1, s2, s3 = Slots(3, bound), Slots(2, bound), Slots(1, bound)
        torch.cuda.synchronize()
        assert encode_batch(L, ctx, [v for v, _ in d1], 3 * W, 95, s1) == OK
        assert L.hsflow_jpeg_encode_device(ctx._h, vp(done.data_ptr()), 3 * W, 95, s3.ptrs[0], bound, vp(s3.words.data_ptr())) == OK
        assert encode_batch(L, ctx, [v for v, _ in d2], 3 * W, 40, s2) == OK
        ctx.synchronize()
        s1.check([hs.encode_jpeg(a, 95) for a in a1])
        s2.check([hs.encode_jpeg(a, 40) for a in a2])
        s3.check([hs.encode_jpeg(one, 95)])
        assert ctx.encode_jpeg(done, 95) == hs.encode_jpeg(one, 95)


def test_single_and_batch_share_one_scratch(hs, gpu_ok):
    """On a fresh context, nothing waited for in between: a single encode, a batch of three (the batched scratch grown), a
    single render-and-encode, a batch of two pairs.  Whatever scratch the two forms share or keep apart: a layout computed
    for another number of pictures than an allocation holds would put one picture's ranges over another's."""
    import torch
    L = hs._lib.load()
    W, H = 64, 48
    one = jpeg_pictures.picture("noise", W, H, 99)
    three = pictures(W, H, 3, seed0=70)
    rng = np.random.default_rng(64)
    flows = [tuple(rng.uniform(-9, 9, (H, W)).astype(np.float32) for _ in range(2)) for _ in range(2)]
    drawn = [refpics.render(u, v, "cv") for u, v in flows]
    assert all((d != 0).any() for d in drawn) and not np.array_equal(drawn[0], drawn[1])
    done, _ = device_picture_at(one, 0, 3 * W)
    d3 = [device_picture_at(a, 0, 3 * W) for a in three]
    dev_flows = [tuple(torch.from_numpy(x).cuda() for x in uv) for uv in flows]
    bound = hs.jpeg_bound(W, H)
    rp = hs.make_render_params("cv")
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        for p, (u, v) in enumerate(dev_flows):
            ctx.set_flow_rows_from(u, v, 0, H, pair=p)
        s1, s3, r1, r2 = Slots(1, bound), Slots(3, bound), Slots(1, bound), Slots(2, bound)
        ctx.synchronize()           # the flows are there; no encode or render has run on this context yet
        assert L.hsflow_jpeg_encode_device(ctx._h, vp(done.data_ptr()), 3 * W, 95, s1.ptrs[0], bound, vp(s1.words.data_ptr())) == OK
        assert encode_batch(L, ctx, [v for v, _ in d3], 3 * W, 95, s3) == OK
        assert L.hsflow_render_flow_jpeg_device(ctx._h, 1, ctypes.byref(rp), 95, r1.ptrs[0], bound, vp(r1.words.data_ptr())) == OK
        assert L.hsflow_render_flow_jpeg_batch_device(ctx._h, 0, 2, ctypes.byref(rp), 95, r2.ptrs, bound, vp(r2.words.data_ptr())) == OK
        ctx.synchronize()
        s1.check([hs.encode_jpeg(one, 95)])
        s3.check([hs.encode_jpeg(a, 95) for a in three])
        r1.check([hs.encode_jpeg(drawn[1], 95)])
        r2.check([hs.encode_jpeg(d, 95) for d in drawn])


# ---- 7. render batch --------------------------------------------------------------------------------------------------

def view_pointers(hs, ctx, pair):
    pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    assert hs._lib.load().hsflow_flow_view_device(ctx._h, pair, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == OK
    return pu.value, pv.value, sb.value


def busy_and_still_pairs(W, H, n):
    """n pairs: translating textures with different seeds and shifts, pair 1 a pair of identical frames (a black picture)."""
    out = []
    for p in range(n):
        A, B = synth.translating_pair(W, H, seed=1 + p, dx=1.0 + 0.5 * p, dy=-1.5 + p)
        out.append((A, A) if p == 1 else (A, B))
    return out


@pytest.mark.parametrize("W,H,N", [(64, 48, 4), (250, 130, 3)])
def test_render_batch(hs, gpu_ok, W, H, N):
    import torch
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p, (A, B) in enumerate(busy_and_still_pairs(W, H, N)):
            ctx.set_frames(A, B, pair=p)
        ctx.solve(lam=1.0, max_iter=60, term_type=ITER)
        before = [view_pointers(hs, ctx, p) for p in range(N)]
        info, flows = ctx.info(), [ctx.flow(p) for p in range(N)]
        singles = [ctx.render("cv", pair=p, **RKW) for p in range(N)]
        assert sum(bool((s != 0).any()) for s in singles) >= 2 and not (singles[1] != 0).any()
        files = ctx.render_jpeg_batch("cv", **RKW)
        assert len(files) == N
        for p in range(N):
            assert files[p] == ctx.render_jpeg("cv", pair=p, **RKW), p
            assert files[p] == hs.encode_jpeg(singles[p], 95), p
        assert ctx.render_jpeg_batch("cv", first_pair=1, n=2, **RKW) == files[1:3]
        assert ctx.render_jpeg_batch("cv", quality=30, first_pair=N - 1, **RKW) == [hs.encode_jpeg(singles[N - 1], 30)]
        # the pictures themselves into caller memory, guards around each
        rowb = 3 * W
        pitch = H * rowb + GUARD
        buf = torch.full((GUARD + N * pitch,), FILL, dtype=torch.uint8, device="cuda")
        views = [torch.as_strided(buf, (H, W, 3), (rowb, 3, 1), storage_offset=GUARD + p * pitch) for p in range(N)]
        torch.cuda.synchronize()
        ctx.render_batch_device(views, "cv", **RKW)
        ctx.synchronize()
        host = buf.cpu().numpy()
        assert (host[:GUARD] == FILL).all()
        for p in range(N):
            o = GUARD + p * pitch
            assert np.array_equal(host[o:o + H * rowb].reshape(H, W, 3), singles[p]), p
            assert (host[o + H * rowb:o + pitch] == FILL).all(), p
        # the device form of render-and-encode
        slots = Slots(N, hs.jpeg_bound(W, H))
        rp = hs.make_render_params("cv", **RKW)
        L = hs._lib.load()
        assert L.hsflow_render_flow_jpeg_batch_device(ctx._h, 0, N, ctypes.byref(rp), 95, slots.ptrs, slots.cap, vp(slots.words.data_ptr())) == OK
        ctx.synchronize()
        slots.check(files)
        assert [np.array_equal(ctx.render("cv", pair=p, **RKW), singles[p]) for p in range(N)] == [True] * N   # the single plane is clean
        assert [view_pointers(hs, ctx, p) for p in range(N)] == before and ctx.info() == info
        for p in range(N):
            u, v = ctx.flow(p)
            assert np.array_equal(u, flows[p][0]) and np.array_equal(v, flows[p][1])


# ---- 8. per-pair stop -------------------------------------------------------------------------------------------------

def _patch_pair(W, H):
    """tests/test_gpu_jpeg.py::_patch_pair: a flat frame with a patch one grey level brighter."""
    a = np.full((H, W), 90, np.uint8)
    b = a.copy()
    rows, cols = slice(H // 4, H // 4 + min(80, H // 2)), slice(W // 5, W // 5 + min(300, W // 2))
    a[rows, cols], b[rows, cols] = 120, 121
    return a, b


def test_per_pair_stop(hs, gpu_ok):
    W, H = 250, 130
    kw = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)
    pairs = [synth.translating_pair(W, H, seed=2, dx=1.5, dy=-1.0), _patch_pair(W, H), synth.translating_pair(W, H, seed=5, dx=-2.0, dy=0.5)]
    wants, iters = [], []
    for A, B in pairs:
        with hs.HSFlow(W, H, own_stream=True) as one:
            one.set_frames(A, B)
            iters.append(one.solve(**kw)["iterations_done"])
            wants.append(one.render_jpeg("cv", **RKW))
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        ctx.set_pair_termination(True)
        for p, (A, B) in enumerate(pairs):
            ctx.set_frames(A, B, pair=p)
        ctx.solve(**kw)
        res = ctx.pair_results()
        print("iterations per pair:", [r["iterations_done"] for r in res], "alone:", iters)
        assert 1 < res[1]["iterations_done"] < 400 and res[1]["iterations_done"] != res[0]["iterations_done"]
        assert [r["iterations_done"] for r in res] == iters
        assert ctx.render_jpeg_batch("cv", **RKW) == wants


# ---- 9. behind an asynchronous solve ----------------------------------------------------------------------------------

def _views(hs, ctx, W, H, pair):
    import torch
    from opticalflowhs_amd.pipeline import _DeviceView
    pu, pv, sb = view_pointers(hs, ctx, pair)
    return tuple(torch.as_tensor(_DeviceView(p, (H, W), (sb, 4)), device="cuda") for p in (pu, pv))


def test_behind_an_asynchronous_solve(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, N = 600, 480, 2
    kw = dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6)
    rp = hs.make_render_params("cv", **RKW)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with hs.HSFlow(W, H, N, stream=s.cuda_stream) as ctx:
        assert L.hsflow_set_async_reduce(ctx._h, 1) == OK
        for p in range(N):
            A, B = synth.translating_pair(W, H, seed=1 + p, dx=3.0 - p, dy=-2.0 + p)
            ctx.set_frames(A, B, pair=p)
        ctx.solve(**kw)
        want = [hs.encode_jpeg(ctx.render("cv", pair=p, **RKW), 95) for p in range(N)]
        assert want[0] != want[1]
        before = [tuple(t.clone() for t in _views(hs, ctx, W, H, p)) for p in range(N)]
        torch.cuda.synchronize()
        ctx.solve_async(**kw)
        assert ctx.render_jpeg_batch("cv", **RKW) == want        # host form right behind the asynchronous solve
        assert L.hsflow_wait_solve(ctx._h) == OK
        slots = Slots(N, hs.jpeg_bound(W, H))

        def enqueue():
            for _ in range(4):
                assert L.hsflow_render_flow_jpeg_batch_device(ctx._h, 0, N, ctypes.byref(rp), 95, slots.ptrs, slots.cap, vp(slots.words.data_ptr())) == OK

        def planes_unchanged():
            for p in range(N):
                uv = _views(hs, ctx, W, H, p)
                assert torch.equal(uv[0].clone(), before[p][0]) and torch.equal(uv[1].clone(), before[p][1])

        ctx.solve_async(**kw)
        enqueue()
        _views(hs, ctx, W, H, 0)
        assert s.query(), "flow_view returned while a batched encode was still in flight"
        planes_unchanged()
        slots.check(want)
        ctx.solve_async(**kw)
        enqueue()
        assert L.hsflow_wait_solve(ctx._h) == OK
        assert s.query(), "wait_solve returned while a batched encode was still in flight"
        planes_unchanged()
        slots.check(want)


# ---- 10. files in, files out, on the reference's pair -----------------------------------------------------------------

def test_files_in_files_out_on_the_reference_pair(hs, gpu_ok):
    f1, f2 = (open(os.path.join(GOLDEN, "ref_city_%d.jpg" % k), "rb").read() for k in (1, 2))
    W, H = 600, 480
    kw = dict(lam=refpics.LAMBDA, max_iter=refpics.ITERATIONS, epsilon=refpics.EPSILON, term_type=ITER | EPS)
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        ctx.set_sequence_jpeg([f1, f2, f1], blur=True)
        ctx.set_pair_termination(True)
        ctx.solve(**kw)
        files = ctx.render_jpeg_batch("cv")
    assert files[0] == open(os.path.join(GOLDEN, "ref_city_cv_out.jpg"), "rb").read()
    with hs.HSFlow(W, H, own_stream=True) as one:
        one.set_frames_jpeg(f2, f1, blur=True)
        one.solve(**kw)
        assert files[1] == one.render_jpeg("cv")
    assert files[1] != files[0]


# ---- 11. argument errors ----------------------------------------------------------------------------------------------

def test_argument_errors(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, N = 64, 48, 3
    bound = hs.jpeg_bound(W, H)
    arrs = pictures(W, H, N, seed0=20)
    dev = [device_picture_at(a, 0, 3 * W) for a in arrs]
    src = (ctypes.c_void_p * N)(*[v.data_ptr() for v, _ in dev])
    holed = (ctypes.c_void_p * N)(src[0], None, src[2])
    rp = hs.make_render_params("cv", **RKW)
    bad_rp = hs.make_render_params("cv", **RKW)
    bad_rp.step = 0
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            ctx.set_frames(*synth.translating_pair(W, H, seed=1 + p), pair=p)
        ctx.solve(lam=1.0, max_iter=20, term_type=ITER)
        slots = Slots(N, bound)
        words, odd_words = vp(slots.words.data_ptr()), vp(slots.words.data_ptr() + 4)
        out_holed = (ctypes.c_void_p * N)(slots.ptrs[0], slots.ptrs[1], None)
        enc, ren = L.hsflow_jpeg_encode_batch_device, L.hsflow_render_flow_batch_device
        rjd, rjh = L.hsflow_render_flow_jpeg_batch_device, L.hsflow_render_flow_jpeg_batch
        h = ctx._h

        def err():
            return L.hsflow_last_error(h)

        cases = [
            (lambda: enc(h, src, 0, 3 * W, 95, slots.ptrs, bound, words), E_ARG, b""),
            (lambda: enc(h, None, N, 3 * W, 95, slots.ptrs, bound, words), E_ARG, b""),
            (lambda: enc(h, holed, N, 3 * W, 95, slots.ptrs, bound, words), E_ARG, b"picture 1"),
            (lambda: enc(h, src, N, 3 * W, 95, None, bound, words), E_ARG, b""),
            (lambda: enc(h, src, N, 3 * W, 95, out_holed, bound, words), E_ARG, b"picture 2"),
            (lambda: enc(h, src, N, 3 * W, 0, slots.ptrs, bound, words), E_ARG, b"quality"),
            (lambda: enc(h, src, N, 3 * W, 101, slots.ptrs, bound, words), E_ARG, b"quality"),
            (lambda: enc(h, src, N, 3 * W, 95, slots.ptrs, bound, None), E_ARG, b""),
            (lambda: enc(h, src, N, 3 * W, 95, slots.ptrs, bound, odd_words), E_ARG, b"aligned"),
            (lambda: enc(h, src, N, 3 * W - 1, 95, slots.ptrs, bound, words), E_SIZE, b"stride"),
            (lambda: ren(h, 0, 0, ctypes.byref(rp), slots.ptrs, 3 * W), E_ARG, b""),
            (lambda: ren(h, 1, N, ctypes.byref(rp), slots.ptrs, 3 * W), E_ARG, b"pairs"),
            (lambda: ren(h, -1, 1, ctypes.byref(rp), slots.ptrs, 3 * W), E_ARG, b"pairs"),
            (lambda: ren(h, 0, N, None, slots.ptrs, 3 * W), E_ARG, b""),
            (lambda: ren(h, 0, N, ctypes.byref(bad_rp), slots.ptrs, 3 * W), E_ARG, b"step"),
            (lambda: ren(h, 0, N, ctypes.byref(rp), None, 3 * W), E_ARG, b""),
            (lambda: ren(h, 0, N, ctypes.byref(rp), out_holed, 3 * W), E_ARG, b"picture 2"),
            (lambda: ren(h, 0, N, ctypes.byref(rp), slots.ptrs, 3 * W - 1), E_SIZE, b"stride"),
            (lambda: rjd(h, 0, N + 1, ctypes.byref(rp), 95, slots.ptrs, bound, words), E_ARG, b"pairs"),
            (lambda: rjd(h, 0, N, ctypes.byref(bad_rp), 95, slots.ptrs, bound, words), E_ARG, b"step"),
            (lambda: rjd(h, 0, N, ctypes.byref(rp), 0, slots.ptrs, bound, words), E_ARG, b"quality"),
            (lambda: rjd(h, 0, N, ctypes.byref(rp), 95, out_holed, bound, words), E_ARG, b"picture 2"),
            (lambda: rjd(h, 0, N, ctypes.byref(rp), 95, slots.ptrs, bound, odd_words), E_ARG, b"aligned"),
            (lambda: rjd(h, 0, N, ctypes.byref(rp), 95, slots.ptrs, bound, None), E_ARG, b""),
        ]
        for k, (call, status, word) in enumerate(cases):
            assert call() == status, k
            assert word in err(), (k, err())
        torch.cuda.synchronize()
        assert slots.untouched()
        # the host form
        host = np.full((N, bound), FILL, np.uint8)
        ptrs = (ctypes.c_void_p * N)(*[host[i].ctypes.data for i in range(N)])
        holed_host = (ctypes.c_void_p * N)(ptrs[0], None, ptrs[2])
        sizes = (ctypes.c_size_t * N)(*([WORD0] * N))
        for k, (call, word) in enumerate([
                (lambda: rjh(h, 0, 0, ctypes.byref(rp), 95, ptrs, bound, sizes), b""),
                (lambda: rjh(h, 2, 2, ctypes.byref(rp), 95, ptrs, bound, sizes), b"pairs"),
                (lambda: rjh(h, 0, N, None, 95, ptrs, bound, sizes), b""),
                (lambda: rjh(h, 0, N, ctypes.byref(rp), 101, ptrs, bound, sizes), b"quality"),
                (lambda: rjh(h, 0, N, ctypes.byref(rp), 95, None, bound, sizes), b""),
                (lambda: rjh(h, 0, N, ctypes.byref(rp), 95, holed_host, bound, sizes), b"picture 1"),
                (lambda: rjh(h, 0, N, ctypes.byref(rp), 95, ptrs, bound, None), b"")]):
            assert call() == E_ARG, k
            assert word in err(), (k, err())
        assert (host == FILL).all() and list(sizes) == [WORD0] * N
        # and everything still works
        files = ctx.render_jpeg_batch("cv", **RKW)
        assert files == [ctx.render_jpeg("cv", pair=p, **RKW) for p in range(N)]
    with pytest.raises(ValueError):
        with hs.HSFlow(W, H, own_stream=True) as ctx:
            ctx.encode_jpeg_batch([])
