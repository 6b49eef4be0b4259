"""A batch of JPEG files decoded by one set of launches (include/hsflow.h: hsflow_jpeg_decode_batch_device,
hsflow_set_sequence_jpeg, hsflow_pipeline_submit_jpeg; the batched kernels of csrc/hs_kernels_jpegd.hip.h) against the
host rule (hsflow_jpeg_decode_host) applied to each file alone, which tests/test_jpegd_host.py pins to PIL and to the
committed fixtures and tests/test_gpu_jpegd.py pins the single device decode to.
Pictures are compared as bytes, every one of them, and so is every byte around them."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import jpegd_cases as jc
import refpics
from conftest import GOLDEN
from jpegd_cases import BGR, E_ARG, E_DATA, E_SIZE, OK, RGB

E_STATE = 5

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))
GUARD = 16
ENV = "HSFLOW_JPEGD_SUBSEQ_BITS"

GROUPS = {
    "17x9": ["c17x9_420_q75_noise", "c17x9_444_q95_smooth_opt"],
    "33x31": ["c33x31_420_q95_noise_rst3_opt", "c33x31_422_q30_smooth", "g33x31_q95_noise_rst3"],     # restart, none, gray + restart
    "48x40": ["c48x40_420_q95_noise_opt", "c48x40_422_q75_noise_rst7"],
    "64x48": ["c64x48_420_q95_noise", "c64x48_444_q30_smooth_rst1"],
    "250x130": ["c250x130_420_q75_smooth", "c250x130_422_q30_noise", "g250x130_q30_noise_opt"],
    "city": ["ref_city_1.jpg", "ref_city_2.jpg"],
    "bunny": ["ref_bunny_1.jpg", "ref_bunny_2.jpg"],
}


@contextlib.contextmanager
def subseq_bits(S):
    old = os.environ.pop(ENV, None)
    os.environ[ENV] = str(S)
    try:
        yield
    finally:
        os.environ.pop(ENV, None)
        if old is not None:
            os.environ[ENV] = old


def blob(name):
    return jc.golden(name) if name.endswith(".jpg") else jc.data(name)


def size_of(hs, data):
    st, info = jc.header(hs, data)
    assert st == OK
    return info.width, info.height


_single = {}


def single(hs, data, order):
    """The file alone by the host rule (hsflow_jpeg_decode_host) as tight rows: (H, 3W) bytes.  Computed once per file and
    order.  (The single device decode is a batch of one: it cannot be the oracle of the batch.)"""
    key = (data, order)
    if key not in _single:
        W, H = size_of(hs, data)
        got = np.ascontiguousarray(hs.jpeg_decode_host(data, "rgb" if order == RGB else "bgr")).reshape(H, 3 * W)
        got.setflags(write=False)
        _single[key] = got
    return _single[key]


class Target(object):
    """n pictures of W x H in one device buffer of 0xA5: GUARD bytes in front, between and behind them, rows `pad` bytes
    longer than tight (the last row of a picture is not padded), and n status words of 77."""

    def __init__(self, W, H, n, pad=0):
        import torch
        self.W, self.H, self.n, self.stride = W, H, n, 3 * W + pad
        self.span = (H - 1) * self.stride + 3 * W
        self.flat = torch.full((GUARD + n * (self.span + GUARD),), 0xA5, dtype=torch.uint8, device="cuda")
        self.words = torch.full((n,), 77, dtype=torch.int32, device="cuda")
        self.offs = [GUARD + i * (self.span + GUARD) for i in range(n)]
        self.pix = (ctypes.c_void_p * n)(*[self.flat.data_ptr() + o for o in self.offs])

    def read(self):
        """(status words, pictures as (H, 3W) arrays, every byte outside the pictures still 0xA5)"""
        host = self.flat.cpu().numpy()
        mask = np.ones(host.size, bool)
        pics = []
        for o in self.offs:
            rows = np.lib.stride_tricks.as_strided(host[o:], (self.H, 3 * self.W), (self.stride, 1))
            pics.append(rows.copy())
            for y in range(self.H):
                mask[o + y * self.stride:o + y * self.stride + 3 * self.W] = False
        return [int(v) for v in self.words.cpu().tolist()], pics, bool((host[mask] == 0xA5).all())


def enqueue(ctx, blobs, order, tgt, first=0):
    """hsflow_jpeg_decode_batch_device of blobs into tgt's pictures first .. first + len(blobs) - 1; nothing waited for."""
    n = len(blobs)
    bufs = [np.frombuffer(b, np.uint8) for b in blobs]
    files = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bufs])
    sizes = (ctypes.c_size_t * n)(*[b.size for b in bufs])
    pix = (ctypes.c_void_p * n)(*[tgt.pix[first + i] for i in range(n)])
    return ctx._lib.hsflow_jpeg_decode_batch_device(ctx._h, files, sizes, n, order, pix, tgt.stride, ctypes.c_void_p(tgt.words.data_ptr() + 4 * first))


def decode_batch(hs, ctx, blobs, order, pad=0):
    import torch
    tgt = Target(ctx.width, ctx.height, len(blobs), pad)
    torch.cuda.synchronize()
    st = enqueue(ctx, blobs, order, tgt)
    torch.cuda.synchronize()      # (not hsflow_synchronize: nothing of the context's state is to be touched)
    return (st,) + tgt.read()


def check_good(hs, got, blobs, order, what):
    st, words, pics, guards = got
    assert st == OK, what
    assert words == [0] * len(blobs), (what, words)
    for i, (b, p) in enumerate(zip(blobs, pics)):
        assert np.array_equal(p, single(hs, b, order)), (what, i)
    assert guards, what


# ---- 1. equals the single decode --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", sorted(GROUPS))
def test_batch_equals_single_decode(hs, gpu_ok, group):
    blobs = [blob(n) for n in GROUPS[group]]
    W, H = size_of(hs, blobs[0])
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        for order in (BGR, RGB):
            for pad in (0, 1, 4):
                check_good(hs, decode_batch(hs, ctx, blobs, order, pad), blobs, order, (group, order, pad))
        if group == "250x130":      # the Python mirror
            out, status = ctx.jpeg_decode_batch(blobs, "bgr")
            assert status == [0, 0, 0]
            for i, b in enumerate(blobs):
                assert np.array_equal(out[i].cpu().numpy().reshape(H, 3 * W), single(hs, b, BGR))


# ---- 2. unequal extents -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [32, 128, 1024])
def test_unequal_extents(hs, gpu_ok, S):
    """Files of 8.8, 11 and 12 KB span different numbers of 256-subsequence groups: workgroups beyond a file's own extent
    return early, and the repair runs its rounds per file."""
    blobs = [blob(n) for n in GROUPS["250x130"]]
    for order in (BGR, RGB):
        for b in blobs:
            single(hs, b, order)                                    # (at the default S: the pixels do not depend on it)
    if S == 32:
        groups = {(jc.scan_range(hs, b)[1] * 8 + S - 1) // S // 256 for b in blobs}
        assert len(groups) > 1, groups
    with hs.HSFlow(250, 130, own_stream=True) as ctx:
        with subseq_bits(S):
            for order in (BGR, RGB):
                check_good(hs, decode_batch(hs, ctx, blobs, order, 1), blobs, order, (S, order))
                check_good(hs, decode_batch(hs, ctx, blobs[::-1], order, 0), blobs[::-1], order, (S, order, "reversed"))


# ---- 3. position and chunking ------------------------------------------------------------------------------------------------

def test_position_and_chunking(hs, gpu_ok, monkeypatch):
    monkeypatch.delenv("HSFLOW_JPEGD_BATCH_MAX", raising=False)      # the header's constant is what cuts the list below
    two = [blob(n) for n in GROUPS["17x9"]]
    n = 2 * hs.JPEGD_BATCH_MAX + 1
    blobs = [two[i % 2] for i in range(n)]
    with hs.HSFlow(17, 9, own_stream=True) as ctx:
        for order in (BGR, RGB):
            check_good(hs, decode_batch(hs, ctx, blobs, order, 1), blobs, order, ("cycle", order))
        x, y = two
        alone = decode_batch(hs, ctx, [x], RGB)
        first = decode_batch(hs, ctx, [x] + [y] * (n - 1), RGB)
        last = decode_batch(hs, ctx, [y] * (n - 1) + [x], RGB)
        check_good(hs, alone, [x], RGB, "alone")
        check_good(hs, first, [x] + [y] * (n - 1), RGB, "first")
        check_good(hs, last, [y] * (n - 1) + [x], RGB, "last")
        assert np.array_equal(alone[2][0], first[2][0]) and np.array_equal(alone[2][0], last[2][-1])


# ---- 4. back to back ----------------------------------------------------------------------------------------------------------

def test_back_to_back_without_synchronisation(hs, gpu_ok):
    """Two batch calls and a single decode enqueued with nothing between them: three uses of the two staging areas, so the
    third waits for the first one's copy, and different files in each, so a staging area reused too early would show."""
    import torch
    a, b, c = [blob(n) for n in GROUPS["250x130"]]
    with hs.HSFlow(250, 130, own_stream=True) as ctx:
        tgt = Target(250, 130, 6, pad=4)
        torch.cuda.synchronize()
        assert enqueue(ctx, [a, b, c], RGB, tgt, 0) == OK
        assert enqueue(ctx, [c, a], RGB, tgt, 3) == OK
        buf = np.frombuffer(b, np.uint8)
        assert ctx._lib.hsflow_jpeg_decode_device(ctx._h, ctypes.c_void_p(buf.ctypes.data), buf.size, RGB, tgt.pix[5], tgt.stride,
                                                  ctypes.c_void_p(tgt.words.data_ptr() + 20)) == OK
        torch.cuda.synchronize()
        check_good(hs, (OK,) + tgt.read(), [a, b, c, c, a, b], RGB, "back to back")


# ---- 5. isolation of bad streams ----------------------------------------------------------------------------------------------

def test_bad_streams_stay_alone(hs, gpu_ok):
    g = blob("g8x8_q75_smooth")
    with hs.HSFlow(8, 8, own_stream=True) as ctx:
        for order in (BGR, RGB):
            st, words, pics, guards = decode_batch(hs, ctx, [g, jc.run_past_63(hs, g), g], order, 1)
            assert st == OK and words == [0, 1, 0] and guards
            assert np.array_equal(pics[0], single(hs, g, order)) and np.array_equal(pics[2], single(hs, g, order))
    a, b, c = [blob(n) for n in GROUPS["33x31"]]
    half = jc.scan_range(hs, b)[1] // 2
    with hs.HSFlow(33, 31, own_stream=True) as ctx:
        for order in (BGR, RGB):
            st, words, pics, guards = decode_batch(hs, ctx, [a, jc.cut_scan(hs, b, half), c], order, 1)
            assert st == OK and words == [0, 2, 0] and guards
            assert np.array_equal(pics[0], single(hs, a, order)) and np.array_equal(pics[2], single(hs, c, order))
        # what the headers show: at once, and nothing is touched
        i = b.index(b"\xff\xc0")
        sof2 = b[:i + 1] + b"\xc2" + b[i + 2:]
        other = blob("c48x40_420_q95_noise_opt")
        for bad, code in ((sof2, E_DATA), (other, E_SIZE)):
            st, words, pics, guards = decode_batch(hs, ctx, [a, c, bad], RGB, 4)
            assert st == code, (st, code)
            assert b"file 2" in ctx._lib.hsflow_last_error(ctx._h), ctx._lib.hsflow_last_error(ctx._h)
            assert words == [77, 77, 77] and guards and all((p == 0xA5).all() for p in pics)
        tgt = Target(33, 31, 1)
        assert enqueue(ctx, [], RGB, tgt) == E_ARG                                   # n < 1
        check_good(hs, decode_batch(hs, ctx, [a, b, c], RGB), [a, b, c], RGB, "and the context still decodes")


# ---- 6. a sequence into a context of N pairs ------------------------------------------------------------------------------------

@pytest.mark.parametrize("group", ["250x130", "33x31"])
def test_sequence(hs, gpu_ok, group):
    blobs = [blob(n) for n in GROUPS[group]]
    W, H = size_of(hs, blobs[0])
    kw = dict(lam=0.1, max_iter=20, term_type=ITER | EPS, epsilon=EPS6)
    with hs.HSFlow(W, H, 2, own_stream=True) as got, hs.HSFlow(W, H, 2, own_stream=True) as want:
        for blur in (True, False):
            got.set_sequence_jpeg(blobs, blur=blur)
            for k in (0, 1):
                want.set_frames_jpeg(blobs[k], blobs[k + 1], blur=blur, pair=k)
            for k in (0, 1):
                for x, y in zip(got.frames(k), want.frames(k)):
                    assert np.array_equal(x, y), (group, blur, k)
            if group == "250x130":
                got.solve(**kw)
                want.solve(**kw)
                for k in (0, 1):
                    for x, y in zip(got.flow(k), want.flow(k)):
                        assert np.array_equal(x, y), (blur, k)
                assert got.pair_results() == want.pair_results()
        # all or nothing
        before = [got.frames(k) for k in (0, 1)]
        half = jc.scan_range(hs, blobs[1])[1] // 2
        with pytest.raises(hs.HsflowError) as e:
            got.set_sequence_jpeg([blobs[2], jc.cut_scan(hs, blobs[1], half), blobs[0]])
        assert e.value.status == E_DATA
        with pytest.raises(hs.HsflowError) as e:
            got.set_sequence_jpeg([blobs[2], blobs[0], blobs[1][:40]])
        assert e.value.status == E_DATA
        with pytest.raises(hs.HsflowError) as e:
            got.set_sequence_jpeg([blobs[2], blobs[0], blob("c48x40_420_q95_noise_opt")])
        assert e.value.status == E_SIZE
        for first_pair, files in ((1, blobs), (2, blobs[:2]), (-1, blobs[:2]), (0, blobs[:1])):
            with pytest.raises(hs.HsflowError) as e:
                got.set_sequence_jpeg(files, first_pair=first_pair)
            assert e.value.status == E_ARG, first_pair
        for k in (0, 1):
            for x, y in zip(got.frames(k), before[k]):
                assert np.array_equal(x, y), k
        # a sequence of two into the second pair alone
        got.set_sequence_jpeg(blobs[:2], blur=False, first_pair=1)
        assert all(np.array_equal(x, y) for x, y in zip(got.frames(0), before[0]))
        want.set_frames_jpeg(blobs[0], blobs[1], blur=False, pair=1)
        assert all(np.array_equal(x, y) for x, y in zip(got.frames(1), want.frames(1)))


def test_sequence_of_the_reference_pair(hs, gpu_ok):
    blobs = [jc.golden("ref_city_%d.jpg" % k) for k in (1, 2)]
    gray = [refpics.read_pgm(os.path.join(GOLDEN, "city_%d_gray.pgm" % k)) for k in (1, 2)]
    H, W = gray[0].shape
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        ctx.set_sequence_jpeg(blobs, blur=False)
        a, b = ctx.frames()
        assert np.array_equal(a, gray[0]) and np.array_equal(b, gray[1])
        ctx.set_sequence_jpeg(blobs, blur=True)
        a, b = ctx.frames()
        assert np.array_equal(a, hs.preprocess_frame(gray[0], "gray_blur")) and np.array_equal(b, hs.preprocess_frame(gray[1], "gray_blur"))


# ---- 7. file pairs through the pipeline -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth,lanes", [(2, 1), (3, 3)])
def test_pipeline_submit_jpeg(hs, gpu_ok, depth, lanes):
    import torch
    W, H = 250, 130
    a, b, c = [blob(n) for n in GROUPS["250x130"]]
    pairs = [(a, b), (b, c), (c, a)]
    kw = dict(lam=0.1, max_iter=20, term_type=ITER | EPS, epsilon=EPS6)
    bgr = {x: torch.from_numpy(single(hs, x, BGR).reshape(H, W, 3).copy()).cuda() for x in (a, b, c)}
    want_frames, want_jpeg = [], []
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        for p, q in pairs:
            ctx.set_frames_jpeg(p, q, blur=True)
            want_frames.append(ctx.frames())
            ctx.solve(**kw)
            want_jpeg.append(ctx.render_jpeg("cv", 95))
    with hs.PairPipeline(W, H, depth=depth, lanes=lanes) as pl, hs.PairPipeline(W, H, depth=depth, lanes=lanes) as ref:
        got, want = [], []
        for i in range(6):
            p, q = pairs[i % 3]
            t = pl.submit_jpeg(p, q, blur=True, **kw)
            r = ref.submit_device(bgr[p], bgr[q], frames="bgr_blur", **kw)
            assert t == r == i
            if i >= depth - 1:                       # the oldest ticket still held by its slot
                got.append(collect(pl, i - depth + 1))
                want.append(collect(ref, i - depth + 1))
        for i in range(6 - depth + 1, 6):
            got.append(collect(pl, i))
            want.append(collect(ref, i))
        assert len(got) == 6
        for i, (g, w) in enumerate(zip(got, want)):
            for x, y in zip(g["frames"], want_frames[i % 3]):
                assert np.array_equal(x, y), (i, "frames")
            for x, y in zip(g["flow"], w["flow"]):
                assert np.array_equal(x, y), (i, "flow")
            assert g["iterations_done"] == w["iterations_done"] and g["eps_rerun"] == w["eps_rerun"], i
        # a truncated curr: its own ticket's error, the tickets around it are right
        half = jc.scan_range(hs, b)[1] // 2
        t0 = pl.submit_jpeg(a, b, blur=True, **kw)
        t1 = pl.submit_jpeg(a, jc.cut_scan(hs, b, half), blur=True, **kw)
        if depth == 2:
            assert np.array_equal(collect(pl, t0)["flow"][0], got[0]["flow"][0])
        t2 = pl.submit_jpeg(b, c, blur=True, **kw)
        if depth > 2:
            assert np.array_equal(collect(pl, t0)["flow"][0], got[0]["flow"][0])
        with pytest.raises(hs.HsflowError) as e:
            pl.wait(t1)
        assert e.value.status == E_DATA
        for call in (pl.flow_device, pl.render, pl.render_jpeg, pl.frames):
            with pytest.raises(hs.HsflowError) as e:
                call(t1)
            assert e.value.status == E_DATA, call
        after = collect(pl, t2)
        assert all(np.array_equal(x, y) for x, y in zip(after["flow"], got[1]["flow"]))
        assert all(np.array_equal(x, y) for x, y in zip(after["frames"], want_frames[1]))
        assert pl.render_jpeg(t2, "cv", 95) == want_jpeg[1]
        # what a header shows: at submit, no ticket
        with pytest.raises(hs.HsflowError) as e:
            pl.submit_jpeg(a, b[:40], blur=True, **kw)
        assert e.value.status == E_DATA
        with pytest.raises(hs.HsflowError) as e:
            pl.submit_jpeg(blob("c48x40_420_q95_noise_opt"), b, blur=True, **kw)
        assert e.value.status == E_SIZE
        assert pl.submit_jpeg(c, a, blur=True, **kw) == t2 + 1
        assert all(np.array_equal(x, y) for x, y in zip(collect(pl, t2 + 1)["flow"], got[2]["flow"]))
        pl.drain()


@pytest.mark.parametrize("depth,lanes", [(2, 1), (3, 3)])
def test_pipeline_bad_ticket_never_waited_for(hs, gpu_ok, depth, lanes):
    """A pair with a truncated file whose ticket nobody waits for: its slot's reuse `depth` submissions later finishes it,
    and that is not the new pair's error.  Afterwards the bad ticket is simply an old one."""
    W, H = 250, 130
    a, b, c = [blob(n) for n in GROUPS["250x130"]]
    kw = dict(lam=0.1, max_iter=20, term_type=ITER | EPS, epsilon=EPS6)
    half = jc.scan_range(hs, b)[1] // 2
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        ctx.set_frames_jpeg(b, c, blur=True)
        want_frames = ctx.frames()
        ctx.solve(**kw)
        want_flow = ctx.flow()
    with hs.PairPipeline(W, H, depth=depth, lanes=lanes) as pl:
        bad = pl.submit_jpeg(a, jc.cut_scan(hs, b, half), blur=True, **kw)
        later = [pl.submit_jpeg(b, c, blur=True, **kw) for _ in range(depth)]      # the last one reuses the bad pair's slot
        assert later[-1] == bad + depth
        for t in later[1:]:                                                        # (later[0]'s slot has been reused as well)
            got = collect(pl, t)
            assert all(np.array_equal(x, y) for x, y in zip(got["frames"], want_frames)), t
            assert all(np.array_equal(x, y) for x, y in zip(got["flow"], want_flow)), t
        pl.wait(bad)                                                               # a ticket of the past: nothing to wait for
        with pytest.raises(hs.HsflowError) as e:
            pl.flow_device(bad)
        assert e.value.status == E_STATE
        pl.drain()


def test_async_pair_entries(hs, gpu_ok):
    """hsflow_set_frames_jpeg_async / hsflow_jpeg_async_status on their own: the planes of hsflow_set_frames_jpeg, one answer
    per call, and status words that a synchronous decode in between does not replace."""
    W, H = 250, 130
    a, b, c = [blob(n) for n in GROUPS["250x130"]]
    cut = jc.cut_scan(hs, b, jc.scan_range(hs, b)[1] // 2)

    def submit(ctx, p, q, blur):
        x, y = np.frombuffer(p, np.uint8), np.frombuffer(q, np.uint8)
        return ctx._lib.hsflow_set_frames_jpeg_async(ctx._h, 0, ctypes.c_void_p(x.ctypes.data), x.size, ctypes.c_void_p(y.ctypes.data), y.size, blur)

    with hs.HSFlow(W, H, own_stream=True) as ctx, hs.HSFlow(W, H, own_stream=True) as want:
        status = lambda: ctx._lib.hsflow_jpeg_async_status(ctx._h)
        assert status() == E_STATE                                                  # nothing asked for yet
        for blur in (1, 0):
            assert submit(ctx, a, b, blur) == OK
            with pytest.raises(hs.HsflowError) as e:                                # a synchronous decode of a bad file in between:
                ctx.jpeg_decode(cut)                                                # its own status word, not the pair's
            assert e.value.status == E_DATA
            assert status() == OK and status() == E_STATE
            want.set_frames_jpeg(a, b, blur=bool(blur))
            assert all(np.array_equal(x, y) for x, y in zip(ctx.frames(), want.frames())), blur
        assert submit(ctx, a, cut, 1) == OK
        assert np.array_equal(ctx.jpeg_decode(c, "bgr").reshape(H, 3 * W), single(hs, c, BGR))    # a good one in between
        assert status() == E_DATA and b"file 1" in ctx._lib.hsflow_last_error(ctx._h)
        assert status() == E_STATE
        before = ctx.frames()
        assert submit(ctx, a, b[:40], 1) == E_DATA and submit(ctx, blob("c48x40_420_q95_noise_opt"), b, 1) == E_SIZE
        assert status() == E_STATE                                                  # nothing was enqueued
        assert all(np.array_equal(x, y) for x, y in zip(ctx.frames(), before))


def collect(pl, ticket):
    info = pl.info(ticket)
    u, v = pl.flow_device(ticket)
    return {"frames": pl.frames(ticket), "flow": (u.cpu().numpy(), v.cpu().numpy()), "iterations_done": info["iterations_done"], "eps_rerun": info["eps_rerun"]}


# ---- 8. behind an asynchronous solve on an async-reduce context ------------------------------------------------------------------

def test_batch_behind_an_asynchronous_solve(hs, gpu_ok):
    """A batch decode enqueued behind hsflow_solve_async on a context that reduces its witness words in-stream leaves the
    solve's result and the check it owes as they are."""
    from opticalflowhs_amd import synth
    W, H = 250, 130
    blobs = [blob(n) for n in GROUPS["250x130"]]
    A, B = synth.translating_pair(W, H, seed=5)
    kw = dict(lam=1.0, max_iter=60, term_type=ITER | EPS, epsilon=EPS6)
    with hs.HSFlow(W, H, own_stream=True) as ref:
        assert ref._lib.hsflow_set_async_reduce(ref._h, 1) == OK
        ref.set_frames(A, B)
        ref.solve_async(**kw)
        verdict = ref.take_verdict()
        want, want_info = ref.flow(), ref.info()
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        assert ctx._lib.hsflow_set_async_reduce(ctx._h, 1) == OK
        ctx.set_frames(A, B)
        ctx.solve_async(**kw)
        check_good(hs, decode_batch(hs, ctx, blobs, RGB, 1), blobs, RGB, "behind the solve")
        assert ctx.take_verdict() == verdict                                        # E_STATE had the decode settled the check
        for x, y in zip(ctx.flow(), want):
            assert np.array_equal(x, y)
        info = ctx.info()
        assert info["iterations_done"] == want_info["iterations_done"] and info["eps_rerun"] == want_info["eps_rerun"]
