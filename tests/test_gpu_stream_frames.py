"""The frame copy of a device-resident submission rides in the solve's first launch (hsflow_solve_async_frames_device, what
hsflow_pipeline_submit_device calls): where that launch is the strip kernel with the derivative pass and the sources are
word-aligned, it reads the caller's planes in place and stores the slot's copy itself; in every other case the copy kernel
runs as before.  Either way the flow is the synchronous solve's, bit for bit, the slot ends up with its own untouched copy
of the frames, and the caller may overwrite its planes once a call has waited for the ticket."""
import numpy as np
import pytest

from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def reference(hs, W, H, frames, kw):
    """The synchronous solve on a plain context: flow (NumPy) and report."""
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        ctx.set_frames(*frames)
        info = ctx.solve(**kw)
        u, v = ctx.flow()
        return np.array(u), np.array(v), info


def flow_np(pl, t):
    u, v = pl.flow_device(t)
    return u.cpu().numpy(), v.cpu().numpy()


def clean(r):
    return (r.ok == 1 and r.iterations_ref == r.iterations_done and r.u.differing == 0 and r.v.differing == 0
            and r.deriv_differing == 0)


HEADLINE = dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6, use_graph=True)
CASES = [
    # (W, H, depth, lanes, params, the copy is elided)
    (1920, 1080, 6, 2, HEADLINE, True),                                                              # bench.py's headline
    (1920, 1080, 2, 2, dict(lam=1.0, max_iter=100, term_type=ITER, use_graph=True), True),           # ITER: solve_fixed, graph
    (1920, 1080, 2, 1, dict(lam=1.0, max_iter=37, term_type=ITER), True),                            # no graph, a tail launch
    (1920, 1080, 3, 2, dict(lam=1.0, max_iter=7, term_type=ITER | EPS, epsilon=EPS6, use_graph=True), True),   # one launch only
    (1920, 1080, 3, 2, dict(lam=1.0, max_iter=12, term_type=ITER, use_graph=True), True),            # one launch only, ITER
    (1922, 1083, 4, 2, HEADLINE, True),                                                              # W % 4 != 0 (pitched tensors below)
    (600, 480, 8, 8, HEADLINE, True),                                                                # the pipeline's own shape (strip kernel)
    (600, 480, 4, 2, HEADLINE, False),                                                               # AUTO: the folded kernel -> copy
    (1920, 1080, 2, 2, dict(lam=1.0, max_iter=20, term_type=ITER, kernel=2, use_graph=True), False),  # LDS-tile kernel -> copy
    (1920, 1080, 2, 2, dict(mode=1, alpha=15.0, max_iter=20, term_type=ITER, use_graph=True), False),  # classic mode -> copy
    # the pipeline's own shape with a tail: launch 0 in place and alone, the cached graph holds 20 + 17 (ITER|EPS: a witness tail)
    (600, 480, 4, 4, dict(lam=1.0, max_iter=57, term_type=ITER | EPS, epsilon=EPS6, use_graph=True), True),
    (600, 480, 4, 4, dict(lam=1.0, max_iter=57, term_type=ITER, use_graph=True), True),
]


@pytest.mark.parametrize("W,H,depth,lanes,kw,elided", CASES)
def test_submit_device_flow_frames_and_counter(hs, gpu_ok, W, H, depth, lanes, kw, elided):
    """>= 14 submissions alternating two pairs: every flow is the synchronous solve's, the slot's frames are the submitted
    ones, hsflow_pipeline_verify is clean, and the counter says whether the copy kernel ran."""
    import torch
    pairs = [synth.translating_pair(W, H, seed=1), synth.random_pair(W, H, seed=3)]
    ref_kw = kw
    if lanes >= 3 and W * H <= 1500000:   # the pipeline's own launch shape (stream_shape): whether the witness proves "no early
        ref_kw = dict(kw, kernel=hs.KERNEL_STRIP, fuse_steps=20, strip_rows=5, threads=768)   # stop" depends on the shape
    refs = [reference(hs, W, H, f, ref_kw) for f in pairs]
    if W % 4:   # rows of a wider allocation: the stride stays a multiple of 4 although the width is not
        wide = [tuple(torch.zeros((H, W + 6), dtype=torch.uint8, device="cuda") for _ in range(2)) for _ in pairs]
        dv = []
        for (a, b), (ta, tb) in zip(pairs, wide):
            ta[:, :W].copy_(dev(a)); tb[:, :W].copy_(dev(b))
            dv.append((ta[:, :W], tb[:, :W]))
    else:
        dv = [(dev(a), dev(b)) for a, b in pairs]
    torch.cuda.synchronize()
    n = max(14, 2 * depth + 2)
    with hs.PairPipeline(W, H, depth=depth, lanes=lanes) as pl:
        p = hs.make_params(**kw)
        tickets = [pl.submit_device(dv[k & 1][0], dv[k & 1][1], params=p) for k in range(n)]
        for k in range(n - depth, n):   # the pairs the slots still hold
            t = tickets[k]
            u, v = flow_np(pl, t)
            ur, vr, ir = refs[k & 1]
            assert np.array_equal(u, ur) and np.array_equal(v, vr), (k, "flow differs from the synchronous solve")
            i = pl.info(t)
            assert i["iterations_done"] == ir["iterations_done"] and i["eps_rerun"] == ir["eps_rerun"], (k, i, ir)
            fa, fb = pl.frames(t)
            assert np.array_equal(fa, pairs[k & 1][0]) and np.array_equal(fb, pairs[k & 1][1]), (k, "the slot's frames")
            if kw.get("mode", 0) == 0:
                assert clean(pl.verify(t)), k
        assert pl.copies_elided() == (n if elided else 0)


def test_sources_may_be_overwritten_after_the_wait(hs, gpu_ok):
    """Once a call has waited for the ticket the caller's planes are its own again: overwritten, the slot's frames, a verify
    and a render of that ticket are still those of the submitted pair -- also for a pair whose early stop fires and which is
    re-solved from the slot's copy."""
    import torch
    W, H = 1920, 1080
    a, _ = synth.random_pair(W, H, seed=5)
    same = (a, a.copy())                                  # identical frames: the early stop fires after one sweep
    moving = synth.translating_pair(W, H, seed=2)
    for frames, stops in ((moving, False), (same, True)):
        ur, vr, ir = reference(hs, W, H, frames, HEADLINE)
        assert (ir["eps_rerun"] == 1) == stops, ir
        with hs.HSFlow(W, H, own_stream=True) as ctx:
            ctx.set_frames(*frames)
            ctx.solve(**HEADLINE)
            pic = np.array(ctx.render())
        da, db = dev(frames[0]), dev(frames[1])
        torch.cuda.synchronize()
        with hs.PairPipeline(W, H, depth=3, lanes=2) as pl:
            p = hs.make_params(**HEADLINE)
            t = pl.submit_device(da, db, params=p)
            pl.wait(t)
            da.fill_(7); db.fill_(200)
            torch.cuda.synchronize()
            assert pl.copies_elided() == 1
            i = pl.info(t)
            assert i["iterations_done"] == ir["iterations_done"] and i["eps_rerun"] == ir["eps_rerun"], (i, ir)
            u, v = flow_np(pl, t)
            assert np.array_equal(u, ur) and np.array_equal(v, vr)
            fa, fb = pl.frames(t)
            assert np.array_equal(fa, frames[0]) and np.array_equal(fb, frames[1])
            assert clean(pl.verify(t))
            assert np.array_equal(np.array(pl.render(t)), pic)


@pytest.mark.parametrize("how", ["pointer+1", "pointer+2", "stride%4"])
def test_unaligned_sources_take_the_copy_path(hs, gpu_ok, how):
    """Pointers that are not 4-byte aligned, or strides that are no multiple of 4: the copy kernel runs, same flow."""
    import torch
    W, H = 1920, 1080
    frames = synth.translating_pair(W, H, seed=1)
    ur, vr, ir = reference(hs, W, H, frames, HEADLINE)
    if how.startswith("pointer"):
        off = int(how[-1])
        views = []
        for f in frames:
            flat = torch.zeros(H * W + 32, dtype=torch.uint8, device="cuda")
            base = (-flat.data_ptr()) % 16 + off            # data_ptr + base is `off` bytes past a 16-byte boundary
            v = flat[base:base + H * W].view(H, W)
            v.copy_(dev(f))
            assert v.data_ptr() % 4 == off
            views.append(v)
    else:
        views = []
        for f in frames:
            wide = torch.zeros((H, W + 2), dtype=torch.uint8, device="cuda")
            wide[:, :W].copy_(dev(f))
            assert wide.stride(0) % 4 == 2
            views.append(wide[:, :W])
    torch.cuda.synchronize()
    with hs.PairPipeline(W, H, depth=3, lanes=2) as pl:
        p = hs.make_params(**HEADLINE)
        ts = [pl.submit_device(views[0], views[1], params=p) for _ in range(5)]
        for t in ts[-3:]:
            u, v = flow_np(pl, t)
            assert np.array_equal(u, ur) and np.array_equal(v, vr)
            fa, fb = pl.frames(t)
            assert np.array_equal(fa, frames[0]) and np.array_equal(fb, frames[1])
        assert pl.copies_elided() == 0


def test_one_context_call_matches_the_two_calls(hs, gpu_ok):
    """hsflow_solve_async_frames_device on a plain context against hsflow_set_frames_u8_device + hsflow_solve_async: same
    flow, same frames and derivatives left behind, warm start included (the first launch then reads the previous flow)."""
    import ctypes
    import torch
    from opticalflowhs_amd import _lib
    W, H = 1920, 1080
    lib = _lib.load()
    pairs = [synth.translating_pair(W, H, seed=1), synth.translating_pair(W, H, seed=2)]
    dv = [(dev(a), dev(b)) for a, b in pairs]
    torch.cuda.synchronize()
    for kw in (HEADLINE, dict(lam=1.0, max_iter=45, term_type=ITER, use_graph=True), dict(lam=1.0, max_iter=45, term_type=ITER)):
        got = []
        for one_call in (False, True):
            with hs.HSFlow(W, H, own_stream=True) as ctx:
                out = []
                for step, (da, db) in enumerate(dv + dv[:1]):
                    p = hs.make_params(**dict(kw, use_previous=1 if step == 2 else 0))
                    args = (ctypes.c_void_p(da.data_ptr()), da.stride(0), ctypes.c_void_p(db.data_ptr()), db.stride(0))
                    if one_call:
                        assert lib.hsflow_solve_async_frames_device(ctx._h, *args, ctypes.byref(p)) == 0
                    else:
                        assert lib.hsflow_set_frames_u8_device(ctx._h, 0, *args) == 0
                        assert lib.hsflow_solve_async(ctx._h, ctypes.byref(p)) == 0
                    ctx.synchronize()
                    u, v = ctx.flow()
                    out.append((np.array(u), np.array(v)) + tuple(np.array(x) for x in ctx.derivatives()))
                n = ctypes.c_uint64()
                assert lib.hsflow_frame_copies_elided(ctx._h, ctypes.byref(n)) == 0
                assert n.value == (3 if one_call else 0)
                got.append(out)
        for s0, s1 in zip(*got):
            for x, y in zip(s0, s1):
                assert np.array_equal(x, y)
