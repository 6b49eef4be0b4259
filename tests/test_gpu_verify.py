"""hsflow_verify on the GPU: the comparison kernel against its host twin and NumPy, every solve path against the
one-sweep reference pass, planted wrong values found exactly, nothing disturbed, batches, refusals, the pair pipeline,
the command line, and the 1080p headline pair once.  Wrong values are ordinary data written through
hsflow_set_flow_device; nothing here provokes a fault."""
import ctypes
import gc
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from opticalflowhs_amd import synth
from test_verify_host import PLANTED, assert_same, bits, numpy_rule, plant

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))
OK, E_ARG, E_SIZE, E_STATE = 0, 1, 2, 5


def clean(r):
    """A report that passes without help from the exemption."""
    return (r.ok == 1 and r.iterations_ref == r.iterations_done and r.u.differing == 0 and r.v.differing == 0 and r.deriv_differing == 0
            and r.u.failing == 0 and r.v.failing == 0 and r.u.first_failing == -1 and r.v.first_failing == -1 and r.deriv_first == -1)


def show(r):
    return dict(ok=r.ok, pair=r.pair, done=r.iterations_done, ref=r.iterations_ref, u=r.u.as_dict(), v=r.v.as_dict(),
                deriv=(r.deriv_differing, r.deriv_first))


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def strided(a, pad, offset):
    """`a` as a CUDA tensor whose rows are W + pad floats apart and whose first element lies `offset` floats into its storage."""
    import torch
    H, W = a.shape
    store = torch.full((H * (W + pad) + offset + 8,), 7.0, dtype=torch.float32, device="cuda")
    view = torch.as_strided(store, (H, W), (W + pad, 1), offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return view


# ---- 4. kernel = host twin = NumPy ------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 3, 5, 63, 64, 65, 257, 600, 1920, 3840])
def test_compare_kernel_equals_host_twin_and_numpy(hs, gpu_ok, W):
    import torch
    H = 24 if W >= 600 else 19
    rng = np.random.default_rng(4000 + W)
    A, B = synth.translating_pair(W, H, seed=3)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        ctx.solve(lam=1.0, max_iter=6, term_type=ITER, kernel=hs.KERNEL_SIMPLE if W < 64 else hs.KERNEL_AUTO)
        u, v = ctx.flow()
        # the flow compared with itself: nothing
        du, dv = ctx.compare_flow(upload(u), upload(v))
        zero = dict(differing=0, failing=0, nonfinite=0, first_failing=-1, max_abs_diff=0, max_ulp=0)
        assert_same(du, zero, (W, "self u"))
        assert_same(dv, zero, (W, "self v"))
        # planted cases: side a goes into the context, side b stays with the caller
        au, bu, av, bv = u.copy(), u.copy(), v.copy(), v.copy()
        plant(au, bu, rng, PLANTED)
        plant(av, bv, rng, PLANTED[::-1])
        ctx.set_flow_rows_from(upload(au), upload(av), 0, H)
        gu, gv = ctx.flow()
        assert np.array_equal(gu.view(np.uint32), au.view(np.uint32)) and np.array_equal(gv.view(np.uint32), av.view(np.uint32))
        wu, wv = hs.compare_planes(gu, bu).as_dict(), hs.compare_planes(gv, bv).as_dict()
        assert_same(wu, numpy_rule(gu, bu), (W, "twin u"))
        assert_same(wv, numpy_rule(gv, bv), (W, "twin v"))
        assert wu["differing"] > wu["failing"] > 0 and wu["nonfinite"] == 5, wu
        # dense and 16-byte aligned (the wide loads wherever W allows), then every way of missing that: a base 4 bytes off,
        # an odd stride, both
        odd = 1 if W % 2 == 0 else 2   # W + odd floats per row: an odd stride
        for pad, off in ((0, 0), (0, 1), (odd, 0), (odd, 1), (4, 4), (odd + 2, 3)):
            du, dv = ctx.compare_flow(strided(bu, pad, off), strided(bv, pad, off))
            assert_same(du, wu, (W, pad, off, "u"))
            assert_same(dv, wv, (W, pad, off, "v"))
        torch.cuda.synchronize()


# ---- 5. every path passes --------------------------------------------------------------------------------------------

def verify_clean(ctx, what):
    r = ctx.verify()
    assert clean(r), (what, show(r))
    return r


@pytest.mark.parametrize("shape", [(203, 117), (600, 480), (424, 240)])
def test_every_cv_path_passes(hs, gpu_ok, shape):
    W, H = shape
    S, F, T, D, A = hs.KERNEL_SIMPLE, hs.KERNEL_FUSED, hs.KERNEL_STRIP, hs.KERNEL_FOLD, hs.KERNEL_AUTO
    for seed, frames in ((1, synth.translating_pair(W, H, seed=1)), (3, synth.random_pair(W, H, seed=3))):
        with hs.HSFlow(W, H, 1, own_stream=True) as ctx, hs.HSFlow(W, H, 1, own_stream=True) as red:
            L = ctx._lib
            assert L.hsflow_set_async_reduce(red._h, 1) == OK
            ctx.set_frames(*frames)
            red.set_frames(*frames)
            for kern in (S, F, T, D, A):
                for graph in (False, True):
                    kw = dict(lam=1.0, max_iter=37, term_type=ITER, kernel=kern, use_graph=graph)
                    i = ctx.solve(**kw)
                    r = verify_clean(ctx, (shape, seed, "sync", kw))
                    assert r.iterations_done == 37 == i["iterations_done"]
                    for c in (ctx, red):
                        c.solve_async(**kw)
                        verify_clean(c, (shape, seed, "async", kw, c is red))
            # explicit launch shapes with a tail launch
            for kw in (dict(kernel=T, fuse_steps=7, strip_rows=2), dict(kernel=D, fuse_steps=5, strip_rows=3), dict(kernel=F, fuse_steps=5)):
                ctx.solve(lam=0.5, max_iter=23, term_type=ITER, **kw)
                verify_clean(ctx, (shape, seed, kw))
            # the reference's call: ITER|EPS, default epsilon -- synchronous on every kernel, asynchronous where it runs
            for kern in (S, F, T, D, A):
                for graph in (False, True):
                    kw = dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6, kernel=kern, use_graph=graph)
                    ctx.solve(**kw)
                    r = verify_clean(ctx, (shape, seed, "sync", kw))
                    assert r.iterations_done == 100
                    if kern in (T, D, A):
                        for c in (ctx, red):
                            c.solve_async(**kw)
                            verify_clean(c, (shape, seed, "async", kw, c is red))
            # a verify repeats: the scratch is reused, the answer is the same
            verify_clean(ctx, (shape, seed, "again"))


def test_eps_paths_pass(hs, gpu_ok):
    d = np.load(os.path.join(GOLDEN, "eps_48x40_l0.002_e1e-3.npz"))
    S, F, T, D, A = hs.KERNEL_SIMPLE, hs.KERNEL_FUSED, hs.KERNEL_STRIP, hs.KERNEL_FOLD, hs.KERNEL_AUTO
    with hs.HSFlow(48, 40, 1, own_stream=True) as ctx:
        ctx.set_frames(d["A"], d["B"])
        for kern in (S, F, T, D, A):
            # the early-stop case: ITER|EPS with a budget of 500 stops near sweep d["iters"]
            i = ctx.solve(lam=0.002, max_iter=500, epsilon=1e-3, term_type=ITER | EPS, kernel=kern)
            r = verify_clean(ctx, ("early stop", kern))
            assert r.iterations_ref == r.iterations_done == i["iterations_done"] < 500 and abs(i["iterations_done"] - int(d["iters"])) <= 1
            # EPS alone
            i = ctx.solve(lam=0.002, max_iter=0, epsilon=1e-3, term_type=EPS, kernel=kern)
            r = verify_clean(ctx, ("EPS alone", kern))
            assert r.iterations_ref == r.iterations_done == i["iterations_done"] < 500
        for kern in (T, D, A):
            ctx.solve_async(lam=0.002, max_iter=500, epsilon=1e-3, term_type=ITER | EPS, kernel=kern)
            r = verify_clean(ctx, ("early stop, async", kern))   # settles the owed check (a re-run) first
            assert r.iterations_done < 500 and ctx.info()["eps_rerun"] == 1


@pytest.mark.parametrize("shape", [(203, 117), (600, 480), (424, 240)])
def test_every_classic_path_passes(hs, gpu_ok, shape):
    W, H = shape
    frames = synth.translating_pair(W, H, seed=1)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(*frames)
        for mode in (hs.MODE_CLASSIC, hs.MODE_CLASSIC_AS_SHIPPED):
            for kern in (hs.KERNEL_SIMPLE, hs.KERNEL_FUSED, hs.KERNEL_STRIP, hs.KERNEL_AUTO):
                for graph in (False, True):
                    kw = dict(mode=mode, alpha=3.0, max_iter=25, term_type=ITER, kernel=kern, use_graph=graph)
                    try:
                        ctx.solve(**kw)
                    except hs.HsflowError as e:   # the classic strip kernel has no shape for every frame
                        assert kern == hs.KERNEL_STRIP and e.status == E_SIZE, (kw, e)
                        continue
                    verify_clean(ctx, (shape, "sync", kw))
                    ctx.solve_async(**kw)
                    verify_clean(ctx, (shape, "async", kw))


def only_context_alive():
    gc.collect()


@pytest.mark.parametrize("shape,iters,T", [((1920, 1080), 100, 0), ((1920, 1080), 93, 20)])
def test_persistent_launch_passes_and_survives_a_verify(hs, gpu_ok, shape, iters, T):
    W, H = shape
    only_context_alive()
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(*synth.translating_pair(W, H, seed=7))
        for graph in (False, True):
            kw = dict(lam=1.0, max_iter=iters, term_type=ITER, kernel=hs.KERNEL_PERSIST, fuse_steps=T, strip_rows=5, use_graph=graph)
            i = ctx.solve(**kw)
            assert i["persistent"] >= 2, i
            verify_clean(ctx, (shape, kw))
            # the scratch of the verify is no second context: the persistent launch still runs
            assert ctx.solve(**kw)["persistent"] == i["persistent"]
            ctx.solve_async(**dict(kw, term_type=ITER | EPS, epsilon=EPS6))
            verify_clean(ctx, (shape, "async ITER|EPS", kw))
            assert ctx.info()["persistent"] == i["persistent"]


def test_row_origin_and_eps_rows_of_the_solve_are_honoured(hs, gpu_ok):
    """The reference pass runs with the row origin and the Eps rows the solve under test ran with -- also when they were
    changed after that solve."""
    W, H = 320, 120
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(*synth.translating_pair(W, H, seed=4))
        ctx.set_row_origin(1)   # the other checkerboard phase: another summation order, other bits
        for kern in (hs.KERNEL_STRIP, hs.KERNEL_FOLD, hs.KERNEL_FUSED, hs.KERNEL_SIMPLE):
            ctx.solve(lam=1.0, max_iter=30, term_type=ITER, kernel=kern)
            verify_clean(ctx, ("origin 1", kern))
        u1, v1 = ctx.flow()
        ctx.set_row_origin(0)
        verify_clean(ctx, "origin changed after the solve")
        ctx.solve(lam=1.0, max_iter=30, term_type=ITER, kernel=hs.KERNEL_STRIP)
        verify_clean(ctx, "origin 0")
        u0, v0 = ctx.flow()
        assert not np.array_equal(u0, u1)   # the origin does change bits: the checks above could tell
        # Eps over a window of rows: strip and simple kernels
        d = np.load(os.path.join(GOLDEN, "eps_48x40_l0.002_e1e-3.npz"))
    with hs.HSFlow(48, 40, 1, own_stream=True) as ctx:
        ctx.set_frames(d["A"], d["B"])
        whole = ctx.solve(lam=0.002, max_iter=500, epsilon=1e-3, term_type=ITER | EPS, kernel=hs.KERNEL_STRIP)["iterations_done"]
        ctx.set_eps_rows(2, 6)
        for kern in (hs.KERNEL_STRIP, hs.KERNEL_SIMPLE):
            i = ctx.solve(lam=0.002, max_iter=500, epsilon=1e-3, term_type=ITER | EPS, kernel=kern)
            r = verify_clean(ctx, ("eps rows", kern))
            assert r.iterations_ref == r.iterations_done == i["iterations_done"] < 500
        print("stopping sweep: whole frame %d, rows 2..7 only %d" % (whole, i["iterations_done"]))
        ctx.set_eps_rows(0, 0)
        verify_clean(ctx, "eps rows changed after the solve")


# ---- 6. a wrong value is found, exactly ------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,kernel", [((600, 480), 0), ((203, 117), 3), ((424, 240), 4)])
def test_a_wrong_value_is_found_exactly(hs, gpu_ok, shape, kernel):
    import torch
    W, H = shape
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(*synth.translating_pair(W, H, seed=2))
        ctx.solve(lam=1.0, max_iter=40, term_type=ITER, kernel=kernel)
        u, v = ctx.flow()
        verify_clean(ctx, "before")
        rng = np.random.default_rng(6)
        big_u, big_v = np.argwhere(np.abs(u) > 1e-3), np.argwhere(np.abs(v) > 1e-3)
        y, x = (int(t) for t in big_u[rng.integers(len(big_u))])
        y2, x2 = (int(t) for t in big_v[rng.integers(len(big_v))])
        rows = sorted({y, y2})
        keep = {}
        for row in rows:   # copy the row out, change it, write it back
            ru, rv = torch.empty((1, W), dtype=torch.float32, device="cuda"), torch.empty((1, W), dtype=torch.float32, device="cuda")
            ctx.flow_rows_to(ru, rv, row, 1)
            ctx.synchronize()
            keep[row] = (ru.clone(), rv.clone())
            hu, hv = ru.cpu().numpy(), rv.cpu().numpy()
            assert np.array_equal(hu[0], u[row]) and np.array_equal(hv[0], v[row])
            if row == y:
                hu[0, x] = bits(int(hu[0, x].view(np.uint32)) ^ 1)
            if row == y2:
                hv[0, x2] = hv[0, x2] + np.float32(0.25)
            ctx.set_flow_rows_from(upload(hu), upload(hv), row, 1)
        want_abs = np.abs((v[y2, x2] + np.float32(0.25)) - v[y2, x2]).astype(np.float32)
        r = ctx.verify()
        assert r.ok == 0 and r.pair == 0, show(r)   # pair = -1 call: the failing pair
        assert (r.u.differing, r.u.failing, r.u.first_failing, r.u.max_ulp) == (1, 1, y * W + x, 1), show(r)
        assert (r.v.differing, r.v.failing, r.v.first_failing) == (1, 1, y2 * W + x2), show(r)
        assert np.float32(r.v.max_abs_diff).view(np.uint32) == want_abs.view(np.uint32), (r.v.max_abs_diff, want_abs)
        assert r.deriv_differing == 0 and r.deriv_first == -1 and r.iterations_ref == r.iterations_done == 40
        assert r.u.nonfinite == 0 and r.v.nonfinite == 0
        r0 = ctx.verify(0)
        assert r0.ok == 0 and r0.pair == 0 and r0.u.first_failing == y * W + x
        for row in rows:   # the original rows back
            ctx.set_flow_rows_from(keep[row][0], keep[row][1], row, 1)
        verify_clean(ctx, "restored")
        un, vn = ctx.flow()
        assert np.array_equal(un, u) and np.array_equal(vn, v)


# ---- 7. nothing is disturbed -----------------------------------------------------------------------------------------

def view_of(ctx, pair=0):
    pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    assert ctx._lib.hsflow_flow_view_device(ctx._h, pair, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == OK
    return pu.value, pv.value, sb.value


def test_a_verify_disturbs_nothing(hs, gpu_ok):
    W, H = 600, 480
    frames = synth.translating_pair(W, H, seed=1)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx, hs.HSFlow(W, H, 1, own_stream=True) as twin:
        for c in (ctx, twin):
            c.set_frames(*frames)
        for kw in (dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6), dict(lam=1.0, max_iter=50, term_type=ITER, use_graph=True),
                   dict(mode=hs.MODE_CLASSIC, alpha=3.0, max_iter=20, term_type=ITER)):
            info = ctx.solve(**kw)
            u, v = ctx.flow()
            d = ctx.derivatives()
            view = view_of(ctx)
            pic = ctx.render("cv")
            for _ in range(2):
                verify_clean(ctx, kw)
                assert ctx.info() == info, (kw, ctx.info(), info)
                assert view_of(ctx) == view
                un, vn = ctx.flow()
                assert np.array_equal(un.view(np.uint32), u.view(np.uint32)) and np.array_equal(vn.view(np.uint32), v.view(np.uint32)), kw
                assert all(np.array_equal(a, b) for a, b in zip(ctx.derivatives(), d))
                assert np.array_equal(ctx.render("cv"), pic)
            # the next solve (cached plan, cached graph) gives the same flow and report
            assert ctx.solve(**kw) == info
            un, vn = ctx.flow()
            assert np.array_equal(un, u) and np.array_equal(vn, v)
        # last_eps of an asynchronous ITER|EPS solve is measured on demand, from the OTHER ping-pong buffer: a verify in
        # between must leave that intact
        for graph in (False, True):
            kw = dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6, use_graph=graph)
            for c in (ctx, twin):
                c.solve_async(**kw)
            verify_clean(ctx, ("async", kw))
            a, b = ctx.info(), twin.info()
            assert a["last_eps"] == b["last_eps"] > 0 and a["iterations_done"] == b["iterations_done"] == 100 and a["eps_rerun"] == b["eps_rerun"], (a, b)
            assert all(np.array_equal(x, y) for x, y in zip(ctx.flow(), twin.flow()))
            verify_clean(ctx, ("async, after info", kw))


# ---- 8. batches ------------------------------------------------------------------------------------------------------

def test_batches(hs, gpu_ok):
    import torch
    W, H, N = 320, 200, 3
    pairs = [synth.translating_pair(W, H, seed=1), synth.random_pair(W, H, seed=3), synth.translating_pair(W, H, seed=2)]
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for k, (A, B) in enumerate(pairs):
            ctx.set_frames(A, B, pair=k)
        for kw in (dict(lam=1.0, max_iter=30, term_type=ITER), dict(lam=1.0, max_iter=30, term_type=ITER, kernel=hs.KERNEL_FUSED, use_graph=True),
                   dict(lam=1.0, max_iter=40, term_type=ITER | EPS, epsilon=EPS6)):
            ctx.solve(**kw)
            r = verify_clean(ctx, kw)
            assert r.pair == -1
            for k in range(N):
                rk = ctx.verify(k)
                assert clean(rk) and rk.pair == k, (kw, k, show(rk))
        # pair 1 corrupted
        u1, v1 = ctx.flow(1)
        y, x = (int(t) for t in np.argwhere(np.abs(u1) > 1e-3)[11])
        bad = u1.copy()
        bad[y, x] *= np.float32(1.5)
        ctx.set_flow_rows_from(upload(bad), upload(v1), 0, H, pair=1)
        r = ctx.verify(-1)
        assert r.ok == 0 and r.pair == 1 and r.u.failing == 1 and r.u.first_failing == y * W + x and r.v.failing == 0, show(r)
        assert ctx.verify(0).ok == 1 and ctx.verify(2).ok == 1
        r1 = ctx.verify(1)
        assert r1.ok == 0 and r1.pair == 1 and r1.u.first_failing == y * W + x, show(r1)
        ctx.set_flow_rows_from(upload(u1), upload(v1), 0, H, pair=1)
        verify_clean(ctx, "restored")
    # an ITER|EPS batch whose stop fires: one stopping sweep for all pairs, found by the reference pass on its own
    d = np.load(os.path.join(GOLDEN, "eps_48x40_l0.002_e1e-3.npz"))
    flat = np.full((40, 48), 100, np.uint8)
    flat[12:20, 16:26] = 102
    with hs.HSFlow(48, 40, 3, own_stream=True) as ctx:
        for k, (A, B) in enumerate([(flat, np.roll(flat, 1, axis=1)), (d["A"], d["B"]), (d["A"], d["A"].copy())]):
            ctx.set_frames(A, B, pair=k)
        for kern in (hs.KERNEL_AUTO, hs.KERNEL_SIMPLE, hs.KERNEL_FUSED):
            i = ctx.solve(lam=0.002, max_iter=500, epsilon=1e-3, term_type=ITER | EPS, kernel=kern)
            r = ctx.verify(-1)
            assert r.ok == 1 and r.u.failing == 0 and r.v.failing == 0 and r.deriv_differing == 0, show(r)
            assert r.iterations_ref == r.iterations_done == i["iterations_done"] and 1 < i["iterations_done"] < 500, (i, show(r))
    torch.cuda.synchronize()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------

def test_refusals(hs, gpu_ok):
    L = hs._lib.load()
    VR, PD = hs._lib.HsflowVerifyReport, hs._lib.HsflowPlaneDiff
    W, H = 96, 64
    A, B = synth.translating_pair(W, H, seed=1)

    def report(size=None):
        r = VR()
        r.struct_size = ctypes.sizeof(VR) if size is None else size
        return r

    def refused(ctx, status, pair=0, r=None, word=None):
        r = report() if r is None else r
        st = L.hsflow_verify(ctx._h, pair, ctypes.byref(r) if r is not False else None)
        msg = L.hsflow_last_error(ctx._h)
        assert st == status and msg, (st, status, msg)
        if word:
            assert word.encode() in msg, msg

    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        refused(ctx, E_STATE, word="no solve yet")
        for k in range(2):
            ctx.set_frames(A, B, pair=k)
        refused(ctx, E_STATE, word="no solve yet")
        ctx.solve(lam=1.0, max_iter=10, term_type=ITER)
        assert ctx.verify().ok == 1
        # arguments
        refused(ctx, E_ARG, r=False)
        refused(ctx, E_ARG, r=report(64))
        refused(ctx, E_ARG, pair=2)
        refused(ctx, E_ARG, pair=-2)
        assert ctx.verify(1).ok == 1
        # the last solve failed
        with pytest.raises(hs.HsflowError):
            ctx.solve(lam=-1.0, max_iter=10, term_type=ITER)
        refused(ctx, E_STATE, word="failed")
        ctx.solve(lam=1.0, max_iter=10, term_type=ITER)
        assert ctx.verify().ok == 1
        # a warm start
        ctx.solve(lam=1.0, max_iter=5, term_type=ITER, use_previous=True)
        refused(ctx, E_STATE, word="use_previous")
        ctx.solve(lam=1.0, max_iter=10, term_type=ITER)
        assert ctx.verify().ok == 1
        # frames set, or pushed, since the last solve
        ctx.set_frames(B, A, pair=1)
        refused(ctx, E_STATE, word="frames")
        ctx.solve(lam=1.0, max_iter=10, term_type=ITER)
        assert ctx.verify().ok == 1
        ctx.push_frame(A, pair=0)
        refused(ctx, E_STATE, word="frames")
        ctx.solve(lam=1.0, max_iter=10, term_type=ITER)
        assert ctx.verify().ok == 1
        # a probe counts as an ITER solve of max_iter sweeps
        ctx.solve_probe(lam=1.0, max_iter=9, term_type=ITER | EPS, epsilon=0.5)
        r = ctx.verify()
        assert clean(r) and r.iterations_done == 9, show(r)
        # writing the flow is NOT a refusal: the flow held now is what is compared
        u, v = ctx.flow(0)
        ctx.set_flow_rows_from(upload(u + np.float32(1.0)), upload(v), 0, H, pair=0)
        r = ctx.verify()
        assert r.ok == 0 and r.pair == 0 and r.u.failing == W * H and r.v.failing == 0, show(r)
        # compare_flow's own arguments
        du, dv = PD(), PD()
        t = upload(u)
        p = ctypes.c_void_p(t.data_ptr())
        f = L.hsflow_compare_flow_device
        assert f(ctx._h, 0, None, W * 4, p, W * 4, ctypes.byref(du), ctypes.byref(dv)) == E_ARG and L.hsflow_last_error(ctx._h)
        assert f(ctx._h, 0, p, W * 4, p, W * 4, None, ctypes.byref(dv)) == E_ARG
        assert f(ctx._h, 2, p, W * 4, p, W * 4, ctypes.byref(du), ctypes.byref(dv)) == E_ARG
        assert f(ctx._h, 0, p, W * 4 - 4, p, W * 4, ctypes.byref(du), ctypes.byref(dv)) == E_SIZE and L.hsflow_last_error(ctx._h)
        assert f(ctx._h, 0, p, W * 4, p, W * 4 + 2, ctypes.byref(du), ctypes.byref(dv)) == E_SIZE
        assert f(ctx._h, 0, ctypes.c_void_p(t.data_ptr() + 2), W * 4, p, W * 4, ctypes.byref(du), ctypes.byref(dv)) == E_SIZE
        with pytest.raises(ValueError):
            ctx.compare_flow(t.double(), t)
    # EPS alone with an epsilon below the iteration's limit cycle ends in HSFLOW_E_NOTERM: nothing to verify
    d = np.load(os.path.join(GOLDEN, "eps_48x40_l0.002_e1e-3.npz"))
    with hs.HSFlow(48, 40, 1, own_stream=True) as ctx:
        ctx.set_frames(d["A"], d["B"])
        with pytest.raises(hs.HsflowError) as e:
            ctx.solve(lam=0.002, max_iter=0, epsilon=1e-30, term_type=EPS)
        assert e.value.status == hs._lib.E_NOTERM
        refused(ctx, E_STATE, word="NOTERM")


# ---- 10. the pair pipeline -------------------------------------------------------------------------------------------

def flat_frames(kind, W, H):
    from test_gpu_pipeline_lanes import make_frames
    return make_frames(kind, W, H)


def test_pipeline_two_lanes(hs, gpu_ok):
    import torch
    W, H, depth = 640, 480, 6
    P1 = dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6, use_graph=True)
    P2 = dict(lam=1.0, max_iter=37, term_type=ITER)
    P3 = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)   # the patch pair stops early
    jobs = [("t1", P1), ("t2", P2), ("patch", P3), ("random", P1), ("t1", P2), ("random", P2)]
    dev = {k: tuple(upload(x) for x in flat_frames(k, W, H)) for k in ("t1", "t2", "random", "patch")}
    torch.cuda.synchronize()
    with hs.PairPipeline(W, H, depth=depth, lanes=2) as pl:
        tickets = [pl.submit_device(*dev[k], params=hs.make_params(**kw)) for k, kw in jobs]
        for t, (k, kw) in zip(tickets, jobs):
            r = pl.verify(t)
            i = pl.info(t)
            assert r.ok == 1 and r.pair == 0 and r.iterations_ref == r.iterations_done == i["iterations_done"], (k, kw, show(r))
            assert r.deriv_differing == 0 and r.u.failing == 0 and r.v.failing == 0
            if k == "patch":
                assert 1 < r.iterations_done < 400 and i["eps_rerun"] == 1, (i, show(r))
                print("two lanes, patch pair: differing u %d v %d" % (r.u.differing, r.v.differing))
            else:
                assert clean(r), (k, kw, show(r))
        # the slot of ticket 0 takes another pair: its verify is refused, the new pair's passes
        t6 = pl.submit_device(*dev["t2"], params=hs.make_params(**P1))
        with pytest.raises(hs.HsflowError) as e:
            pl.verify(tickets[0])
        assert e.value.status == E_STATE
        with pytest.raises(hs.HsflowError) as e:
            pl.verify(t6 + 1)   # never issued
        assert e.value.status == E_ARG
        assert clean(pl.verify(t6))
        assert clean(pl.verify(tickets[1]))


def test_pipeline_own_launch_shape_on_flat_frames(hs, gpu_ok):
    """Depth 6 on 3 lanes: the pipeline picks the launch shape itself.  On the flat synthetic pairs flow decays below 1e-30,
    where the strip kernels' bits depend on the launch boundaries: here `differing` may be non-zero, `failing`
    may not."""
    import torch
    from test_gpu_pipeline_lanes import FLAT_KINDS
    W, H, depth = 640, 480, 6
    P1 = dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6, use_graph=True)
    P2 = dict(lam=1.0, max_iter=37, term_type=ITER)
    P3 = dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4)
    dev = {k: tuple(upload(x) for x in flat_frames(k, W, H)) for k in FLAT_KINDS}
    torch.cuda.synchronize()
    with hs.PairPipeline(W, H, depth=depth, lanes=3) as pl:
        jobs = [(k, kw) for k in FLAT_KINDS for kw in (P1, P2, P3)]
        tickets = [pl.submit_device(*dev[k], params=hs.make_params(**kw)) for k, kw in jobs]
        for t, (k, kw) in zip(tickets, jobs):
            r = pl.verify(t)
            i = pl.info(t)
            print("three lanes %s %s: kernel %d T %d rows %d threads %d, differing u %d v %d, max_abs_diff %g %g" % (
                k, kw["max_iter"], i["kernel"], i["fuse_steps"], i["groups_per_thread"], i["threads"], r.u.differing, r.v.differing,
                r.u.max_abs_diff, r.v.max_abs_diff))
            assert i["kernel"] == hs.KERNEL_STRIP and i["groups_per_thread"] == 5, i   # the pipeline's own shape
            assert r.ok == 1 and r.u.failing == 0 and r.v.failing == 0 and r.deriv_differing == 0, (k, kw, show(r))
            assert r.iterations_ref == r.iterations_done == i["iterations_done"]
            assert r.u.max_abs_diff < 1e-30 and r.v.max_abs_diff < 1e-30, show(r)


def test_strip_against_one_sweep_kernel_below_1e30(hs, gpu_ok):
    """The input on which the strip kernels and the one-sweep kernel are known to part below 1e-30 (the 640x400 flat frame
    with a textured patch of test_scaled_state_matches_canonical_arithmetic_down_to_denormals): a verify passes, by the
    exemption where it has to, and the differences stay below that test's own bound of 1e-41."""
    W, H = 640, 400
    rng = np.random.default_rng(3)
    A = np.full((H, W), 90, np.uint8)
    A[40:90, 50:110] = rng.integers(0, 256, (50, 60), dtype=np.uint8)
    B = np.roll(A, 1, axis=1)
    seen = 0
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        for it in (60, 150):
            for kern, kw in ((hs.KERNEL_STRIP, {}), (hs.KERNEL_FOLD, {}), (hs.KERNEL_STRIP, dict(fuse_steps=24)), (hs.KERNEL_FOLD, dict(fuse_steps=7))):
                ctx.solve(lam=1.0, max_iter=it, term_type=ITER, kernel=kern, **kw)
                r = ctx.verify()
                print("640x400 patch, %d sweeps, kernel %d %r: differing u %d v %d, max_abs_diff %g %g, max_ulp %d %d" % (
                    it, kern, kw, r.u.differing, r.v.differing, r.u.max_abs_diff, r.v.max_abs_diff, r.u.max_ulp, r.v.max_ulp))
                assert r.ok == 1 and r.u.failing == 0 and r.v.failing == 0 and r.deriv_differing == 0, (it, kern, kw, show(r))
                assert r.u.max_abs_diff < 1e-41 and r.v.max_abs_diff < 1e-41, show(r)
                seen += r.u.differing + r.v.differing
    print("640x400 patch: %d differing elements in all (0: the exemption has no witness in this suite)" % seen)


# ---- 11. command line ------------------------------------------------------------------------------------------------

def _cli(args, extra_env=None):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for name in ("HSFLOW_RENDER_DEVICE", "HSFLOW_VERIFY"):
        env.pop(name, None)
    env.update(extra_env or {})
    return subprocess.run([cli] + args, env=env, capture_output=True, text=True, timeout=300)


def verdict_lines(stdout):
    return [l for l in stdout.splitlines() if l.startswith("Passed!") or l.startswith("Failed")]


@pytest.mark.parametrize("route", ["cv", "cl"])
def test_cli_disk_routes_verify(hs, gpu_ok, tmp_path, route):
    a, b = os.path.join(GOLDEN, "ref_city_1.jpg"), os.path.join(GOLDEN, "ref_city_2.jpg")
    files = {}
    for mode in ("plain", "verify", "verify_device"):
        out = str(tmp_path / (mode + ".jpg"))
        args = ["-cv", "-hd", a, b, out, ".1", "10"] if route == "cv" else ["-cl", "-hd", a, b, out, "15", "10", "1", "GPU"]
        env = {} if mode == "plain" else {"HSFLOW_VERIFY": "1"}
        if mode == "verify_device":
            env["HSFLOW_RENDER_DEVICE"] = "1"
        r = _cli(args, env)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = verdict_lines(r.stdout)
        if mode == "plain":
            assert lines == [] and "differing" not in r.stdout, r.stdout
        else:
            assert len(lines) == 1 and lines[0].startswith("Passed!") and "failing 0" in lines[0], r.stdout
        assert "Avg time" in r.stdout
        files[mode] = open(out, "rb").read()
    assert files["plain"] == files["verify"] == files["verify_device"] and len(files["plain"]) > 1000
    # HSFLOW_VERIFY=0 is off
    out = str(tmp_path / "zero.jpg")
    args = ["-cv", "-hd", a, b, out, ".1", "10"] if route == "cv" else ["-cl", "-hd", a, b, out, "15", "10", "1", "GPU"]
    assert verdict_lines(_cli(args, {"HSFLOW_VERIFY": "0"}).stdout) == []


@pytest.mark.parametrize("route", ["cv", "cl"])
def test_cli_camera_routes_verify(hs, gpu_ok, tmp_path, route):
    W, H, n = 160, 96, 4
    cam = tmp_path / "cam"
    cam.mkdir()
    for i in range(n):
        _, moved = synth.translating_pair(W, H, seed=77, dx=1.5 * i, dy=-0.75 * i)
        with open(str(cam / ("frame_%04d.pgm" % i)), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (W, H) + moved.tobytes())
    args = ["-cv", "-cam", ".1", "12"] if route == "cv" else ["-cl", "-cam", "3", "12", "1", "GPU"]
    files = {}
    for mode in ("plain", "verify"):
        out = tmp_path / mode
        out.mkdir()
        env = {"HSFLOW_CAMERA_DIR": str(cam), "HSFLOW_CAMERA_OUT": str(out)}
        if mode == "verify":
            env["HSFLOW_VERIFY"] = "1"
        r = _cli(args, env)
        assert r.returncode == 0 and "Avg time" in r.stdout, r.stdout + r.stderr
        lines = verdict_lines(r.stdout)
        if mode == "plain":
            assert lines == [], r.stdout
        else:
            assert len(lines) == n - 1 and all(l.startswith("Passed!") for l in lines), r.stdout
        files[mode] = {p: open(str(out / p), "rb").read() for p in sorted(os.listdir(str(out)))}
    assert sorted(files["plain"]) == ["flow_%04d.ppm" % i for i in range(1, n)]
    assert files["plain"] == files["verify"]


# ---- 12. 1080p once --------------------------------------------------------------------------------------------------

def test_headline_pair_verifies(hs, gpu_ok):
    W, H = 1920, 1080
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(*synth.translating_pair(W, H, seed=1))
        i = ctx.solve()   # the defaults: ITER|EPS, 100 sweeps, AUTO
        r = verify_clean(ctx, "1080p")
        assert r.iterations_done == 100 == i["iterations_done"]
        ctx.solve_async(use_graph=True)
        verify_clean(ctx, "1080p async graph")
