"""The global motion of a flow field fitted on the GPU (include/hsflow.h, ABI 0.23: hsflow_gmotion_fit*, hsflow_gmotion_warp*;
kernels in opticalflowhs_amd/csrc/hs_kernels_gmotion.hip.h) against the rule on the host (hsflow_gmotion_fit_host and
hsflow_gmotion_warp_host, which tests/test_gmotion_host.py holds to a NumPy restatement).  Model, threshold, flags and class
counts are compared exactly, the mask byte for byte, the residual planes bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import gmotion_ref as G
from conftest import ROOT
from opticalflowhs_amd import synth
from test_gpu_chain import DevIn, cuda, layouts, ptr_list
from test_gpu_fb import FILL, DevPlane, dev_stats, put_flow

pytestmark = pytest.mark.gpu

F = np.float32
ITER, EPS = 1, 2
OK, E_ARG, E_SIZE = 0, 1, 2
VALUES = (200, 90, 40, 7)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def rec_tuple(r):
    return (tuple(np.array(r.p[:], F).view(np.uint32).tolist()), int(F(r.threshold).view(np.uint32)), int(r.flags), tuple(int(x) for x in r.cls))


def host_want(hs, u, v, state, gp):
    """(record tuple, mask, ru bits, rv bits) of the host rule."""
    rec, mask, ru, rv = hs.global_motion_host(u, v, state=state, mask=True, residual=True, params=gp)
    return rec_tuple(rec), mask, bits(ru), bits(rv)


def check_device(hs, outs, dr, want, label, n=1, k=0):
    """The DevPlanes (mask, ru, rv; None where not asked for) and record k of dr against the host's; nothing written around them."""
    for d, w in zip(outs, want[1:]):
        if d is None:
            continue
        rows, clean = d.rows_and_rest()
        got = np.ascontiguousarray(rows).view(np.uint32) if w.dtype == np.uint32 else rows
        assert np.array_equal(got, w), label
        assert clean, label
    if dr is not None:
        assert rec_tuple(hs.gmotion_result_from(dr, n)[k] if n > 1 else hs.gmotion_result_from(dr)) == want[0], label
        assert bool((dr[64 * n:] == FILL).all().item()), label


# ---- G1. device against host ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", G.SHAPES)
@pytest.mark.parametrize("kind", [G.TRANSLATION, G.SIMILARITY, G.AFFINE])
def test_device_equals_host(hs, gpu_ok, W, H, kind):
    L = hs._lib.load()
    u, v, state = G.field(W, H, seed=100 * W + H)
    lay = layouts(W)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for mode in (G.FIXED, G.AUTO):
            for passes in (1, 3):
                gp = hs.make_gmotion_params(kind, passes, mode, inlier_px=0.8, scale2=5.0, min_thr2=0.01, values=VALUES)
                wants = {True: host_want(hs, u, v, state, gp), False: host_want(hs, u, v, None, gp)}
                for k, ((foff, fstride), (boff, bstride)) in enumerate(lay):
                    with_state = (k + passes) % 2 == 0
                    label = (W, H, kind, mode, passes, k)
                    du, dv = DevIn(u, foff, fstride), DevIn(v, foff, fstride)
                    ds = DevIn(state, boff, bstride) if with_state else None
                    outs = [DevPlane(H, W, (boff + 1) % 4, bstride), DevPlane(H, 4 * W, foff, fstride), DevPlane(H, 4 * W, foff, fstride)]
                    dr = dev_stats()
                    assert L.hsflow_gmotion_fit_planes_device(ctx._h, du.ptr, dv.ptr, fstride, ds.ptr if ds else None, bstride, ctypes.byref(gp), outs[0].ptr, bstride,
                                                              outs[1].ptr, outs[2].ptr, fstride, ctypes.c_void_p(dr.data_ptr())) == OK, label
                    ctx.synchronize()
                    check_device(hs, outs, dr, wants[with_state], label)
                    assert du.rows_and_rest()[1] and dv.rows_and_rest()[1]
                # the context's own flow: the device form and the synchronous form
                rec, mask, ru, rv = ctx.global_motion(state=cuda(state), mask=True, residual=True, params=gp, device=True)
                ctx.synchronize()
                got = (rec_tuple(hs.gmotion_result_from(rec)), mask.cpu().numpy(), bits(ru.cpu().numpy()), bits(rv.cpu().numpy()))
                assert got[0] == wants[True][0] and all(np.array_equal(a, b) for a, b in zip(got[1:], wants[True][1:])), (W, H, kind, mode, passes)
                rec, mask, ru, rv = ctx.global_motion(mask=True, residual=True, params=gp)
                got = (rec_tuple(rec), mask, bits(ru), bits(rv))
                assert got[0] == wants[False][0] and all(np.array_equal(a, b) for a, b in zip(got[1:], wants[False][1:])), (W, H, kind, mode, passes)
        gu, gv = ctx.flow(0)                                              # the flow is read and never changed
        assert np.array_equal(bits(gu), bits(u)) and np.array_equal(bits(gv), bits(v))


# ---- G1b. degenerate sets: both sides take the same branch ---------------------------------------------------------------------------

def test_degenerate_sets_on_the_device(hs, gpu_ok):
    """No usable pixel, one pixel, one row, one column, one diagonal: the fallback the host takes, with its flag, model and class
    counts, through the planes form one by one and through ONE batch that holds all five."""
    from test_gmotion_host import degenerate_fields
    L = hs._lib.load()
    sets = degenerate_fields()
    names = ["none", "one", "row", "column", "diagonal"]
    H, W = sets["none"][0].shape
    with hs.HSFlow(W, H, len(names), own_stream=True) as ctx:
        for p, name in enumerate(names):
            put_flow(ctx, sets[name][0], sets[name][1], pair=p)
        for kind in ("affine", "similarity", "translation"):
            for mode, passes in (("fixed", 1), ("fixed", 3), ("auto", 1), ("auto", 3)):
                gp = hs.make_gmotion_params(kind, passes, mode, inlier_px=50.0, scale2=1e5, values=VALUES)
                wants = [host_want(hs, sets[name][0], sets[name][1], None, gp) for name in names]
                dr = dev_stats(len(names))
                ctx.global_motion_batch_device(0, len(names), results=dr, params=gp)
                ctx.synchronize()
                got = hs.gmotion_result_from(dr, len(names))
                for p, name in enumerate(names):
                    label = (name, kind, mode, passes)
                    assert rec_tuple(got[p]) == wants[p][0], label
                    if kind == "affine":
                        assert got[p].flags == (sets[name][2] << 8 | hs.GMOTION_FLAG_FALLBACK), label
                    rec, mask, ru, rv = ctx.global_motion_planes_device(cuda(sets[name][0]), cuda(sets[name][1]), mask=True, residual=True, params=gp)
                    ctx.synchronize()
                    assert rec_tuple(hs.gmotion_result_from(rec)) == wants[p][0], label
                    assert np.array_equal(mask.cpu().numpy(), wants[p][1]) and np.array_equal(bits(ru.cpu().numpy()), wants[p][2]), label


def sums_full(s, W, cols):
    """The sums of G.sums_of taken on the last `cols` columns alone, moved to the coordinates of the W-wide frame: Xi grows by W - cols."""
    d = W - cols
    n, x, y, xx, xy, yy, u, ux, uy, v, vx, vy = s
    return [n, x + d * n, y, xx + 2 * d * x + d * d * n, xy + d * y, yy, u, ux + d * u, uy, v, vx + d * v, vy]


def test_far_edge_columns_of_the_widest_frame(hs, gpu_ok):
    """Beyond n * Sxx = 2^53 the spreads and the determinant are rounded doubles: two adjacent columns at the far edge of a
    16384-wide frame (the narrowest spread that is no fallback, n * Sxx = 2^54), and one such column (a fallback), give on
    the device the flags, model and class counts of the host -- which are those of the restated solve on big-integer sums --
    through the planes form and the batch form."""
    import torch
    W, H = 16384, 4096
    rng = np.random.default_rng(2)
    Yi = (2 * np.arange(H) - (H - 1)) * 0.5
    for cols, used in ((2, G.AFFINE), (1, G.SIMILARITY)):
        u, v = np.full((H, W), np.nan, F), np.full((H, W), np.nan, F)
        for k in range(cols):
            u[:, W - 1 - k] = (2.0 + 0.5 * k + 0.001 * Yi + rng.normal(0, 0.1, H)).astype(F)
            v[:, W - 1 - k] = (-1.0 - 0.25 * k + 0.002 * Yi + rng.normal(0, 0.1, H)).astype(F)
        sums = G.sums_of(u[:, W - cols:], v[:, W - cols:], np.ones((H, cols), bool))
        n, sxx = sums[0], sum((2 * (W - 1 - k) - (W - 1)) ** 2 for k in range(cols)) * H
        assert cols == 1 or n * sxx > 2 ** 53
        gp = hs.make_gmotion_params("affine", 1, "fixed", inlier_px=1.0)
        want = hs.global_motion_host(u, v, params=gp)[0]
        assert want.flags == (used << 8 | (hs.GMOTION_FLAG_FALLBACK if used != G.AFFINE else 0)) and want.cls[3] == (W - cols) * H
        p, flags = G.solve(sums_full(sums, W, cols), G.AFFINE)
        assert flags == want.flags and np.array_equal(p.view(np.uint32), np.array(want.p[:], F).view(np.uint32))
        with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
            du, dv = cuda(u), cuda(v)
            rec = ctx.global_motion_planes_device(du, dv, params=gp)[0]
            ctx.synchronize()
            assert rec_tuple(hs.gmotion_result_from(rec)) == rec_tuple(want), cols
            ctx.set_flow_rows_from(du, dv, 0, H)
            ctx.synchronize()
            dr = dev_stats()
            ctx.global_motion_batch_device(0, 1, results=dr, params=gp)
            ctx.synchronize()
            assert rec_tuple(hs.gmotion_result_from(dr)) == rec_tuple(want), cols
        del du, dv
        torch.cuda.empty_cache()


def test_each_output_alone(hs, gpu_ok):
    W, H = 260, 37
    u, v, state = G.field(W, H, seed=4)
    gp = hs.make_gmotion_params("affine", 2, "auto", values=VALUES)
    want = host_want(hs, u, v, state, gp)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for device in (False, True):
            s = cuda(state) if device else state
            for wm, wr, wrec in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
                rec, mask, ru, rv = ctx.global_motion(state=s, mask=bool(wm), residual=bool(wr), result=bool(wrec), params=gp, device=device)
                ctx.synchronize()
                get = lambda x: x.cpu().numpy() if device else x
                assert (mask is None) == (not wm) and (ru is None) == (not wr) and (rv is None) == (not wr) and (rec is None) == (not wrec)
                if wm:
                    assert np.array_equal(get(mask), want[1]), (device, wm, wr, wrec)
                if wr:
                    assert np.array_equal(bits(get(ru)), want[2]) and np.array_equal(bits(get(rv)), want[3]), (device, wm, wr, wrec)
                if wrec:
                    assert rec_tuple(hs.gmotion_result_from(rec) if device else rec) == want[0], (device, wm, wr, wrec)
        L = hs._lib.load()
        assert L.hsflow_gmotion_fit_device(ctx._h, 0, None, 0, ctypes.byref(gp), None, 0, None, None, 0, None) == E_ARG          # nothing asked for
        dr = dev_stats()
        assert L.hsflow_gmotion_fit_device(ctx._h, 0, None, 0, ctypes.byref(gp), None, 0, None, None, 0, ctypes.c_void_p(dr.data_ptr() + 4)) == E_ARG
        assert L.hsflow_gmotion_fit_device(ctx._h, 1, None, 0, ctypes.byref(gp), None, 0, None, None, 0, ctypes.c_void_p(dr.data_ptr())) == E_ARG
        pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        assert L.hsflow_flow_view_device(ctx._h, 0, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == OK
        assert L.hsflow_gmotion_fit_device(ctx._h, 0, None, 0, ctypes.byref(gp), None, 0, pu, pv, sb.value, None) == E_ARG          # onto the context's flow


# ---- G2. batches, scratch growth ---------------------------------------------------------------------------------------------------

def test_batch_equals_single_calls(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, N = 96, 64, 7
    fields = [G.field(W, H, seed=30 + p) for p in range(N)]
    for mode in ("fixed", "auto"):
        gp = hs.make_gmotion_params("affine", 3, mode, values=VALUES)
        with hs.HSFlow(W, H, N, own_stream=True) as ctx:
            for p in range(N):
                put_flow(ctx, fields[p][0], fields[p][1], pair=p)
            small = ctx.global_motion(pair=6, params=gp)[0]                 # the scratch holds one record ...
            for n, first in ((1, 3), (2, 1), (5, 2)):                       # ... and grows with the batch
                states = [cuda(fields[first + k][2]) if k % 2 == 0 else None for k in range(n)]
                masks = [torch.full((H, W), FILL, dtype=torch.uint8, device="cuda") if k != 1 else None for k in range(n)]
                rus = [torch.zeros((H, W), dtype=torch.float32, device="cuda") if k != 0 else None for k in range(n)]
                rvs = [torch.zeros((H, W), dtype=torch.float32, device="cuda") if k != 0 else None for k in range(n)]
                dr = dev_stats(n)
                ctx.global_motion_batch_device(first, n, state=states, mask=masks, res_u=rus, res_v=rvs, results=dr, params=gp)
                ctx.synchronize()
                for k in range(n):
                    want = host_want(hs, fields[first + k][0], fields[first + k][1], fields[first + k][2] if k % 2 == 0 else None, gp)
                    single = ctx.global_motion(pair=first + k, state=fields[first + k][2] if k % 2 == 0 else None, mask=True, residual=True, params=gp)
                    assert rec_tuple(single[0]) == want[0] and np.array_equal(single[1], want[1]) and np.array_equal(bits(single[2]), want[2])
                    assert rec_tuple(hs.gmotion_result_from(dr, n)[k] if n > 1 else hs.gmotion_result_from(dr)) == want[0], (n, first, k)
                    if masks[k] is not None:
                        assert np.array_equal(masks[k].cpu().numpy(), want[1]), (n, first, k)
                    if rus[k] is not None:
                        assert np.array_equal(bits(rus[k].cpu().numpy()), want[2]) and np.array_equal(bits(rvs[k].cpu().numpy()), want[3]), (n, first, k)
                assert bool((dr[64 * n:] == FILL).all().item())
            assert rec_tuple(ctx.global_motion(pair=6, params=gp)[0]) == rec_tuple(small)      # the small frame again
            assert L.hsflow_gmotion_fit_batch_device(ctx._h, 3, 5, None, 0, ctypes.byref(gp), None, 0, None, None, 0, ctypes.c_void_p(dev_stats(5).data_ptr())) == E_ARG
            assert L.hsflow_gmotion_fit_batch_device(ctx._h, -1, 1, None, 0, ctypes.byref(gp), None, 0, None, None, 0, ctypes.c_void_p(dev_stats(5).data_ptr())) == E_ARG


def test_planes_of_a_chain_with_lost_pixels(hs, gpu_ok):
    """The fit on the U and V that hsflow_chain_planes_device leaves on the device, NaN where a pixel was lost."""
    from test_chain_host import chain_fields
    W, H, n = 96, 64, 4
    us, vs, ss = chain_fields(W, H, n, seed=21, pad=0)
    gp = hs.make_gmotion_params("similarity", 3, "auto", values=VALUES)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        U, V, status, _, _ = ctx.chain_planes_device([cuda(x) for x in us], [cuda(x) for x in vs], state=[cuda(s) for s in ss], status=True)
        rec, mask, ru, rv = ctx.global_motion_planes_device(U, V, state=status, mask=True, residual=True, params=gp)
        ctx.synchronize()
        hU, hV, hS = U.cpu().numpy(), V.cpu().numpy(), status.cpu().numpy()
        assert np.isnan(hU).any() and (hS == 0).any()
        want = host_want(hs, hU, hV, hS, gp)
        assert rec_tuple(hs.gmotion_result_from(rec)) == want[0] and want[0][3][3] > 0
        assert np.array_equal(mask.cpu().numpy(), want[1]) and np.array_equal(bits(ru.cpu().numpy()), want[2]) and np.array_equal(bits(rv.cpu().numpy()), want[3])


# ---- G3. ordering ------------------------------------------------------------------------------------------------------------------

def test_behind_real_solves(hs, gpu_ok):
    """After hsflow_solve_async under ITER|EPS -- the owed check may re-run the solve into the other buffer of the flow's two --
    a fit sees the settled flow: it equals a fit made after hsflow_wait_solve; hsflow_wait_solve and hsflow_flow_view_device
    behind an enqueued fit see finished work."""
    import torch
    L = hs._lib.load()
    W, H = 96, 64
    frames = [synth.translating_pair(W, H, seed=5, dx=1.25 * i, dy=-0.5 * i)[1] for i in range(3)]
    dev = [cuda(f) for f in frames]
    gp = hs.make_gmotion_params("affine", 2, "auto", values=VALUES)
    for async_reduce in (0, 1):
        for eps in (3e-2, 5e-3):
            kw = dict(lam=0.1, max_iter=100, term_type=ITER | EPS, epsilon=eps)
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            with hs.HSFlow(W, H, 2, stream=s.cuda_stream) as ctx:
                assert L.hsflow_set_async_reduce(ctx._h, async_reduce) == OK
                ctx.set_sequence_device(dev, "gray_blur", reblur=True)
                ctx.solve_async(**kw)
                got = ctx.global_motion(pair=1, mask=True, residual=True, params=gp)                  # the synchronous form, at once
                ctx.solve_async(**kw)
                assert L.hsflow_wait_solve(ctx._h) == OK
                after = ctx.global_motion(pair=1, mask=True, residual=True, params=gp)
                u, v = ctx.flow(1)
                want = host_want(hs, u, v, None, gp)
                for g in (got, after):
                    assert rec_tuple(g[0]) == want[0] and np.array_equal(g[1], want[1]) and np.array_equal(bits(g[2]), want[2]), (async_reduce, eps)
                assert want[0][3][0] > W * H // 2 and u.any()
                ctx.solve_async(**kw)
                rec, mask, ru, rv = ctx.global_motion(pair=1, mask=True, residual=True, params=gp, device=True)     # the device form
                assert L.hsflow_wait_solve(ctx._h) == OK                 # (behind an enqueued fit: waits for the stream)
                pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
                assert L.hsflow_flow_view_device(ctx._h, 1, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == OK
                assert rec_tuple(hs.gmotion_result_from(rec)) == want[0] and np.array_equal(mask.cpu().numpy(), want[1]), (async_reduce, eps)
                assert np.array_equal(bits(rv.cpu().numpy()), want[3]), (async_reduce, eps)


# ---- G4. the warp by a model -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3])
def test_warp_by_model(hs, gpu_ok, C):
    import torch
    L = hs._lib.load()
    W, H = 260, 37
    rng = np.random.default_rng(C)
    src = rng.integers(0, 256, (H, W) if C == 1 else (H, W, C), dtype=np.uint8)
    ref = rng.integers(0, 256, src.shape, dtype=np.uint8)
    m = np.array([3.25, 0.05, -0.08, -2.5, 0.08, 0.05], F)
    models = [m, hs.gmotion_invert(m), hs.gmotion_compose(m, m), np.array([-300.0, 0, 0, 4.0, 0, 0], F)]
    inside = outside = 0
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for model in models:
            for border in ("constant", "replicate"):
                for t in (1.0, -0.5):
                    want, ws = hs.gmotion_warp_host(model, src, ref=ref, t=t, border=border, fill=(9, 8, 7), return_stats=True)
                    inside, outside = inside + ws.inside, outside + ws.outside
                    got, gs = ctx.gmotion_warp(model, src, ref=ref, t=t, border=border, fill=(9, 8, 7), return_stats=True)     # synchronous
                    assert np.array_equal(got, want) and bytes(gs) == bytes(ws), (C, border, t)
                for off, stride in ((0, (C * W + 3) // 4 * 4), (1, C * W + 3)):
                    dsrc, dref = DevIn(src.reshape(H, -1), off, stride), DevIn(ref.reshape(H, -1), off, stride)
                    dst, ds = DevPlane(H, C * W, off, stride), dev_stats()
                    wp = hs.make_warp_params(C, 1.0, border, (9, 8, 7))
                    want, ws = hs.gmotion_warp_host(model, src, ref=ref, params=wp, return_stats=True)
                    mm = (ctypes.c_float * 6)(*[float(x) for x in model])
                    assert L.hsflow_gmotion_warp_device(ctx._h, mm, ctypes.byref(wp), dsrc.ptr, stride, dref.ptr, stride, dst.ptr, stride, ctypes.c_void_p(ds.data_ptr())) == OK
                    ctx.synchronize()
                    rows, clean = dst.rows_and_rest()
                    assert np.array_equal(rows, want.reshape(H, -1)) and clean, (C, border, off)
                    assert bytes(hs.warp_stats_from(ds)) == bytes(ws) and bool((ds[64:] == FILL).all().item())
    assert inside > 0 and outside > 0


# ---- G5. Python round trip -------------------------------------------------------------------------------------------------------

def test_python_global_motion_and_stabilize(hs, gpu_ok):
    """A textured frame moved by a known similarity: solve, fit, and warp the second frame back by the model alone."""
    W, H = 160, 120
    prev, curr = synth.translating_pair(W, H, seed=8, dx=1.5, dy=-1.0)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(prev, curr)
        ctx.solve(lam=0.02, max_iter=400, term_type=ITER)
        u, v = ctx.flow()
        rec, mask, ru, rv = ctx.global_motion(mask=True, residual=True, params=hs.make_gmotion_params("translation", 3, "auto"))
        want = hs.global_motion_host(u, v, mask=True, residual=True, params=hs.make_gmotion_params("translation", 3, "auto"))
        assert rec_tuple(rec) == rec_tuple(want[0]) and np.array_equal(mask, want[1]) and np.array_equal(bits(ru), bits(want[2]))
        out, model = ctx.stabilize(curr, params=hs.make_gmotion_params("translation", 3, "auto"), return_model=True)
        assert rec_tuple(model) == rec_tuple(rec)
        assert np.array_equal(out, hs.gmotion_warp_host(model, curr))
        dout = ctx.stabilize(cuda(curr), params=hs.make_gmotion_params("translation", 3, "auto"))
        ctx.synchronize()
        assert np.array_equal(dout.cpu().numpy(), out)


# ---- G6. the command line ----------------------------------------------------------------------------------------------------------

def test_cli_stabilised_frame(hs, gpu_ok, tmp_path):
    """HSFLOW_PICTURE=stab on a synthetic PPM pair: the file the Python path produces from the same frames, by either route."""
    from test_gpu_warp import _cli
    W, H = 96, 64
    A, B = synth.translating_pair(W, H, seed=1)
    tint = np.array([1.0, 0.8, 0.6])
    frames = [np.clip(np.rint(g[..., None] * tint), 0, 255).astype(np.uint8) for g in (A, B)]   # a small colour pair
    names = [str(tmp_path / ("frame%d.ppm" % k)) for k in range(2)]
    for name, f in zip(names, frames):
        with open(name, "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (W, H) + f.tobytes())
    head = len(b"P6\n%d %d\n255\n" % (W, H))
    for args in (["-cv", "-hd", names[0], names[1], None, ".1", "100"], ["-cl", "-hd", names[0], names[1], None, "3", "50", "1", "GPU"]):
        for choice, gp in ((None, hs.make_gmotion_params()), ("similarity,2,auto", hs.make_gmotion_params("similarity", 2, "auto")),
                           ("translation,1,0.5", hs.make_gmotion_params("translation", 1, "fixed", 0.5))):
            files, lines = {}, {}
            extra = {"HSFLOW_GMOTION": choice} if choice else {}
            for route, env in (("host", {}), ("device", {"HSFLOW_RENDER_DEVICE": "1"})):
                out = str(tmp_path / ("%s_%s.ppm" % (args[0][1:], route)))
                r = _cli([out if a is None else a for a in args], dict(env, HSFLOW_PICTURE="stab", **extra))
                files[route] = open(out, "rb").read()
                lines[route] = [ln for ln in r.stdout.splitlines() if ln.startswith("stab:")]
                assert len(lines[route]) == 1
            assert files["host"] == files["device"] and lines["host"] == lines["device"]
            words = lines["host"][0].split()
            assert words[1] == "model" and words[8] == "inliers" and 0.0 <= float(words[9]) <= 1.0
            if args[0] == "-cv":                                   # the library's own solve of the same frames, through Python
                with hs.HSFlow(W, H, own_stream=True) as ctx:
                    ctx.set_frames_bgr(np.ascontiguousarray(frames[0][..., ::-1]), np.ascontiguousarray(frames[1][..., ::-1]), blur=True)
                    ctx.solve(lam=0.1, max_iter=100)
                    want, model = ctx.stabilize(frames[1], params=gp, return_model=True)
                pic = np.frombuffer(files["host"][head:], np.uint8).reshape(H, W, 3)
                assert np.array_equal(pic, want)
                assert [float(w) for w in words[2:8]] == [float("%.9g" % x) for x in model.p]
                assert abs(float(words[9]) - model.cls[0] / float(W * H)) < 1e-4
    for bad in ({"HSFLOW_PICTURE": "stab", "HSFLOW_GMOTION": "rigid"}, {"HSFLOW_GMOTION": "affine,9"}, {"HSFLOW_GMOTION": "affine,2,0"},
                {"HSFLOW_GMOTION": "affine,2,auto,1"}):
        r = _cli(["-cv", "-hd", names[0], names[1], str(tmp_path / "bad.ppm"), ".1", "10"], bad, ok=False)
        assert r.returncode == 1 and "HSFLOW_GMOTION" in r.stdout
    r = _cli(["-cv", "-cam"], {"HSFLOW_PICTURE": "stab"}, ok=False)
    assert r.returncode == 1 and "HSFLOW_PICTURE=stab needs a pair of files" in r.stdout


def test_cli_model_of_the_chained_flow(hs, gpu_ok, tmp_path):
    """HSFLOW_CAMERA_CHAIN=1 on the batched camera route prints, per batch, the model fitted to the accumulated flow; HSFLOW_GMOTION
    selects the fit."""
    from test_gpu_chain import run_cli
    W, H = 160, 96
    frames = [synth.translating_pair(W, H, seed=77, dx=1.5 * i, dy=-0.75 * i)[1] for i in range(4)]
    cam = tmp_path / "cam"
    cam.mkdir()
    for i, f in enumerate(frames):
        with open(str(cam / ("frame_%04d.pgm" % i)), "wb") as fh:
            fh.write(b"P5\n%d %d\n255\n" % (W, H) + np.ascontiguousarray(f, np.uint8).tobytes())
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        ctx.set_pair_termination(True)
        ctx.set_sequence_device([cuda(f) for f in frames], "gray_blur", reblur=True)
        ctx.solve(lam=0.1, max_iter=12, term_type=ITER | EPS, epsilon=float(np.float32(1e-6)))
        flows = [ctx.flow(p) for p in range(3)]
    U, V, _, _, _ = hs.chain_flow_host([f[0] for f in flows], [f[1] for f in flows])
    for k, (choice, gp) in enumerate(((None, hs.make_gmotion_params()), ("translation,2,auto", hs.make_gmotion_params("translation", 2, "auto")))):
        extra = {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_CHAIN": "1"}
        if choice:
            extra["HSFLOW_GMOTION"] = choice
        _, r = run_cli(cam, tmp_path / ("out%d" % k), extra)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("chain ")]
        want = hs.global_motion_host(U, V, params=gp)[0]
        assert lines == ["chain 0003: model " + " ".join("%.9g" % x for x in want.p) + " inliers %.4f" % (want.cls[0] / float(W * H))], (lines, want.as_dict())
    _, r = run_cli(cam, tmp_path / "plain", {"HSFLOW_CAMERA_BATCH": "3"})
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("chain ")]
    _, r = run_cli(cam, tmp_path / "bad", {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_CHAIN": "1", "HSFLOW_GMOTION": "rigid"}, ok=False)
    assert r.returncode == 1 and "HSFLOW_GMOTION" in r.stdout
