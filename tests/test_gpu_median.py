"""The median filter and the hole filling of the flow on the GPU (include/hsflow.h, ABI 0.19: hsflow_median*,
hsflow_pipeline_median*; kernel in opticalflowhs_amd/csrc/hs_kernels_median.hip.h) against the rule on the host
(hsflow_median_host, which tests/test_median_host.py holds to a NumPy restatement).  Flow planes are compared bit for bit,
states byte for byte, records exactly."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from opticalflowhs_amd import synth
from test_gpu_fb import DevPlane, FILL, _batch_max, dev_stats, put_flow, same_bits
from test_median_host import SHAPES as HOST_SHAPES, field, stat_tuple

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
OK, E_ARG, E_SIZE, E_STATE = 0, 1, 2, 5
# The kernel's tile is kMedTileX x kMedTileY = 64 x 16 pixels (hs_kernels_median.hip.h): 150 x 41 spans three tiles either
# way with ragged ends (22 columns, 9 rows).  2050 x 530 has 33 x 34 = 1122 tiles: with statistics a workgroup then takes
# two tiles (hs_median.hip.h gives a workgroup several once there are more than four per compute unit).
SHAPES = HOST_SHAPES + [(1030, 70), (150, 41)]
BIG_SHAPE = (2050, 530)
CASES = [(1, "filter", 1), (1, "fill", 2), (2, "filter", 5), (2, "fill", 1)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def host_want(hs, u, v, state, passes=1, **kw):
    """(u bits, v bits, state, statistics tuple) of the host rule."""
    uo, vo, so, rec = hs.median_host(u, v, state, state_out=True, stats=True, passes=passes, **kw)
    return bits(uo), bits(vo), so, stat_tuple(rec)


def cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def view(hs, ctx, W, H, pair=0):
    """hsflow_flow_view_device: the context's own flow planes as CUDA tensors (no copy)."""
    import torch
    from opticalflowhs_amd.pipeline import _DeviceView
    pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    assert hs._lib.load().hsflow_flow_view_device(ctx._h, pair, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == OK
    return tuple(torch.as_tensor(_DeviceView(p.value, (H, W), (sb.value, 4)), device="cuda") for p in (pu, pv))


# ---- 1. device against host ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SHAPES + [BIG_SHAPE])
def test_device_equals_host(hs, gpu_ok, W, H):
    u, v, state = field(W, H, 11 * W + H)
    ds = cuda(state)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for radius, mode, votes in (CASES if (W, H) != BIG_SHAPE else CASES[2:]):
            kw = dict(radius=radius, mode=mode, min_votes=votes)
            for st, dst in ((state, ds), (None, None)):
                wu, wv, ws, wstats = host_want(hs, u, v, st, **kw)
                gu, gv, gs, rec = ctx.median(0, dst, state_out=True, stats=True, device=True, **kw)       # device memory, enqueued
                ctx.synchronize()
                case = (radius, mode, votes, st is not None)
                assert np.array_equal(bits(gu.cpu().numpy()), wu) and np.array_equal(bits(gv.cpu().numpy()), wv), case
                assert np.array_equal(gs.cpu().numpy(), ws), case
                assert stat_tuple(hs.median_stats_from(rec)) == wstats, case
                assert bytes(rec[40:64].cpu().numpy()) == b"\0" * 24
                gu, gv, gs, rec = ctx.median(0, st, state_out=True, stats=True, **kw)                    # host memory, synchronous
                assert np.array_equal(bits(gu), wu) and np.array_equal(bits(gv), wv) and np.array_equal(gs, ws) and stat_tuple(rec) == wstats, case
        fu, fv = ctx.flow()                                            # the flow is read and never changed
        assert same_bits(fu, u) and same_bits(fv, v)


def test_each_output_alone(hs, gpu_ok):
    W, H = 150, 41
    u, v, state = field(W, H, 5)
    kw = dict(radius=2, mode="fill", min_votes=2)
    wu, wv, ws, wstats = host_want(hs, u, v, state, **kw)
    ds = cuda(state)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for device in (False, True):
            for want_flow, want_state, want_stats in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
                gu, gv, gs, rec = ctx.median(0, ds if device else state, flow=bool(want_flow), state_out=bool(want_state), stats=bool(want_stats),
                                             device=device, **kw)
                ctx.synchronize()
                case = (device, want_flow, want_state, want_stats)
                assert (gu is None) == (not want_flow) and (gv is None) == (not want_flow) and (gs is None) == (not want_state) and (rec is None) == (not want_stats)
                host = lambda t: t.cpu().numpy() if device else t
                if want_flow:
                    assert np.array_equal(bits(host(gu)), wu) and np.array_equal(bits(host(gv)), wv), case
                if want_state:
                    assert np.array_equal(host(gs), ws), case
                if want_stats:
                    assert stat_tuple(hs.median_stats_from(rec) if device else rec) == wstats, case


# ---- 2. alignment and strides ---------------------------------------------------------------------------------------------

def test_alignment_and_strides(hs, gpu_ok):
    """Byte planes at odd addresses, fp32 outputs that are 4- but not 16-byte aligned, strides that are no multiples of
    16, and canaries behind every row and plane."""
    import torch
    L = hs._lib.load()
    W, H = 150, 41
    u, v, state = field(W, H, 9)
    layouts = [((1, W + 1), (4, 4 * W + 4), (3, W + 5)), ((3, W), (8, 4 * W + 12), (1, W + 2)), ((2, W + 7), (12, 4 * W), (0, W)),
               ((0, (W + 3) // 4 * 4), (0, (4 * W + 15) // 16 * 16), (5, W + 3))]   # (state in, flow out, state out): (offset from a 256-byte multiple, stride)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for k, ((soff, sstride), (foff, fstride), (ooff, ostride)) in enumerate(layouts):
            radius, mode, votes = CASES[k]
            mp = hs.make_median_params(radius, mode, votes)
            wu, wv, ws, wstats = host_want(hs, u, v, state, radius=radius, mode=mode, min_votes=votes)
            din = DevPlane(H, W, soff, sstride)
            rows = din.buf[din.base:din.base + H * sstride].view(H, sstride)
            rows[:, :W] = cuda(state)
            du, dv, dso, drec = DevPlane(H, 4 * W, foff, fstride), DevPlane(H, 4 * W, foff, fstride), DevPlane(H, W, ooff, ostride), dev_stats()
            torch.cuda.synchronize()
            assert L.hsflow_median_device(ctx._h, 0, ctypes.byref(mp), din.ptr, sstride, du.ptr, dv.ptr, fstride, dso.ptr, ostride,
                                          ctypes.c_void_p(drec.data_ptr())) == OK
            ctx.synchronize()
            for plane, want in ((du, wu), (dv, wv)):
                got, clean = plane.rows_and_rest()
                assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), want), (k, int((np.ascontiguousarray(got).view(np.uint32) != want).sum()))
                assert clean, k                                         # nothing beyond W floats of a row
            got, clean = dso.rows_and_rest()
            assert np.array_equal(got, ws) and clean, k                 # nothing beyond W bytes of a row
            got, clean = din.rows_and_rest()
            assert np.array_equal(got, state) and clean, k              # the input is only read
            assert stat_tuple(hs.median_stats_from(drec)) == wstats
            assert bool((drec[64:] == FILL).all().item())


# ---- 3. batch and chunking ------------------------------------------------------------------------------------------------

def test_batch_and_chunking(hs, gpu_ok):
    """Batches of 1 .. 3 pairs with HSFLOW_JPEG_BATCH_MAX=2: output i does not depend on n, position or chunking."""
    import torch
    W, H, N = 96, 64, 4
    fields = [field(W, H, 60 + p) for p in range(N)]
    kw = dict(radius=2, mode="fill", min_votes=3)
    wants = [host_want(hs, *fields[p], **kw) for p in range(N)]
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, fields[p][0], fields[p][1], pair=p)
        for value in ("2", None, "1"):
            with _batch_max(value):
                for first, n in ((0, 1), (3, 1), (1, 2), (0, 3), (1, 3), (0, 4)):
                    states = cuda(np.stack([fields[first + i][2] for i in range(n)]))
                    uo = torch.full((n, H, W), -7.0, dtype=torch.float32, device="cuda")
                    vo = torch.full((n, H, W), -7.0, dtype=torch.float32, device="cuda")
                    so = torch.full((n, H, W), FILL, dtype=torch.uint8, device="cuda")
                    rec = dev_stats(n)
                    ctx.median_batch_device(first, n, state=states, u_out=uo, v_out=vo, state_out=so, stats=rec, **kw)
                    ctx.synchronize()
                    got = hs.median_stats_from(rec, n)
                    got = got if n > 1 else [got]
                    for i in range(n):
                        w = wants[first + i]
                        case = (value, first, n, i)
                        assert np.array_equal(bits(uo[i].cpu().numpy()), w[0]) and np.array_equal(bits(vo[i].cpu().numpy()), w[1]), case
                        assert np.array_equal(so[i].cpu().numpy(), w[2]) and stat_tuple(got[i]) == w[3], case
                    assert bool((rec[64 * n:] == FILL).all().item())   # records 64 bytes apart, nothing behind the last
                rec = dev_stats(3)
                ctx.median_batch_device(1, 3, stats=rec, radius=1)     # statistics only, no state plane
                ctx.synchronize()
                assert [stat_tuple(g) for g in hs.median_stats_from(rec, 3)] == [host_want(hs, fields[p][0], fields[p][1], None, radius=1)[3] for p in (1, 2, 3)]
        with _batch_max("0"):
            with pytest.raises(hs.HsflowError) as e:
                ctx.median_batch_device(0, 2, stats=dev_stats(2))
            assert e.value.status == E_ARG and "HSFLOW_JPEG_BATCH_MAX" in str(e.value)


# ---- 4. chained passes, apply ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius,mode", [(1, "fill"), (2, "filter")])
def test_planes_chained_equal_apply_equal_host(hs, gpu_ok, radius, mode):
    W, H = 150, 41
    u, v, state = field(W, H, 21)
    kw = dict(radius=radius, mode=mode, min_votes=2)
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        cu, cv, cs, ds = cuda(u), cuda(v), cuda(state), cuda(state)
        for k in range(1, 5):
            wu, wv, ws, wstats = host_want(hs, u, v, state, passes=k, **kw)
            cu, cv, cs, crec = ctx.median_planes_device(cu, cv, cs, state_out=True, stats=True, **kw)   # pass k of the chain
            ctx.synchronize()
            assert np.array_equal(bits(cu.cpu().numpy()), wu) and np.array_equal(bits(cv.cpu().numpy()), wv), k
            assert np.array_equal(cs.cpu().numpy(), ws) and stat_tuple(hs.median_stats_from(crec)) == wstats, k
            put_flow(ctx, u, v, pair=1)
            so, rec = ctx.median_apply(1, ds, passes=k, state_out=True, stats=True, **kw)
            fu, fv = ctx.flow(1)
            assert np.array_equal(bits(fu), wu) and np.array_equal(bits(fv), wv), k
            assert np.array_equal(so.cpu().numpy(), ws) and stat_tuple(hs.median_stats_from(rec)) == wstats, k
        # the synchronous form with several passes, on the other pair; its flow stays
        put_flow(ctx, u, v, pair=0)
        for k in (1, 2, 3):
            wu, wv, ws, wstats = host_want(hs, u, v, state, passes=k, **kw)
            gu, gv, gs, grec = ctx.median(0, state, state_out=True, stats=True, passes=k, **kw)
            assert np.array_equal(bits(gu), wu) and np.array_equal(bits(gv), wv) and np.array_equal(gs, ws) and stat_tuple(grec) == wstats, k
            assert stat_tuple(ctx.median(0, state, flow=False, stats=True, passes=k, **kw)[3]) == wstats
        fu, fv = ctx.flow(0)
        assert same_bits(fu, u) and same_bits(fv, v)


# ---- 5. after median_apply ---------------------------------------------------------------------------------------------------

def test_after_apply_everything_reads_the_new_flow(hs, gpu_ok):
    W, H = 150, 41
    A, B = synth.translating_pair(W, H, seed=1)
    u, v, state = field(W, H, 33, special=False)
    kw = dict(radius=1, mode="filter", min_votes=1)
    wu, wv, _, _ = host_want(hs, u, v, state, passes=3, **kw)
    want_u, want_v = wu.view(np.float32), wv.view(np.float32)
    solve = dict(lam=0.1, max_iter=20, term_type=ITER, use_previous=True)
    with hs.HSFlow(W, H, own_stream=True) as ctx, hs.HSFlow(W, H, own_stream=True) as other:
        ctx.set_frames(A, B)
        ctx.solve(lam=0.1, max_iter=20, term_type=ITER)               # (a cached graph, and the planes in the solver's hands)
        put_flow(ctx, u, v)
        ds = cuda(state)
        ctx.median_apply(0, ds, passes=3, **kw)
        vu, vv = view(hs, ctx, W, H)                                   # the view waits for the passes
        assert np.array_equal(bits(vu.cpu().numpy()), wu) and np.array_equal(bits(vv.cpu().numpy()), wv)
        assert np.array_equal(ctx.color(), hs.color_flow_host(want_u, want_v))
        ctx.solve(**solve)
        got = ctx.flow()
        other.set_frames(A, B)
        other.solve(lam=0.1, max_iter=20, term_type=ITER)
        put_flow(other, want_u, want_v)
        other.solve(**solve)
        ref = other.flow()
        assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1])
        assert not same_bits(got[0], want_u)


# ---- 6. ordering ---------------------------------------------------------------------------------------------------------------

def test_every_form_reads_the_final_flow_behind_an_owed_check(hs, gpu_ok):
    """hsflow_solve_async under ITER|EPS with epsilons that fire early: the owed check re-runs the solve, which may end in
    the other buffer of the flow's two; every form settles first and only then names the planes.  With and without
    hsflow_set_pair_termination, and on a context with hsflow_set_async_reduce."""
    import torch
    L = hs._lib.load()
    W, H = 96, 64
    A, B = synth.translating_pair(W, H, seed=1)
    mkw = dict(radius=1, mode="filter", min_votes=1)
    for async_reduce, per_pair in ((0, False), (1, False), (0, True)):
        for eps in (3e-2, 5e-3):
            kw = dict(lam=0.1, max_iter=100, term_type=ITER | EPS, epsilon=eps)
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            with hs.HSFlow(W, H, 2, stream=s.cuda_stream) as ctx:
                assert L.hsflow_set_async_reduce(ctx._h, async_reduce) == OK
                ctx.set_pair_termination(per_pair)
                ctx.set_frames(A, B, pair=0)
                ctx.set_frames_reversed(1, 0)
                info = ctx.solve(**kw)
                if not per_pair:
                    assert 1 < info["iterations_done"] < 100, info     # its early stop fires
                flows = [ctx.flow(p) for p in range(2)]
                wants = [host_want(hs, flows[p][0], flows[p][1], None, **mkw) for p in range(2)]
                wants2 = [host_want(hs, flows[p][0], flows[p][1], None, passes=2, **mkw) for p in range(2)]
                case = (async_reduce, per_pair, eps)
                ctx.solve_async(**kw)
                gu, gv, gs, rec = ctx.median(1, state_out=True, stats=True, **mkw)                   # the synchronous form, at once
                assert np.array_equal(bits(gu), wants[1][0]) and np.array_equal(bits(gv), wants[1][1]) and stat_tuple(rec) == wants[1][3], case
                after = [ctx.flow(p) for p in range(2)]
                assert all(same_bits(a, b) for p in range(2) for a, b in zip(after[p], flows[p])), case
                ctx.solve_async(**kw)
                gu, gv, gs, rec = ctx.median(0, stats=True, device=True, **mkw)                       # the device form
                ctx.synchronize()
                assert np.array_equal(bits(gu.cpu().numpy()), wants[0][0]) and stat_tuple(hs.median_stats_from(rec)) == wants[0][3], case
                ctx.solve_async(**kw)
                uo = torch.zeros((2, H, W), dtype=torch.float32, device="cuda")
                vo = torch.zeros((2, H, W), dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                ctx.median_batch_device(0, 2, u_out=uo, v_out=vo, **mkw)                             # the batch
                assert L.hsflow_wait_solve(ctx._h) == OK
                ctx.synchronize()
                for p in range(2):
                    assert np.array_equal(bits(uo[p].cpu().numpy()), wants[p][0]) and np.array_equal(bits(vo[p].cpu().numpy()), wants[p][1]), case
                ctx.solve_async(**kw)
                ctx.median_apply(1, passes=2, **mkw)                                                 # in place
                fu, fv = ctx.flow(1)
                assert np.array_equal(bits(fu), wants2[1][0]) and np.array_equal(bits(fv), wants2[1][1]), case
                fu, fv = ctx.flow(0)
                assert same_bits(fu, flows[0][0]) and same_bits(fv, flows[0][1]), case


# ---- 7. pipeline ------------------------------------------------------------------------------------------------------------

def test_pipeline(hs, gpu_ok):
    import torch
    W, H = 96, 64
    kw = dict(lam=0.1, max_iter=60, term_type=ITER)
    A, B = synth.translating_pair(W, H, seed=1)
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        ctx.solve(**kw)
        u, v = ctx.flow()
    rng = np.random.default_rng(4)
    state = (rng.random((H, W)) < 0.8).astype(np.uint8) * 255
    mkw = dict(radius=2, mode="fill", min_votes=2)
    want = host_want(hs, u, v, state, passes=2, **mkw)
    dA, dB = cuda(A), cuda(B)
    with hs.PairPipeline(W, H, depth=2, lanes=2) as pl:
        t0 = pl.submit_device(dA, dB, **kw)
        t1 = pl.submit_device(dA, dB, **kw)
        gu, gv, gs, rec = pl.median(t0, state, state_out=True, stats=True, passes=2, **mkw)      # host planes; the slot's flow stays
        assert np.array_equal(bits(gu), want[0]) and np.array_equal(bits(gv), want[1]) and np.array_equal(gs, want[2]) and stat_tuple(rec) == want[3]
        ds = cuda(state)
        so, drec = pl.median_apply(t1, ds, passes=2, state_out=True, stats=True, **mkw)          # in place, complete on return
        assert np.array_equal(so.cpu().numpy(), want[2]) and stat_tuple(hs.median_stats_from(drec)) == want[3]
        gu, gv, _, _ = pl.median(t1, None, radius=1, min_votes=9, mode="fill")                  # (nothing unknown, nothing to fill: the slot's flow as it is)
        assert np.array_equal(bits(gu), want[0]) and np.array_equal(bits(gv), want[1])
        gu, gv, _, _ = pl.median(t0, None, radius=1, min_votes=9, mode="fill")
        assert same_bits(gu, u) and same_bits(gv, v)
        t2 = pl.submit_device(dA, dB, **kw)
        t3 = pl.submit_device(dA, dB, **kw)
        for call in (lambda: pl.median(t0, state), lambda: pl.median_apply(t1, ds)):    # a slot has been reused since
            with pytest.raises(hs.HsflowError) as e:
                call()
            assert e.value.status == E_STATE
        assert stat_tuple(pl.median(t3, state, flow=False, stats=True, passes=2, **mkw)[3]) == want[3]   # the pipeline still works
        pl.wait(t2)


# ---- 8. end to end --------------------------------------------------------------------------------------------------------------

def test_end_to_end_fill_from_the_fb_mask(hs, gpu_ok):
    """A synthetic pair solved forwards and backwards, the hsflow_fb mask as the state, FILL: record and planes are those of
    the host chain."""
    W, H = 150, 70
    A, B = synth.translating_pair(W, H, seed=2)
    mkw = dict(radius=2, mode="fill", min_votes=3)
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        ctx.set_frames(A, B, pair=0)
        ctx.set_frames_reversed(1, 0)
        ctx.solve(lam=0.1, max_iter=100, term_type=ITER)
        (uf, vf), (ub, vb) = ctx.flow(0), ctx.flow(1)
        mask_host = hs.fb_host(uf, vf, ub, vb, beta=0.02)[0]
        want = host_want(hs, uf, vf, mask_host, passes=3, **mkw)
        mask = ctx.fb(0, 1, mask=True, beta=0.02, device=True)[0]
        so, rec = ctx.median_apply(0, mask, passes=3, state_out=True, stats=True, **mkw)
        fu, fv = ctx.flow(0)
        rec = hs.median_stats_from(rec)
        print("fb mask: %d of %d untrusted; after 3 passes: kept %d filled %d unfilled %d" % (int((mask_host == 0).sum()), W * H, rec.kept, rec.filled, rec.unfilled))
        assert 0 < int((mask_host == 0).sum()) < W * H
        assert np.array_equal(mask.cpu().numpy(), mask_host)
        assert np.array_equal(bits(fu), want[0]) and np.array_equal(bits(fv), want[1]) and np.array_equal(so.cpu().numpy(), want[2])
        assert stat_tuple(rec) == want[3] and rec.filled > 0
        bu, bv = ctx.flow(1)
        assert same_bits(bu, ub) and same_bits(bv, vb)


# ---- 9. command line ----------------------------------------------------------------------------------------------------------

def _cli(args, extra_env=None, ok=True):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for name in ("HSFLOW_RENDER_DEVICE", "HSFLOW_JPEG_DEVICE", "HSFLOW_PICTURE", "HSFLOW_COLOR_MAX", "HSFLOW_WARP_T", "HSFLOW_FB_ALPHA", "HSFLOW_FB_BETA",
                 "HSFLOW_MEDIAN"):
        env.pop(name, None)
    env.update(extra_env or {})
    r = subprocess.run([cli] + args, env=env, capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_cli(hs, gpu_ok, tmp_path):
    W, H = 96, 64
    A, B = synth.translating_pair(W, H, seed=1)
    tint = np.array([1.0, 0.8, 0.6])
    frames = [np.clip(np.rint(g[..., None] * tint), 0, 255).astype(np.uint8) for g in (A, B)]   # a small colour pair
    names = [str(tmp_path / ("frame%d.ppm" % k)) for k in range(2)]
    for name, f in zip(names, frames):
        with open(name, "wb") as fh:
            fh.write(b"P6\n%d %d\n255\n" % (W, H) + f.tobytes())
    head = b"P6\n%d %d\n255\n" % (W, H)
    args = lambda out: ["-cv", "-hd", names[0], names[1], out, ".1", "100"]

    def chain(fill, radius, passes, beta=None):
        """The picture and the record of the Python chain."""
        with hs.HSFlow(W, H, 2 if fill else 1, own_stream=True) as ctx:
            ctx.set_frames_bgr(np.ascontiguousarray(frames[0][..., ::-1]), np.ascontiguousarray(frames[1][..., ::-1]), blur=True)
            if fill:
                ctx.set_frames_reversed(1, 0)
            ctx.solve(lam=0.1, max_iter=100)
            rec = None
            if fill:
                mask = ctx.fb(0, 1, mask=True, device=True, **(dict(beta=beta) if beta is not None else {}))[0]
                _, rec = ctx.median_apply(0, mask, passes=passes, stats=True, radius=radius, mode="fill")
            elif radius:
                ctx.median_apply(0, passes=passes, radius=radius)
            pic = ctx.color()
            return pic, (hs.median_stats_from(rec) if rec is not None else None)

    plain, _ = chain(False, 0, 0)
    files = {}
    for value, fill, radius, passes, extra in ((None, False, 0, 0, {}), ("1", False, 1, 1, {}), ("2,3", False, 2, 3, {}), ("2,3,fill", True, 2, 3, {}),
                                               ("1,2,fill", True, 1, 2, {"HSFLOW_FB_BETA": "0.02"})):
        pic, rec = chain(fill, radius, passes, 0.02 if extra else None)
        for route, env in (("host", {}), ("device", {"HSFLOW_RENDER_DEVICE": "1"})):
            out = str(tmp_path / ("out_%s_%s.ppm" % (value, route)))
            envs = dict(env, HSFLOW_PICTURE="color", **extra)
            if value is not None:
                envs["HSFLOW_MEDIAN"] = value
            r = _cli(args(out), envs)
            data = open(out, "rb").read()
            assert data == head + np.ascontiguousarray(pic).tobytes(), (value, route)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("median:")]
            assert len(lines) == (1 if fill else 0), r.stdout
            if fill:
                words = lines[0].split()
                assert words[1::2] == ["kept", "filled", "unfilled", "newly_filled", "changed"]
                assert [int(x) for x in words[2::2]] == list(stat_tuple(rec)), (value, route)
        files[value] = data
    assert files[None] == head + np.ascontiguousarray(plain).tobytes()   # with the variable unset: the file as it always was
    assert len(set(files.values())) == len(files)
    for bad in ("0", "3", "1,0", "1,65", "1,2,full", "1,2,fill,", "x", "1,", ",2", "2;3"):
        r = _cli(args(str(tmp_path / "bad.ppm")), {"HSFLOW_MEDIAN": bad}, ok=False)
        assert r.returncode == 1 and "HSFLOW_MEDIAN" in r.stdout, bad
    for route in (["-cv", "-cam"], ["-cl", "-cam", "x", "3", "5", "1", "GPU"]):
        r = _cli(route, {"HSFLOW_MEDIAN": "1"}, ok=False)
        assert r.returncode == 1 and "HSFLOW_MEDIAN" in r.stdout


# ---- 10. errors ----------------------------------------------------------------------------------------------------------------

def test_argument_errors(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, N = 64, 4, 2
    u, v, state = field(W, H, 3)
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, u, v, pair=p)
        uo = torch.full((N, H, W + 1), -7.0, dtype=torch.float32, device="cuda")
        vo = torch.full((N, H, W + 1), -7.0, dtype=torch.float32, device="cuda")
        so = torch.full((N, H, W), FILL, dtype=torch.uint8, device="cuda")
        st = cuda(np.stack([state, state]))
        planes = torch.zeros((2, H, W), dtype=torch.float32, device="cuda")
        stats = dev_stats(N)
        torch.cuda.synchronize()
        lst = lambda ptrs: (ctypes.c_void_p * N)(*ptrs)
        ul, vl, sl, il = (lst([t[i].data_ptr() for i in range(N)]) for t in (uo, vo, so, st))
        holed = (ctypes.c_void_p * N)(ul[0], None)
        sp = ctypes.c_void_p(stats.data_ptr())
        os_ = (W + 1) * 4
        pu, pv = ctypes.c_void_p(planes[0].data_ptr()), ctypes.c_void_p(planes[1].data_ptr())
        dev = lambda mp, p=0, i=il[0], is_=W, a=ul[0], b=vl[0], fs=os_, s=sl[0], ss=W, r=sp, h=ctx._h: L.hsflow_median_device(h, p, mp, i, is_, a, b, fs, s, ss, r)
        bat = lambda mp, f=0, n=N, i=il, is_=W, a=ul, b=vl, fs=os_, s=sl, ss=W, r=sp: L.hsflow_median_batch_device(ctx._h, f, n, mp, i, is_, a, b, fs, s, ss, r)
        pln = lambda mp, x=pu, y=pv, ps=W * 4, i=il[0], is_=W, a=ul[0], b=vl[0], fs=os_, s=sl[0], ss=W, r=sp: L.hsflow_median_planes_device(
            ctx._h, mp, x, y, ps, i, is_, a, b, fs, s, ss, r)
        app = lambda mp, p=0, k=1, i=il[0], is_=W, s=sl[0], ss=W, r=sp: L.hsflow_median_apply(ctx._h, p, mp, k, i, is_, s, ss, r)
        hu, hv, hso = np.full((H, W), -7.0, np.float32), np.full((H, W), -7.0, np.float32), np.full((H, W), FILL, np.uint8)
        hrec = hs.HsflowMedianStats()
        ctypes.memset(ctypes.byref(hrec), FILL, 64)
        syn = lambda mp, p=0, k=1, i=state.ctypes.data, is_=W, a=hu.ctypes.data, b=hv.ctypes.data, fs=W * 4, s=hso.ctypes.data, ss=W: L.hsflow_median(
            ctx._h, p, mp, k, i, is_, a, b, fs, s, ss, ctypes.byref(hrec))
        bad = []
        for change in (dict(struct_size=12), dict(radius=0), dict(radius=3), dict(mode=2), dict(mode=-1), dict(min_votes=0), dict(min_votes=10),
                       dict(radius=2, min_votes=26)):
            b = hs.make_median_params()
            for k, val in change.items():
                setattr(b, k, val)
            bad.append(ctypes.byref(b))
        for b in bad + [None]:
            assert dev(b) == E_ARG and bat(b) == E_ARG and pln(b) == E_ARG and app(b) == E_ARG and syn(b) == E_ARG
        r = ctypes.byref(hs.make_median_params())
        assert dev(r, p=N) == E_ARG and dev(r, p=-1) == E_ARG and dev(r, h=None) == E_ARG and app(r, p=N) == E_ARG and syn(r, p=-1) == E_ARG
        assert bat(r, n=0) == E_ARG and bat(r, n=-1) == E_ARG and bat(r, f=1) == E_ARG and bat(r, f=-1) == E_ARG and bat(r, n=N + 1) == E_ARG
        for k in (0, -1, 65):
            assert app(r, k=k) == E_ARG and syn(r, k=k) == E_ARG
        assert bat(r, a=holed) == E_ARG and bat(r, b=holed) == E_ARG and bat(r, i=holed) == E_ARG and bat(r, s=holed) == E_ARG
        assert dev(r, a=None) == E_ARG and dev(r, b=None) == E_ARG and bat(r, a=None) == E_ARG and pln(r, b=None) == E_ARG   # one flow output without the other
        assert syn(r, a=None) == E_ARG
        assert dev(r, a=None, b=None, s=None, r=None) == E_ARG and bat(r, a=None, b=None, s=None, r=None) == E_ARG            # nothing asked for
        assert pln(r, a=None, b=None, s=None, r=None) == E_ARG
        assert L.hsflow_median(ctx._h, 0, r, 1, None, 0, None, None, 0, None, 0, None) == E_ARG
        assert pln(r, x=None) == E_ARG and pln(r, y=None) == E_ARG and pln(r, x=ctypes.c_void_p(planes[0].data_ptr() + 2)) == E_ARG
        assert pln(r, ps=W * 4 - 4) == E_SIZE and pln(r, ps=W * 4 + 2) == E_SIZE
        # an output that is, or overlaps, an input
        assert pln(r, a=pu) == E_ARG and pln(r, b=pu) == E_ARG and pln(r, a=ctypes.c_void_p(planes[0].data_ptr() + 4 * W)) == E_ARG
        assert dev(r, s=il[0]) == E_ARG and app(r, s=il[0]) == E_ARG and bat(r, s=lst([sl[0], il[0]])) == E_ARG and pln(r, s=il[0]) == E_ARG
        vu, vv = view(hs, ctx, W, H, pair=1)
        assert dev(r, p=1, a=ctypes.c_void_p(vu.data_ptr()), fs=vu.stride(0) * 4) == E_ARG
        assert app(r, p=1, s=ctypes.c_void_p(vv.data_ptr())) == E_ARG
        for odd in (1, 4):                                            # the records are 64-bit counters: 8-byte aligned or refused
            off = ctypes.c_void_p(stats.data_ptr() + odd)
            assert dev(r, r=off) == E_ARG and bat(r, r=off) == E_ARG and pln(r, r=off) == E_ARG and app(r, r=off) == E_ARG
        for odd in (1, 2):                                            # the flow is written as floats
            off = ctypes.c_void_p(uo.data_ptr() + odd)
            assert dev(r, a=off) == E_ARG and pln(r, b=off) == E_ARG and bat(r, a=lst([ul[0], off.value])) == E_ARG
        for f in (dev, bat, pln):
            assert f(r, is_=W - 1) == E_SIZE and f(r, ss=W - 1) == E_SIZE and f(r, fs=W * 4 - 4) == E_SIZE and f(r, fs=W * 4 + 2) == E_SIZE
        assert app(r, is_=W - 1) == E_SIZE and app(r, ss=W - 1) == E_SIZE
        assert syn(r, is_=W - 1) == E_SIZE and syn(r, ss=W - 1) == E_SIZE and syn(r, fs=W * 4 - 4) == E_SIZE and syn(r, fs=W * 4 + 2) == E_SIZE
        with _batch_max("33"):
            assert bat(r) == E_ARG and dev(r) == E_ARG and "HSFLOW_JPEG_BATCH_MAX" in ctx._lib.hsflow_last_error(ctx._h).decode()
        ctx.synchronize()
        assert bool((uo == -7.0).all().item()) and bool((vo == -7.0).all().item()) and bool((so == FILL).all().item()) and bool((stats == FILL).all().item())
        assert (hu == -7.0).all() and (hv == -7.0).all() and (hso == FILL).all() and bytes(hrec) == bytes([FILL]) * 64   # nothing was written
        fu, fv = ctx.flow(0)
        assert same_bits(fu, u) and same_bits(fv, v)
        want = host_want(hs, u, v, state)
        assert syn(r) == OK                                           # the context still works
        assert np.array_equal(bits(hu), want[0]) and np.array_equal(bits(hv), want[1]) and np.array_equal(hso, want[2]) and stat_tuple(hrec) == want[3]
        assert bat(r) == OK
        ctx.synchronize()
        assert np.array_equal(bits(uo[1, :, :W].cpu().numpy()), want[0]) and np.array_equal(so[1].cpu().numpy(), want[2])
