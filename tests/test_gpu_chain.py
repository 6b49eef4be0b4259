"""Pixels and points followed through a sequence of flows on the GPU (include/hsflow.h, ABI 0.22: hsflow_chain_flow*,
hsflow_chain_planes_device, hsflow_track_points*; kernels in opticalflowhs_amd/csrc/hs_kernels_chain.hip.h) against the rule on
the host (hsflow_chain_flow_host, hsflow_track_points_host, which tests/test_chain_host.py holds to a NumPy restatement).
U, V and the tracks are compared bit for bit, status and age byte for byte, statistics exactly."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from opticalflowhs_amd import synth
from test_chain_host import VALUES, chain_fields, point_starts, rotation_plane, start_fields, stat_tuple
from test_gpu_fb import FILL, DevPlane, dev_stats, put_flow, same_bits

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
OK, E_ARG, E_SIZE = 0, 1, 2
SHAPES = [(13, 7), (260, 37), (1027, 9), (96, 64)]
PAIRS = {1: [3], 2: [0, 1], 5: [4, 2, 7, 0, 5], 32: [(5 * k + k // 8) % 8 for k in range(32)]}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


class DevIn(DevPlane):
    """A DevPlane that holds the rows of `arr`."""

    def __init__(self, arr, off, stride):
        import torch
        rows = np.ascontiguousarray(arr).view(np.uint8).reshape(arr.shape[0], -1)
        DevPlane.__init__(self, rows.shape[0], rows.shape[1], off, stride)
        host = np.full(self.buf.numel(), FILL, np.uint8)
        for y in range(self.H):
            host[self.base + y * stride:self.base + y * stride + self.rowb] = rows[y]
        self.buf.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()


def ptr_list(items):
    return (ctypes.c_void_p * len(items))(*[(x.ptr.value if isinstance(x, DevPlane) else x.data_ptr()) if x is not None else None for x in items])


def view(hs, ctx, W, H, pair=0):
    """hsflow_flow_view_device: (u pointer, v pointer, stride in bytes) of the context's own flow planes."""
    pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    assert hs._lib.load().hsflow_flow_view_device(ctx._h, pair, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == OK
    return pu.value, pv.value, sb.value


def host_want(hs, us, vs, state, start, cp):
    U, V, st, ag, rec = hs.chain_flow_host(us, vs, state=state, start=start, status=True, age=True, stats=True, params=cp)
    return bits(U), bits(V), st, ag, stat_tuple(rec)


def check_outputs(hs, outs, ds, want, label):
    """The four DevPlanes and the record of a device call against the host's; nothing written around them."""
    dU, dV, dS, dA = outs
    for d, w in ((dU, want[0]), (dV, want[1])):
        rows, clean = d.rows_and_rest()
        assert np.array_equal(np.ascontiguousarray(rows).view(np.uint32), w), label
        assert clean, label                                                    # nothing beyond W floats of a row
    for d, w in ((dS, want[2]), (dA, want[3])):
        rows, clean = d.rows_and_rest()
        assert np.array_equal(rows, w), label
        assert clean, label                                                    # nothing beyond W bytes of a row
    assert stat_tuple(hs.chain_stats_from(ds)) == want[4], label
    assert bool((ds[64:] == FILL).all().item()) and bytes(ds[44:64].cpu().numpy()) == b"\0" * 20


def layouts(W):
    """(offset from a 256-byte multiple, stride) of a float plane and of a byte plane, four each: 16-byte aligned, 4-byte offset,
    ragged strides; bytes at offsets 0 .. 3."""
    f16 = (4 * W + 15) // 16 * 16
    return [((0, f16), (0, (W + 3) // 4 * 4)), ((4, 4 * W + 4), (1, W + 1)), ((16, 4 * W), (2, W)), ((8, f16 + 16), (3, W + 5))]


# ---- G1. device against host -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SHAPES)
def test_device_equals_host(hs, gpu_ok, W, H):
    L = hs._lib.load()
    us, vs, ss = chain_fields(W, H, 8, seed=1000 * W + H, pad=0)
    start = start_fields(W, H, seed=W + H, pad=0)
    cp = hs.make_chain_params(VALUES)
    lay = layouts(W)
    with hs.HSFlow(W, H, 8, own_stream=True) as ctx:
        for p in range(8):
            put_flow(ctx, us[p], vs[p], pair=p)
        for n, pairs in PAIRS.items():
            ints = (ctypes.c_int * n)(*pairs)
            pu, pv = [us[p] for p in pairs], [vs[p] for p in pairs]
            states = [ss[p] for p in pairs]
            if n > 1:
                states[1] = None
            for combo, (state, st0) in enumerate(((None, None), (states, None), (None, start), (states, start))):
                want = host_want(hs, pu, pv, state, st0, cp)
                label = (W, H, n, combo)
                # the synchronous form, host memory
                gU, gV, gS, gA, rec = ctx.chain_flow(pairs, state=state, start=st0, status=True, age=True, stats=True, params=cp)
                assert np.array_equal(bits(gU), want[0]) and np.array_equal(bits(gV), want[1]) and np.array_equal(gS, want[2]), label
                assert np.array_equal(gA, want[3]) and stat_tuple(rec) == want[4], label
                for k in (combo, (combo + 2) % 4):
                    (foff, fstride), (boff, bstride) = lay[k]
                    dstate = [DevIn(s, boff, bstride) if s is not None else None for s in state] if state is not None else None
                    dstart = [DevIn(x, foff, fstride) for x in st0] if st0 is not None else None
                    outs = [DevPlane(H, 4 * W, foff, fstride), DevPlane(H, 4 * W, foff, fstride), DevPlane(H, W, boff, bstride),
                            DevPlane(H, W, (boff + 1) % 4, bstride)]
                    ds = dev_stats()
                    assert L.hsflow_chain_flow_device(ctx._h, ints, n, ptr_list(dstate) if dstate else None, bstride, dstart[0].ptr if dstart else None,
                                                      dstart[1].ptr if dstart else None, fstride, ctypes.byref(cp), outs[0].ptr, outs[1].ptr, fstride, outs[2].ptr,
                                                      bstride, outs[3].ptr, bstride, ctypes.c_void_p(ds.data_ptr())) == OK, label + (k,)
                    ctx.synchronize()
                    check_outputs(hs, outs, ds, want, label + (k,))
        for p in range(8):                                            # the flows are read and never changed
            u, v = ctx.flow(p)
            assert same_bits(u, us[p]) and same_bits(v, vs[p])


def test_each_output_alone(hs, gpu_ok):
    W, H = 260, 37
    us, vs, ss = chain_fields(W, H, 3, seed=9, pad=0)
    want = host_want(hs, us, vs, ss, None, hs.make_chain_params())
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        for p in range(3):
            put_flow(ctx, us[p], vs[p], pair=p)
        for device in (False, True):
            state = [cuda(s) for s in ss] if device else ss
            for flow, status, age, stats in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 0, 1), (1, 1, 1, 1)):
                gU, gV, gS, gA, rec = ctx.chain_flow(state=state, flow=bool(flow), status=bool(status), age=bool(age), stats=bool(stats), device=device)
                ctx.synchronize()
                get = lambda x: x.cpu().numpy() if device else x
                assert (gU is None) == (not flow) and (gS is None) == (not status) and (gA is None) == (not age) and (rec is None) == (not stats)
                if flow:
                    assert np.array_equal(bits(get(gU)), want[0]) and np.array_equal(bits(get(gV)), want[1]), (device, flow, status, age, stats)
                if status:
                    assert np.array_equal(get(gS), want[2])
                if age:
                    assert np.array_equal(get(gA), want[3])
                if stats:
                    assert stat_tuple(hs.chain_stats_from(rec) if device else rec) == want[4]


def test_repeated_pairs_rotate(hs, gpu_ok):
    """The rotation of tests/test_chain_host.py on a context of one pair named 8 times."""
    W, H, n, theta = 96, 64, 8, 0.02
    ru, rv = rotation_plane(W, H, theta)
    want = host_want(hs, [ru] * n, [rv] * n, None, None, hs.make_chain_params())
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        put_flow(ctx, ru, rv)
        U, V, st, ag, rec = ctx.chain_flow([0] * n, status=True, age=True, stats=True)
    assert np.array_equal(bits(U), want[0]) and np.array_equal(bits(V), want[1]) and np.array_equal(st, want[2]) and np.array_equal(ag, want[3])
    assert stat_tuple(rec) == want[4]
    live = st == 255
    x, y = np.meshgrid(np.arange(W, dtype=np.float64) - (W - 1) / 2.0, np.arange(H, dtype=np.float64) - (H - 1) / 2.0)
    c, s = np.cos(n * theta), np.sin(n * theta)
    err = np.hypot(U - (c * x - s * y - x), V - (s * x + c * y - y))[live]
    assert live.sum() > W * H // 2 and err.max() <= 1e-4


# ---- G2. points ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [1, 255, 256, 257, 4099])
def test_points(hs, gpu_ok, m):
    import torch
    W, H, n = 96, 64, 5
    us, vs, ss = chain_fields(W, H, n, seed=77, pad=0)
    xy = point_starts(W, H, m, seed=m)
    cp = hs.make_chain_params(VALUES)
    with hs.HSFlow(W, H, n, own_stream=True) as ctx:
        for p in range(n):
            put_flow(ctx, us[p], vs[p], pair=p)
        for state in (None, ss):
            for pairs in (None, [4, 4, 0]):
                order = list(range(n)) if pairs is None else pairs
                sub = [state[p] for p in order] if state is not None else None
                wl, wt, wst, wag, wrec = hs.track_points_host([us[p] for p in order], [vs[p] for p in order], xy, state=sub, track=True, status=True, age=True,
                                                              stats=True, params=cp)
                want = (bits(wl), bits(wt), wst, wag, stat_tuple(wrec))
                last, tr, st, ag, rec = ctx.track_points(xy, pairs, state=sub, track=True, status=True, age=True, stats=True, params=cp)   # synchronous
                assert np.array_equal(bits(last), want[0]) and np.array_equal(bits(tr), want[1]) and np.array_equal(st, want[2]), (m, pairs)
                assert np.array_equal(ag, want[3]) and stat_tuple(rec) == want[4], (m, pairs)
                dstate = [cuda(s) for s in sub] if sub is not None else None
                raw = torch.zeros(2 * m + 2, dtype=torch.float32, device="cuda")
                for off in (0, 1):                                      # 8-byte aligned points, and 4 bytes off
                    dxy = raw[off:off + 2 * m].view(m, 2)
                    dxy.copy_(torch.from_numpy(xy))
                    torch.cuda.synchronize()
                    last, tr, st, ag, rec = ctx.track_points(dxy, pairs, state=dstate, track=True, status=True, age=True, stats=True, params=cp)
                    ctx.synchronize()
                    assert np.array_equal(bits(last.cpu().numpy()), want[0]) and np.array_equal(bits(tr.cpu().numpy()), want[1]), (m, pairs, off)
                    assert np.array_equal(st.cpu().numpy(), want[2]) and np.array_equal(ag.cpu().numpy(), want[3]), (m, pairs, off)
                    assert stat_tuple(hs.chain_stats_from(rec)) == want[4], (m, pairs, off)
                last, tr, st, ag, rec = ctx.track_points(dxy, pairs, state=dstate)   # the last positions alone
                ctx.synchronize()
                assert np.array_equal(bits(last.cpu().numpy()), want[0]) and tr is None and st is None and ag is None and rec is None


# ---- G3. the forms agree ---------------------------------------------------------------------------------------------------------

def test_forms_agree(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, n = 260, 37, 5
    us, vs, ss = chain_fields(W, H, n, seed=31, pad=0)
    start = start_fields(W, H, seed=2, pad=0)
    cp = hs.make_chain_params(VALUES)
    want = host_want(hs, us, vs, ss, start, cp)
    with hs.HSFlow(W, H, n, own_stream=True) as ctx:
        for p in range(n):
            put_flow(ctx, us[p], vs[p], pair=p)
        dstate, dstart = [cuda(s) for s in ss], [cuda(x) for x in start]
        got = [ctx.chain_flow(state=ss, start=start, status=True, age=True, stats=True, params=cp),
               ctx.chain_flow(state=dstate, start=dstart, status=True, age=True, stats=True, params=cp)]
        ctx.synchronize()
        views = [view(hs, ctx, W, H, p) for p in range(n)]
        assert len(set(v[2] for v in views)) == 1
        f16 = (4 * W + 15) // 16 * 16
        for planes_u, planes_v, stride in (([v[0] for v in views], [v[1] for v in views], views[0][2]),
                                           ([DevIn(u, 4, 4 * W + 4) for u in us], [DevIn(v, 4, 4 * W + 4) for v in vs], 4 * W + 4),
                                           ([DevIn(u, 0, f16) for u in us], [DevIn(v, 0, f16) for v in vs], f16)):
            lists = [(ctypes.c_void_p * n)(*[x.ptr.value if isinstance(x, DevPlane) else x for x in part]) for part in (planes_u, planes_v)]
            outs = [DevPlane(H, 4 * W, 0, f16), DevPlane(H, 4 * W, 0, f16), DevPlane(H, W, 0, W), DevPlane(H, W, 0, W)]
            ds = dev_stats()
            assert L.hsflow_chain_planes_device(ctx._h, n, lists[0], lists[1], stride, ptr_list(dstate), W, ctypes.c_void_p(dstart[0].data_ptr()),
                                                ctypes.c_void_p(dstart[1].data_ptr()), 4 * W, ctypes.byref(cp), outs[0].ptr, outs[1].ptr, f16, outs[2].ptr, W,
                                                outs[3].ptr, W, ctypes.c_void_p(ds.data_ptr())) == OK
            ctx.synchronize()
            check_outputs(hs, outs, ds, want, stride)
        # and through the Python wrapper of the planes form
        tu = [torch.from_numpy(u).cuda() for u in us]
        tv = [torch.from_numpy(v).cuda() for v in vs]
        torch.cuda.synchronize()
        got.append(ctx.chain_planes_device(tu, tv, state=dstate, start=dstart, status=True, age=True, stats=True, params=cp))
        ctx.synchronize()
    for k, (U, V, st, ag, rec) in enumerate(got):
        get = lambda x: x if isinstance(x, np.ndarray) else x.cpu().numpy()
        assert np.array_equal(bits(get(U)), want[0]) and np.array_equal(bits(get(V)), want[1]) and np.array_equal(get(st), want[2]), k
        assert np.array_equal(get(ag), want[3]) and stat_tuple(rec if k == 0 else hs.chain_stats_from(rec)) == want[4], k


# ---- G4. ordering ------------------------------------------------------------------------------------------------------------------

def test_behind_real_solves(hs, gpu_ok):
    """A 3-pair sequence of a translating texture.  After hsflow_solve_async under ITER|EPS -- the owed check may re-run the
    solve into the other buffer of the flow's two -- with and without hsflow_set_pair_termination and hsflow_set_async_reduce,
    the chain equals the host rule on the flows read afterwards; hsflow_wait_solve and hsflow_flow_view_device behind an
    enqueued chain see finished work; and the same after hsflow_solve_pyramid."""
    import torch
    L = hs._lib.load()
    W, H = 96, 64
    frames = [synth.translating_pair(W, H, seed=5, dx=1.25 * i, dy=-0.5 * i)[1] for i in range(4)]
    dev = [cuda(f) for f in frames]
    cp = hs.make_chain_params(VALUES)
    xy = point_starts(W, H, 300, seed=1)
    for async_reduce, per_pair in ((0, False), (1, False), (0, True), (1, True)):
        for eps in (3e-2, 5e-3):
            kw = dict(lam=0.1, max_iter=100, term_type=ITER | EPS, epsilon=eps)
            case = (async_reduce, per_pair, eps)
            s = torch.cuda.Stream()
            torch.cuda.synchronize()
            with hs.HSFlow(W, H, 3, stream=s.cuda_stream) as ctx:
                assert L.hsflow_set_async_reduce(ctx._h, async_reduce) == OK
                ctx.set_pair_termination(per_pair)
                ctx.set_sequence_device(dev, "gray_blur", reblur=True)
                ctx.solve_async(**kw)
                got = ctx.chain_flow(status=True, age=True, stats=True, params=cp)                    # the synchronous form, at once
                flows = [ctx.flow(p) for p in range(3)]
                assert all(f[0].any() for f in flows)
                us, vs = [f[0] for f in flows], [f[1] for f in flows]
                want = host_want(hs, us, vs, None, None, cp)
                assert np.array_equal(bits(got[0]), want[0]) and np.array_equal(bits(got[1]), want[1]) and np.array_equal(got[2], want[2]), case
                assert np.array_equal(got[3], want[3]) and stat_tuple(got[4]) == want[4], case
                assert want[4][0] > W * H // 2, want[4]
                ctx.solve_async(**kw)
                gU, gV, gS, gA, rec = ctx.chain_flow(status=True, age=True, stats=True, params=cp, device=True)   # the device form
                assert L.hsflow_wait_solve(ctx._h) == OK             # (behind an enqueued chain: waits for the stream)
                view(hs, ctx, W, H, 0)
                assert np.array_equal(bits(gU.cpu().numpy()), want[0]) and np.array_equal(gS.cpu().numpy(), want[2]), case
                assert stat_tuple(hs.chain_stats_from(rec)) == want[4], case
                ctx.solve_async(**kw)
                last, tr, st, ag, prec = ctx.track_points(xy, track=True, status=True, age=True, stats=True, params=cp)
                wl, wt, wst, wag, wrec = hs.track_points_host(us, vs, xy, track=True, status=True, age=True, stats=True, params=cp)
                assert np.array_equal(bits(last), bits(wl)) and np.array_equal(bits(tr), bits(wt)) and np.array_equal(st, wst), case
                assert stat_tuple(prec) == stat_tuple(wrec), case
                after = [ctx.flow(p) for p in range(3)]
                assert all(same_bits(a, b) for p in range(3) for a, b in zip(after[p], flows[p])), case
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        ctx.set_sequence_device(dev, "gray_blur", reblur=True)
        ctx.solve_pyramid(lam=0.1, max_iter=30, term_type=ITER, levels=2)
        gU, gV, gS, gA, rec = ctx.chain_flow(status=True, age=True, stats=True, params=cp, device=True)
        ctx.synchronize()
        flows = [ctx.flow(p) for p in range(3)]
        want = host_want(hs, [f[0] for f in flows], [f[1] for f in flows], None, None, cp)
        assert np.array_equal(bits(gU.cpu().numpy()), want[0]) and np.array_equal(bits(gV.cpu().numpy()), want[1])
        assert np.array_equal(gA.cpu().numpy(), want[3]) and stat_tuple(hs.chain_stats_from(rec)) == want[4]
        got = ctx.chain_flow(status=True, params=cp)
        assert np.array_equal(bits(got[0]), want[0]) and np.array_equal(got[2], want[2])


# ---- G5. refusals leave every output untouched --------------------------------------------------------------------------------------

def test_refusals(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, n = 40, 12, 3
    us, vs, ss = chain_fields(W, H, n, seed=4, pad=0)
    with hs.HSFlow(W, H, n, own_stream=True) as ctx:
        for p in range(n):
            put_flow(ctx, us[p], vs[p], pair=p)
        cp = hs.make_chain_params()
        bad = hs.make_chain_params()
        bad.struct_size += 4
        dstate = [cuda(s) for s in ss]
        dstart = [cuda(us[0]), cuda(vs[0])]
        outs = [DevPlane(H, 4 * W, 0, 4 * W), DevPlane(H, 4 * W, 0, 4 * W), DevPlane(H, W, 0, W), DevPlane(H, W, 0, W)]
        ds = dev_stats()
        fu, fv, fstride = view(hs, ctx, W, H, 1)
        P = lambda t: ctypes.c_void_p(t.data_ptr())

        def dense(**kw):
            a = dict(pairs=(ctypes.c_int * n)(0, 1, 2), n=n, state=ptr_list(dstate), ss=W, U0=P(dstart[0]), V0=P(dstart[1]), s0s=4 * W, cp=ctypes.byref(cp),
                     U=outs[0].ptr, V=outs[1].ptr, os=4 * W, st=outs[2].ptr, sts=W, ag=outs[3].ptr, ags=W, stats=ctypes.c_void_p(ds.data_ptr()))
            a.update(kw)
            return L.hsflow_chain_flow_device(ctx._h, a["pairs"], a["n"], a["state"], a["ss"], a["U0"], a["V0"], a["s0s"], a["cp"], a["U"], a["V"], a["os"], a["st"],
                                              a["sts"], a["ag"], a["ags"], a["stats"])
        cases = [(dict(cp=None), E_ARG), (dict(cp=ctypes.byref(bad)), E_ARG), (dict(n=0), E_ARG), (dict(n=33), E_ARG), (dict(pairs=None), E_ARG),
                 (dict(pairs=(ctypes.c_int * n)(0, 3, 1)), E_ARG), (dict(pairs=(ctypes.c_int * n)(0, -1, 1)), E_ARG), (dict(U0=None), E_ARG), (dict(V0=None), E_ARG),
                 (dict(U=None), E_ARG), (dict(V=None), E_ARG), (dict(U=None, V=None, st=None, ag=None, stats=None), E_ARG),
                 (dict(U=ctypes.c_void_p(fu)), E_ARG), (dict(V=ctypes.c_void_p(fv + 8)), E_ARG), (dict(st=P(dstate[2])), E_ARG), (dict(U=P(dstart[1])), E_ARG),
                 (dict(ag=ctypes.c_void_p(fu + fstride)), E_ARG), (dict(stats=ctypes.c_void_p(ds.data_ptr() + 4)), E_ARG),
                 (dict(U=ctypes.c_void_p(outs[0].ptr.value + 2)), E_ARG), (dict(U0=ctypes.c_void_p(dstart[0].data_ptr() + 2)), E_ARG),
                 (dict(os=4 * W - 4), E_SIZE), (dict(os=4 * W + 2), E_SIZE), (dict(s0s=4 * W - 4), E_SIZE), (dict(s0s=4 * W + 2), E_SIZE), (dict(ss=W - 1), E_SIZE),
                 (dict(sts=W - 1), E_SIZE), (dict(ags=W - 1), E_SIZE)]
        for kw, code in cases:
            assert dense(**kw) == code, kw
        lists = [(ctypes.c_void_p * n)(*[view(hs, ctx, W, H, p)[k] for p in range(n)]) for k in (0, 1)]

        def planes(**kw):
            a = dict(n=n, u=lists[0], v=lists[1], fs=fstride)
            a.update(kw)
            return L.hsflow_chain_planes_device(ctx._h, a["n"], a["u"], a["v"], a["fs"], None, 0, None, None, 0, ctypes.byref(cp), outs[0].ptr, outs[1].ptr, 4 * W, outs[2].ptr,
                                                W, outs[3].ptr, W, ctypes.c_void_p(ds.data_ptr()))
        holed = (ctypes.c_void_p * n)(lists[0][0], None, lists[0][2])
        odd = (ctypes.c_void_p * n)(lists[0][0] + 2, lists[0][1], lists[0][2])
        mine = (ctypes.c_void_p * n)(lists[0][0], outs[0].ptr.value, lists[0][2])
        for kw, code in ((dict(u=None), E_ARG), (dict(v=None), E_ARG), (dict(u=holed), E_ARG), (dict(u=odd), E_ARG), (dict(u=mine), E_ARG), (dict(n=0), E_ARG),
                         (dict(n=33), E_ARG), (dict(fs=4 * W - 4), E_SIZE), (dict(fs=fstride + 2), E_SIZE)):
            assert planes(**kw) == code, kw
        m = 7
        dxy = cuda(point_starts(W, H, m, seed=0))
        pt = torch.full(((n + 1) * m * 2 + 2 * m,), -7.0, dtype=torch.float32, device="cuda")
        pb = torch.full((2 * m,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def points(**kw):
            a = dict(pairs=(ctypes.c_int * n)(0, 1, 2), n=n, xy=P(dxy), m=m, track=P(pt), last=ctypes.c_void_p(pt.data_ptr() + (n + 1) * m * 8), st=P(pb),
                     ag=ctypes.c_void_p(pb.data_ptr() + m), stats=ctypes.c_void_p(ds.data_ptr()), cp=ctypes.byref(cp))
            a.update(kw)
            return L.hsflow_track_points_device(ctx._h, a["pairs"], a["n"], None, 0, a["cp"], a["xy"], a["m"], a["track"], a["last"], a["st"], a["ag"], a["stats"])
        for kw in (dict(cp=None), dict(n=0), dict(n=33), dict(pairs=None), dict(pairs=(ctypes.c_int * n)(0, 1, 5)), dict(m=0), dict(m=(1 << 24) + 1), dict(xy=None),
                   dict(track=None, last=None, st=None, ag=None, stats=None), dict(stats=ctypes.c_void_p(ds.data_ptr() + 4)), dict(last=P(dxy)),
                   dict(track=ctypes.c_void_p(fu)), dict(xy=ctypes.c_void_p(dxy.data_ptr() + 2))):
            assert points(**kw) == E_ARG, kw
        # the synchronous forms refuse the same way, and nothing was written anywhere
        hU = np.full((H, W), -7, np.float32)
        with pytest.raises(hs.HsflowError):
            ctx.chain_flow([0, 9], flow=(hU, hU.copy()))
        with pytest.raises(hs.HsflowError):
            ctx.chain_flow(flow=False)
        with pytest.raises(hs.HsflowError):
            ctx.chain_flow(start=(hU, hU.copy()), flow=(hU, hU.copy()))
        with pytest.raises(ValueError):
            ctx.chain_flow(list(range(3)) * 11)
        assert (hU == -7).all()
        ctx.synchronize()
        for d in outs:
            host = d.buf.cpu().numpy()
            assert (host == FILL).all()
        assert bool((ds == FILL).all().item()) and bool((pt == -7).all().item()) and bool((pb == FILL).all().item())
        assert dense() == OK and planes() == OK and points() == OK     # and the context still works
        ctx.synchronize()


# ---- G6. the drop-in CLI -----------------------------------------------------------------------------------------------------------

def run_cli(cam, out, extra, ok=True):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    out.mkdir()
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               HSFLOW_CAMERA_DIR=str(cam), HSFLOW_CAMERA_OUT=str(out))
    for name in ("HSFLOW_RENDER_DEVICE", "HSFLOW_VERIFY", "HSFLOW_CAMERA_BATCH", "HSFLOW_CAMERA_CHAIN", "HSFLOW_JPEG_IN_DEVICE", "HSFLOW_JPEG_DEVICE", "HSFLOW_PICTURE"):
        env.pop(name, None)
    env.update(extra)
    r = subprocess.run([cli, "-cv", "-cam", ".1", "12"], env=env, capture_output=True, text=True, timeout=120)
    if ok:
        assert r.returncode == 0 and "Avg time" in r.stdout, (extra, r.stdout + r.stderr)
    return {name: open(str(out / name), "rb").read() for name in sorted(os.listdir(str(out)))}, r


def test_cli_chain_picture(hs, gpu_ok, tmp_path):
    W, H = 160, 96
    frames = [synth.translating_pair(W, H, seed=77, dx=1.5 * i, dy=-0.75 * i)[1] for i in range(4)]
    cam = tmp_path / "cam"
    cam.mkdir()
    for i, f in enumerate(frames):
        with open(str(cam / ("frame_%04d.pgm" % i)), "wb") as fh:
            fh.write(b"P5\n%d %d\n255\n" % (W, H) + np.ascontiguousarray(f, np.uint8).tobytes())
    plain, _ = run_cli(cam, tmp_path / "plain", {"HSFLOW_CAMERA_BATCH": "3"})
    got, _ = run_cli(cam, tmp_path / "chain", {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_CHAIN": "1"})
    assert sorted(plain) == ["flow_%04d.ppm" % i for i in (1, 2, 3)]
    assert sorted(got) == ["chain_0003.ppm"] + sorted(plain)
    assert all(got[k] == plain[k] for k in plain)                     # the flow pictures stay byte for byte
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        ctx.set_pair_termination(True)
        ctx.set_sequence_device([cuda(f) for f in frames], "gray_blur", reblur=True)
        ctx.solve(lam=0.1, max_iter=12, term_type=ITER | EPS, epsilon=float(np.float32(1e-6)))
        flows = [ctx.flow(p) for p in range(3)]
    U, V, _, _, _ = hs.chain_flow_host([f[0] for f in flows], [f[1] for f in flows])
    want = hs.color_flow_host(U, V)
    assert got["chain_0003.ppm"] == b"P6\n%d %d\n255\n" % (W, H) + want.tobytes()
    assert np.frombuffer(got["chain_0003.ppm"], np.uint8)[15:].any()
    two, _ = run_cli(cam, tmp_path / "two", {"HSFLOW_CAMERA_BATCH": "2", "HSFLOW_CAMERA_CHAIN": "1"})   # a batch of two and a tail of one
    assert sorted(two) == ["chain_0002.ppm", "chain_0003.ppm"] + sorted(plain) and all(two[k] == plain[k] for k in plain)
    for k, extra in enumerate(({"HSFLOW_CAMERA_CHAIN": "1"}, {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_CHAIN": "yes"}, {"HSFLOW_CAMERA_BATCH": "0", "HSFLOW_CAMERA_CHAIN": "1"})):
        files, r = run_cli(cam, tmp_path / ("bad%d" % k), extra, ok=False)
        assert r.returncode == 1 and "HSFLOW_CAMERA_" in r.stdout and not files, (extra, r.stdout)
