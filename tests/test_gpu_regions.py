"""Connected regions on the GPU (include/hsflow.h, ABI 0.24: hsflow_regions*; kernels in
opticalflowhs_amd/csrc/hs_kernels_regions.hip.h) against the rule on the host (hsflow_regions_host, which
tests/test_regions_host.py holds to a breadth-first restatement).  Labels, records and headers are compared as bytes: there
is no tolerance anywhere."""
import ctypes
import os

import numpy as np
import pytest

import regions_ref as R
from test_gpu_chain import DevIn, cuda, layouts, ptr_list
from test_gpu_fb import FILL, DevPlane, dev_stats, put_flow

pytestmark = pytest.mark.gpu

F = np.float32
OK, E_ARG, E_SIZE = 0, 1, 2
CASES = R.cases()
# which outputs a call asks for: (labels, records, result)
ASKS = [(True, True, True), (True, False, False), (False, True, True), (False, False, True), (False, True, False), (True, True, False)]


def dev_records(capacity):
    """capacity records and 64 bytes more, all FILL."""
    import torch
    t = torch.full((capacity * 64 + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert t.data_ptr() % 8 == 0
    return t


def host_want(hs, mask, u, v, rp, capacity, shape):
    """(label plane, the bytes of the records written, the header's 64 bytes) of the host rule."""
    res, labels, recs = hs.regions_host(mask, u, v, labels=True, records=True, capacity=capacity, params=rp, shape=shape)
    return labels, bytes(recs)[:res.n_written * 64], bytes(res), res


def check_outputs(dl, dr, ds, want, label):
    """The label DevPlane, the record tensor and the header tensor of a device call (None: not asked for) against the
    host's; nothing written around them."""
    labels, recs, head, res = want
    if dl is not None:
        rows, clean = dl.rows_and_rest()
        assert np.array_equal(np.ascontiguousarray(rows).view(np.int32), labels), label
        assert clean, label                                                  # nothing beyond W labels of a row
    if dr is not None:
        got = bytes(dr.cpu().numpy())
        assert got[:len(recs)] == recs, label
        assert got[len(recs):] == bytes([FILL]) * (len(got) - len(recs)), label   # no record from n_written on
    if ds is not None:
        got = bytes(ds.cpu().numpy())
        assert got[:64] == head, (label, res.as_dict())
        assert got[64:] == bytes([FILL]) * (len(got) - 64), label


# ---- G1. the planes form against the host form ------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", R.SHAPES)
def test_planes_device_equals_host(hs, gpu_ok, W, H):
    L = hs._lib.load()
    lay = layouts(W)
    k = 0
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for case, _, _, _ in CASES:
            mask, u, v, join = R.planes(case, W, H)
            for conn in (4, 8):
                k += 1
                min_area = (1, 2, 5)[k % 3]
                rp = hs.make_regions_params(connectivity=conn, min_area=min_area, join_px=join)
                n_all = hs.regions_host(mask, u, v, records=False, capacity=0, params=rp, shape=(H, W))[0].n_regions
                capacity = 3 if k % 2 else n_all + 2
                want = host_want(hs, mask, u, v, rp, capacity, (H, W))
                (foff, fstride), (boff, bstride) = lay[k % 4]
                dm = DevIn(mask, boff, bstride) if mask is not None else None
                du, dv = (DevIn(u, foff, fstride), DevIn(v, foff, fstride)) if u is not None else (None, None)
                want_l, want_r, want_s = ASKS[k % len(ASKS)]
                dl = DevPlane(H, 4 * W, foff, fstride) if want_l else None
                dr = dev_records(capacity) if want_r else None
                ds = dev_stats() if want_s else None
                st = L.hsflow_regions_planes_device(ctx._h, dm.ptr if dm else None, bstride, du.ptr if du else None, dv.ptr if dv else None, fstride, ctypes.byref(rp),
                                                    dl.ptr if dl else None, fstride, dr.data_ptr() if dr is not None else None, capacity,
                                                    ds.data_ptr() if ds is not None else None)
                assert st == OK, ctx._lib.hsflow_last_error(ctx._h)
                ctx.synchronize()
                label = (case, W, H, conn, min_area, capacity, k % 4)
                check_outputs(dl, dr, ds, want, label)
                for d, a in ((dm, mask), (du, u), (dv, v)):                     # the inputs are as they were
                    if d is not None:
                        rows, clean = d.rows_and_rest()
                        assert clean and np.array_equal(rows, np.ascontiguousarray(a).view(np.uint8).reshape(H, -1)), label


# ---- G2. the forms on a context's own flow ----------------------------------------------------------------------------------

def test_context_forms_read_the_context_flow(hs, gpu_ok):
    W, H = 260, 37
    for flow, mname in (("two_blocks", None), ("ramp", "random80"), ("sprinkled", "random80")):
        u, v = R.flow_of(flow, W, H)
        mask = R.mask_of(mname, W, H) if mname else None
        with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
            put_flow(ctx, np.zeros((H, W), F), np.zeros((H, W), F), pair=0)
            put_flow(ctx, u, v, pair=1)
            for conn in (4, 8):
                rp = hs.make_regions_params(connectivity=conn, min_area=2, join_px=R.JOIN_PX)
                want = host_want(hs, mask, u, v, rp, 40, (H, W))
                # the synchronous form, host memory
                res, labels, recs = ctx.regions(pair=1, mask=mask, labels=True, records=True, capacity=40, params=rp)
                assert np.array_equal(labels, want[0]) and bytes(res) == want[2], (flow, conn, res.as_dict(), want[3].as_dict())
                assert bytes(recs)[:res.n_written * 64] == want[1] and bytes(recs)[res.n_written * 64:] == b"\0" * (40 - res.n_written) * 64
                # only enqueued
                dres, dlab, drec = ctx.regions(pair=1, mask=cuda(mask) if mask is not None else None, labels=True, records=True, capacity=40, params=rp, device=True)
                ctx.synchronize()
                got = hs.regions_result_from(dres)
                assert bytes(got) == want[2] and np.array_equal(dlab.cpu().numpy(), want[0])
                assert bytes(drec.cpu().numpy())[:got.n_written * 64] == want[1]
                assert [r.as_dict() for r in hs.regions_records_from(drec, got.n_written)] == [r.as_dict() for r in hs.regions_records_from(recs, res.n_written)]
                # pair 0 holds another flow: everything joins there
                res0, _, _ = ctx.regions(pair=0, mask=mask, records=False, capacity=0, params=rp)
                assert bytes(res0) == host_want(hs, mask, np.zeros((H, W), F), np.zeros((H, W), F), rp, 0, (H, W))[2]


def test_batch_is_one_call_per_pair_and_the_host(hs, gpu_ok):
    """A batch of 5 pairs with different patterns, and one of 10 (more than one set of launches), with holes in the lists."""
    import torch
    L = hs._lib.load()
    W, H, N = 96, 64, 10
    names = ["checker", "spiral", None, "random59", "diagonals", "comb", "empty", "random30", "full", "serpentine"]
    flows = ["sprinkled", "ramp", "two_blocks", "sprinkled", "ramp", "two_blocks", "ramp", "sprinkled", "ramp", "two_blocks"]
    masks = [R.mask_of(n, W, H) if n else None for n in names]
    uv = [R.flow_of(f, W, H) for f in flows]
    lay = layouts(W)
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, uv[p][0], uv[p][1], pair=p)
        for first, n, conn, join, capacity in ((2, 5, 8, 0.0, 6), (0, 10, 4, R.JOIN_PX, 50), (5, 5, 8, R.JOIN_PX, 3)):
            rp = hs.make_regions_params(connectivity=conn, min_area=2, join_px=join)
            (foff, fstride), (boff, bstride) = lay[(first + n) % 4]
            pairs = list(range(first, first + n))
            dm = [DevIn(masks[p], boff, bstride) if masks[p] is not None else None for p in pairs]
            dl = [DevPlane(H, 4 * W, foff, fstride) for _ in pairs]
            dr = [dev_records(capacity) for _ in pairs]
            dl[1] = None                                       # holes: no labels for one pair, no records for another
            dr[n - 1] = None
            ds = dev_stats(n)
            st = L.hsflow_regions_batch_device(ctx._h, first, n, ptr_list(dm), bstride, ctypes.byref(rp), ptr_list(dl), fstride,
                                               (ctypes.c_void_p * n)(*[r.data_ptr() if r is not None else None for r in dr]), capacity, ds.data_ptr())
            assert st == OK, ctx._lib.hsflow_last_error(ctx._h)
            ctx.synchronize()
            heads = bytes(ds.cpu().numpy())
            assert heads[64 * n:] == bytes([FILL]) * 64
            for k, p in enumerate(pairs):
                want = host_want(hs, masks[p], uv[p][0], uv[p][1], rp, capacity, (H, W))
                check_outputs(dl[k], dr[k], None, want, (first, n, p))
                assert heads[64 * k:64 * k + 64] == want[2], (first, n, p, want[3].as_dict())
                # the pair's own call
                one_s, one_r = dev_stats(), dev_records(capacity)
                one_l = DevPlane(H, 4 * W, foff, fstride)
                assert L.hsflow_regions_device(ctx._h, p, dm[k].ptr if dm[k] else None, bstride, ctypes.byref(rp), one_l.ptr, fstride, one_r.data_ptr(), capacity,
                                               one_s.data_ptr()) == OK
                ctx.synchronize()
                check_outputs(one_l, one_r, one_s, want, (first, n, p, "one"))
        torch.cuda.synchronize()


# ---- G3. reuse ----------------------------------------------------------------------------------------------------------------

def test_second_call_with_fewer_regions_leaves_nothing_behind(hs, gpu_ok):
    """The scratch and the record arrays are reused without a memset: many regions, then few, then many again, into the
    SAME outputs; whatever a call does not write keeps what the call before left there."""
    L = hs._lib.load()
    W, H = 260, 37
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        dl = DevPlane(H, 4 * W, 0, 4 * W)
        dr, ds = dev_records(64), dev_stats()
        before = bytes(dr.cpu().numpy())
        for name, conn in (("checker", 4), ("u", 8), ("random59", 4), ("empty", 8), ("diagonals", 8), ("full", 4)):
            mask = R.mask_of(name, W, H)
            rp = hs.make_regions_params(connectivity=conn)
            want = host_want(hs, mask, None, None, rp, 64, (H, W))
            dm = DevIn(mask, 0, W)
            assert L.hsflow_regions_planes_device(ctx._h, dm.ptr, W, None, None, 0, ctypes.byref(rp), dl.ptr, 4 * W, dr.data_ptr(), 64, ds.data_ptr()) == OK
            ctx.synchronize()
            rows, clean = dl.rows_and_rest()
            assert clean and np.array_equal(np.ascontiguousarray(rows).view(np.int32), want[0]), name
            assert bytes(ds.cpu().numpy())[:64] == want[2], (name, want[3].as_dict())
            got = bytes(dr.cpu().numpy())
            assert got[:len(want[1])] == want[1], name
            assert got[len(want[1]):] == before[len(want[1]):], name        # records from n_written on: as the call found them
            before = got


# ---- G4. the composition the operator exists for ----------------------------------------------------------------------------

def moving_scene(W=96, H=64):
    """An affine background flow with two rectangles that move on their own: (u, v, the rectangles as (x0, y0, x1, y1))."""
    yy, xx = np.mgrid[0:H, 0:W].astype(F)
    u = (F(0.5) + F(0.01) * (xx - F(47.5)) - F(0.004) * (yy - F(31.5))).astype(F)
    v = (F(-0.25) + F(0.004) * (xx - F(47.5)) + F(0.01) * (yy - F(31.5))).astype(F)
    rects = [(10, 8, 29, 21), (60, 30, 71, 55)]
    for (x0, y0, x1, y1), (a, b) in zip(rects, ((4.0, -3.0), (-3.5, 2.5))):
        u[y0:y1 + 1, x0:x1 + 1] = F(a)
        v[y0:y1 + 1, x0:x1 + 1] = F(b)
    return u, v, rects


def test_moving_objects_from_the_flow(hs, gpu_ok):
    W, H = 96, 64
    u, v, rects = moving_scene(W, H)
    gp = hs.make_gmotion_params(values=(0, 255, 0, 0))
    rp = hs.make_regions_params(connectivity=8, min_area=4)
    _, hmask, _, _ = hs.global_motion_host(u, v, mask=True, params=gp)
    hres, hlab, hrec = hs.regions_host(hmask, u, v, labels=True, records=True, capacity=16, params=rp)
    recs = hs.regions_records_from(hrec, hres.n_written)
    assert hres.n_regions == 2 and [(r.x0, r.y0, r.x1, r.y1) for r in recs] == rects          # the host rule finds the rectangles
    assert [r.area for r in recs] == [(x1 - x0 + 1) * (y1 - y0 + 1) for x0, y0, x1, y1 in rects]
    assert [(r.sum_qu, r.sum_qv) for r in recs] == [(1024 * recs[0].area, -768 * recs[0].area), (-896 * recs[1].area, 640 * recs[1].area)]
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        _, dmask, _, _ = ctx.global_motion(mask=True, result=False, params=gp, device=True)
        dres, dlab, drec = ctx.regions(mask=dmask, labels=True, records=True, capacity=16, params=rp)
        ctx.synchronize()
        assert np.array_equal(dmask.cpu().numpy(), hmask)
        got = hs.regions_result_from(dres)
        assert bytes(got) == bytes(hres) and np.array_equal(dlab.cpu().numpy(), hlab)
        assert bytes(drec.cpu().numpy())[:got.n_written * 64] == bytes(hrec)[:hres.n_written * 64]


# ---- G5. refusals enqueue nothing ---------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_alone(hs, gpu_ok):
    L = hs._lib.load()
    W, H = 40, 12
    mask = R.mask_of("random59", W, H)
    u, v = R.flow_of("sprinkled", W, H)
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        dm, du, dv = DevIn(mask, 0, W), DevIn(u, 0, 4 * W), DevIn(v, 0, 4 * W)
        dl = DevPlane(H, 4 * W, 0, 4 * W)
        dr, ds = dev_records(4), dev_stats()
        good = hs.make_regions_params()

        def params(**kw):
            rp = hs.make_regions_params()
            for k, x in kw.items():
                setattr(rp, k, x)
            return rp

        def planes(rp=good, m=dm.ptr.value, ms=W, a=None, b=None, fs=4 * W, lab=dl.ptr.value, ls=4 * W, rec=dr.data_ptr(), cap=4, res=ds.data_ptr()):
            return L.hsflow_regions_planes_device(ctx._h, m, ms, a, b, fs, ctypes.byref(rp) if rp is not None else None, lab, ls, rec, cap, res)

        def batch(first, n, rp=good, res=ds.data_ptr()):
            arr = (ctypes.c_void_p * max(n, 1))(*([dm.ptr.value] * max(n, 1)))
            return L.hsflow_regions_batch_device(ctx._h, first, n, arr, W, ctypes.byref(rp), None, 0, None, 0, res)

        uu, vv = du.ptr.value, dv.ptr.value
        assert planes(rp=None) == E_ARG
        assert planes(rp=params(struct_size=31)) == E_ARG
        assert planes(rp=params(connectivity=3)) == E_ARG
        assert planes(rp=params(fg_lo=3, fg_hi=2)) == E_ARG
        assert planes(rp=params(min_area=0)) == E_ARG
        assert planes(rp=params(join_px=float("nan")), a=uu, b=vv) == E_ARG
        assert planes(rp=params(join_px=1.0)) == E_ARG                          # join without flow
        assert planes(a=uu) == E_ARG and planes(b=vv) == E_ARG                  # one flow plane
        assert planes(a=uu + 2, b=vv) == E_ARG
        assert planes(lab=dl.ptr.value + 2) == E_ARG
        assert planes(rec=dr.data_ptr() + 4) == E_ARG                           # records and result: multiples of 8
        assert planes(res=ds.data_ptr() + 4) == E_ARG
        assert planes(lab=None, rec=None, res=None) == E_ARG                    # nothing asked for
        assert planes(lab=dm.ptr.value) == E_ARG                                # an output on an input
        assert planes(a=uu, b=vv, rec=uu) == E_ARG
        assert planes(rec=dl.ptr.value + 8) == E_ARG                            # two outputs on one another
        assert planes(ms=W - 1) == E_SIZE
        assert planes(a=uu, b=vv, fs=4 * W - 4) == E_SIZE and planes(a=uu, b=vv, fs=4 * W + 2) == E_SIZE
        assert planes(ls=4 * W - 4) == E_SIZE and planes(ls=4 * W + 2) == E_SIZE
        assert batch(0, 0) == E_ARG and batch(-1, 1) == E_ARG and batch(1, 2) == E_ARG
        assert batch(0, 2, res=ds.data_ptr() + 4) == E_ARG
        vu, vvv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        assert L.hsflow_flow_view_device(ctx._h, 1, ctypes.byref(vu), ctypes.byref(vvv), ctypes.byref(sb)) == OK
        assert L.hsflow_regions_device(ctx._h, 1, dm.ptr, W, ctypes.byref(good), vu, sb.value, None, 0, None) == E_ARG      # labels in the context's flow
        assert L.hsflow_regions_device(ctx._h, 2, dm.ptr, W, ctypes.byref(good), dl.ptr, 4 * W, None, 0, None) == E_ARG      # no such pair
        assert L.hsflow_regions(ctx._h, 0, None, 0, ctypes.byref(good), None, 0, None, 0, None) == E_ARG
        ctx.synchronize()
        rows, clean = dl.rows_and_rest()
        assert clean and (rows == FILL).all()
        assert (dr.cpu().numpy() == FILL).all() and (ds.cpu().numpy() == FILL).all()
        for d, a in ((dm, mask), (du, u), (dv, v)):
            rows, clean = d.rows_and_rest()
            assert clean and np.array_equal(rows, np.ascontiguousarray(a).view(np.uint8).reshape(H, -1))
        # and the same arguments, put right, are taken
        assert planes(a=uu, b=vv, rp=params(join_px=0.5)) == OK
        ctx.synchronize()
        check_outputs(dl, dr, ds, host_want(hs, mask, u, v, params(join_px=0.5), 4, (H, W)), "good")


# ---- G6. the command line -------------------------------------------------------------------------------------------------------

def test_cli_prints_the_same_regions_by_either_route(hs, gpu_ok, tmp_path):
    from opticalflowhs_amd import synth
    from test_gpu_warp import _cli
    W, H = 96, 64
    A, B = synth.translating_pair(W, H, seed=5)
    B = np.array(B, copy=True)
    B[20:36, 30:50] = A[17:33, 36:56]                       # a patch that moves against the rest
    names = [str(tmp_path / ("frame%d.pgm" % k)) for k in range(2)]
    for name, f in zip(names, (A, B)):
        with open(name, "wb") as fh:
            fh.write(b"P5\n%d %d\n255\n" % (W, H) + np.ascontiguousarray(f, np.uint8).tobytes())
    routes = (("host", {}), ("device", {"HSFLOW_RENDER_DEVICE": "1"}))
    for args in (["-cv", "-hd", names[0], names[1], None, ".1", "100"], ["-cl", "-hd", names[0], names[1], None, "3", "50", "1", "GPU"]):
        plain = {}
        for route, env in routes:
            out = str(tmp_path / "plain.ppm")
            _cli([out if a is None else a for a in args], env)
            plain[route] = open(out, "rb").read()
        for choice in ("4,8", "1,4,0.25"):
            lines = {}
            for route, env in routes:
                out = str(tmp_path / ("%s_%s.ppm" % (args[0][1:], route)))
                r = _cli([out if a is None else a for a in args], dict(env, HSFLOW_REGIONS=choice))
                lines[route] = [ln for ln in r.stdout.splitlines() if ln.startswith("regions:") or ln.startswith("region ")]
                assert open(out, "rb").read() == plain[route]                    # the picture is unchanged
            assert lines["host"] == lines["device"], (args[0], choice)
            head = lines["host"][0].split()
            assert head[0] == "regions:" and head[1] == "kept" and head[3] == "dropped" and head[5] == "foreground" and head[7] == "largest"
            assert len(lines["host"]) == 1 + min(int(head[2]), 16)
            for k, ln in enumerate(lines["host"][1:]):
                words = ln.split()
                assert words[:3] == ["region", "%d:" % (k + 1), "area"] and words[4] == "box" and words[9] == "centre" and words[12] == "motion" and len(words) == 15
    for bad in ("0", "4,6", "4,8,-1", "4,8,nan", "x", "4,8,0.5,1"):
        r = _cli(["-cv", "-hd", names[0], names[1], str(tmp_path / "bad.ppm"), ".1", "10"], {"HSFLOW_REGIONS": bad}, ok=False)
        assert r.returncode == 1 and "HSFLOW_REGIONS" in r.stdout, bad
