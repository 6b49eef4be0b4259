"""The operators on a solved flow at the sizes where their kernels take another path than at the small shapes of their own
files (13x7 .. 300x70), against the same rules on the host, byte for byte:

A.  Once statistics are asked for, hs_postops.hip.h's stats_rows gives a workgroup per = clamp(units_x * units_y * cnt /
    (2 * compute units), 1, 8) rows, and the y loop of k_warp_batch, k_fb_batch, the three interpolation kernels, the dense
    chain kernel and k_gm_warp runs more than once per lane: the 32-bit statistics of a lane are carried over rows, the last
    trip is uneven (some workgroups take one row fewer), and `continue` on a NULL destination sits inside a loop that goes
    on.  The frames are tall and narrow -- 13 x (16 cus + 3), 13 x (4 cus + 1), 1027 x (3 cus + 2), and four pictures of
    13 x (cus + 3) -- and every test asserts the `per` it means to reach from the device's own number of compute units before
    its first launch.  (The median's kernel is not here: its test_device_equals_host at BIG_SHAPE = 2050 x 530 has 33 x 34
    = 1122 tiles, which with statistics is per == 2 on 256 compute units.)
B.  k_rg_scan (hs_kernels_regions.hip.h) is one workgroup of 1024 lanes over n_counts = ceil(W / 256) * H words: beyond 1024
    words it goes round again and carries `carry` and `roots`, beyond 128 words waves 2 .. 15 hold sums, a batch's second
    field starts n_counts words on, and beyond 65535 regions a label no longer fits a count word's half.

Nothing here has a tolerance."""
import ctypes

import numpy as np
import pytest

import regions_ref as R
from test_chain_host import VALUES as CHAIN_VALUES, chain_fields, start_fields, stat_tuple as chain_stat_tuple
from test_fb_host import stat_tuple as fb_stat_tuple
from test_gpu_chain import DevIn, check_outputs as check_chain_outputs, host_want as chain_host_want, layouts, ptr_list
from test_gpu_fb import FILL, DevPlane, dev_stats, host_want as fb_host_want, put_flow, two_fields
from test_gpu_interp import field as interp_field, pictures, stat_tuple as interp_stat_tuple
from test_gpu_regions import check_outputs, dev_records, host_want
from test_gpu_warp import field, stat_tuple

pytestmark = pytest.mark.gpu

F = np.float32
OK = 0

# ---- A. the row loop of the statistics kernels ----------------------------------------------------------------------------------

# name: (W, a, b, per): H = a * cus + b, and the rows per workgroup that stats_rows then asks for with one picture
TALL = {"per8": (13, 16, 3, 8), "per2": (13, 4, 1, 2), "per3": (1027, 3, 2, 3)}
BATCH = (13, 1, 3, 4, 2)                 # W, a, b, pictures, per: reached through cnt alone


def compute_units():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def rows_per_workgroup(W, H, cnt, cus):
    """stats_rows of hs_postops.hip.h restated for the kernels whose unit is a row of 1024 columns: (per, gridDim.y)."""
    units_x = (W + 1023) // 1024
    per = min(max(units_x * H * cnt // (2 * cus), 1), 8)
    return per, (H + per - 1) // per


def in_regime(W, H, cnt, want=None):
    """Asserts that cnt pictures of W x H loop: `per` is `want` (None: at least 2), the last trip is uneven, and the grid's
    65535 cap is far.  Returns per."""
    cus = compute_units()
    per, gy = rows_per_workgroup(W, H, cnt, cus)
    assert (per == want) if want is not None else (per >= 2), (W, H, cnt, cus, per)
    assert H % per != 0 and H % gy != 0 and gy < H and gy < 65535, (W, H, cnt, cus, per, gy)
    return per


def tall(name, cnt=1):
    W, a, b, per = TALL[name]
    H = a * compute_units() + b
    in_regime(W, H, cnt, per if cnt == 1 else None)
    return W, H


def batch_shape():
    W, a, b, cnt, per = BATCH
    H = a * compute_units() + b
    assert rows_per_workgroup(W, H, 1, compute_units())[0] == 1      # one picture alone would not loop
    in_regime(W, H, cnt, per)
    return W, H, cnt


def byte_layouts(rowb):
    """(offset from a 256-byte multiple, stride) of a picture: one aligned, one odd."""
    return [(0, (rowb + 3) // 4 * 4), (3, rowb + 5)]


def record_bytes(t, n=1):
    """The n records of a statistics tensor, after asserting that the 64 bytes behind them are still FILL."""
    raw = bytes(t.cpu().numpy())
    assert raw[64 * n:] == bytes([FILL]) * 64
    return raw[:64 * n]


def check_picture(d, want, label):
    rows, clean = d.rows_and_rest()
    assert np.array_equal(rows, np.ascontiguousarray(want).view(np.uint8).reshape(rows.shape)), label
    assert clean, label                                               # nothing outside the rows


def untouched(d):
    return bool((d.buf.cpu().numpy() == FILL).all())


# ---- A1. warp ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", sorted(TALL))
def test_warp(hs, gpu_ok, name, C):
    L = hs._lib.load()
    W, H = tall(name)
    rng = np.random.default_rng(W + H + C)
    src = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    ref = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    u, v = field(W, H, 7 * W + H)
    rowb = W * C
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for border in ("constant", "replicate"):
            for t in (1.0, -0.5):
                wp = hs.make_warp_params(C, t, border, (7, 200, 33))
                want, ws = hs.warp_host(u, v, src, ref=ref, params=wp, return_stats=True)
                assert min(ws.inside, ws.outside) > 0 and ws.unknown >= 6 and ws.sad_warped > 0
                for k, (off, stride) in enumerate(byte_layouts(rowb)):
                    s_off, s_stride = byte_layouts(rowb)[1 - k]
                    label = (name, C, border, t, off, stride)
                    dsrc, dref = DevIn(src, s_off, s_stride), DevIn(ref, off, stride)
                    # with the reference and statistics
                    ddst, dst = DevPlane(H, rowb, off, stride), dev_stats()
                    assert L.hsflow_warp_device(ctx._h, 0, ctypes.byref(wp), dsrc.ptr, s_stride, dref.ptr, stride, ddst.ptr, stride, ctypes.c_void_p(dst.data_ptr())) == OK
                    ctx.synchronize()
                    check_picture(ddst, want, label)
                    assert stat_tuple(hs.warp_stats_from(dst)) == stat_tuple(ws), label
                    assert record_bytes(dst) == bytes(ws), label
                    # statistics only: d_dst == NULL, the `continue` of every trip
                    dst = dev_stats()
                    assert L.hsflow_warp_device(ctx._h, 0, ctypes.byref(wp), dsrc.ptr, s_stride, dref.ptr, stride, None, 0, ctypes.c_void_p(dst.data_ptr())) == OK
                    ctx.synchronize()
                    assert record_bytes(dst) == bytes(ws), label
                    # no statistics: one row per workgroup, the control
                    ddst = DevPlane(H, rowb, off, stride)
                    assert L.hsflow_warp_device(ctx._h, 0, ctypes.byref(wp), dsrc.ptr, s_stride, None, 0, ddst.ptr, stride, None) == OK
                    ctx.synchronize()
                    check_picture(ddst, want, label)
                    assert dsrc.rows_and_rest()[1] and dref.rows_and_rest()[1]


def test_warp_batch_of_four(hs, gpu_ok):
    """Four pictures that loop only because they are four: every record holds its own picture's sums."""
    L = hs._lib.load()
    W, H, N = batch_shape()
    C = 3
    rng = np.random.default_rng(5)
    srcs = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
    refs = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
    flows = [field(W, H, 40 + p, sigma=1.0 + 2.0 * p) for p in range(N)]
    rowb = W * C
    wp = hs.make_warp_params(C, 1.0, "replicate", (1, 2, 3))
    wants = [hs.warp_host(flows[p][0], flows[p][1], srcs[p], ref=refs[p], params=wp, return_stats=True) for p in range(N)]
    assert len(set(bytes(s) for _, s in wants)) == N
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, *flows[p], pair=p)
        for off, stride in byte_layouts(rowb):
            dsrc, dref = [DevIn(s, off, stride) for s in srcs], [DevIn(r, off, stride) for r in refs]
            for with_dst in (True, False):
                ddst, dst = [DevPlane(H, rowb, off, stride) for _ in range(N)], dev_stats(N)
                assert L.hsflow_warp_batch_device(ctx._h, 0, N, ctypes.byref(wp), ptr_list(dsrc), stride, ptr_list(dref), stride, ptr_list(ddst) if with_dst else None,
                                                  stride if with_dst else 0, ctypes.c_void_p(dst.data_ptr())) == OK
                ctx.synchronize()
                assert record_bytes(dst, N) == b"".join(bytes(s) for _, s in wants), (off, with_dst)
                for p in range(N):
                    if with_dst:
                        check_picture(ddst[p], wants[p][0], (off, p))
                    else:
                        assert untouched(ddst[p])


# ---- A2. forward-backward check ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(TALL))
def test_fb(hs, gpu_ok, name):
    L = hs._lib.load()
    W, H = tall(name)
    flows = two_fields(W, H, 7 * W + H)
    mask_layouts = byte_layouts(W)
    err2_layouts = [(0, (4 * W + 15) // 16 * 16), (4, 4 * W + 4)]
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        for p in range(2):
            put_flow(ctx, *flows[p], pair=p)
        for kw in (dict(), dict(alpha=0.0, beta=0.0, values=(1, 2, 3, 4))):
            fp = hs.make_fb_params(**kw)
            for fwd, bwd in ((0, 1), (1, 0)):
                mask, bits, st = fb_host_want(hs, flows[fwd], flows[bwd], params=fp)
                assert all(n > 0 for n in st[1:4]) and (st[0] > 0 or kw) and st[4] > 0, st     # (alpha = beta = 0: nothing is consistent)
                for k in range(2):
                    (off, stride), (eoff, estride) = mask_layouts[k], err2_layouts[k]
                    label = (name, kw, fwd, k)
                    for with_planes, with_stats in ((True, True), (False, True), (True, False)):
                        dm, de, ds = DevPlane(H, W, off, stride), DevPlane(H, 4 * W, eoff, estride), dev_stats()
                        assert L.hsflow_fb_device(ctx._h, fwd, bwd, ctypes.byref(fp), dm.ptr if with_planes else None, stride, de.ptr if with_planes else None, estride,
                                                  ctypes.c_void_p(ds.data_ptr()) if with_stats else None) == OK
                        ctx.synchronize()
                        if with_planes:
                            check_picture(dm, mask, label)
                            check_picture(de, bits, label)
                        else:
                            assert untouched(dm) and untouched(de)
                        if with_stats:
                            assert fb_stat_tuple(hs.fb_stats_from(ds)) == st, label
                            raw = record_bytes(ds)
                            assert raw[44:] == b"\0" * 20
                        else:
                            assert bool((ds == FILL).all().item())


def test_fb_batch_of_four(hs, gpu_ok):
    L = hs._lib.load()
    W, H, N = batch_shape()
    fwd, bwd = [0, 1, 2, 3], [1, 0, 3, 2]
    flows = []
    for p in range(2):
        a, b = two_fields(W, H, 60 + p)
        flows += [a, b]
    fp = hs.make_fb_params(values=(200, 100, 50, 25))
    wants = [fb_host_want(hs, flows[f], flows[b], params=fp) for f, b in zip(fwd, bwd)]
    assert len(set(w[2] for w in wants)) == N
    ints = lambda v: (ctypes.c_int * len(v))(*v)
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, *flows[p], pair=p)
        for with_planes in (True, False):
            dm, de, ds = [DevPlane(H, W, 1, W + 3) for _ in range(N)], [DevPlane(H, 4 * W, 4, 4 * W + 4) for _ in range(N)], dev_stats(N)
            assert L.hsflow_fb_batch_device(ctx._h, N, ints(fwd), ints(bwd), ctypes.byref(fp), ptr_list(dm) if with_planes else None, W + 3,
                                            ptr_list(de) if with_planes else None, 4 * W + 4, ctypes.c_void_p(ds.data_ptr())) == OK
            ctx.synchronize()
            record_bytes(ds, N)
            assert [fb_stat_tuple(g) for g in hs.fb_stats_from(ds, N)] == [w[2] for w in wants], with_planes
            for i in range(N):
                if with_planes:
                    check_picture(dm[i], wants[i][0], i)
                    check_picture(de[i], wants[i][1], i)
                else:
                    assert untouched(dm[i]) and untouched(de[i])


# ---- A3. intermediate frames ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,C", [("per8", 3), ("per2", 1), ("per2", 3), ("per3", 1)])
def test_interp(hs, gpu_ok, name, C):
    """One call for the times 0, 0.5 and 1 (three pictures: `per` comes from all three) and a single call, through the
    splat, fill and blend kernels' one grid."""
    L = hs._lib.load()
    W, H = tall(name)
    times = [0.0, 0.5, 1.0]
    N = len(times)
    in_regime(W, H, N)
    prev, curr, _, vp, vc = pictures(W, H, C, W + C)
    refs = np.random.default_rng(1).integers(0, 256, (N, H, W, C), dtype=np.uint8)
    u, v = interp_field(W, H, 7 * W + H)
    ip = hs.make_interp_params(C, 1, 1, 2)
    wants = [hs.interp_host(u, v, prev, curr, t=t, vis_prev=vp, vis_curr=vc, ref=refs[k], classes=True, stats=True, params=ip) for k, t in enumerate(times)]
    assert all(w[2].sad > 0 and w[2].holes > 0 and w[2].unknown >= 6 for w in wants[1:]) and wants[0][2].sad > 0
    rowb = W * C
    with hs.HSFlow(W, H, own_stream=True) as ctx:
        put_flow(ctx, u, v)
        for off, stride in byte_layouts(rowb):
            dprev, dcurr = DevIn(prev, off, stride), DevIn(curr, 3 - off, rowb + 5 if off == 0 else (rowb + 3) // 4 * 4)
            dvp, dvc = DevIn(vp, 1, W + 3), DevIn(vc, 0, W)
            drefs = [DevIn(r, off, stride) for r in refs]
            for with_dst in (True, False):
                ddst, dcls, dst = [DevPlane(H, rowb, off, stride) for _ in range(N)], [DevPlane(H, W, 1, W + 1) for _ in range(N)], dev_stats(N)
                assert L.hsflow_interp_batch_device(ctx._h, 0, N, (ctypes.c_float * N)(*times), ctypes.byref(ip), dprev.ptr, dprev.stride, dcurr.ptr, dcurr.stride,
                                                    dvp.ptr, W + 3, dvc.ptr, W, ptr_list(drefs), stride, ptr_list(ddst) if with_dst else None, stride,
                                                    ptr_list(dcls) if with_dst else None, W + 1, ctypes.c_void_p(dst.data_ptr())) == OK
                ctx.synchronize()
                record_bytes(dst, N)
                assert [interp_stat_tuple(g) for g in hs.interp_stats_from(dst, N)] == [interp_stat_tuple(w[2]) for w in wants], (name, C, off, with_dst)
                for k in range(N):
                    if with_dst:
                        check_picture(ddst[k], wants[k][0], (name, C, off, k))
                        check_picture(dcls[k], wants[k][1], (name, C, off, k))
                    else:
                        assert untouched(ddst[k]) and untouched(dcls[k])
            # one time alone: the `per` of one picture
            ddst, dcls, dst = DevPlane(H, rowb, off, stride), DevPlane(H, W, 2, W + 2), dev_stats()
            assert L.hsflow_interp_device(ctx._h, 0, times[1], ctypes.byref(ip), dprev.ptr, dprev.stride, dcurr.ptr, dcurr.stride, dvp.ptr, W + 3, dvc.ptr, W,
                                          drefs[1].ptr, stride, ddst.ptr, stride, dcls.ptr, W + 2, ctypes.c_void_p(dst.data_ptr())) == OK
            ctx.synchronize()
            check_picture(ddst, wants[1][0], (name, C, off))
            check_picture(dcls, wants[1][1], (name, C, off))
            assert record_bytes(dst) == bytes(wants[1][2]), (name, C, off)
            assert all(d.rows_and_rest()[1] for d in [dprev, dcurr, dvp, dvc] + drefs)


# ---- A4. the dense chain ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(TALL))
def test_chain(hs, gpu_ok, name):
    L = hs._lib.load()
    W, H = tall(name)
    n = 3
    us, vs, ss = chain_fields(W, H, n, seed=1000 * W + H, pad=0)
    start = start_fields(W, H, seed=W + H, pad=0)
    cp = hs.make_chain_params(CHAIN_VALUES)
    lay = layouts(W)
    pairs = [2, 0, 1]
    ints = (ctypes.c_int * n)(*pairs)
    with hs.HSFlow(W, H, n, own_stream=True) as ctx:
        for p in range(n):
            put_flow(ctx, us[p], vs[p], pair=p)
        pu, pv, states = [us[p] for p in pairs], [vs[p] for p in pairs], [ss[pairs[0]], None, ss[pairs[2]]]
        for combo, (state, st0) in enumerate(((None, None), (states, start))):
            want = chain_host_want(hs, pu, pv, state, st0, cp)
            assert all(c > 0 for k, c in enumerate(want[4][:4]) if k != 2 or state) and want[4][4] > 0, want[4]   # (untrusted: only with state planes)
            (foff, fstride), (boff, bstride) = lay[(0, 3)[combo]]
            dstate = [DevIn(s, boff, bstride) if s is not None else None for s in state] if state is not None else None
            dstart = [DevIn(x, foff, fstride) for x in st0] if st0 is not None else None
            for with_planes in (True, False):
                outs = [DevPlane(H, 4 * W, foff, fstride), DevPlane(H, 4 * W, foff, fstride), DevPlane(H, W, boff, bstride), DevPlane(H, W, (boff + 1) % 4, bstride)]
                ds = dev_stats()
                o = [d.ptr if with_planes else None for d in outs]
                assert L.hsflow_chain_flow_device(ctx._h, ints, n, ptr_list(dstate) if dstate else None, bstride, dstart[0].ptr if dstart else None,
                                                  dstart[1].ptr if dstart else None, fstride, ctypes.byref(cp), o[0], o[1], fstride, o[2], bstride, o[3], bstride,
                                                  ctypes.c_void_p(ds.data_ptr())) == OK, (name, combo)
                ctx.synchronize()
                if with_planes:
                    check_chain_outputs(hs, outs, ds, want, (name, combo))
                else:
                    assert chain_stat_tuple(hs.chain_stats_from(ds)) == want[4], (name, combo)
                    assert all(untouched(d) for d in outs)
                record_bytes(ds)


# ---- A5. the warp by a model ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name", sorted(TALL))
def test_model_warp(hs, gpu_ok, name, C):
    L = hs._lib.load()
    W, H = tall(name)
    rng = np.random.default_rng(C + H)
    src = rng.integers(0, 256, (H, W) if C == 1 else (H, W, C), dtype=np.uint8)
    ref = rng.integers(0, 256, src.shape, dtype=np.uint8)
    # (hs_gmotion_rule.h: the model is evaluated at 2 x - (W - 1), 2 y - (H - 1): small slopes over a tall frame)
    models = [np.array([1.25, 0.01, -0.002, -2.5, 0.0005, 0.0002], F), np.array([-3.0, 0, 0, 40.0, 0, 0], F)]
    rowb = W * C
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for model in models:
            mm = (ctypes.c_float * 6)(*[float(x) for x in model])
            for border in ("constant", "replicate"):
                wp = hs.make_warp_params(C, 1.0, border, (9, 8, 7))
                want, ws = hs.gmotion_warp_host(model, src, ref=ref, params=wp, return_stats=True)
                assert ws.inside > 0 and ws.outside > 0 and ws.sad_warped > 0
                for off, stride in byte_layouts(rowb):
                    label = (name, C, border, off)
                    dsrc, dref = DevIn(src, off, stride), DevIn(ref, off, stride)
                    dst, ds = DevPlane(H, rowb, off, stride), dev_stats()
                    assert L.hsflow_gmotion_warp_device(ctx._h, mm, ctypes.byref(wp), dsrc.ptr, stride, dref.ptr, stride, dst.ptr, stride, ctypes.c_void_p(ds.data_ptr())) == OK
                    ctx.synchronize()
                    check_picture(dst, want, label)
                    assert record_bytes(ds) == bytes(ws), label
                    ds = dev_stats()                                   # statistics only
                    assert L.hsflow_gmotion_warp_device(ctx._h, mm, ctypes.byref(wp), dsrc.ptr, stride, dref.ptr, stride, None, 0, ctypes.c_void_p(ds.data_ptr())) == OK
                    ctx.synchronize()
                    assert record_bytes(ds) == bytes(ws), label
                    dst = DevPlane(H, rowb, off, stride)               # no statistics: the control
                    assert L.hsflow_gmotion_warp_device(ctx._h, mm, ctypes.byref(wp), dsrc.ptr, stride, None, 0, dst.ptr, stride, None) == OK
                    ctx.synchronize()
                    check_picture(dst, want, label)


# ---- A6. sums in closed form: no host rule involved -----------------------------------------------------------------------------------

def test_sums_in_closed_form(hs, gpu_ok):
    """Zero flow, every source byte 255, every reference byte 0, three channels, eight rows per workgroup: every pixel adds
    765 to both sums of a warp and to the sum of an interpolation; a backward flow of (3, 4) everywhere adds 25 * 256 to a
    check's; every pixel of a chain of three zero flows is alive at age 3."""
    import torch
    W, H = tall("per8")
    C, n = 3, W * H
    zero = np.zeros((H, W), F)
    white, black = np.full((H, W, C), 255, np.uint8), np.zeros((H, W, C), np.uint8)
    dwhite, dblack = torch.from_numpy(white).cuda(), torch.from_numpy(black).cuda()
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        for p in range(3):
            put_flow(ctx, zero, zero, pair=p)
        put_flow(ctx, np.full((H, W), 3.0, F), np.full((H, W), 4.0, F), pair=1)
        out, st = ctx.warp(dwhite, ref=dblack, return_stats=True)
        ctx.synchronize()
        assert stat_tuple(hs.warp_stats_from(st)) == (n, 0, 0, 765 * n, 765 * n, 255, 255) and bool((out == 255).all().item())
        out, st = ctx.gmotion_warp(np.zeros(6, F), dwhite, ref=dblack, return_stats=True)
        ctx.synchronize()
        assert stat_tuple(hs.warp_stats_from(st)) == (n, 0, 0, 765 * n, 765 * n, 255, 255) and bool((out == 255).all().item())
        out, _, st = ctx.interp(0.5, dwhite, dwhite, ref=dblack, stats=True, params=hs.make_interp_params(C))
        ctx.synchronize()
        s = hs.interp_stats_from(st)
        assert (s.blended, s.sad, s.max_diff, s.holes, s.unknown, s.left) == (n, 765 * n, 255, 0, 0, 0) and bool((out == 255).all().item())
        # |f + b(x + f)|^2 = 25 > 0.01 * 25 + 0.5: every pixel inconsistent, err2 = 25 exactly
        _, _, st = ctx.fb(0, 1, mask=False, stats=True, device=True)
        ctx.synchronize()
        assert fb_stat_tuple(hs.fb_stats_from(st)) == (0, n, 0, 0, 25 * 256 * n, int(F(25.0).view(np.uint32)))
        _, _, _, _, st = ctx.chain_flow([0, 2, 0], flow=False, stats=True, device=True)
        ctx.synchronize()
        s = hs.chain_stats_from(st)
        assert tuple(int(x) for x in s.cls) == (n, 0, 0, 0) and (int(s.sum_age), int(s.max_mag2_bits)) == (3 * n, 0)


# ---- B. regions: rounds of the scan, all sixteen waves, more than 65535 labels -------------------------------------------------

SCAN_SHAPES = [(13, 1024, 1024), (13, 1025, 1025), (257, 513, 1026), (13, 4099, 4099), (300, 520, 1040)]   # W, H, n_counts
SCAN_MASKS = ["checker", "random30", "vsnake", "comb", "u"]
ROUND = 1024                                                           # lanes of k_rg_scan's one workgroup


def count_words(W, H):
    """(words per row, n_counts): one count word per 256 pixels of a row."""
    bx = (W + 255) // 256
    return bx, bx * H


def scan_regime(res, labels, mask, W, H, name, conn, min_area):
    """From the host's answer alone: which of the scan's carried sums this case needs."""
    bx, n_counts = count_words(W, H)
    last = (n_counts - 1) // ROUND * ROUND                             # the first word of the last round
    flat = labels.reshape(-1)
    word = lambda idx: idx // W * bx + idx % W // 256
    words = word(np.arange(W * H))
    fg = (mask.reshape(-1) != 0)
    assert fg[words >= last].any() and fg[words < ROUND].any(), (name, W, H)
    if name == "checker" and conn == 4 and min_area > 1:
        # every root is dropped: n_dropped is the difference of two sums that are carried through every round
        assert res.n_regions == 0 and res.n_dropped == int(fg.sum()) and res.n_dropped > (ROUND if n_counts > ROUND else 0)
        return
    assert res.n_regions > 0 and res.n_regions == int(flat.max()), (name, W, H, conn, min_area)
    vals, first = np.unique(flat, return_index=True)                   # a region's root is its first pixel in raster order
    root_word = dict(zip(vals.tolist(), word(first).tolist()))
    spread = root_word[res.n_regions] >= last                          # the largest label is handed out in the last round
    in_last = np.unique(flat[(words >= last) & (flat > 0)])
    reaches = any(root_word[int(v)] < ROUND for v in in_last)          # a first-round root owns pixels of the last round
    if name == "checker" and conn == 4:
        assert spread and res.n_regions == int(fg.sum())
        if (W, H) == (300, 520):
            assert res.n_regions > 65535
    elif name in ("random30", "sprinkled"):                             # many small regions everywhere
        assert spread or reaches, (W, H, conn, min_area)
        assert res.n_dropped > 0 or min_area == 1
    else:
        assert reaches, (name, W, H, conn, min_area)


@pytest.mark.parametrize("W,H,n_counts", SCAN_SHAPES)
def test_regions_scan_rounds(hs, gpu_ok, W, H, n_counts):
    L = hs._lib.load()
    assert count_words(W, H)[1] == n_counts
    lay = layouts(W)
    k = 0
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for name in SCAN_MASKS:
            mask = R.mask_of(name, W, H)
            for conn in (4, 8):
                for min_area in (1, 2):
                    rp = hs.make_regions_params(connectivity=conn, min_area=min_area)
                    res, labels, _ = hs.regions_host(mask, None, None, labels=True, records=False, capacity=0, params=rp)
                    scan_regime(res, labels, mask, W, H, name, conn, min_area)
                    for capacity in (3, res.n_regions + 2):
                        k += 1
                        want = host_want(hs, mask, None, None, rp, capacity, (H, W))
                        (foff, fstride), (boff, bstride) = lay[k % 4]
                        dm = DevIn(mask, boff, bstride)
                        dl, dr, ds = DevPlane(H, 4 * W, foff, fstride), dev_records(capacity), dev_stats()
                        assert L.hsflow_regions_planes_device(ctx._h, dm.ptr, bstride, None, None, 0, ctypes.byref(rp), dl.ptr, fstride, dr.data_ptr(), capacity,
                                                              ds.data_ptr()) == OK, ctx._lib.hsflow_last_error(ctx._h)
                        ctx.synchronize()
                        check_outputs(dl, dr, ds, want, (name, W, H, conn, min_area, capacity))
                        assert dm.rows_and_rest()[1]
        # with a flow: joined only where the flows agree, the sums of the records from a field with NaN and far vectors
        mask = R.mask_of("random30", W, H)
        u, v = R.flow_of("sprinkled", W, H)
        rp = hs.make_regions_params(connectivity=8, min_area=2, join_px=0.5)
        res, labels, _ = hs.regions_host(mask, u, v, labels=True, records=False, capacity=0, params=rp)
        scan_regime(res, labels, mask, W, H, "sprinkled", 8, 2)
        assert res.unknown_flow_px > 0
        capacity = res.n_regions + 2
        want = host_want(hs, mask, u, v, rp, capacity, (H, W))
        (foff, fstride), (boff, bstride) = lay[1]
        dm, du, dv = DevIn(mask, boff, bstride), DevIn(u, foff, fstride), DevIn(v, foff, fstride)
        dl, dr, ds = DevPlane(H, 4 * W, foff, fstride), dev_records(capacity), dev_stats()
        assert L.hsflow_regions_planes_device(ctx._h, dm.ptr, bstride, du.ptr, dv.ptr, fstride, ctypes.byref(rp), dl.ptr, fstride, dr.data_ptr(), capacity,
                                              ds.data_ptr()) == OK, ctx._lib.hsflow_last_error(ctx._h)
        ctx.synchronize()
        check_outputs(dl, dr, ds, want, ("sprinkled", W, H))


def test_regions_batch_second_field_behind_a_second_round(hs, gpu_ok):
    """Two pairs at 13 x 1025: field 1's count words start 1025 words on, both fields go round twice."""
    L = hs._lib.load()
    W, H, N = 13, 1025, 2
    assert count_words(W, H)[1] == ROUND + 1
    (foff, fstride), (boff, bstride) = layouts(W)[1]
    uv = [tuple(np.array(a) for a in R.flow_of("sprinkled", W, H)), (np.zeros((H, W), F), np.zeros((H, W), F))]
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, uv[p][0], uv[p][1], pair=p)
        for names, conn, min_area, join, capacity in ((("random30", "checker"), 4, 1, 0.0, 7000), (("checker", "random30"), 4, 2, 0.0, 3),
                                                      (("random30", "vsnake"), 8, 1, 0.5, 40)):
            masks = [R.mask_of(nm, W, H) for nm in names]
            rp = hs.make_regions_params(connectivity=conn, min_area=min_area, join_px=join)
            wants = [host_want(hs, masks[p], uv[p][0], uv[p][1], rp, capacity, (H, W)) for p in range(N)]
            assert wants[0][2] != wants[1][2] and all(w[3].n_regions + w[3].n_dropped > 0 for w in wants)
            dm = [DevIn(m, boff, bstride) for m in masks]
            dl = [DevPlane(H, 4 * W, foff, fstride) for _ in range(N)]
            dr = [dev_records(capacity) for _ in range(N)]
            ds = dev_stats(N)
            assert L.hsflow_regions_batch_device(ctx._h, 0, N, ptr_list(dm), bstride, ctypes.byref(rp), ptr_list(dl), fstride,
                                                 (ctypes.c_void_p * N)(*[r.data_ptr() for r in dr]), capacity, ds.data_ptr()) == OK, ctx._lib.hsflow_last_error(ctx._h)
            ctx.synchronize()
            heads = record_bytes(ds, N)
            for p in range(N):
                check_outputs(dl[p], dr[p], None, wants[p], (names, p))
                assert heads[64 * p:64 * p + 64] == wants[p][2], (names, p, wants[p][3].as_dict())
                # the pair's own call
                one_l, one_r, one_s = DevPlane(H, 4 * W, foff, fstride), dev_records(capacity), dev_stats()
                assert L.hsflow_regions_device(ctx._h, p, dm[p].ptr, bstride, ctypes.byref(rp), one_l.ptr, fstride, one_r.data_ptr(), capacity, one_s.data_ptr()) == OK
                ctx.synchronize()
                check_outputs(one_l, one_r, one_s, wants[p], (names, p, "one"))
