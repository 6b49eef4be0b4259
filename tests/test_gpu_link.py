"""Regions linked across pairs on the GPU (include/hsflow.h, ABI 0.25: hsflow_link_regions*; kernels in
opticalflowhs_amd/csrc/hs_kernels_link.hip.h) against the rule on the host (hsflow_link_regions_host, which
tests/test_link_host.py holds to a NumPy restatement).  Links, sides and headers are compared as bytes: there is no
tolerance anywhere."""
import ctypes

import numpy as np
import pytest

import link_ref as R
from test_gpu_chain import DevIn, cuda, layouts
from test_gpu_fb import FILL, DevPlane, put_flow

pytestmark = pytest.mark.gpu

F = np.float32
OK, E_ARG, E_SIZE = 0, 1, 2
# which outputs a call asks for: (links, side_a, side_b, result)
ASKS = [(1, 1, 1, 1), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 0, 1), (0, 1, 1, 0)]


def dev_bytes(n):
    """n bytes and 64 more, all FILL."""
    import torch
    t = torch.full((n + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert t.data_ptr() % 8 == 0
    return t


def host_want(hs, A, B, u, v, cap_a, cap_b, capacity):
    """The bytes of (links written, side_a, side_b, header) of the host rule, and the header."""
    res, links, sa, sb = hs.link_regions_host(A, B, u, v, link_capacity=capacity, params=hs.make_link_params(cap_a, cap_b))
    return bytes(links)[:res.n_written * 16], bytes(sa)[:cap_a * 32], bytes(sb)[:cap_b * 32], bytes(res), res


def outputs(cap_a, cap_b, capacity, ask=(1, 1, 1, 1)):
    sizes = (capacity * 16, cap_a * 32, cap_b * 32, 64)
    return [dev_bytes(n) if a else None for n, a in zip(sizes, ask)]


def dptr(t):
    return t.data_ptr() if t is not None else None


def check_outputs(outs, want, label, already=None):
    """The four tensors of a device call (None: not asked for) against the host's; nothing written behind the links that
    were written, behind a side array or behind the header.  already: what the bytes behind held before (default FILL)."""
    for k, (t, w) in enumerate(zip(outs, want[:4])):
        if t is None:
            continue
        got = bytes(t.cpu().numpy())
        assert got[:len(w)] == w, (label, k, want[4].as_dict())
        rest = already[k][len(w):] if already is not None else bytes([FILL]) * (len(got) - len(w))
        assert got[len(w):] == rest, (label, k, "written behind")


def link_planes(hs, ctx, A, B, u, v, cap_a, cap_b, capacity, lay, ask=(1, 1, 1, 1), outs=None):
    (foff, fstride), _ = lay
    H, W = A.shape
    da, db = DevIn(A, foff, fstride), DevIn(B, (foff + 4) % 16, fstride + 4)
    du, dv = DevIn(u, foff, fstride), DevIn(v, foff, fstride)
    outs = outs if outs is not None else outputs(cap_a, cap_b, capacity, ask)
    lp = hs.make_link_params(cap_a, cap_b)
    st = hs._lib.load().hsflow_link_regions_planes_device(ctx._h, da.ptr, fstride, db.ptr, fstride + 4, du.ptr, dv.ptr, fstride, ctypes.byref(lp), dptr(outs[0]),
                                                           capacity, dptr(outs[1]), dptr(outs[2]), dptr(outs[3]))
    assert st == OK, ctx._lib.hsflow_last_error(ctx._h)
    ctx.synchronize()
    for d, a in ((da, A), (db, B), (du, u), (dv, v)):                              # the inputs are as they were
        rows, clean = d.rows_and_rest()
        assert clean and np.array_equal(rows, np.ascontiguousarray(a).view(np.uint8).reshape(H, -1))
    return outs


# ---- G1. the planes form against the host form ------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", R.SHAPES)
def test_planes_device_equals_host(hs, gpu_ok, W, H):
    lay = layouts(W)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for k, case in enumerate(R.CASES):
            A, B, u, v, cap_a, cap_b = R.planes(case, W, H)
            n_all = host_want(hs, A, B, u, v, cap_a, cap_b, 0)[4].n_links
            capacity = (0, max(n_all - 1, 0), n_all + 2)[(k + W) % 3]
            want = host_want(hs, A, B, u, v, cap_a, cap_b, capacity)
            assert (want[4].flags == 1) == (capacity < n_all) and want[4].n_written == min(n_all, capacity)
            ask = ASKS[(k + H) % len(ASKS)]
            if capacity == 0 and ask == (1, 0, 0, 0):                               # a link array of no records alone is nothing asked for
                ask = (1, 0, 0, 1)
            outs = link_planes(hs, ctx, A, B, u, v, cap_a, cap_b, capacity, lay[k % 4], ask)
            check_outputs(outs, want, (case, W, H, capacity, ask))


def test_link_capacity_zero_short_and_ample(hs, gpu_ok):
    W, H = 130, 37
    A, B, u, v, cap_a, cap_b = R.planes(R.CASES[7], W, H)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        n_all = host_want(hs, A, B, u, v, cap_a, cap_b, 0)[4].n_links
        assert n_all > 20
        for capacity in (0, n_all - 1, n_all + 2):
            want = host_want(hs, A, B, u, v, cap_a, cap_b, capacity)
            assert want[4].flags == (1 if capacity < n_all else 0) and len(want[0]) == 16 * min(capacity, n_all)
            recs = hs.link_records_from(want[0] + b"", min(capacity, n_all)) if capacity else []
            assert [(r.a, r.b) for r in recs] == sorted((r.a, r.b) for r in recs)
            check_outputs(link_planes(hs, ctx, A, B, u, v, cap_a, cap_b, capacity, layouts(W)[1]), want, capacity)


def test_each_output_alone_and_all_together(hs, gpu_ok):
    W, H = 67, 19
    A, B, u, v, cap_a, cap_b = R.planes(R.CASES[8], W, H)
    want = host_want(hs, A, B, u, v, cap_a, cap_b, 50)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for ask in ASKS:
            check_outputs(link_planes(hs, ctx, A, B, u, v, cap_a, cap_b, 50, layouts(W)[2], ask), want, ask)
        lp = hs.make_link_params(cap_a, cap_b)
        da, du = DevIn(A, 0, 4 * W), DevIn(u, 0, 4 * W)
        st = hs._lib.load().hsflow_link_regions_planes_device(ctx._h, da.ptr, 4 * W, da.ptr, 4 * W, du.ptr, du.ptr, 4 * W, ctypes.byref(lp), None, 50, None, None, None)
        assert st == E_ARG                                                         # nothing asked for
        links = dev_bytes(16)
        st = hs._lib.load().hsflow_link_regions_planes_device(ctx._h, da.ptr, 4 * W, da.ptr, 4 * W, du.ptr, du.ptr, 4 * W, ctypes.byref(lp), links.data_ptr(), 0, None,
                                                               None, None)
        assert st == E_ARG                                                         # ... nor with a link array of no records
        ctx.synchronize()
        assert bool((links == FILL).all().item())


# ---- G2. more than one row per workgroup --------------------------------------------------------------------------------------

def rows_per_workgroup(W, H, cnt, cus):
    """stats_rows of hs_postops.hip.h restated for the voting kernel, whose unit is a row of 256 columns: (per, gridDim.y)."""
    units_x = (W + 255) // 256
    per = min(max(units_x * H * cnt // (2 * cus), 1), 8)
    return per, (H + per - 1) // per


@pytest.mark.parametrize("a,b,per", [(4, 1, 2), (16, 3, 8)])
def test_tall_frames_loop_over_rows(hs, gpu_ok, a, b, per):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, H = 13, a * cus + b
    got, gy = rows_per_workgroup(W, H, 1, cus)
    assert got == per and H % gy != 0 and gy < H and gy < 65535, (W, H, cus, got, gy)      # `per` rows, the last trip uneven
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for k, case in enumerate((R.CASES[1], R.CASES[5], R.CASES[6])):
            A, B, u, v, cap_a, cap_b = R.planes(case, W, H)
            want = host_want(hs, A, B, u, v, cap_a, cap_b, 300)
            check_outputs(link_planes(hs, ctx, A, B, u, v, cap_a, cap_b, 300, layouts(W)[k]), want, (case, W, H))


# ---- G3. caps that walk the compaction scan ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 16, 17, 512, 513, 4096])
def test_caps_walk_the_scan(hs, gpu_ok, cap):
    W, H = 130, 37
    n_counts = (cap * cap + 255) // 256
    assert {1: n_counts == 1, 16: n_counts == 1, 17: n_counts == 2, 512: n_counts == 1024, 513: 1024 < n_counts <= 2048, 4096: n_counts == 65536}[cap]
    rng = np.random.RandomState(cap)
    A, B = rng.randint(0, cap + 2, size=(H, W)).astype(np.int32), rng.randint(0, cap + 2, size=(H, W)).astype(np.int32)
    A[H - 1, W - 1], B[H - 1, W - 1] = cap, cap                                    # the last cell of the matrix, in the last count word
    u, v = R.flow_of("random", W, H)
    u[H - 1, W - 1] = v[H - 1, W - 1] = 0
    want = host_want(hs, A, B, u, v, cap, cap, 5000)
    links = hs.link_records_from(want[0] + b"", want[4].n_written)
    assert (links[-1].a, links[-1].b) == (cap, cap) and (cap < 513 or links[0].a * cap < 1024 * 256 < links[-1].a * cap)   # links on both sides of a scan round
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        check_outputs(link_planes(hs, ctx, A, B, u, v, cap, cap, 5000, layouts(W)[cap % 4]), want, cap)


def test_full_hash_neighbourhood_goes_to_the_global_table(hs, gpu_ok):
    """Caps 512 x 512 take the voting kernel's LDS hash (hs_kernels_link.hip.h: kLnSlots slots, kLnProbes probes from the
    home slot (word * 2654435761) >> 20).  24 pixels of one row -- one workgroup -- carry 24 different cells that share one
    home slot: at most 8 find a slot, the others take the kernel's last branch, the add to the global table itself."""
    W, H, cap, slots, probes, n = 130, 37, 512, 4096, 8, 24
    home = lambda w: ((w * 2654435761) & 0xffffffff) >> 20
    assert cap * cap + 2 * cap + 1 > 8192                                          # not the dense copy
    words = [w for w in range(cap * cap) if home(w) == home(12345)][:n]
    assert len(words) == n > 2 * probes and home(12345) < slots
    rng = np.random.RandomState(3)
    A, B = rng.randint(0, cap + 1, size=(H, W)).astype(np.int32), rng.randint(0, cap + 1, size=(H, W)).astype(np.int32)
    u, v = R.flow_of("random", W, H)
    y = 11
    for k, w in enumerate(words):                                                  # zero flow there: pixel k of the row votes for cell words[k]
        A[y, 40 + k], B[y, 40 + k] = w // cap + 1, w % cap + 1
        u[y, 40 + k] = v[y, 40 + k] = 0
    want = host_want(hs, A, B, u, v, cap, cap, 6000)
    cells = {(r.a - 1) * cap + r.b - 1 for r in hs.link_records_from(want[0] + b"", want[4].n_written)}
    assert set(words) <= cells
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for lay in layouts(W)[:2]:
            check_outputs(link_planes(hs, ctx, A, B, u, v, cap, cap, 6000, lay), want, "spill")


def test_caps_above_the_limit_enqueue_nothing(hs, gpu_ok):
    W, H = 64, 16
    A, u = R.labels_of("one", W, H), np.zeros((H, W), F)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        da, du = DevIn(A, 0, 4 * W), DevIn(u, 0, 4 * W)
        for cap_a, cap_b, capacity, code in ((4097, 4096, 8, E_SIZE), (1 << 16, 1 << 16, 8, E_SIZE), ((1 << 30) + 1, 1, 8, E_SIZE), (4, 4, (1 << 24) + 1, E_SIZE),
                                             (0, 4, 8, E_ARG)):
            res = dev_bytes(64)
            lp = hs.make_link_params(cap_a, cap_b)
            st = hs._lib.load().hsflow_link_regions_planes_device(ctx._h, da.ptr, 4 * W, da.ptr, 4 * W, du.ptr, du.ptr, 4 * W, ctypes.byref(lp), None, capacity, None,
                                                                   None, res.data_ptr())
            assert st == code, (cap_a, cap_b, capacity)
            ctx.synchronize()
            assert bool((res == FILL).all().item())


# ---- G4. batches on the context's own flow -------------------------------------------------------------------------------------

def batch_fields(W, H, n_steps, cap, seed):
    rng = np.random.RandomState(seed)
    labels = [rng.randint(-1, cap + 3, size=(H, W)).astype(np.int32) for _ in range(n_steps + 1)]
    flows = [R.flow_of("sprinkled" if p % 2 else "random", W, H, seed=seed + p) for p in range(n_steps)]
    return labels, flows


def run_batch(hs, ctx, first, n, labels, cap_a, cap_b, capacity, holes=True):
    H, W = labels[0].shape
    (foff, fstride), _ = layouts(W)[(first + n) % 4]
    dl = [DevIn(x, foff, fstride) for x in labels]
    outs = [outputs(cap_a, cap_b, capacity) for _ in range(n)]
    if holes and n > 2:
        outs[1][0] = None
        outs[n - 1][1] = None
        outs[0][2] = None
    res = dev_bytes(64 * n)
    lp = hs.make_link_params(cap_a, cap_b)
    lists = [(ctypes.c_void_p * n)(*[dptr(o[k]) for o in outs]) for k in range(3)]
    st = hs._lib.load().hsflow_link_regions_batch_device(ctx._h, first, n, (ctypes.c_void_p * (n + 1))(*[d.ptr.value for d in dl]), fstride, ctypes.byref(lp),
                                                          lists[0], capacity, lists[1], lists[2], res.data_ptr())
    assert st == OK, ctx._lib.hsflow_last_error(ctx._h)
    ctx.synchronize()
    heads = bytes(res.cpu().numpy())
    assert heads[64 * n:] == bytes([FILL]) * 64
    return outs, heads


def test_batch_of_three_is_three_single_calls_and_the_host(hs, gpu_ok):
    W, H, N, cap = 96, 64, 4, 20
    labels, flows = batch_fields(W, H, N, cap, 5)
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, *flows[p], pair=p)
        first, n = 1, 3
        outs, heads = run_batch(hs, ctx, first, n, labels[first:first + n + 1], cap, cap + 1, 70)
        for i in range(n):
            p = first + i
            want = host_want(hs, labels[p], labels[p + 1], flows[p][0], flows[p][1], cap, cap + 1, 70)
            assert heads[64 * i:64 * i + 64] == want[3], (i, want[4].as_dict())
            check_outputs(outs[i][:3], want, ("batch", i))
            one = outputs(cap, cap + 1, 70)
            da, db = DevIn(labels[p], 4, 4 * W + 4), DevIn(labels[p + 1], 4, 4 * W + 4)
            lp = hs.make_link_params(cap, cap + 1)
            st = hs._lib.load().hsflow_link_regions_device(ctx._h, p, da.ptr, db.ptr, 4 * W + 4, ctypes.byref(lp), dptr(one[0]), 70, dptr(one[1]), dptr(one[2]), dptr(one[3]))
            assert st == OK, ctx._lib.hsflow_last_error(ctx._h)
            ctx.synchronize()
            check_outputs(one, want, ("single", i))
        L = hs._lib.load()
        lp = hs.make_link_params(cap, cap)
        ptrs = (ctypes.c_void_p * 5)(*[DevIn(x, 0, 4 * W).ptr.value for x in labels])
        res = dev_bytes(64 * 4)
        for fp, ns in ((-1, 2), (2, 3), (0, 0)):                                     # bad pair ranges
            assert L.hsflow_link_regions_batch_device(ctx._h, fp, ns, ptrs, 4 * W, ctypes.byref(lp), None, 0, None, None, res.data_ptr()) == E_ARG
        ctx.synchronize()
        assert bool((res == FILL).all().item())


@pytest.mark.parametrize("n,cap", [(9, 64), (3, 2048)])
def test_batch_chunks(hs, gpu_ok, n, cap):
    """9 steps at cap 64 are a chunk of 8 and one of 1; at cap 2048 a chunk holds 4 steps: 3 steps are one set of launches
    whose tables are 16 MiB apart."""
    chunk = max(1, min(8, (1 << 24) // (cap * cap)))
    assert chunk == (8 if cap == 64 else 4)
    W, H = 67, 19
    labels, flows = batch_fields(W, H, n, cap, 40 + n)
    with hs.HSFlow(W, H, n, own_stream=True) as ctx:
        for p in range(n):
            put_flow(ctx, *flows[p], pair=p)
        outs, heads = run_batch(hs, ctx, 0, n, labels, cap, cap, 1300)
        for i in range(n):
            want = host_want(hs, labels[i], labels[i + 1], flows[i][0], flows[i][1], cap, cap, 1300)
            assert heads[64 * i:64 * i + 64] == want[3], (i, want[4].as_dict())
            check_outputs(outs[i][:3], want, (n, cap, i))


# ---- G5. nothing is carried from one call to the next -----------------------------------------------------------------------------

def test_stale_scratch_and_stale_outputs(hs, gpu_ok):
    W, H = 130, 37
    rng = np.random.RandomState(9)
    many_a, many_b = rng.randint(0, 41, size=(H, W)).astype(np.int32), rng.randint(0, 41, size=(H, W)).astype(np.int32)
    few = R.labels_of("halves", W, H)
    u, v = R.flow_of("random", W, H)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        outs = outputs(40, 40, 1700)
        before = None
        for k, (A, B, cap_a, cap_b) in enumerate(((many_a, many_b, 40, 40), (few, few, 3, 2), (many_a, many_b, 40, 40), (few, many_b, 2, 40), (many_b, many_a, 33, 7))):
            want = host_want(hs, A, B, u, v, cap_a, cap_b, 1700)
            assert (want[4].n_links > 1000, want[4].n_links < 90) == ((k in (0, 2)), (k in (1, 3)))           # many, few, many, few, some
            link_planes(hs, ctx, A, B, u, v, cap_a, cap_b, 1700, layouts(W)[k % 4], outs=outs)
            check_outputs(outs, want, k, already=before)
            before = [bytes(t.cpu().numpy()) for t in outs]


# ---- G6. the synchronous entry and the Python wrappers ----------------------------------------------------------------------------

def test_synchronous_form_and_wrappers(hs, gpu_ok):
    W, H, N, cap = 130, 37, 3, 30
    labels, flows = batch_fields(W, H, N, cap, 77)
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, *flows[p], pair=p)
        lp = hs.make_link_params(cap, cap)
        wants = [host_want(hs, labels[p], labels[p + 1], flows[p][0], flows[p][1], cap, cap, 200) for p in range(N)]
        for p in range(N):
            want = wants[p]
            # synchronous, host memory; the caller's links behind n_written stay as they were
            links = (hs.HsflowLinkRecord * 200)()
            ctypes.memset(links, FILL, ctypes.sizeof(links))
            res, links, sa, sb = ctx.link_regions(pair=p, labels_a=labels[p], labels_b=labels[p + 1], links=links, link_capacity=200, params=lp)
            assert bytes(res) == want[3] and bytes(sa) == want[1] and bytes(sb) == want[2], (p, res.as_dict(), want[4].as_dict())
            assert bytes(links)[:len(want[0])] == want[0] and bytes(links)[len(want[0]):] == bytes([FILL]) * (3200 - len(want[0]))
            # only enqueued
            dres, dlinks, dsa, dsb = ctx.link_regions(pair=p, labels_a=cuda(labels[p]), labels_b=cuda(labels[p + 1]), link_capacity=200, params=lp)
            ctx.synchronize()
            got = hs.link_result_from(dres)
            assert bytes(got) == want[3] and bytes(dlinks.cpu().numpy())[:got.n_written * 16] == want[0]
            assert bytes(hs.link_sides_from(dsa, cap)) == want[1] and bytes(hs.link_sides_from(dsb, cap)) == want[2]
            assert [r.as_dict() for r in hs.link_records_from(dlinks, got.n_written)] == [r.as_dict() for r in hs.link_records_from(links, res.n_written)]
            # caller planes
            pres, plinks, psa, psb = ctx.link_regions_planes_device(cuda(labels[p]), cuda(labels[p + 1]), cuda(flows[p][0]), cuda(flows[p][1]), link_capacity=200, params=lp)
            ctx.synchronize()
            assert bytes(hs.link_result_from(pres)) == want[3] and bytes(psa.cpu().numpy())[:cap * 32] == want[1]
            # the header alone
            only, none_l, none_a, none_b = ctx.link_regions(pair=p, labels_a=labels[p], labels_b=labels[p + 1], links=False, side_a=False, side_b=False, link_capacity=200, params=lp)
            assert bytes(only) == want[3] and none_l is None and none_a is None and none_b is None
        import torch
        results = torch.empty(64 * N, dtype=torch.uint8, device="cuda")
        sides_a = [torch.empty(32 * cap, dtype=torch.uint8, device="cuda") for _ in range(N)]
        sides_b = [torch.empty(32 * cap, dtype=torch.uint8, device="cuda") for _ in range(N)]
        ctx.link_regions_batch_device(0, N, [cuda(x) for x in labels], side_a=sides_a, side_b=sides_b, results=results, link_capacity=200, params=lp)
        ctx.synchronize()
        assert [bytes(r) for r in hs.link_result_from(results, N)] == [w[3] for w in wants]
        assert [bytes(hs.link_sides_from(t, cap)) for t in sides_a] == [w[1] for w in wants]
        # ids over the three steps from the device's sides equal those from the host's
        counts = [int(x.max()) for x in labels]
        ids, n_tracks = hs.link_tracks([hs.link_sides_from(t, cap) for t in sides_a], [hs.link_sides_from(t, cap) for t in sides_b], counts, cap, 0)
        want_ids, want_n = hs.link_tracks([hs.link_sides_from(w[1], cap) for w in wants], [hs.link_sides_from(w[2], cap) for w in wants], counts, cap, 0)
        assert np.array_equal(ids, want_ids) and n_tracks == want_n >= cap


# ---- G7. label planes from a real labelling: a square that moves ---------------------------------------------------------------------

def test_moving_square_keeps_its_id(hs, gpu_ok):
    import torch
    W, H, N = 96, 64, 3
    masks, flows = [], []
    for k in range(N + 1):
        m = np.zeros((H, W), np.uint8)
        m[20:36, 10 + 5 * k:30 + 5 * k] = 255                                       # the square, 5 pixels further each frame
        m[50:54, 80:90] = 255                                                        # a second object that stands still
        masks.append(m)
    for k in range(N):
        u = np.zeros((H, W), F)
        u[20:36, 10 + 5 * k:30 + 5 * k] = 5
        flows.append((u, np.zeros((H, W), F)))
    with hs.HSFlow(W, H, N + 1, own_stream=True) as ctx:
        for p in range(N):
            put_flow(ctx, *flows[p], pair=p)
        put_flow(ctx, np.zeros((H, W), F), np.zeros((H, W), F), pair=N)
        labels = [torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in range(N + 1)]
        heads = torch.empty(64 * (N + 1), dtype=torch.uint8, device="cuda")
        ctx.regions_batch_device(0, N + 1, mask=[cuda(m) for m in masks], labels=labels, results=heads)
        cap = 8
        sa = [torch.empty(32 * cap, dtype=torch.uint8, device="cuda") for _ in range(N)]
        sb = [torch.empty(32 * cap, dtype=torch.uint8, device="cuda") for _ in range(N)]
        results = torch.empty(64 * N, dtype=torch.uint8, device="cuda")
        lp = hs.make_link_params(cap, cap)
        ctx.link_regions_batch_device(0, N, labels, side_a=sa, side_b=sb, results=results, params=lp)
        ctx.synchronize()
        counts = [r.n_regions for r in hs.regions_result_from(heads, N + 1)]
        assert counts == [2] * (N + 1)
        for p, r in enumerate(hs.link_result_from(results, N)):
            want = host_want(hs, labels[p].cpu().numpy(), labels[p + 1].cpu().numpy(), flows[p][0], flows[p][1], cap, cap, 256)
            assert bytes(r) == want[3] and bytes(sa[p].cpu().numpy()) == want[1] and bytes(sb[p].cpu().numpy()) == want[2]
            assert (r.n_links, r.n_mutual, r.voted_px, r.gone_px, r.unmatched_px) == (2, 2, 16 * 20 + 4 * 10, 0, 0)
        ids, n = hs.link_tracks([hs.link_sides_from(t, cap) for t in sa], [hs.link_sides_from(t, cap) for t in sb], counts, cap)
        assert n == 2 and ids[:, :2].tolist() == [[1, 2]] * (N + 1) and not ids[:, 2:].any()


# ---- G8. the drop-in CLI ---------------------------------------------------------------------------------------------------------------

def test_cli_objects_file(hs, gpu_ok, tmp_path):
    """HSFLOW_CAMERA_OBJECTS on the batched camera route writes, per batch, the regions of every pair with ids that hold over
    the batch: the same composition through the Python entries gives the same file."""
    import torch
    from opticalflowhs_amd import synth
    from test_gpu_chain import run_cli
    ITER, EPS = hs.TERM_ITER, hs.TERM_EPS
    W, H, N = 160, 96, 3
    frames = []
    for i in range(N + 1):
        f = np.ascontiguousarray(synth.translating_pair(W, H, seed=77, dx=0.0, dy=0.0)[1], np.uint8).copy()
        f[30:54, 20 + 3 * i:52 + 3 * i] = (np.arange(24)[:, None] * 9 + np.arange(32)[None, :] * 7) % 200 + 30       # a textured square, 3 px a frame
        frames.append(f)
    cam = tmp_path / "cam"
    cam.mkdir()
    for i, f in enumerate(frames):
        with open(str(cam / ("frame_%04d.pgm" % i)), "wb") as fh:
            fh.write(b"P5\n%d %d\n255\n" % (W, H) + f.tobytes())
    got, _ = run_cli(cam, tmp_path / "objects", {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_OBJECTS": "6,100"})
    assert sorted(got) == ["flow_%04d.ppm" % i for i in (1, 2, 3)] + ["objects_0003.txt"]
    cap = 256
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        ctx.set_pair_termination(True)
        ctx.set_sequence_device([cuda(f) for f in frames], "gray_blur", reblur=True)
        ctx.solve(lam=0.1, max_iter=12, term_type=ITER | EPS, epsilon=float(np.float32(1e-6)))
        masks = [torch.empty((H, W), dtype=torch.uint8, device="cuda") for _ in range(N)]
        labels = [torch.empty((H, W), dtype=torch.int32, device="cuda") for _ in range(N)]
        recs = [torch.empty(64 * cap, dtype=torch.uint8, device="cuda") for _ in range(N)]
        heads = torch.empty(64 * N, dtype=torch.uint8, device="cuda")
        sa = [torch.empty(32 * cap, dtype=torch.uint8, device="cuda") for _ in range(N - 1)]
        sb = [torch.empty(32 * cap, dtype=torch.uint8, device="cuda") for _ in range(N - 1)]
        ctx.global_motion_batch_device(0, N, mask=masks, params=hs.make_gmotion_params(values=(0, 255, 0, 0)))
        ctx.regions_batch_device(0, N, mask=masks, labels=labels, records=recs, capacity=cap, results=heads, params=hs.make_regions_params(min_area=6))
        ctx.link_regions_batch_device(0, N - 1, labels, side_a=sa, side_b=sb, params=hs.make_link_params(cap, cap))
        ctx.synchronize()
        res = hs.regions_result_from(heads, N)
        ids, _ = hs.link_tracks([hs.link_sides_from(t, cap) for t in sa], [hs.link_sides_from(t, cap) for t in sb], [r.n_regions for r in res], cap, 100)
        lines = []
        for k in range(N):
            for j, q in enumerate(hs.regions_records_from(recs[k], res[k].n_written)):
                lines.append("%d %d %d %d %d %d %d %d %d %d %d %d\n" % (k, ids[k, j], q.area, q.x0, q.y0, q.x1, q.y1, q.sum_x, q.sum_y, q.n_flow, q.sum_qu, q.sum_qv))
    assert len(lines) >= N and got["objects_0003.txt"].decode() == "".join(lines)
    two, _ = run_cli(cam, tmp_path / "two", {"HSFLOW_CAMERA_BATCH": "2", "HSFLOW_CAMERA_OBJECTS": "6"})             # ids restart with the tail's batch
    tail = [line.split()[:2] for line in two["objects_0003.txt"].decode().splitlines()]
    assert "objects_0002.txt" in two and tail == [["2", str(j + 1)] for j in range(len(tail))]
    for k, extra in enumerate(({"HSFLOW_CAMERA_OBJECTS": "6"}, {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_OBJECTS": "0"},
                               {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_OBJECTS": "6,257"})):
        files, r = run_cli(cam, tmp_path / ("bad%d" % k), extra, ok=False)
        assert r.returncode == 1 and "HSFLOW_CAMERA_OBJECTS" in r.stdout and not files, (extra, r.stdout)
    import os
    import subprocess
    from conftest import ROOT
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""), HSFLOW_CAMERA_DIR=str(cam),
               HSFLOW_CAMERA_BATCH="3", HSFLOW_CAMERA_OBJECTS="6")
    env.pop("HSFLOW_CAMERA_OUT", None)                                              # nowhere to write the file: refused, not ignored
    r = subprocess.run([os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli"), "-cv", "-cam", ".1", "12"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "HSFLOW_CAMERA_OBJECTS needs HSFLOW_CAMERA_OUT" in r.stdout, r.stdout
