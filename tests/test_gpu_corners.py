"""Corner detection on the GPU (include/hsflow.h, ABI 0.26: hsflow_corners*; kernels in
opticalflowhs_amd/csrc/hs_kernels_corners.hip.h) against the rule on the host (hsflow_corners_host, which
tests/test_corners_host.py holds to a NumPy restatement).  Records, xy and headers are compared as bytes: there is no
tolerance anywhere.  The kernels' sizes that the shapes below are chosen around: the score pass works on tiles of 64 x 16
pixels, the suppression on 256 x 8 (a row SEGMENT is 256 pixels), the scan takes 1024 segments per round in wavefronts of
64, the ranking streams 1024 candidates per LDS chunk and ranks 256 per workgroup."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import corners_ref as R
from conftest import ROOT
from opticalflowhs_amd import synth
from test_gpu_chain import DevIn, cuda, layouts, ptr_list
from test_gpu_fb import FILL, put_flow

pytestmark = pytest.mark.gpu

F = np.float32
OK, E_ARG, E_SIZE, E_STATE = 0, 1, 2, 5
SEG, SCAN_ROUND, RANK_CHUNK, RANK_LANES = 256, 1024, 1024, 256


def dev_fill(nbytes, off=0):
    """(tensor, pointer) of nbytes + 64 bytes of FILL, the pointer `off` bytes behind an 8-byte multiple."""
    import torch
    t = torch.full((nbytes + 64 + 8,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert t.data_ptr() % 8 == 0
    return t, t.data_ptr() + off


def host_want(hs, g, mask, prm, capacity):
    """(the bytes of the records written, the bytes of all capacity xy pairs, the header's 64 bytes, the header)."""
    res, rec, xy = hs.corners_host(g, mask=mask, capacity=capacity, records=True, xy=True, params=prm)
    return bytes(rec)[:res.n_written * 16], xy[:capacity].tobytes() if capacity else b"", bytes(res), res


def planes_call(hs, ctx, g, mask, prm, capacity, ask=(True, True, True), lay=0, xy_off=0):
    """hsflow_corners_planes_device on planes in the byte layout `lay`; returns what host_want returns, after checking the
    guard bands: nothing is written behind capacity records, capacity pairs or the header, and no record from n_written on."""
    H, W = g.shape
    boff, bstride = layouts(W)[lay][1]
    dg = DevIn(g, boff, bstride)
    dm = DevIn(mask, (boff + 1) % 4, bstride) if mask is not None else None
    rec, rp = dev_fill(capacity * 16) if ask[0] else (None, None)
    xy, xp = dev_fill(capacity * 8, xy_off) if ask[1] else (None, None)
    res, sp = dev_fill(64) if ask[2] else (None, None)
    st = hs._lib.load().hsflow_corners_planes_device(ctx._h, dg.ptr, bstride, dm.ptr if dm else None, bstride, ctypes.byref(prm), rp, capacity, xp, sp)
    assert st == OK, ctx._lib.hsflow_last_error(ctx._h)
    ctx.synchronize()
    for d, a in ((dg, g), (dm, mask)):                                         # the inputs are as they were
        if d is not None:
            rows, clean = d.rows_and_rest()
            assert clean and np.array_equal(rows, a)
    out = [None, None, None]
    if ask[2]:
        raw = bytes(res.cpu().numpy())
        assert raw[64:] == bytes([FILL]) * (len(raw) - 64)
        out[2] = raw[:64]
    if ask[1]:
        raw = bytes(xy.cpu().numpy())
        assert raw[:xy_off] == bytes([FILL]) * xy_off and raw[xy_off + capacity * 8:] == bytes([FILL]) * (len(raw) - xy_off - capacity * 8)
        out[1] = raw[xy_off:xy_off + capacity * 8]
    if ask[0]:
        out[0] = bytes(rec.cpu().numpy())
    return out


def check(got, want, label):
    recs, xy, head, res = want
    if got[2] is not None:
        assert got[2] == head, (label, res.as_dict())
    if got[1] is not None:
        assert got[1] == xy, label
    if got[0] is not None:
        assert got[0][:len(recs)] == recs, label
        assert got[0][len(recs):] == bytes([FILL]) * (len(got[0]) - len(recs)), label      # no record from n_written on, none behind capacity


# ---- G1. shapes around every tile, segment and round ------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(64, 16), (67, 19), (256, 8), (259, 11), (255, 9), (257, 9), (1, 1), (1, 7), (5, 1)])
def test_planes_device_equals_host(hs, gpu_ok, W, H):
    k = 0
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for name in ("noise", "sines", "checker"):
            g = R.plane(name, W, H)
            for kind in ("min_eigen", "harris"):
                for block_r, nms_r in ((1, 1), (1, 3), (3, 8), (2, 5)):
                    k += 1
                    prm = hs.make_corners_params(kind=kind, block_r=block_r, nms_r=nms_r, border=(0, 0, 2)[k % 3])
                    n_all = hs.corners_host(g, capacity=0, records=False, params=prm)[0].n_survivors
                    capacity = 3 if k % 2 else n_all + 2
                    want = host_want(hs, g, None, prm, capacity)
                    got = planes_call(hs, ctx, g, None, prm, capacity, lay=k % 4, xy_off=4 * (k % 2))
                    check(got, want, (name, W, H, kind, block_r, nms_r, capacity))


def test_strongest_pixel_on_each_side_of_a_tile_border(hs, gpu_ok):
    """block_r = 3, nms_r = 8 on 24-pixel checkerboards (every crossing is a plateau of equal scores some pixels wide; further
    apart than that plus nms_r, or equal scores would suppress one another along the whole board), shifted pixel by pixel so
    that the surviving pixel of a crossing lies on each side of the borders x = 64 (score tile) and x = 256 (suppression
    tile, segment), y = 8 and y = 16, and in the tiles' corners; the host's survivors say that it did."""
    W, H = 300, 40
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for kind in ("min_eigen", "harris"):
            prm = hs.make_corners_params(kind=kind, block_r=3, nms_r=8)
            seen = set()
            for ox in range(3, 10):
                for oy in (3, 4, 5, 6, 11, 12, 13, 14):
                    g = R.checker(W, H, cell=24, ox=ox, oy=oy)
                    want = host_want(hs, g, None, prm, 200)
                    got = planes_call(hs, ctx, g, None, prm, 200)
                    check(got, want, (kind, ox, oy))
                    assert want[3].n_written >= 8
                    seen |= {(r.x, r.y) for r in hs.corners_records_from(ctypes.create_string_buffer(want[0]), want[3].n_written)}
            assert all((x, y) in seen for x in (63, 64, 255, 256) for y in (7, 8, 15, 16)), sorted(seen)


@pytest.mark.parametrize("W,H", [(5, 63), (5, 64), (5, 65), (5, 1023), (5, 1024), (5, 1025), (5, 1100), (257, 520)])
def test_scan_rounds(hs, gpu_ok, W, H):
    """The scan's count vector holds ceil(W / 256) * H segments, one lane each, 1024 per round: one below, at and one above
    a wavefront and a round, and two rounds with survivors in the second."""
    g = R.noise(W, H, seed=H)
    n_segs = (W + SEG - 1) // SEG * H
    assert n_segs in (63, 64, 65, 1023, 1024, 1025, 1100, 1040)
    prm = hs.make_corners_params(nms_r=1)
    want = host_want(hs, g, None, prm, 16384)
    recs = hs.corners_records_from(ctypes.create_string_buffer(want[0]), want[3].n_written)
    assert want[3].n_written == want[3].n_survivors > H // 16
    seg_of = [(r.y * ((W + SEG - 1) // SEG) + r.x // SEG) for r in recs]
    if n_segs >= 1100 or W > SEG:
        assert max(seg_of) >= SCAN_ROUND                                       # a survivor whose offset needs the first round's carry
    if W > SEG:
        assert any(r.x >= SEG for r in recs)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        check(planes_call(hs, ctx, g, None, prm, 16384), want, (W, H))


def test_candidates_span_lds_chunks_and_workgroups(hs, gpu_ok):
    W, H = 520, 300
    g = R.noise(W, H)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for kind in ("min_eigen", "harris"):
            prm = hs.make_corners_params(kind=kind, nms_r=1, quality_q16=0)
            want = host_want(hs, g, None, prm, 16384)
            assert want[3].n_candidates > 3 * RANK_CHUNK and want[3].n_candidates > 3 * RANK_LANES and want[3].flags == 0
            check(planes_call(hs, ctx, g, None, prm, 16384), want, kind)
            # a capacity inside the list, and TRUNCATED in the middle of a chunk
            check(planes_call(hs, ctx, g, None, prm, 1500), host_want(hs, g, None, prm, 1500), kind)
            prm.max_candidates = 2500
            want = host_want(hs, g, None, prm, 4000)
            assert want[3].flags == R.TRUNCATED and want[3].n_written == 2500
            check(planes_call(hs, ctx, g, None, prm, 4000), want, kind)


def test_truncated_masks_each_output_alone(hs, gpu_ok):
    W, H = 259, 37
    g = R.noise(W, H)
    mask = (R.noise(W, H, seed=5) % 3).astype(np.uint8)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        for kind in ("min_eigen", "harris"):
            seven = hs.make_corners_params(kind=kind, nms_r=1, max_candidates=7)
            want = host_want(hs, g, None, seven, 20)
            assert want[3].flags == R.TRUNCATED and want[3].n_candidates == 7
            check(planes_call(hs, ctx, g, None, seven, 20), want, kind)
            want = host_want(hs, g, None, seven, 3)
            assert want[3].flags == R.TRUNCATED | R.OVERFLOW
            check(planes_call(hs, ctx, g, None, seven, 3), want, kind)
            for fg in ((1, 255), (0, 0), (2, 2)):
                prm = hs.make_corners_params(kind=kind, fg=fg)
                want = host_want(hs, g, mask, prm, 64)
                assert 0 < want[3].allowed_px < W * H
                for lay in range(4):
                    check(planes_call(hs, ctx, g, mask, prm, 64, lay=lay), want, (kind, fg, lay))
            prm = hs.make_corners_params(kind=kind)
            want = host_want(hs, g, mask, prm, 40)
            for one in range(3):
                ask = tuple(k == one for k in range(3))
                got = planes_call(hs, ctx, g, mask, prm, 40, ask=ask)
                assert got[one] is not None and all(x is None for k, x in enumerate(got) if k != one)
                check(got, want, (kind, one))
            check(planes_call(hs, ctx, g, mask, prm, 0, ask=(False, False, True)), host_want(hs, g, mask, prm, 0), "capacity 0")


# ---- G2. the forms on a context's own frames ------------------------------------------------------------------------------------

def frames_of(W, H, n):
    return [synth.translating_pair(W, H, seed=31 + i, dx=1.0, dy=0.5) for i in range(n)]


def test_batch_equals_single_calls_and_the_host(hs, gpu_ok):
    import torch
    L = hs._lib.load()
    W, H, N = 260, 37, 3
    pairs = frames_of(W, H, N)
    masks = [None, (R.noise(W, H, seed=9) % 2 * 255).astype(np.uint8), None]
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p, (a, b) in enumerate(pairs):
            ctx.set_frames(a, b, pair=p)
        own = [ctx.frames(p) for p in range(N)]
        prm = hs.make_corners_params(nms_r=2)
        capacity = 50
        for which in (0, 1):
            wants = [host_want(hs, own[p][which], masks[p], prm, capacity) for p in range(N)]
            assert len({w[2] for w in wants}) == N and all(w[3].n_written > 5 for w in wants)
            dm = [cuda(m) if m is not None else None for m in masks]
            recs, xys = [dev_fill(capacity * 16) for _ in range(N)], [dev_fill(capacity * 8) for _ in range(N)]
            res, rp = dev_fill(64 * N)
            st = L.hsflow_corners_batch_device(ctx._h, 0, N, which, ptr_list(dm), W, ctypes.byref(prm), (ctypes.c_void_p * N)(*[r[1] for r in recs]), capacity,
                                               (ctypes.c_void_p * N)(*[x[1] for x in xys]), rp)
            assert st == OK, ctx._lib.hsflow_last_error(ctx._h)
            ctx.synchronize()
            heads = bytes(res.cpu().numpy())
            assert heads[64 * N:] == bytes([FILL]) * (len(heads) - 64 * N)
            for p in range(N):
                check([bytes(recs[p][0].cpu().numpy()), bytes(xys[p][0].cpu().numpy())[:capacity * 8], heads[64 * p:64 * p + 64]], wants[p], (which, p))
                # the single call and the Python wrappers
                dres, drec, dxy = ctx.corners(pair=p, which=which, mask=dm[p], capacity=capacity, records=True, xy=True, params=prm, device=True)
                ctx.synchronize()
                assert bytes(dres.cpu().numpy()) == wants[p][2] and dxy.cpu().numpy().tobytes() == wants[p][1]
                assert bytes(drec.cpu().numpy())[:len(wants[p][0])] == wants[p][0]
                # the synchronous form: host memory
                hres, hrec, hxy = ctx.corners(pair=p, which=which, mask=masks[p], capacity=capacity, records=True, xy=True, params=prm)
                assert bytes(hres) == wants[p][2] and hxy.tobytes() == wants[p][1]
                assert bytes(hrec)[:len(wants[p][0])] == wants[p][0] and bytes(hrec)[len(wants[p][0]):] == b"\0" * (capacity * 16 - len(wants[p][0]))
            # the wrapper of the batch, with holes
            out = torch.full((64 * N,), FILL, dtype=torch.uint8, device="cuda")
            xl = [torch.zeros((capacity, 2), dtype=torch.float32, device="cuda") if p != 1 else None for p in range(N)]
            ctx.corners_batch_device(0, N, which=which, mask=dm, xy=xl, capacity=capacity, results=out, params=prm)
            ctx.synchronize()
            got = hs.corners_result_from(out, N)
            assert [bytes(g) for g in got] == [w[2] for w in wants]
            assert all(xl[p].cpu().numpy().tobytes() == wants[p][1] for p in (0, 2))


def test_more_fields_than_one_set_of_launches(hs, gpu_ok):
    W, H, N = 67, 19, 10
    pairs = frames_of(W, H, N)
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p, (a, b) in enumerate(pairs):
            ctx.set_frames(a, b, pair=p)
        prm = hs.make_corners_params()
        import torch
        out = torch.full((64 * N,), FILL, dtype=torch.uint8, device="cuda")
        ctx.corners_batch_device(0, N, which=1, capacity=9, results=out, params=prm)
        ctx.synchronize()
        got = hs.corners_result_from(out, N)
        for p in range(N):
            assert bytes(got[p]) == host_want(hs, ctx.frames(p)[1], None, prm, 9)[2], p


def test_consecutive_calls_carry_nothing_over(hs, gpu_ok):
    W, H = 259, 37
    g1, g2 = R.noise(W, H), R.sines(W, H)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        a = hs.make_corners_params(kind="harris", nms_r=1, quality_q16=0)
        b = hs.make_corners_params(kind="min_eigen", nms_r=8, block_r=3, quality_q16=30000, border=5)
        for g, prm in ((g1, a), (g2, b), (g1, b), (g2, a), (g2, a)):
            check(planes_call(hs, ctx, g, None, prm, 300), host_want(hs, g, None, prm, 300), "again")


# ---- G3. corners into the tracker, no read-back ------------------------------------------------------------------------------------

def test_xy_goes_straight_into_track_points(hs, gpu_ok):
    W, H, N, capacity = 96, 64, 3, 40
    pairs = frames_of(W, H, N)
    rng = np.random.default_rng(5)
    us = [(rng.standard_normal((H, W)) * 0.7 + 1.0).astype(F) for _ in range(N)]
    vs = [(rng.standard_normal((H, W)) * 0.7 - 0.5).astype(F) for _ in range(N)]
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for p, (a, b) in enumerate(pairs):
            ctx.set_frames(a, b, pair=p)
            put_flow(ctx, us[p], vs[p], pair=p)
        prm = hs.make_corners_params(nms_r=6, quality_q16=6000)
        first = ctx.frames(0)[0]
        hres, _, hxy = hs.corners_host(first, capacity=capacity, records=False, xy=True, params=prm)
        assert 3 <= hres.n_written < capacity                                   # a NaN tail to carry through
        _, _, dxy = ctx.corners(pair=0, which=0, capacity=capacity, records=False, xy=True, result=False, params=prm, device=True)
        chp = hs.make_chain_params(values=(hs.CHAIN_ALIVE, hs.CHAIN_LEFT, hs.CHAIN_UNTRUSTED, hs.CHAIN_UNKNOWN))   # the status bytes are the classes
        last, _, status, _, _ = ctx.track_points(dxy, list(range(N)), status=True, params=chp)   # m = capacity, enqueued behind the corners
        ctx.synchronize()
        wl, _, wst, _, _ = hs.track_points_host(us, vs, hxy, status=True, params=chp)
        assert dxy.cpu().numpy().tobytes() == hxy.tobytes()
        assert last.cpu().numpy().tobytes() == wl.tobytes() and np.array_equal(status.cpu().numpy(), wst)
        assert (wst[hres.n_written:] == hs.CHAIN_UNKNOWN).all() and (wst[:hres.n_written] != hs.CHAIN_UNKNOWN).any()


# ---- G4. refusals --------------------------------------------------------------------------------------------------------------

def test_refusals_enqueue_nothing(hs, gpu_ok):
    L = hs._lib.load()
    W, H = 67, 19
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        prm = hs.make_corners_params()
        g = cuda(R.noise(W, H))
        rec, rp = dev_fill(16 * 4)
        res, sp = dev_fill(64)
        assert L.hsflow_corners_device(ctx._h, 0, 0, None, 0, ctypes.byref(prm), rp, 4, None, sp) == E_STATE          # no frames were set
        a, b = synth.translating_pair(W, H, seed=1, dx=1.0, dy=0.0)
        ctx.set_frames(a, b, pair=0)
        ctx.set_frames(a, b, pair=1)
        assert L.hsflow_corners_device(ctx._h, 0, 2, None, 0, ctypes.byref(prm), rp, 4, None, sp) == E_ARG            # which
        assert L.hsflow_corners_device(ctx._h, 2, 0, None, 0, ctypes.byref(prm), rp, 4, None, sp) == E_ARG            # pair
        assert L.hsflow_corners_batch_device(ctx._h, 1, 2, 0, None, 0, ctypes.byref(prm), None, 4, None, sp) == E_ARG
        assert L.hsflow_corners_device(ctx._h, 0, 0, None, 0, ctypes.byref(prm), rp + 4, 4, None, sp) == E_ARG
        assert L.hsflow_corners_device(ctx._h, 0, 0, None, 0, ctypes.byref(prm), None, 4, None, None) == E_ARG
        assert L.hsflow_corners_device(ctx._h, 0, 0, g.data_ptr(), W - 1, ctypes.byref(prm), rp, 4, None, sp) == E_SIZE
        assert L.hsflow_corners_planes_device(ctx._h, None, W, None, 0, ctypes.byref(prm), rp, 4, None, sp) == E_ARG
        assert L.hsflow_corners_planes_device(ctx._h, g.data_ptr(), W - 1, None, 0, ctypes.byref(prm), rp, 4, None, sp) == E_SIZE
        assert L.hsflow_corners_planes_device(ctx._h, g.data_ptr(), W, None, 0, ctypes.byref(prm), g.data_ptr(), 4, None, sp) == E_ARG     # overlap
        bad = hs.make_corners_params(nms_r=9)
        assert L.hsflow_corners_planes_device(ctx._h, g.data_ptr(), W, None, 0, ctypes.byref(bad), rp, 4, None, sp) == E_ARG
        ctx.synchronize()
        assert bool((rec == FILL).all().item()) and bool((res == FILL).all().item())
        assert L.hsflow_corners_device(ctx._h, 1, 1, None, 0, ctypes.byref(prm), rp, 4, None, sp) == OK
        ctx.synchronize()
        assert bytes(res.cpu().numpy())[:64] == host_want(hs, ctx.frames(1)[1], None, prm, 4)[2]


# ---- G5. the drop-in CLI -----------------------------------------------------------------------------------------------------------

def test_cli_points(hs, gpu_ok, tmp_path):
    from test_gpu_chain import run_cli, ITER, EPS
    W, H, n = 160, 96, 24
    frames = [synth.translating_pair(W, H, seed=77, dx=1.5 * i, dy=-0.75 * i)[1] for i in range(4)]
    cam = tmp_path / "cam"
    cam.mkdir()
    for i, f in enumerate(frames):
        with open(str(cam / ("frame_%04d.pgm" % i)), "wb") as fh:
            fh.write(b"P5\n%d %d\n255\n" % (W, H) + np.ascontiguousarray(f, np.uint8).tobytes())
    plain, _ = run_cli(cam, tmp_path / "plain", {"HSFLOW_CAMERA_BATCH": "3"})
    got, _ = run_cli(cam, tmp_path / "points", {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_POINTS": "%d,2000,5" % n})
    assert sorted(got) == sorted(plain) + ["points_0003.txt"]
    assert all(got[k] == plain[k] for k in plain)                     # the flow pictures stay byte for byte
    prm = hs.make_corners_params(quality_q16=2000, nms_r=5)
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        ctx.set_pair_termination(True)
        ctx.set_sequence_device([cuda(f) for f in frames], "gray_blur", reblur=True)
        ctx.solve(lam=0.1, max_iter=12, term_type=ITER | EPS, epsilon=float(np.float32(1e-6)))
        flows = [ctx.flow(p) for p in range(3)]
        first = ctx.frames(0)[0]
    res, rec, xy = hs.corners_host(first, capacity=n, records=True, xy=True, params=prm)
    last, _, status, age, _ = hs.track_points_host([f[0] for f in flows], [f[1] for f in flows], xy, status=True, age=True)

    def num(a):
        return "nan" if a != a else "%.9g" % float(a)

    lines = ["%d %d %d %d %s %s %d %d\n" % (k, r.x, r.y, r.score, num(last[k, 0]), num(last[k, 1]), status[k], age[k])
             for k, r in enumerate(hs.corners_records_from(rec, res.n_written))]
    assert 3 <= res.n_written <= n and got["points_0003.txt"].decode() == "".join(lines)
    two, _ = run_cli(cam, tmp_path / "two", {"HSFLOW_CAMERA_BATCH": "2", "HSFLOW_CAMERA_POINTS": "5"})   # a batch of two and a tail of one
    assert sorted(two) == sorted(plain) + ["points_0002.txt", "points_0003.txt"] and all(two[k] == plain[k] for k in plain)
    assert len(two["points_0002.txt"].decode().splitlines()) == 5
    for k, extra in enumerate(({"HSFLOW_CAMERA_POINTS": "5"}, {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_POINTS": "0"}, {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_POINTS": "5,70000"},
                               {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_POINTS": "5,100,9"}, {"HSFLOW_CAMERA_BATCH": "3", "HSFLOW_CAMERA_POINTS": "five"})):
        files, r = run_cli(cam, tmp_path / ("bad%d" % k), extra, ok=False)
        assert r.returncode == 1 and "HSFLOW_CAMERA_" in r.stdout and not files, (extra, r.stdout)
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd"), HSFLOW_CAMERA_DIR=str(cam), HSFLOW_CAMERA_BATCH="3", HSFLOW_CAMERA_POINTS="5")
    env.pop("HSFLOW_CAMERA_OUT", None)
    r = subprocess.run([os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli"), "-cv", "-cam", ".1", "12"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "HSFLOW_CAMERA_POINTS needs HSFLOW_CAMERA_OUT" in r.stdout
