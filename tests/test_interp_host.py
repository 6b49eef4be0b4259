"""hsflow_interp_host / hsflow_project_flow_host: the rule of csrc/hs_interp_rule.h on the host -- the forward flow projected
to time t, its holes filled, both frames fetched along the projected vector and blended.  No GPU work: the device side is
held to these bits by tests/test_gpu_interp.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SHAPES = [(13, 7), (260, 37), (96, 64)]
F = np.float32
NEXT_ABOVE_1E9 = np.nextafter(F(1e9), F(np.inf))


# ---- the rule restated in NumPy: every operation an array operation of one type, and so rounded on its own ---------------

def known_of(u, v):
    return ~(np.isnan(u) | np.isnan(v) | (np.abs(u) > F(1e9)) | (np.abs(v) > F(1e9)))


def locate(a, b, t, W, H, replicate, f=F):
    """hswarp::locate for whole planes of known vectors: (inside, x0, x1, y0, y1, ax, ay)."""
    xs = np.broadcast_to(np.arange(W, dtype=f)[None, :], (H, W))
    ys = np.broadcast_to(np.arange(H, dtype=f)[:, None], (H, W))
    fx = (xs + (a.astype(f) * f(t)).astype(f)).astype(f)
    fy = (ys + (b.astype(f) * f(t)).astype(f)).astype(f)
    inside = (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
    sample = inside | replicate
    fx = np.where(sample, np.clip(fx, f(0), f(W - 1)), f(0))
    fy = np.where(sample, np.clip(fy, f(0), f(H - 1)), f(0))
    x0 = np.floor(fx).astype(np.int64)
    y0 = np.floor(fy).astype(np.int64)
    return inside, x0, np.minimum(x0 + 1, W - 1), y0, np.minimum(y0 + 1, H - 1), (fx - x0.astype(f)).astype(f), (fy - y0.astype(f)).astype(f)


def bilinear(pic, x0, x1, y0, y1, ax, ay, f=F):
    """The warp's order of operations, unrounded: (H, W, C) of type f."""
    p00, p10, p01, p11 = (pic[yy, xx].astype(f) for yy, xx in ((y0, x0), (y0, x1), (y1, x0), (y1, x1)))
    ax, ay = ax[..., None], ay[..., None]
    top = (p00 + (ax * (p10 - p00).astype(f)).astype(f)).astype(f)
    bot = (p01 + (ax * (p11 - p01).astype(f)).astype(f)).astype(f)
    return (top + (ay * (bot - top).astype(f)).astype(f)).astype(f)


def to_byte(val, f=F):
    return np.minimum((val + f(0.5)).astype(f).astype(np.int64), 255)


def restate_project(u, v, prev, curr, t):
    """P: (ut, vt, state, counters).  prev, curr: (H, W, C)."""
    H, W, _ = prev.shape
    known = known_of(u, v)
    a = np.where(known, u, F(0))
    b = np.where(known, v, F(0))
    inside, x0, x1, y0, y1, ax, ay = locate(a, b, 1.0, W, H, False)
    warped = to_byte(bilinear(curr, x0, x1, y0, y1, ax, ay))
    cost = np.where(inside, np.abs(prev.astype(np.int64) - warped).sum(axis=2), 1023)
    xs = np.broadcast_to(np.arange(W, dtype=F)[None, :], (H, W))
    ys = np.broadcast_to(np.arange(H, dtype=F)[:, None], (H, W))
    hx = ((xs + (a * F(t)).astype(F)).astype(F) + F(0.5)).astype(F)
    hy = ((ys + (b * F(t)).astype(F)).astype(F) + F(0.5)).astype(F)
    lands = known & (hx >= 0) & (hx < F(W)) & (hy >= 0) & (hy < F(H))
    qx = np.floor(np.where(lands, hx, F(0))).astype(np.int64)
    qy = np.floor(np.where(lands, hy, F(0))).astype(np.int64)
    index = np.arange(W * H, dtype=np.uint64).reshape(H, W)
    key = (cost.astype(np.uint64) << np.uint64(32)) | index
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = np.full(W * H, empty, np.uint64)
    np.minimum.at(keys, (qy * W + qx)[lands], key[lands])
    have = keys != empty
    src = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    src[~have] = 0
    ut = np.where(have, u.ravel()[src], F(0)).reshape(H, W)
    vt = np.where(have, v.ravel()[src], F(0)).reshape(H, W)
    counters = dict(holes=int((~have).sum()), collisions=int(lands.sum()) - int(have.sum()), left=int((known & ~lands).sum()), unknown=int((~known).sum()))
    return ut, vt, have.reshape(H, W).astype(np.uint8), counters


def restate_fill(ut, vt, state, radius, min_votes):
    """One pass of hs_median_rule.h in FILL mode: a hole with at least min_votes valid neighbours in its clipped window takes
    the lower median of their keys, u and v on their own."""
    H, W = ut.shape
    valid = (state != 0) & known_of(ut, vt)

    def keys_of(x):
        bits = x.view(np.uint32).astype(np.uint64)
        return np.where(bits >> np.uint64(31) != 0, bits ^ np.uint64(0xFFFFFFFF), bits ^ np.uint64(0x80000000))

    def back(k):
        k = k.astype(np.uint64)
        return np.where(k >> np.uint64(31) != 0, k ^ np.uint64(0x80000000), k ^ np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32)
    big = np.uint64(1) << np.uint64(40)
    pads = [np.pad(np.where(valid, keys_of(x), big), radius, constant_values=big) for x in (ut, vt)]
    stack = [np.sort(np.stack([p[dy:dy + H, dx:dx + W] for dy in range(2 * radius + 1) for dx in range(2 * radius + 1)]), axis=0) for p in pads]
    n = (stack[0] != big).sum(axis=0)
    rank = np.maximum(n - 1, 0) >> 1
    fill = (state == 0) & (n >= min_votes)
    med = [np.take_along_axis(s, rank[None], axis=0)[0] for s in stack]
    uo = np.where(fill, back(np.where(fill, med[0], 0)), ut)
    vo = np.where(fill, back(np.where(fill, med[1], 0)), vt)
    return uo, vo, np.where(fill, 2, state).astype(np.uint8)


def restate_blend(ut, vt, prev, curr, t, vis_prev=None, vis_curr=None, f=F):
    """B: (picture, class plane)."""
    H, W, _ = prev.shape
    wA = f(F(1.0) - F(t)) if f is F else f(1.0) - f(F(t))
    wB = f(F(t))
    sides = []
    for pic, vis, frac in ((prev, vis_prev, -f(F(t))), (curr, vis_curr, wA)):
        inside, x0, x1, y0, y1, ax, ay = locate(ut, vt, frac, W, H, True, f)
        val = bilinear(pic, x0, x1, y0, y1, ax, ay, f)
        occ = np.zeros((H, W), bool)
        if vis is not None:
            occ = vis[np.where(ay >= 0.5, y1, y0), np.where(ax >= 0.5, x1, x0)] == 0
        sides.append((inside, val, occ))
    (inA, fa, occA), (inB, fb, occB) = sides
    both = inA & inB
    cls = np.where(both, np.where(occA & ~occB, 1, np.where(occB & ~occA, 2, 0)), np.where(inA, 1, np.where(inB, 2, 3)))
    mix = ((wA * fa).astype(f) + (wB * fb).astype(f)).astype(f)
    m = np.where((cls == 1)[..., None], fa, np.where((cls == 2)[..., None], fb, mix))
    return to_byte(m, f).astype(np.uint8), cls.astype(np.uint8)


def restate(u, v, prev, curr, t, passes=4, radius=1, min_votes=1, vis_prev=None, vis_curr=None):
    ut, vt, state, counters = restate_project(u, v, prev, curr, t)
    for _ in range(passes):
        ut, vt, state = restate_fill(ut, vt, state, radius, min_votes)
    counters["unfilled"] = int((state == 0).sum())
    pic, cls = restate_blend(ut, vt, prev, curr, t, vis_prev, vis_curr)
    return ut, vt, state, counters, pic, cls


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def padded(rng, shape, dtype, pad):
    """A random array of `shape` as a view into rows that are `pad` elements longer, and the whole buffer."""
    H, rest = shape[0], int(np.prod(shape[1:]))
    whole = rng.integers(0, 256, (H, rest + pad), dtype=np.uint8) if dtype == np.uint8 else np.zeros((H, rest + pad), dtype)
    return whole[:, :rest].reshape(shape), whole


def gaussian_flow(rng, W, H, sigma=6.0, pad=0):
    u, _ = padded(rng, (H, W), np.float32, pad)
    v, _ = padded(rng, (H, W), np.float32, pad)
    u[...] = rng.standard_normal((H, W)) * sigma
    v[...] = rng.standard_normal((H, W)) * sigma
    return u, v


def smooth_picture(rng, W, H, C):
    """A picture with structure, so that the costs differ and collisions are decided by them."""
    ys, xs = np.mgrid[0:H, 0:W]
    base = 128 + 60 * np.sin(xs / 5.0) + 50 * np.cos(ys / 3.0)
    pic = base[..., None] + rng.integers(-20, 21, (H, W, C))
    return np.clip(pic, 0, 255).astype(np.uint8)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------

def test_version(hs):
    assert hs._lib.load().hsflow_version() >= 20
    text = open(os.path.join(ROOT, "include", "hsflow.h")).read()
    assert int(re.search(r"#define HSFLOW_VERSION_MINOR (\d+)", text).group(1)) >= 20


def test_struct_sizes_and_defaults(hs):
    assert ctypes.sizeof(hs.HsflowInterpStats) == 64
    assert ctypes.sizeof(hs.HsflowInterpParams) == 20
    ip = hs.HsflowInterpParams()
    ctypes.memset(ctypes.byref(ip), 0xff, ctypes.sizeof(ip))
    hs._lib.load().hsflow_default_interp_params(ctypes.byref(ip))
    assert (ip.struct_size, ip.channels, ip.fill_radius, ip.fill_min_votes, ip.fill_passes) == (20, 1, 1, 1, 4)
    hs._lib.load().hsflow_default_interp_params(None)  # (ignored)
    assert (hs.INTERP_BLENDED, hs.INTERP_PREV_ONLY, hs.INTERP_CURR_ONLY, hs.INTERP_CLAMPED, hs.INTERP_BATCH_MAX) == (0, 1, 2, 3, 8)


def call(hs, u, v, t, ip, prev, curr, vp, vc, ref, dst, cls, stats, width=None, height=None, strides=None):
    """hsflow_interp_host with raw arguments; strides: (u, v, prev, curr, vis_prev, vis_curr, ref, dst, cls) in bytes."""
    H, W = (height, width) if u is None else u.shape[:2]
    arrays = (u, v, prev, curr, vp, vc, ref, dst, cls)
    st = strides or tuple(x.strides[0] if x is not None else 0 for x in arrays)
    p = lambda x: ctypes.c_void_p(x.ctypes.data) if x is not None else None
    return hs._lib.load().hsflow_interp_host(p(u), st[0], p(v), st[1], W if width is None else width, H if height is None else height, t,
                                             ctypes.byref(ip) if ip is not None else None, p(prev), st[2], p(curr), st[3], p(vp), st[4], p(vc), st[5],
                                             p(ref), st[6], p(dst), st[7], p(cls), st[8], ctypes.byref(stats) if stats is not None else None)


def test_argument_errors(hs):
    from opticalflowhs_amd._lib import E_ARG, E_SIZE, OK
    W, H = 6, 4
    u = np.zeros((H, W), np.float32)
    prev = np.zeros((H, W, 3), np.uint8)
    curr = np.zeros((H, W, 3), np.uint8)
    ref = np.zeros((H, W, 3), np.uint8)
    dst = np.zeros((H, W, 3), np.uint8)
    vis = np.ones((H, W), np.uint8)
    vis2 = np.ones((H, W), np.uint8)
    cls = np.zeros((H, W), np.uint8)
    good = lambda **kw: hs.make_interp_params(channels=3, **kw)
    stats = hs.HsflowInterpStats()
    assert call(hs, u, u, 0.5, good(), prev, curr, vis, vis2, ref, dst, cls, stats) == OK
    full = (W * 4, W * 4, W * 3, W * 3, W, W, W * 3, W * 3, W)
    for k in range(4):  # a null flow plane or frame
        args = [u, u, prev, curr]
        args[k] = None
        assert call(hs, args[0], args[1], 0.5, good(), args[2], args[3], None, None, None, dst, None, None, width=W, height=H, strides=full) == E_ARG
    assert call(hs, u, u, 0.5, None, prev, curr, None, None, None, dst, None, None) == E_ARG
    assert call(hs, u, u, 0.5, good(), prev, curr, None, None, None, None, None, None) == E_ARG  # nothing asked for
    assert call(hs, u, u, 0.5, good(), prev, curr, None, None, None, prev, None, None) == E_ARG  # onto an input
    assert call(hs, u, u, 0.5, good(), prev, curr, None, None, None, curr, None, None) == E_ARG
    assert call(hs, u, u, 0.5, good(), prev, curr, None, None, ref, ref, None, None) == E_ARG
    assert call(hs, u, u, 0.5, good(), prev, curr, vis, None, None, None, vis, None) == E_ARG
    bad = good()
    bad.struct_size -= 4
    assert call(hs, u, u, 0.5, bad, prev, curr, None, None, None, dst, None, None) == E_ARG
    for field, values in (("channels", (0, 2, 4, -1)), ("fill_radius", (0, 3, -1)), ("fill_min_votes", (0, 10, -1)), ("fill_passes", (-1, 65))):
        for x in values:
            bad = good()
            setattr(bad, field, x)
            assert call(hs, u, u, 0.5, bad, prev, curr, None, None, None, dst, None, None) == E_ARG, (field, x)
    assert call(hs, u, u, 0.5, good(fill_radius=2, fill_min_votes=25, fill_passes=64), prev, curr, None, None, None, dst, None, None) == OK
    assert call(hs, u, u, 0.5, good(fill_passes=0), prev, curr, None, None, None, dst, None, None) == OK
    for t in (float("nan"), float("inf"), -float("inf"), -1e-6, 1.000001):
        assert call(hs, u, u, t, good(), prev, curr, None, None, None, dst, None, None) == E_ARG
    for t in (0.0, 1.0):
        assert call(hs, u, u, t, good(), prev, curr, None, None, None, dst, None, None) == OK
    for k in range(9):
        short = list(full)
        short[k] -= 4 if k < 2 else 1
        assert call(hs, u, u, 0.5, good(), prev, curr, vis, vis2, ref, dst, cls, stats, strides=tuple(short)) == E_SIZE, k
    assert call(hs, u, u, 0.5, good(), prev, curr, None, None, None, dst, None, None, strides=(W * 4 + 2, W * 4, W * 3, W * 3, 0, 0, 0, W * 3, 0)) == E_SIZE
    assert call(hs, u, u, 0.5, good(), prev, curr, None, None, None, dst, None, None, width=0) == E_SIZE
    assert call(hs, u, u, 0.5, good(), prev, curr, None, None, None, dst, None, None, height=-1) == E_SIZE
    # the projection alone
    L = hs._lib.load()
    p = lambda x: ctypes.c_void_p(x.ctypes.data) if x is not None else None
    uo, vo, so = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32), np.zeros((H, W), np.uint8)
    proj = lambda a, b, s, rec, os_=W * 4, sos=W, t=1.0, ip=good(): L.hsflow_project_flow_host(
        p(u), W * 4, p(u), W * 4, W, H, t, ctypes.byref(ip), p(prev), W * 3, p(curr), W * 3, p(a), p(b), os_, p(s), sos, ctypes.byref(rec) if rec else None)
    assert proj(uo, vo, so, stats) == OK
    assert proj(None, None, None, None) == E_ARG      # nothing asked for
    assert proj(uo, None, None, None) == E_ARG        # one plane of the two
    assert proj(u, vo, None, None) == E_ARG           # onto the input
    assert proj(uo, vo, None, None, t=1.5) == E_ARG
    assert proj(uo, vo, None, None, os_=W * 4 - 4) == E_SIZE
    assert proj(uo, vo, None, None, os_=W * 4 + 2) == E_SIZE
    assert proj(None, None, so, None, sos=W - 1) == E_SIZE
    assert proj(None, None, so, None) == OK and proj(None, None, None, stats) == OK


# ---- the rule, bit for bit --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("W,H", SHAPES)
def test_rule_against_fp32_restatement(hs, W, H, channels):
    """Projected planes, state, class plane, picture and every counter, with padded strides everywhere, t in {0, 0.25, 0.5,
    1}, with and without vis planes, fill_passes in {0, 1, 4}, a Gaussian flow of sigma 6."""
    rng = np.random.default_rng(1000 * W + channels)
    u, v = gaussian_flow(rng, W, H, pad=3)
    prev, _ = padded(rng, (H, W, channels), np.uint8, 5)
    curr, _ = padded(rng, (H, W, channels), np.uint8, 2)
    prev[...] = smooth_picture(rng, W, H, channels)
    curr[...] = smooth_picture(rng, W, H, channels)
    ref, _ = padded(rng, (H, W, channels), np.uint8, 1)
    vis = [padded(rng, (H, W), np.uint8, 3)[0] for _ in range(2)]
    for x in vis:
        x[...] = (rng.random((H, W)) < 0.8) * 255
    seen = dict(holes=0, collisions=0, left=0)
    for t in (0.0, 0.25, 0.5, 1.0):
        for passes, radius, votes, with_vis in ((0, 1, 1, False), (1, 2, 3, True), (4, 1, 1, True), (4, 1, 1, False)):
            ip = hs.make_interp_params(channels, radius, votes, passes)
            vp, vc = (vis[0], vis[1]) if with_vis else (None, None)
            dst, whole = padded(rng, (H, W, channels), np.uint8, 4)
            cls, cwhole = padded(rng, (H, W), np.uint8, 6)
            before, cbefore = whole.copy(), cwhole.copy()
            out, classes, s = hs.interp_host(u, v, prev, curr, t=t, vis_prev=vp, vis_curr=vc, ref=ref, out=dst, classes=cls, stats=True, params=ip)
            ut, vt, state, want, pic, kinds = restate(u, v, prev, curr, t, passes, radius, votes, vp, vc)
            tag = (t, passes, with_vis)
            assert np.array_equal(dst, pic), (tag, int((dst != pic).sum()))
            assert np.array_equal(cls, kinds), tag
            assert np.array_equal(whole[:, W * channels:], before[:, W * channels:]) and np.array_equal(cwhole[:, W:], cbefore[:, W:])  # beyond the rows: untouched
            assert [s.blended, s.prev_only, s.curr_only, s.clamped] == [int((kinds == k).sum()) for k in range(4)], tag
            d = np.abs(pic.astype(np.int64) - ref.astype(np.int64))
            assert (s.sad, s.max_diff) == (int(d.sum()), int(d.max())), tag
            assert dict(holes=s.holes, collisions=s.collisions, left=s.left, unknown=s.unknown, unfilled=s.unfilled) == want, tag
            # the identities of the counters
            assert s.blended + s.prev_only + s.curr_only + s.clamped == W * H
            landed = W * H - s.left - s.unknown
            assert s.collisions == landed - (W * H - s.holes)
            # the projection alone: the same planes, padded outputs
            uo, uwhole = padded(rng, (H, W), np.float32, 2)
            vo, _ = padded(rng, (H, W), np.float32, 2)
            so, swhole = padded(rng, (H, W), np.uint8, 3)
            uwhole[:, W:] = 7.0
            sbefore = swhole.copy()
            _, _, _, ps = hs.project_flow_host(u, v, prev, curr, t=t, flow=(uo, vo), state=so, stats=True, params=ip)
            assert np.array_equal(bits(uo), bits(ut)) and np.array_equal(bits(vo), bits(vt)) and np.array_equal(so, state), tag
            assert np.all(uwhole[:, W:] == 7.0) and np.array_equal(swhole[:, W:], sbefore[:, W:])
            assert (ps.holes, ps.unfilled, ps.collisions, ps.left, ps.unknown) == (s.holes, s.unfilled, s.collisions, s.left, s.unknown)
            assert (ps.blended, ps.prev_only, ps.curr_only, ps.clamped, ps.sad, ps.max_diff) == (0, 0, 0, 0, 0, 0)
            assert int((so == 1).sum()) + ps.holes == W * H and int((so == 0).sum()) == ps.unfilled
            for k in seen:
                seen[k] += getattr(s, k)
    assert all(seen.values()), seen  # collisions, holes and `left` all occur


@pytest.mark.parametrize("channels", [1, 3])
def test_end_points_give_the_frames(hs, channels):
    """t = 0 gives prev and t = 1 gives curr byte for byte, for a random flow with NaN, Inf and +-1e9 in it."""
    W, H = 31, 17
    rng = np.random.default_rng(5)
    prev = rng.integers(0, 256, (H, W, channels), dtype=np.uint8)
    curr = rng.integers(0, 256, (H, W, channels), dtype=np.uint8)
    u, v = gaussian_flow(rng, W, H, sigma=9.0)
    u[3, 4], v[5, 6], u[7, 8], v[9, 10], u[11, 12], v[2, 2] = np.nan, np.inf, -np.inf, 1e9, -1e9, NEXT_ABOVE_1E9
    for passes in (0, 4):
        ip = hs.make_interp_params(channels, fill_passes=passes)
        first, _, s0 = hs.interp_host(u, v, prev, curr, t=0.0, ref=prev, stats=True, params=ip)
        last, _, s1 = hs.interp_host(u, v, prev, curr, t=1.0, ref=curr, stats=True, params=ip)
        assert np.array_equal(first, prev) and np.array_equal(last, curr)
        assert s0.sad == 0 and s1.sad == 0 and s0.unknown == 4 and s1.unknown == 4
        assert s0.left == 0 and s0.holes == 4 and s0.collisions == 0  # at t = 0 every known source stays where it is
        assert s1.left >= 2                                            # the +-1e9 components leave at t = 1


def test_whole_number_flow(hs):
    """A constant whole-number flow (dx, dy) with t dx and t dy whole: in the interior the exact mix of the shifted pictures."""
    W, H = 40, 24
    rng = np.random.default_rng(8)
    prev = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    curr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    dx, dy, t = 4, -2, 0.5
    u = np.full((H, W), dx, np.float32)
    v = np.full((H, W), dy, np.float32)
    out, cls, s = hs.interp_host(u, v, prev, curr, t=t, classes=True, stats=True)
    ax, ay = int(t * dx), int(t * dy)      # the output pixel (x, y) comes from prev (x - 2, y + 1) and curr (x + 2, y - 1)
    ys, xs = slice(1, H - 1), slice(2, W - 2)
    a = prev[1 + 1:H - 1 + 1, 2 - 2:W - 2 - 2].astype(np.float32)
    b = curr[1 - 1:H - 1 - 1, 2 + 2:W - 2 + 2].astype(np.float32)
    assert (ax, ay) == (2, -1)
    want = np.minimum((F(0.5) * a + F(0.5) * b + F(0.5)).astype(np.int64), 255)
    assert np.array_equal(out[ys, xs], want) and np.all(cls[ys, xs] == hs.INTERP_BLENDED)
    assert s.collisions == 0 and s.left == W * H - (W - 2) * (H - 1) and s.unfilled == 0


def test_collisions_are_decided_by_cost_then_index(hs):
    W, H = 8, 3
    prev = np.zeros((H, W, 1), np.uint8)
    curr = np.zeros((H, W, 1), np.uint8)
    u = np.zeros((H, W), np.float32)
    v = np.zeros((H, W), np.float32)
    # sources (1, 1) and (5, 1) both land on (3, 1) at t = 1: flows +2 and -2
    u[1, 1], u[1, 5] = 2.0, -2.0
    prev[1, 1], prev[1, 5] = 100, 100
    curr[1, 3] = 100                          # equal cost (0 both): the lower index, (1, 1), wins
    ip = hs.make_interp_params(1, fill_passes=0)
    ut, vt, state, s = hs.project_flow_host(u, v, prev, curr, t=1.0, state=True, stats=True, params=ip)
    assert ut[1, 3] == 2.0 and state[1, 3] == 1
    # the pixel (3, 1) itself, flow 0, lands there too: prev 0 against curr 100, cost 100 -- it loses to both
    assert s.collisions == 2 and s.holes == 2 and state[1, 1] == 0 and state[1, 5] == 0
    prev[1, 1] = 90                           # now (1, 1) costs 10 and (5, 1) costs 0: the cost decides against the index
    ut, _, _, _ = hs.project_flow_host(u, v, prev, curr, t=1.0, params=ip)
    assert ut[1, 3] == -2.0
    prev[1, 1], prev[1, 5] = 100, 80          # and the other way round
    ut, _, _, _ = hs.project_flow_host(u, v, prev, curr, t=1.0, params=ip)
    assert ut[1, 3] == 2.0
    u[1, 5] = -200.0                          # taps outside at t = 1: cost 1023, loses to anything; and it leaves the frame
    ut, _, _, s = hs.project_flow_host(u, v, prev, curr, t=1.0, stats=True, params=ip)
    assert ut[1, 3] == 2.0 and s.left == 1
    ut, _, _, s = hs.project_flow_host(u, v, prev, curr, t=0.01, stats=True, params=ip)  # (5 - 2 + 0.5 = 3.5: lands on 3, cost 1023)
    assert s.left == 0 and ut[1, 3] == 0.0    # the cell's own source (cost 100) beats 1023


@pytest.mark.parametrize("radius", [1, 2])
def test_hole_depth_and_passes(hs, radius):
    """A hole at Chebyshev depth d is filled in pass ceil(d / r)."""
    W, H = 21, 21
    prev = np.zeros((H, W, 1), np.uint8)
    u = np.zeros((H, W), np.float32)
    v = np.zeros((H, W), np.float32)
    # the 9 x 9 block in the middle leaves the frame: at t = 1 it is a hole whose centre has depth 5
    u[6:15, 6:15] = 1e9
    depth = np.zeros((H, W), int)
    for y in range(6, 15):
        for x in range(6, 15):
            depth[y, x] = min(x - 5, 15 - x, y - 5, 15 - y)
    for passes in range(0, 7):
        ip = hs.make_interp_params(1, radius, 1, passes)
        _, _, state, s = hs.project_flow_host(u, v, prev, prev, t=1.0, state=True, stats=True, params=ip)
        filled_by = -(-depth // radius)  # ceil
        want = np.where(depth == 0, 1, np.where(filled_by <= passes, 2, 0))
        assert np.array_equal(state, want), passes
        assert (s.holes, s.left, s.unfilled, s.collisions) == (81, 81, int((want == 0).sum()), 0)


def test_extreme_components_leave_without_overflow(hs):
    W, H = 9, 5
    rng = np.random.default_rng(2)
    prev = rng.integers(0, 256, (H, W, 1), dtype=np.uint8)
    u = np.zeros((H, W), np.float32)
    v = np.zeros((H, W), np.float32)
    u[0, 0], u[1, 1], v[2, 2], v[3, 3] = 1e9, -1e9, 1e9, -1e9
    u[4, 4] = NEXT_ABOVE_1E9
    for t in (1.0, 0.5, 1e-3):
        _, _, state, s = hs.project_flow_host(u, v, prev, prev, t=t, state=True, stats=True, params=hs.make_interp_params(1, fill_passes=0))
        assert (s.left, s.unknown, s.holes, s.collisions) == (4, 1, 5, 0)
        assert [state[k, k] for k in range(5)] == [0] * 5 and int(state.sum()) == W * H - 5
    _, _, _, s = hs.project_flow_host(u, v, prev, prev, t=0.0, stats=True)
    assert (s.left, s.unknown, s.holes) == (0, 1, 1)


def test_blend_against_float64(hs):
    """Step B alone, from a given flow at t and without vis planes, against the same formula in float64: every byte within
    one level."""
    W, H = 260, 37
    differing = worst = 0
    for seed in range(10):
        rng = np.random.default_rng(seed)
        u, v = gaussian_flow(rng, W, H)
        prev = rng.integers(0, 256, (H, W, 1), dtype=np.uint8)
        curr = rng.integers(0, 256, (H, W, 1), dtype=np.uint8)
        t = (0.25, 0.5, 0.75, 0.3)[seed % 4]
        ut, vt, _, _ = hs.project_flow_host(u, v, prev, curr, t=t)
        got, _, _ = hs.interp_host(u, v, prev, curr, t=t)
        want, _ = restate_blend(ut, vt, prev, curr, t, f=np.float64)
        d = np.abs(got.astype(int) - want.astype(int))
        differing += int((d != 0).sum())
        worst = max(worst, int(d.max()))
    print("bytes that differ from float64: %d of %d, by at most %d" % (differing, 10 * W * H, worst))
    assert worst <= 1


def test_stats_modes(hs):
    W, H = 40, 12
    rng = np.random.default_rng(3)
    u, v = gaussian_flow(rng, W, H, sigma=2.0)
    prev = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    curr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    ref = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    out, _, with_ref = hs.interp_host(u, v, prev, curr, ref=ref, stats=True)
    _, _, without = hs.interp_host(u, v, prev, curr, stats=True)
    assert (without.sad, without.max_diff) == (0, 0) and with_ref.sad > 0
    assert bytes(without)[:32] == bytes(with_ref)[:32] and bytes(without)[40:60] == bytes(with_ref)[40:60]
    none, kinds, only = hs.interp_host(u, v, prev, curr, ref=ref, out=False, classes=True, stats=True)
    assert none is None and bytes(only) == bytes(with_ref)
    pic, none, rec = hs.interp_host(u, v, prev, curr)
    assert np.array_equal(pic, out) and none is None and rec is None


@pytest.mark.parametrize("W,H", [(96, 64), (260, 37)])
def test_physical_sense(hs, W, H):
    """With the oracle's flow of a translating pair the interpolated frame is closer to the true frame at t than the
    cross-fade (the rule's own blend with zero flow): 3 sad_interp < 2 sad_crossfade for t in {0.25, 0.5, 0.75}."""
    from oracle import hs_numpy
    from opticalflowhs_amd.synth import translating_pair
    prev, curr = translating_pair(W, H, seed=1, dx=2.0, dy=-1.5)
    u, v = hs_numpy.calc_optical_flow_hs(prev, curr, 0.1, 100, term_type=hs_numpy.TERMCRIT_ITER)
    zero = np.zeros_like(u)
    for t in (0.25, 0.5, 0.75):
        true = translating_pair(W, H, seed=1, dx=2.0 * t, dy=-1.5 * t)[1]
        _, _, interp = hs.interp_host(u, v, prev, curr, t=t, ref=true, stats=True)
        fade, _, cross = hs.interp_host(zero, zero, prev, curr, t=t, ref=true, stats=True)
        print("%dx%d t=%.2f: interp %d, cross-fade %d, ratio %.3f" % (W, H, t, interp.sad, cross.sad, interp.sad / cross.sad))
        assert 3 * interp.sad < 2 * cross.sad
        w = np.float32(t)
        mix = (np.float32(1) - w) * prev.astype(np.float32) + w * curr.astype(np.float32)
        assert np.array_equal(fade, np.minimum((mix + np.float32(0.5)).astype(np.int64), 255))


# ---- the rule as a stand-alone program under the sanitizers ----------------------------------------------------------------

SANITIZER_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "hs_interp_rule.h"
#include "hs_median_rule.h"

template <int C> static void run(float t, int passes, bool with_vis)
{
    const int W = 5, H = 3;
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float big = std::nextafterf(1e9f, inf);
    const float us[15] = {nan, 0.f, 0.f, -inf, -4.f, 1e9f, 0.f, 2.f, 3e38f, std::nextafterf(-4.f, -5.f), big, 0.f, -0.f, 1.000001f, -1e9f};
    const float vs[15] = {0.f, 2.f, inf, 0.f, 0.f, 0.f, -1e9f, 0.f, -3e38f, 0.f, 0.f, -big, -0.f, 0.f, 1e9f};
    // exact-size heap blocks: a tap or a cell beyond a plane is a finding
    std::vector<float> u(us, us + 15), v(vs, vs + 15);
    std::vector<uint8_t> prev(W * H * C), curr(W * H * C), ref(W * H * C), dst(W * H * C), cls(W * H), vp(W * H), vc(W * H);
    for (size_t k = 0; k < prev.size(); k++) { prev[k] = (uint8_t)(17 * k + 3); curr[k] = (uint8_t)(29 * k + 11); ref[k] = (uint8_t)(255 - 5 * k); }
    for (int k = 0; k < W * H; k++) { vp[k] = (uint8_t)(k % 3 ? 255 : 0); vc[k] = (uint8_t)(k % 4 ? 1 : 0); }
    std::vector<uint64_t> keys(W * H);
    std::vector<float> fu[2] = {std::vector<float>(W * H), std::vector<float>(W * H)}, fv[2] = {std::vector<float>(W * H), std::vector<float>(W * H)};
    std::vector<uint8_t> fs[2] = {std::vector<uint8_t>(W * H), std::vector<uint8_t>(W * H)};
    hsinterp::Sums s = {};
    hsinterp::project_rows<C>(u.data(), W * 4, v.data(), W * 4, W, H, t, prev.data(), W * C, curr.data(), W * C, keys.data(), fu[0].data(), fv[0].data(),
                              fs[0].data(), &s);
    for (int j = 1; j <= passes; j++) {
        const int a = (j - 1) & 1, b = j & 1;
        hsmed::Sums ms = {0, 0, 0, 0, 0};
        hsmed::median_rows(1, fu[a].data(), W * 4, fv[a].data(), W * 4, fs[a].data(), W, W, H, 1, 1, fu[b].data(), fv[b].data(), W * 4, fs[b].data(), W, &ms);
        s.unfilled = (uint32_t)ms.unfilled;
    }
    const int k = passes & 1;
    hsinterp::blend_rows<C>(fu[k].data(), fv[k].data(), W, H, t, prev.data(), W * C, curr.data(), W * C, with_vis ? vp.data() : nullptr, W,
                            with_vis ? vc.data() : nullptr, W, ref.data(), W * C, dst.data(), W * C, cls.data(), W, &s);
    std::printf("%d %g %d %d", C, (double)t, passes, (int)with_vis);
    for (uint8_t b : dst) std::printf(" %u", (unsigned)b);
    std::printf(" |");
    for (uint8_t b : cls) std::printf(" %u", (unsigned)b);
    std::printf(" |");
    for (uint8_t b : fs[k]) std::printf(" %u", (unsigned)b);
    std::printf(" | %llu %llu %llu %llu %llu %u %u %u %u %u %u\n", (unsigned long long)s.blended, (unsigned long long)s.prev_only, (unsigned long long)s.curr_only,
                (unsigned long long)s.clamped, (unsigned long long)s.sad, s.holes, s.unfilled, s.collisions, s.left, s.unknown, s.max_diff);
}

int main()
{
    const float ts[] = {0.f, 0.25f, 0.5f, 1.f};
    for (float t : ts)
        for (int passes = 0; passes < 3; passes++)
            for (int vis = 0; vis < 2; vis++) { run<1>(t, passes, vis != 0); run<3>(t, passes, vis != 0); }
    return 0;
}
"""


def test_rule_under_sanitizers(hs, tmp_path):
    """The host rule as a stand-alone program under AddressSanitizer and UBSan: special values and extreme flows on a 5x3
    picture in exact-size heap blocks; its bytes, planes and sums are the library's."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    main = tmp_path / "interp_rule_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = str(tmp_path / "interp_rule")
    base = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program where the compiler has them as archives: the program then starts whatever the
    # environment it inherits preloads; the environment itself is left as it is
    for flags in (base + ["-static-libasan", "-static-libubsan"], base):
        if subprocess.run([gxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True).returncode == 0:
            break
    else:
        pytest.skip("the sanitizer runtimes do not link here")
    if subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, timeout=60).returncode != 0:
        pytest.skip("a sanitized program does not start in this environment (the runtime's link-order check)")
    r = subprocess.run([gxx] + flags + ["-Wall", "-Wextra", "-I", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), str(main), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 48
    W, H = 5, 3
    inf, nan, big = np.float32(np.inf), np.float32(np.nan), NEXT_ABOVE_1E9
    u = np.array([nan, 0, 0, -inf, -4, 1e9, 0, 2, 3e38, np.nextafter(np.float32(-4), np.float32(-5)), big, 0, -0.0,
                  1.000001, -1e9], np.float32).reshape(H, W)
    v = np.array([0, 2, inf, 0, 0, 0, -1e9, 0, -3e38, 0, 0, -big, -0.0, 0, 1e9], np.float32).reshape(H, W)
    n = np.arange(W * H)
    vp = np.where(n % 3, 255, 0).astype(np.uint8).reshape(H, W)
    vc = np.where(n % 4, 1, 0).astype(np.uint8).reshape(H, W)
    for line in lines:
        head, kinds, states, tail = line.split(" |")
        words = head.split()
        C, t, passes, with_vis = int(words[0]), float(words[1]), int(words[2]), int(words[3])
        k = np.arange(W * H * C)
        prev = ((17 * k + 3) % 256).astype(np.uint8).reshape(H, W, C)
        curr = ((29 * k + 11) % 256).astype(np.uint8).reshape(H, W, C)
        ref = ((255 - 5 * k) % 256).astype(np.uint8).reshape(H, W, C)
        ip = hs.make_interp_params(C, fill_passes=passes)
        out, cls, s = hs.interp_host(u, v, prev, curr, t=t, vis_prev=vp if with_vis else None, vis_curr=vc if with_vis else None, ref=ref, classes=True,
                                     stats=True, params=ip)
        _, _, state, _ = hs.project_flow_host(u, v, prev, curr, t=t, flow=False, state=True, params=ip)
        assert [int(x) for x in words[4:]] == out.ravel().tolist(), line
        assert [int(x) for x in kinds.split()] == cls.ravel().tolist(), line
        assert [int(x) for x in states.split()] == state.ravel().tolist(), line
        assert [int(x) for x in tail.split()] == [s.blended, s.prev_only, s.curr_only, s.clamped, s.sad, s.holes, s.unfilled, s.collisions, s.left,
                                                  s.unknown, s.max_diff], line
