"""hsflow_median_host: the rule of csrc/hs_median_rule.h on the host -- the median filter and the hole filling of a flow
field, the output state and exact integer statistics.  No GPU work: the device side is held to these bits by
tests/test_gpu_median.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SHAPES = [(1, 1), (3, 2), (13, 7), (260, 37), (96, 64)]  # (W, H)
OK, E_ARG, E_SIZE = 0, 1, 2
BIG = np.nextafter(np.float32(1e9), np.float32(np.inf))
# (tests/test_gpu_warp.py's list)
SPECIAL = [(np.nan, 1.0), (1.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (BIG, 0.0), (0.0, -BIG), (1e9, 0.0), (0.0, -1e9), (0.0, 0.0), (-0.0, -0.0),
           (1e-42, -1e-42), (2.0, -0.0), (0.5, 0.5), (-1e9, 1e9)]
STAT_FIELDS = ("kept", "filled", "unfilled", "newly_filled", "changed")
GOLDEN = os.path.join(ROOT, "tests", "golden", "synth_256x128_s1_l1_i100.npz")


def known(a, b):
    with np.errstate(invalid="ignore"):
        return ~(np.isnan(a) | np.isnan(b) | (np.abs(a) > np.float32(1e9)) | (np.abs(b) > np.float32(1e9)))


def keys_of(plane):
    bits = np.ascontiguousarray(plane, np.float32).view(np.uint32)
    return bits ^ np.where(bits >> 31, np.uint32(0xffffffff), np.uint32(0x80000000))


def bits_of(keys):
    keys = keys.astype(np.uint32)
    return keys ^ np.where(keys >> 31, np.uint32(0x80000000), np.uint32(0xffffffff))


def restate(u, v, state=None, radius=1, mode="filter", min_votes=1):
    """One pass of the rule restated in NumPy: sort the voters' keys, take rank (n - 1) >> 1.  Returns (u bits, v bits,
    s_out, the five statistics, n)."""
    H, W = u.shape
    r = radius
    byte = np.full((H, W), 255, np.uint8) if state is None else np.asarray(state, np.uint8)
    s = np.where(~known(u, v) | (byte == 0), 0, np.where(byte == 2, 2, 1)).astype(np.uint8)
    far = np.uint64(1) << np.uint64(40)  # sorts behind every key
    meds = []
    valid = np.zeros((H + 2 * r, W + 2 * r), bool)
    valid[r:r + H, r:r + W] = s != 0
    for plane in (u, v):
        k = np.full((H + 2 * r, W + 2 * r), far, np.uint64)
        k[r:r + H, r:r + W] = np.where(s != 0, keys_of(plane).astype(np.uint64), far)
        stack = np.stack([k[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)])
        stack.sort(axis=0)
        meds.append(stack)
    n = np.sum([valid[dy:dy + H, dx:dx + W] for dy in range(2 * r + 1) for dx in range(2 * r + 1)], axis=0).astype(np.int64)
    rank = np.maximum((n - 1) >> 1, 0)[None]
    mu, mv = (bits_of(np.take_along_axis(m, rank, axis=0)[0] & np.uint64(0xffffffff)) for m in meds)
    ub, vb = np.ascontiguousarray(u, np.float32).view(np.uint32), np.ascontiguousarray(v, np.float32).view(np.uint32)
    enough = n >= min_votes
    take = enough & (s == 0) if mode == "fill" else enough
    uo, vo = np.where(take, mu, ub), np.where(take, mv, vb)
    so = np.where(take & (s == 0), 2, s).astype(np.uint8)
    stats = (int((so == 1).sum()), int((so == 2).sum()), int((so == 0).sum()), int(((s == 0) & (so == 2)).sum()), int(((uo != ub) | (vo != vb)).sum()))
    return uo, vo, so, stats, n


def stat_tuple(s):
    return tuple(int(getattr(s, k)) for k in STAT_FIELDS)


def padded(shape, dtype, pad, fill=0):
    """An array of `shape` as a view into rows that are `pad` elements longer, and the whole buffer."""
    whole = np.full((shape[0], shape[1] + pad), fill, dtype)
    return whole[:, :shape[1]], whole


def field(W, H, seed, pad=0, special=True):
    """A smooth field plus Gaussian noise with outliers and the special values scattered in; a state plane of bytes 0, 1,
    2, 7 and 255 with a block of zeros.  Rows `pad` elements longer than W."""
    rng = np.random.default_rng(seed)
    u, v = (padded((H, W), np.float32, pad)[0] for _ in range(2))
    ys, xs = np.mgrid[0:H, 0:W]
    u[...] = np.sin(xs / 9.0) * 3 + rng.standard_normal((H, W)) * 0.5
    v[...] = np.cos(ys / 7.0) * 2 + rng.standard_normal((H, W)) * 0.5
    out = rng.random((H, W)) < 0.05
    u[out] = rng.uniform(-50, 50, int(out.sum())).astype(np.float32)
    q = rng.random((H, W)) < 0.1   # (ties: quantised values, both zeros among them)
    u[q] = np.round(u[q])
    v[q] = -np.round(v[q] * 0.25)
    if special:
        n = min(len(SPECIAL), max(1, W * H // 8))
        for k, (sa, sb) in zip(rng.permutation(W * H)[:n], SPECIAL):
            u[divmod(int(k), W)], v[divmod(int(k), W)] = sa, sb
    state = padded((H, W), np.uint8, pad)[0]
    state[...] = rng.choice(np.array([0, 1, 2, 7, 255], np.uint8), size=(H, W), p=[0.3, 0.2, 0.15, 0.05, 0.3])
    state[H // 3:H // 3 + 6, W // 4:W // 4 + 9] = 0
    return u, v, state


def call(hs, u, v, state, mp, passes, uo, vo, so, stats, width=None, height=None, strides=None, out_strides=None):
    """hsflow_median_host with raw arguments."""
    first = next(p for p in (u, v, uo, vo, so) if p is not None)
    H, W = first.shape
    p = lambda x: ctypes.c_void_p(x.ctypes.data) if x is not None else None
    st = strides or tuple(x.strides[0] if x is not None else 0 for x in (u, v, state))
    os_ = out_strides or ((uo if uo is not None else vo).strides[0] if (uo is not None or vo is not None) else 0, so.strides[0] if so is not None else 0)
    return hs._lib.load().hsflow_median_host(p(u), st[0], p(v), st[1], p(state), st[2], W if width is None else width, H if height is None else height,
                                             ctypes.byref(mp) if mp is not None else None, passes, p(uo), p(vo), os_[0], p(so), os_[1],
                                             ctypes.byref(stats) if stats is not None else None)


# ---- 1. version, sizes, defaults -----------------------------------------------------------------------------------

def test_version_sizes_and_defaults(hs, tmp_path):
    L = hs._lib.load()
    assert L.hsflow_version() >= 19
    text = open(os.path.join(ROOT, "include", "hsflow.h")).read()
    assert int(re.search(r"#define HSFLOW_VERSION_MINOR (\d+)", text).group(1)) >= 19
    assert ctypes.sizeof(hs.HsflowMedianParams) == 16 and ctypes.sizeof(hs.HsflowMedianStats) == 64
    mp = hs.HsflowMedianParams()
    ctypes.memset(ctypes.byref(mp), 0xff, ctypes.sizeof(mp))
    L.hsflow_default_median_params(ctypes.byref(mp))
    assert (mp.struct_size, mp.radius, mp.mode, mp.min_votes) == (16, 1, hs.MEDIAN_FILTER, 1)
    L.hsflow_default_median_params(None)  # (ignored)
    assert (hs.MEDIAN_FILTER, hs.MEDIAN_FILL, hs.MEDIAN_UNFILLED, hs.MEDIAN_KEPT, hs.MEDIAN_FILLED, hs.MEDIAN_MAX_PASSES) == (0, 1, 0, 1, 2, 64)
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    src = tmp_path / "median.c"
    src.write_text('#include <stddef.h>\n#include "hsflow.h"\n'
                   "typedef char a[sizeof(hsflow_median_stats) == 64 ? 1 : -1];\n"
                   "typedef char b[sizeof(hsflow_median_params) == 16 ? 1 : -1];\n"
                   "typedef char c[offsetof(hsflow_median_stats, changed) == 32 ? 1 : -1];\n"
                   "typedef char d[HSFLOW_MEDIAN_FILL == 1 && HSFLOW_MEDIAN_FILLED == 2 && HSFLOW_MEDIAN_MAX_PASSES == 64 ? 1 : -1];\n"
                   "static int (*p0)(const float *, size_t, const float *, size_t, const uint8_t *, size_t, int, int, const hsflow_median_params *, int, float *,"
                   " float *, size_t, uint8_t *, size_t, hsflow_median_stats *) = hsflow_median_host;\n"
                   "static int (*p1)(hsflow_ctx *, int, const hsflow_median_params *, int, const void *, size_t, void *, size_t, hsflow_median_stats *) = hsflow_median_apply;\n"
                   "int main(void) { return p0 && p1 ? 0 : 1; }\n")
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "median.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- 2. argument errors ----------------------------------------------------------------------------------------------

def test_argument_errors(hs):
    W, H = 6, 4
    u, v = np.zeros((H, W), np.float32), np.ones((H, W), np.float32)
    uo, vo = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
    state, so = np.ones((H, W), np.uint8), np.zeros((H, W), np.uint8)
    stats = hs.HsflowMedianStats()
    good = hs.make_median_params
    assert call(hs, u, v, state, good(), 1, uo, vo, so, stats) == OK
    assert call(hs, u, v, None, good(), 1, None, None, None, stats) == OK
    full = (W * 4, W * 4, W)
    assert call(hs, None, v, None, good(), 1, uo, vo, None, None, strides=full) == E_ARG
    assert call(hs, u, None, None, good(), 1, uo, vo, None, None, strides=full) == E_ARG
    assert call(hs, u, v, None, None, 1, uo, vo, None, None) == E_ARG
    bad = good()
    bad.struct_size -= 4
    assert call(hs, u, v, None, bad, 1, uo, vo, None, None) == E_ARG
    for radius in (0, 3, -1):
        bad = good()
        bad.radius = radius
        assert call(hs, u, v, None, bad, 1, uo, vo, None, None) == E_ARG
    for mode in (-1, 2):
        bad = good()
        bad.mode = mode
        assert call(hs, u, v, None, bad, 1, uo, vo, None, None) == E_ARG
    for radius, votes, want in ((1, 0, E_ARG), (1, 10, E_ARG), (1, 9, OK), (2, 25, OK), (2, 26, E_ARG), (2, -1, E_ARG)):
        assert call(hs, u, v, None, good(radius=radius, min_votes=votes), 1, uo, vo, None, None) == want
    for passes, want in ((0, E_ARG), (-1, E_ARG), (65, E_ARG), (64, OK)):
        assert call(hs, u, v, None, good(), passes, uo, vo, None, None) == want
    assert call(hs, u, v, None, good(), 1, None, None, None, None) == E_ARG      # nothing asked for
    assert call(hs, u, v, None, good(), 1, uo, None, None, None) == E_ARG        # one flow output without the other
    assert call(hs, u, v, None, good(), 1, None, vo, None, None) == E_ARG
    # an output that is, or overlaps, an input
    assert call(hs, u, v, None, good(), 1, u, vo, None, None) == E_ARG
    assert call(hs, u, v, None, good(), 1, uo, v, None, None) == E_ARG
    assert call(hs, u, v, None, good(), 1, v, u, None, None) == E_ARG
    assert call(hs, u, v, state, good(), 1, None, None, state, None) == E_ARG
    long_ = np.zeros((H + 1, W), np.float32)
    assert call(hs, long_[:H], v, None, good(), 1, long_[1:], vo, None, None) == E_ARG
    bytes_ = np.zeros((H + 1, W), np.uint8)
    assert call(hs, u, v, bytes_[1:], good(), 1, None, None, bytes_[:H], None) == E_ARG
    assert call(hs, u, v, None, good(), 1, uo, vo, None, None, width=0) == E_SIZE
    assert call(hs, u, v, None, good(), 1, uo, vo, None, None, height=-1) == E_SIZE
    for k in range(2):
        short, odd = list(full), list(full)
        short[k] -= 4
        odd[k] += 2
        assert call(hs, u, v, None, good(), 1, uo, vo, None, None, strides=tuple(short)) == E_SIZE
        assert call(hs, u, v, None, good(), 1, uo, vo, None, None, strides=tuple(odd)) == E_SIZE
    assert call(hs, u, v, state, good(), 1, uo, vo, None, None, strides=(W * 4, W * 4, W - 1)) == E_SIZE
    assert call(hs, u, v, None, good(), 1, uo, vo, None, None, out_strides=(W * 4 - 4, 0)) == E_SIZE
    assert call(hs, u, v, None, good(), 1, uo, vo, None, None, out_strides=(W * 4 + 2, 0)) == E_SIZE
    assert call(hs, u, v, None, good(), 1, None, None, so, None, out_strides=(0, W - 1)) == E_SIZE
    assert call(hs, u, v, None, good(), 1, None, None, None, stats, out_strides=(0, 0)) == OK  # (absent outputs: their strides are not looked at)
    with pytest.raises(ValueError):
        hs.make_median_params(mode="both")


# ---- 3. the rule against the restatement -------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SHAPES)
def test_rule_against_restatement(hs, W, H):
    """Flow bits (NaN patterns included), the output state and the five statistics; padded strides everywhere, with
    canaries behind every row."""
    u, v, state = field(W, H, 11 * W + H, pad=3)
    for radius in (1, 2):
        for mode in ("filter", "fill"):
            for votes in (1, 2, 5, (2 * radius + 1) ** 2):
                for st in (state, None):
                    wu, wv, ws, wstats, _ = restate(u, v, st, radius, mode, votes)
                    uo, uwhole = padded((H, W), np.float32, 2, -7.0)
                    vo, vwhole = padded((H, W), np.float32, 2, -7.0)
                    so, swhole = padded((H, W), np.uint8, 5, 0xA5)
                    ru, rv, rs, rec = hs.median_host(u, v, st, flow=(uo, vo), state_out=so, stats=True, radius=radius, mode=mode, min_votes=votes)
                    case = (radius, mode, votes, st is not None)
                    assert ru is uo and rv is vo and rs is so
                    assert np.array_equal(uo.view(np.uint32), wu) and np.array_equal(vo.view(np.uint32), wv), case
                    assert np.array_equal(so, ws), case
                    assert (uwhole[:, W:] == -7.0).all() and (vwhole[:, W:] == -7.0).all() and (swhole[:, W:] == 0xA5).all()  # beyond W: untouched
                    assert stat_tuple(rec) == wstats, case
                    assert sum(wstats[:3]) == W * H
                    assert bytes(rec)[40:] == b"\0" * 24
    if W * H >= 13 * 7:  # the restatement alone sees every state, both outcomes of a hole and a changed pixel
        _, _, ws, wstats, n = restate(u, v, state, 1, "fill", 5)
        print("%dx%d fill, 5 votes: kept / filled / unfilled / newly / changed = %r" % (W, H, wstats))
        assert all(x > 0 for x in wstats)


def test_each_output_alone(hs):
    u, v, state = field(13, 7, 5)
    wu, wv, ws, wstats, _ = restate(u, v, state, 2, "fill", 2)
    kw = dict(radius=2, mode="fill", min_votes=2)
    uo, vo, none, rec = hs.median_host(u, v, state, **kw)
    assert none is None and rec is None and np.array_equal(uo.view(np.uint32), wu) and np.array_equal(vo.view(np.uint32), wv)
    assert np.array_equal(hs.median_host(u, v, state, flow=False, state_out=True, **kw)[2], ws)
    assert stat_tuple(hs.median_host(u, v, state, flow=False, stats=True, **kw)[3]) == wstats


# ---- 4. pinned cases -------------------------------------------------------------------------------------------------------

def test_signed_zeros_and_the_lower_median(hs):
    u = np.array([[-0.0, 0.0]], np.float32)
    uo, vo, _, _ = hs.median_host(u, u[:, ::-1].copy())
    assert np.all(uo.view(np.uint32) == 0x80000000) and np.all(vo.view(np.uint32) == 0x80000000)   # -0.0 < +0.0, n = 2: the lower one
    u = np.array([[4.0, 1.0, 3.0, 2.0]], np.float32)                                                  # windows {4,1} {4,1,3} {1,3,2} {3,2}
    uo = hs.median_host(u, np.zeros_like(u))[0]
    assert uo.tolist() == [[1.0, 3.0, 2.0, 2.0]]
    # n = 4 of a 3x3 window at a corner: ranks 0..3, the lower median is rank 1
    u = np.array([[9.0, 2.0], [7.0, 5.0]], np.float32)
    assert np.all(hs.median_host(u, np.zeros_like(u))[0] == 5.0)


def test_corner_of_a_5x5_window_has_nine_voters(hs):
    W, H = 8, 6
    u = np.arange(W * H, dtype=np.float32).reshape(H, W)
    for votes, filtered in ((9, True), (10, False)):
        uo, _, _, rec = hs.median_host(u, u, stats=True, radius=2, min_votes=votes)
        # the corner's window is rows 0..2, columns 0..2: values 0,1,2,8,9,10,16,17,18 -> rank 4 is 9
        assert uo[0, 0] == (9.0 if filtered else 0.0)
        assert uo[H - 1, W - 1] == (u[H - 2, W - 2] if filtered else u[H - 1, W - 1])
    assert restate(u, u, None, 2)[4][0, 0] == 9


def test_the_limit_of_known_votes(hs):
    # 1e9 votes (and, as the largest of three, does not win); the next float above it does not vote: n drops to 2
    for top, want_n, want in ((1e9, 3, 2.0), (BIG, 2, 1.0)):
        u = np.array([[1.0, top, 2.0]], np.float32)
        v = np.zeros_like(u)
        uo, _, so, _ = hs.median_host(u, v, state_out=True)
        assert restate(u, v)[4][0, 1] == want_n
        assert uo[0, 0] == 1.0 and uo[0, 1] == np.float32(want)
        assert so[0, 1] == (1 if want_n == 3 else 2)  # FILTER fills an unknown pixel that has voters
    u = np.array([[1e9, 1e9, 5.0]], np.float32)
    assert hs.median_host(u, np.zeros_like(u))[0][0, 1] == np.float32(1e9)


def test_nan_is_copied_bit_for_bit_where_unfilled(hs):
    patterns = np.array([0x7fc00001, 0xffc12345, 0x7f800001, 0x7fffffff], np.uint32)
    u = np.zeros((4, 9), np.float32)
    v = np.zeros((4, 9), np.float32)
    u.view(np.uint32)[:, 4] = patterns
    v.view(np.uint32)[:, 4] = patterns[::-1]
    v[:, 0] = np.inf
    state = np.ones((4, 9), np.uint8)
    state[:, 3:6] = 0                      # the NaN column has no valid neighbour
    for mode in ("filter", "fill"):
        uo, vo, so, rec = hs.median_host(u, v, state, state_out=True, stats=True, mode=mode)
        assert np.array_equal(uo.view(np.uint32)[:, 4], patterns) and np.array_equal(vo.view(np.uint32)[:, 4], patterns[::-1])
        assert np.all(so[:, 4] == 0) and np.all(so[:, 3] == 2) and np.all(so[:, 5] == 2)
        assert rec.unfilled == 4 + 0 and rec.newly_filled == 8 + 4  # (column 0 is unknown too, and has voters)
    # too few votes: copied as well, with its neighbours
    uo, vo, so, _ = hs.median_host(u, v, state, state_out=True, mode="fill", min_votes=9)
    assert np.array_equal(uo.view(np.uint32), u.view(np.uint32)) and np.array_equal(vo.view(np.uint32), v.view(np.uint32))
    assert np.all(so[:, 3:6] == 0)


def test_state_bytes_map_to_kept_and_filled(hs):
    u = np.zeros((1, 6), np.float32)
    state = np.array([[2, 255, 1, 7, 0, 254]], np.uint8)
    for mode in ("filter", "fill"):
        so = hs.median_host(u, u, state, flow=False, state_out=True, mode=mode)[2]
        assert so.tolist() == [[2, 1, 1, 1, 2, 1]]
    so = hs.median_host(u, u, state, flow=False, state_out=True, mode="fill", min_votes=3)[2]
    assert so.tolist() == [[2, 1, 1, 1, 0, 1]]


def test_components_come_from_different_pixels(hs):
    u = np.array([[1.0, 2.0, 3.0]], np.float32)
    v = np.array([[5.0, 9.0, 7.0]], np.float32)
    uo, vo, _, _ = hs.median_host(u, v)
    assert (uo[0, 1], vo[0, 1]) == (2.0, 7.0)      # u of pixel 1, v of pixel 2: no input vector


# ---- 5. passes -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius,mode", [(1, "filter"), (2, "fill"), (1, "fill"), (2, "filter")])
def test_passes_equal_chained_single_passes(hs, radius, mode):
    u, v, state = field(37, 23, 3)
    kw = dict(radius=radius, mode=mode, min_votes=3)
    cu, cv, cs = u, v, state
    for k in range(1, 5):
        cu, cv, cs, crec = hs.median_host(cu, cv, cs, state_out=True, stats=True, **kw)
        wu, wv, ws, wstats, _ = restate(*((u, v, state) if k == 1 else prev), radius, mode, 3)
        assert np.array_equal(cu.view(np.uint32), wu) and np.array_equal(cs, ws) and stat_tuple(crec) == wstats
        prev = (cu, cv, cs)
        mu, mv, ms, mrec = hs.median_host(u, v, state, state_out=True, stats=True, passes=k, **kw)
        assert np.array_equal(mu.view(np.uint32), cu.view(np.uint32)) and np.array_equal(mv.view(np.uint32), cv.view(np.uint32)), k
        assert np.array_equal(ms, cs) and stat_tuple(mrec) == stat_tuple(crec), k
        # the statistics alone, and without a state plane
        assert stat_tuple(hs.median_host(u, v, state, flow=False, stats=True, passes=k, **kw)[3]) == stat_tuple(crec)
    a = hs.median_host(u, v, None, passes=3, **kw)
    b = hs.median_host(*hs.median_host(*hs.median_host(u, v, None, state_out=True, **kw)[:3], state_out=True, **kw)[:3], **kw)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


# ---- 6. a hole closes from its rim ------------------------------------------------------------------------------------------

def test_hole_closes_in_depth_over_radius_passes(hs):
    """A 21 x 31 hole in a valid 256 x 128 field, FILL, min_votes 1: a hole pixel at Chebyshev depth d is filled in pass
    ceil(d / r), and the deepest is at 11."""
    W, H = 256, 128
    ys, xs = np.mgrid[0:H, 0:W]
    u, v = (xs * 0.01).astype(np.float32), (ys * 0.02).astype(np.float32)
    state = np.ones((H, W), np.uint8)
    state[40:71, 100:121] = 0
    left = lambda r, k: int(hs.median_host(u, v, state, flow=False, stats=True, radius=r, mode="fill", passes=k)[3].unfilled)
    seq = [left(1, k) for k in range(1, 12)]
    print("unfilled after passes 1 .. 11, r = 1:", seq)
    assert seq == [(21 - 2 * k) * (31 - 2 * k) for k in range(1, 11)] + [0]
    assert seq[0] == 551 and seq[1] == 459 and seq[9] == 11 and seq[9] > 0 and seq[10] == 0
    assert left(2, 5) > 0 and left(2, 6) == 0
    uo, vo, so, rec = hs.median_host(u, v, state, state_out=True, stats=True, mode="fill", passes=11)
    assert (rec.kept, rec.filled, rec.unfilled, rec.newly_filled) == (W * H - 651, 651, 0, 11)
    assert np.all(so[40:71, 100:121] == 2) and np.array_equal(uo[state == 1], u[state == 1])


# ---- 7. meaning ------------------------------------------------------------------------------------------------------------

def test_meaning_on_a_corrupted_solved_flow(hs):
    """2 % of a solved flow replaced by outliers of +-50 px.  RMS = sqrt(mean(du^2 + dv^2)) against the clean field.
    Measured with the restatement: corrupted 5.92, FILTER r = 1 0.165 (the clean field filtered: 0.164, the floor),
    FILL with state = ~bad 0.028."""
    g = np.load(GOLDEN)
    cu, cv = g["u"].astype(np.float32), g["v"].astype(np.float32)
    rng = np.random.default_rng(5)
    bad = rng.random(cu.shape) < 0.02
    u, v = cu.copy(), cv.copy()
    u[bad] = rng.uniform(-50, 50, int(bad.sum())).astype(np.float32)
    v[bad] = rng.uniform(-50, 50, int(bad.sum())).astype(np.float32)
    rms = lambda a, b: float(np.sqrt(np.mean((a.astype(np.float64) - cu) ** 2 + (b.astype(np.float64) - cv) ** 2)))
    before = rms(u, v)
    fu, fv, _, _ = hs.median_host(u, v)
    floor = rms(*hs.median_host(cu, cv)[:2])
    lu, lv, _, rec = hs.median_host(u, v, (~bad).astype(np.uint8) * 255, stats=True, mode="fill")
    print("rms: corrupted %.4f filtered %.4f (clean field filtered %.4f) filled %.4f; unfilled %d" % (before, rms(fu, fv), floor, rms(lu, lv), rec.unfilled))
    assert rms(fu, fv) <= before / 10
    assert rec.unfilled == 0 and rec.newly_filled == int(bad.sum())
    assert rms(lu, lv) <= before / 50
    assert np.array_equal(lu[~bad], u[~bad]) and np.array_equal(lv[~bad], v[~bad])


# ---- 8. the rule header under sanitizers -----------------------------------------------------------------------------------

def sanitizer_planes(W, H, pad):
    """The planes of run() in tests/median_rule_main.cpp."""
    sa = np.array([np.nan, 1, np.inf, 0, BIG, 0, 1e9, 0, 0, -0.0, 1e-42, 2, 0.5, -1e9], np.float32)
    sb = np.array([1, np.nan, 0, -np.inf, 0, -BIG, 0, -1e9, 0, -0.0, -1e-42, -0.0, 0.5, 1e9], np.float32)
    n = (W + pad) * (H - 1) + W
    view = lambda flat: flat[:(W + pad) * H].reshape(H, W + pad)[:, :W]
    u, v = (view(np.zeros(n + pad, np.float32)) for _ in range(2))
    s = view(np.zeros(n + pad, np.uint8))
    j = np.arange(W * H).reshape(H, W)
    u[...] = ((j * 7 % 11) - 5).astype(np.float32) * np.float32(0.5)
    v[...] = ((j * 5 % 13) - 6).astype(np.float32) * np.float32(0.25)
    m = j % 7 == 3
    u[m], v[m] = sa[j[m] // 7 % 14], sb[j[m] // 7 % 14]
    s[...] = np.array([255, 0, 1, 2, 7], np.uint8)[j % 5]
    return u, v, s, n, view


def test_rule_under_sanitizers(hs, tmp_path):
    """The host rule as a stand-alone program (tests/median_rule_main.cpp) under AddressSanitizer and UBSan: the
    selection network on every zero-one input, the sentinel identity, and fields with special values, 1-pixel-wide and
    1-pixel-high frames and strided rows in exact-size heap blocks; its records and checksums are the library's."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "median_rule")
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
    r = subprocess.run([gxx] + flags + ["-Wall", "-Wextra", "-I", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), os.path.join(ROOT, "tests", "median_rule_main.cpp"),
                                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr)
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 20
    for line in lines:
        head, mid, tail = line.split(" | ")
        W, H, pad, radius, fill, votes = (int(x) for x in head.split())
        u, v, s, n, view = sanitizer_planes(W, H, pad)
        uw, vw, sw = np.full(n + pad, -7.0, np.float32), np.full(n + pad, -7.0, np.float32), np.full(n + pad, 0xA5, np.uint8)
        _, _, _, rec = hs.median_host(u, v, s, flow=(view(uw), view(vw)), state_out=view(sw), stats=True, radius=radius, mode="fill" if fill else "filter",
                                      min_votes=votes)
        assert [int(x) for x in mid.split()] == list(stat_tuple(rec)), line
        total = 0
        for a, b, c in zip(uw[:n].view(np.uint32).tolist(), vw[:n].view(np.uint32).tolist(), sw[:n].tolist()):
            total = (total * 31 + a + 3 * b + c) % (1 << 64)
        assert int(tail) == total, line
