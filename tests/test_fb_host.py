"""hsflow_fb_host: the rule of csrc/hs_fb_rule.h on the host -- the forward-backward consistency of two flow fields as a
mask of four classes, the squared error and exact integer statistics.  No GPU work: the device side is held to these
bits by tests/test_gpu_fb.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SHAPES = [(13, 7), (260, 37), (96, 64)]
ITER = 1
OK, E_ARG, E_SIZE = 0, 1, 2
NAN_BITS = 0x7fc00000
BIG = np.nextafter(np.float32(1e9), np.float32(np.inf))
# (tests/test_gpu_warp.py's list)
SPECIAL = [(np.nan, 1.0), (1.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (BIG, 0.0), (0.0, -BIG), (1e9, 0.0), (0.0, -1e9), (0.0, 0.0), (-0.0, -0.0),
           (1e-42, -1e-42), (2.0, -0.0), (0.5, 0.5), (-1e9, 1e9)]
PARAM_SETS = [dict(), dict(alpha=0.0, beta=0.0), dict(alpha=1e6, beta=1e30), dict(values=(1, 2, 3, 4))]
STAT_FIELDS = ("consistent", "inconsistent", "outside", "unknown", "sum_err2_q", "max_err2_bits")


def known(a, b):
    with np.errstate(invalid="ignore"):
        return ~(np.isnan(a) | np.isnan(b) | (np.abs(a) > np.float32(1e9)) | (np.abs(b) > np.float32(1e9)))


def restate(uf, vf, ub, vb, alpha=0.01, beta=0.5, f=np.float32):
    """The rule restated in NumPy, every operation an array operation of type `f` and so rounded on its own.  Returns
    (class plane, err2 of type f -- meaningful where the class is 0 or 1)."""
    H, W = uf.shape
    kf = known(uf, vf)
    a = np.where(kf, uf, np.float32(0)).astype(f)
    b = np.where(kf, vf, np.float32(0)).astype(f)
    xs = np.broadcast_to(np.arange(W, dtype=f)[None, :], (H, W))
    ys = np.broadcast_to(np.arange(H, dtype=f)[:, None], (H, W))
    fx = (xs + a).astype(f)
    fy = (ys + b).astype(f)
    within = kf & (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
    fx = np.where(within, fx, f(0))
    fy = np.where(within, fy, f(0))
    x0 = np.floor(fx).astype(np.int64)
    y0 = np.floor(fy).astype(np.int64)
    x1 = np.minimum(x0 + 1, W - 1)
    y1 = np.minimum(y0 + 1, H - 1)
    ax = (fx - x0.astype(f)).astype(f)
    ay = (fy - y0.astype(f)).astype(f)
    taps = [(y0, x0), (y0, x1), (y1, x0), (y1, x1)]
    tk = np.ones((H, W), bool)
    for yy, xx in taps:
        tk &= known(ub[yy, xx], vb[yy, xx])
    ev = within & tk

    def sample(plane):
        p00, p10, p01, p11 = (np.where(ev, plane[yy, xx], np.float32(0)).astype(f) for yy, xx in taps)
        top = (p00 + (ax * (p10 - p00).astype(f)).astype(f)).astype(f)
        bot = (p01 + (ax * (p11 - p01).astype(f)).astype(f)).astype(f)
        return (top + (ay * (bot - top).astype(f)).astype(f)).astype(f)

    c, d = sample(ub), sample(vb)
    ex, ey = (a + c).astype(f), (b + d).astype(f)
    err2 = ((ex * ex).astype(f) + (ey * ey).astype(f)).astype(f)
    mag2 = (((a * a).astype(f) + (b * b).astype(f)).astype(f) + ((c * c).astype(f) + (d * d).astype(f)).astype(f)).astype(f)
    bound = ((f(np.float32(alpha)) * mag2).astype(f) + f(np.float32(beta))).astype(f)
    cls = np.where(~kf, 3, np.where(~within, 2, np.where(~tk, 3, np.where(err2 <= bound, 0, 1)))).astype(np.uint8)
    return cls, err2


def stats_of(cls, err2):
    """The six statistics from a class plane and a float32 err2 plane."""
    ev = cls <= 1
    e = err2[ev].astype(np.float32)
    q = np.minimum((e * np.float32(256.0)).astype(np.float32), np.float32(65535.0)).astype(np.uint32)
    return tuple(int((cls == k).sum()) for k in range(4)) + (int(q.astype(np.uint64).sum()), int(e.view(np.uint32).max()) if e.size else 0)


def stat_tuple(s):
    return tuple(int(getattr(s, k)) for k in STAT_FIELDS)


def err2_bits(cls, err2):
    return np.where(cls <= 1, err2.astype(np.float32).view(np.uint32), np.uint32(NAN_BITS)).astype(np.uint32)


def padded(shape, dtype, pad, fill=0):
    """An array of `shape` as a view into rows that are `pad` elements longer, and the whole buffer."""
    whole = np.full((shape[0], shape[1] + pad), fill, dtype)
    return whole[:, :shape[1]], whole


def fields(W, H, seed, pad=0):
    """Forward: Gaussian sigma 2, its left quarter the constant (3, -2).  Backward: Gaussian sigma 2, its left half (-3, 2)
    plus Gaussian noise sigma 0.5.  The special values scattered over both, and over backward taps of known forward
    pixels.  Rows `pad` floats longer than W.  Returns uf, vf, ub, vb."""
    rng = np.random.default_rng(seed)
    uf, vf, ub, vb = (padded((H, W), np.float32, pad)[0] for _ in range(4))
    for p in (uf, vf, ub, vb):
        p[...] = rng.standard_normal((H, W)) * 2.0
    q, h = max(1, W // 4), W // 2
    uf[:, :q], vf[:, :q] = 3.0, -2.0
    ub[:, :h] = -3.0 + rng.standard_normal((H, h)) * 0.5
    vb[:, :h] = 2.0 + rng.standard_normal((H, h)) * 0.5
    n = min(len(SPECIAL), W * H // 8)
    for pu, pv in ((uf, vf), (ub, vb)):
        spots = rng.permutation(W * H)[:n]
        for k, (sa, sb) in zip(spots, SPECIAL):
            pu[divmod(int(k), W)], pv[divmod(int(k), W)] = sa, sb
    # over the backward taps of known forward pixels that land inside
    fx, fy = np.arange(W)[None, :] + uf, np.arange(H)[:, None] + vf
    with np.errstate(invalid="ignore"):
        inside = known(uf, vf) & (fx >= 0) & (fx <= W - 1) & (fy >= 0) & (fy <= H - 1)
    ys, xs = np.nonzero(inside)
    pick = rng.permutation(len(ys))[:n]
    for j, (sa, sb) in zip(pick, SPECIAL):
        ty = min(int(np.floor(fy[ys[j], xs[j]])) + (j & 1), H - 1)
        tx = min(int(np.floor(fx[ys[j], xs[j]])) + ((j >> 1) & 1), W - 1)
        ub[ty, tx], vb[ty, tx] = sa, sb
    return uf, vf, ub, vb


def call(hs, planes, fp, mask, err2, stats, width=None, height=None, strides=None, out_strides=None):
    """hsflow_fb_host with raw arguments; planes: uf, vf, ub, vb (None allowed with strides given)."""
    first = next(p for p in planes if p is not None)
    H, W = first.shape
    st = strides or tuple(p.strides[0] for p in planes)
    os_ = out_strides or (mask.strides[0] if mask is not None else 0, err2.strides[0] if err2 is not None else 0)
    p = lambda x: ctypes.c_void_p(x.ctypes.data) if x is not None else None
    flows = []
    for x, s in zip(planes, st):
        flows += [p(x), s]
    return hs._lib.load().hsflow_fb_host(*(flows + [W if width is None else width, H if height is None else height,
                                                    ctypes.byref(fp) if fp is not None else None, p(mask), os_[0], p(err2), os_[1],
                                                    ctypes.byref(stats) if stats is not None else None]))


# ---- 1. version, sizes, defaults -----------------------------------------------------------------------------------

def test_version_sizes_and_defaults(hs):
    L = hs._lib.load()
    assert L.hsflow_version() >= 18
    text = open(os.path.join(ROOT, "include", "hsflow.h")).read()
    assert int(re.search(r"#define HSFLOW_VERSION_MINOR (\d+)", text).group(1)) >= 18
    assert ctypes.sizeof(hs.HsflowFbParams) == 16 and ctypes.sizeof(hs.HsflowFbStats) == 64
    fp = hs.HsflowFbParams()
    ctypes.memset(ctypes.byref(fp), 0xff, ctypes.sizeof(fp))
    L.hsflow_default_fb_params(ctypes.byref(fp))
    assert (fp.struct_size, fp.alpha, fp.beta, list(fp.value)) == (16, float(np.float32(0.01)), 0.5, [255, 0, 0, 0])
    L.hsflow_default_fb_params(None)  # (ignored)


# ---- 2. argument errors ----------------------------------------------------------------------------------------------

def test_argument_errors(hs):
    W, H = 6, 4
    u = np.zeros((H, W), np.float32)
    mask = np.zeros((H, W), np.uint8)
    err2 = np.zeros((H, W), np.float32)
    stats = hs.HsflowFbStats()
    good = hs.make_fb_params
    four = (u, u, u, u)
    full = (W * 4,) * 4
    assert call(hs, four, good(), mask, err2, stats) == OK
    for k in range(4):
        planes = list(four)
        planes[k] = None
        assert call(hs, planes, good(), mask, None, None, strides=full) == E_ARG
    assert call(hs, four, None, mask, None, None) == E_ARG
    assert call(hs, four, good(), None, None, None) == E_ARG  # nothing asked for
    bad = good()
    bad.struct_size -= 4
    assert call(hs, four, bad, mask, None, None) == E_ARG
    for alpha in (float("nan"), float("inf"), -1e-6, 1.0001e6, -float("inf")):
        assert call(hs, four, good(alpha=alpha), mask, None, None) == E_ARG
    for beta in (float("nan"), float("inf"), -1e-6, 1.0001e30):
        assert call(hs, four, good(beta=beta), mask, None, None) == E_ARG
    for kw in (dict(alpha=0.0), dict(alpha=1e6), dict(beta=0.0), dict(beta=1e30)):  # the limits themselves
        assert call(hs, four, good(**kw), mask, None, None) == OK
    assert call(hs, four, good(), mask, None, None, width=0) == E_SIZE
    assert call(hs, four, good(), mask, None, None, height=-1) == E_SIZE
    for k in range(4):
        short, odd = list(full), list(full)
        short[k] -= 4
        odd[k] += 2
        assert call(hs, four, good(), mask, None, None, strides=tuple(short)) == E_SIZE
        assert call(hs, four, good(), mask, None, None, strides=tuple(odd)) == E_SIZE
    assert call(hs, four, good(), mask, None, None, out_strides=(W - 1, 0)) == E_SIZE
    assert call(hs, four, good(), None, err2, None, out_strides=(0, W * 4 - 4)) == E_SIZE
    assert call(hs, four, good(), None, err2, None, out_strides=(0, W * 4 + 2)) == E_SIZE
    assert call(hs, four, good(), None, None, stats, out_strides=(0, 0)) == OK  # (absent outputs: their strides are not looked at)
    with pytest.raises(ValueError):
        hs.make_fb_params(values=(1, 2, 3))


# ---- 3. the rule against the fp32 restatement ------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SHAPES)
def test_rule_against_fp32_restatement(hs, W, H):
    """Mask bytes, err2 bit patterns (NaN included) and all six statistics, with padded strides everywhere; the
    restatement alone gives all four classes."""
    uf, vf, ub, vb = fields(W, H, 7 * W + H, pad=3)
    for kw in PARAM_SETS:
        fp = hs.make_fb_params(**kw)
        cls, e = restate(uf, vf, ub, vb, fp.alpha, fp.beta)
        counts = [int((cls == k).sum()) for k in range(4)]
        print("%dx%d %r: consistent / inconsistent / outside / unknown = %r" % (W, H, kw, counts))
        if not kw:
            assert all(n > 0 for n in counts), counts
        mask, mwhole = padded((H, W), np.uint8, 5, 0xA5)
        err2, ewhole = padded((H, W), np.float32, 2, -7.0)
        m2, e2, s = hs.fb_host(uf, vf, ub, vb, mask=mask, err2=err2, stats=True, params=fp)
        assert m2 is mask and e2 is err2
        assert np.array_equal(mask, np.asarray(list(fp.value), np.uint8)[cls]), kw
        assert np.array_equal(err2.view(np.uint32), err2_bits(cls, e)), kw
        assert (mwhole[:, W:] == 0xA5).all() and (ewhole[:, W:] == -7.0).all()  # beyond W: untouched
        assert stat_tuple(s) == stats_of(cls, e), kw
        assert sum(stat_tuple(s)[:4]) == W * H
        assert bytes(s)[44:] == b"\0" * 20


# ---- 4. exact cases ----------------------------------------------------------------------------------------------------

def test_whole_number_flows_cancel_exactly(hs):
    W, H = 31, 17
    uf, vf = np.full((H, W), 3.0, np.float32), np.full((H, W), -2.0, np.float32)
    mask, err2, s = hs.fb_host(uf, vf, -uf, -vf, err2=True, stats=True, alpha=0.0, beta=0.0, values=(9, 8, 7, 6))
    inside = np.zeros((H, W), bool)
    inside[2:, :W - 3] = True
    assert np.all(mask[inside] == 9) and np.all(mask[~inside] == 7)
    assert np.all(err2[inside] == 0.0) and np.all(err2.view(np.uint32)[~inside] == NAN_BITS)
    assert stat_tuple(s) == ((W - 3) * (H - 2), 0, W * H - (W - 3) * (H - 2), 0, 0, 0)


def test_edges_and_special_values(hs):
    W, H = 5, 3
    z = lambda: np.zeros((H, W), np.float32)
    uf, vf, ub, vb = z(), z(), z(), z()
    uf[1, 2] = 2.0                                   # fx == W-1 exactly: inside
    vf[0, 1] = 2.0                                   # fy == H-1 exactly
    uf[1, 0] = 1e9                                   # known, and outside
    uf[2, 0] = BIG                                   # the next float above: unknown
    uf[2, 3] = 1.000001                              # just beyond W-1
    uf[0, 4] = -4.0                                  # fx == 0 exactly
    ub[1, 4], ub[2, 1], ub[0, 0] = -2.0, 0.0, 4.0    # the exact opposites where the three land
    vb[2, 1] = -2.0
    cls = hs.fb_host(uf, vf, ub, vb, alpha=0.0, beta=0.0, values=(0, 1, 2, 3))[0]
    want, _ = restate(uf, vf, ub, vb, 0.0, 0.0)
    assert np.array_equal(cls, want)
    assert cls[1, 2] == 0 and cls[0, 1] == 0 and cls[0, 4] == 0
    assert cls[1, 0] == 2 and cls[2, 0] == 3 and cls[2, 3] == 2
    # a NaN at a zero-weight tap: pixel (1, 1) with zero flow lands on (1, 1) with ax = ay = 0; its taps are x 1..2, y 1..2
    for ty, tx in ((1, 2), (2, 1), (2, 2)):
        ub2 = ub.copy()
        ub2[ty, tx] = np.nan
        assert hs.fb_host(uf, vf, ub2, vb, values=(0, 1, 2, 3))[0][1, 1] == 3
    vb2 = vb.copy()
    vb2[2, 2] = BIG
    assert hs.fb_host(uf, vf, ub, vb2, values=(0, 1, 2, 3))[0][1, 1] == 3
    # err2 without a mask: OUTSIDE and UNKNOWN read the quiet NaN
    none, err2, _ = hs.fb_host(uf, vf, ub, vb, mask=False, err2=True)
    assert none is None
    bits = err2.view(np.uint32)
    assert bits[1, 0] == NAN_BITS and bits[2, 0] == NAN_BITS and bits[2, 3] == NAN_BITS and bits[1, 2] == 0


def test_saturation(hs):
    W, H = 4, 2
    z = lambda: np.zeros((H, W), np.float32)
    uf, vf, ub, vb = z(), z(), z(), z()
    ub[0, 0] = 16.0      # err2 == 256 exactly
    ub[0, 1] = 1000.0    # far beyond
    ub[1, 1] = 0.5       # 0.25 px^2 -> 64
    ub[1, 2] = 15.96875  # 255.0009765625 -> 65280
    _, err2, s = hs.fb_host(uf, vf, ub, vb, err2=True, stats=True)
    assert err2[0, 0] == 256.0 and err2[0, 1] == 1e6
    assert s.sum_err2_q == 65535 + 65535 + 64 + 65280
    assert s.max_err2_bits == int(np.float32(1e6).view(np.uint32))
    assert s.consistent + s.inconsistent == W * H


# ---- 5. against float64 --------------------------------------------------------------------------------------------------

MEASURED_WORST = 0.2424      # (this test's own measurement, see its docstring)
MEASURED_ORDINARY = 9.24e-5


def test_rule_against_float64(hs):
    """The same formula in float64 on 20 fields of 260x37 (seeds 100 .. 119), default parameters.  The class planes may
    differ at no more than 20 of 192 400 pixels; measured: 0.  Over the evaluated pixels whose forward components are below
    1e8, |err2_32 - err2_64| / (err2_64 + 0.5) was 0.2424 at worst with these fields, and 4 x that is asserted.  That worst
    case is a pixel whose backward taps hold +1e9 and -1e9 side by side: the bilinear sample cancels them and keeps an
    absolute rounding error of some tens of pixels.  So the same figure is also taken over the pixels whose eight tap
    components are all below 1e3 in magnitude: 9.24e-5 at worst (the rounding of fl(x + a) at x up to 259 moves the tap
    weights by 1.5e-5), and 4 x that is asserted too."""
    W, H = 260, 37
    differing, worst, ordinary = 0, 0.0, 0.0
    for seed in range(100, 120):
        uf, vf, ub, vb = fields(W, H, seed)
        cls, err2, _ = hs.fb_host(uf, vf, ub, vb, err2=True, values=(0, 1, 2, 3))
        cls64, e64 = restate(uf, vf, ub, vb, f=np.float64)
        differing += int((cls != cls64).sum())
        with np.errstate(invalid="ignore"):
            sel = (cls <= 1) & (cls64 <= 1) & (np.abs(uf) < 1e8) & (np.abs(vf) < 1e8)
        rel = np.where(sel, np.abs(err2.astype(np.float64) - e64) / (e64 + 0.5), 0.0)
        worst = max(worst, float(rel.max()))
        fx, fy = np.where(sel, np.arange(W)[None, :] + uf, 0.0), np.where(sel, np.arange(H)[:, None] + vf, 0.0)
        x0, y0 = np.floor(fx).astype(int), np.floor(fy).astype(int)
        small = sel.copy()
        for yy, xx in ((y0, x0), (y0, np.minimum(x0 + 1, W - 1)), (np.minimum(y0 + 1, H - 1), x0), (np.minimum(y0 + 1, H - 1), np.minimum(x0 + 1, W - 1))):
            small &= (np.abs(ub[yy, xx]) < 1e3) & (np.abs(vb[yy, xx]) < 1e3)
        ordinary = max(ordinary, float(rel[small].max()))
    print("classes that differ from float64: %d of %d; worst relative err2 deviation %.4e, with ordinary taps %.4e" % (differing, 20 * W * H, worst, ordinary))
    assert differing <= 20
    assert worst <= 4 * MEASURED_WORST
    assert ordinary <= 4 * MEASURED_ORDINARY


# ---- 6. meaning ------------------------------------------------------------------------------------------------------------

def test_meaning_on_solved_flows(hs, oracle):
    """The check carries meaning on this solver's flow: a translating pair is mostly consistent, noise is not."""
    from opticalflowhs_amd import synth
    shares = []
    for prev, curr in (synth.translating_pair(96, 64, seed=1), synth.random_pair(96, 64, seed=3)):
        uf, vf = oracle.calc_optical_flow_hs(prev, curr, 0.1, 100, term_type=ITER)
        ub, vb = oracle.calc_optical_flow_hs(curr, prev, 0.1, 100, term_type=ITER)
        s = hs.fb_host(uf, vf, ub, vb, stats=True)[2]
        shares.append(s.consistent / float(s.consistent + s.inconsistent))
        print("evaluated %d consistent %d share %.3f" % (s.consistent + s.inconsistent, s.consistent, shares[-1]))
    assert shares[0] >= 0.85
    assert shares[1] <= 0.15


# ---- 7. the rule header under sanitizers -----------------------------------------------------------------------------------

SANITIZER_MAIN = r"""
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "hs_fb_rule.h"

// W x H planes whose rows are `pad` floats longer than W, in exact-size heap blocks: a tap beyond the plane is a finding.
static void run(int W, int H, int pad, float alpha, float beta)
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float big = std::nextafterf(1e9f, inf);
    const float sa[14] = {nan, 1.f, inf, 0.f, big, 0.f, 1e9f, 0.f, 0.f, -0.f, 1e-42f, 2.f, 0.5f, -1e9f};
    const float sb[14] = {1.f, nan, 0.f, -inf, 0.f, -big, 0.f, -1e9f, 0.f, -0.f, -1e-42f, -0.f, 0.5f, 1e9f};
    const size_t P = (size_t)W + pad, n = P * (H - 1) + W;
    std::vector<float> uf(n), vf(n), ub(n), vb(n), err2(n, -7.f);
    std::vector<uint8_t> mask(n, 0xA5);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t k = (size_t)y * P + x, j = (size_t)y * W + x;
            uf[k] = (float)((int)(j * 7 % 5) - 2) * 0.75f; vf[k] = (float)((int)(j * 3 % 5) - 2) * 0.5f;
            ub[k] = -uf[k] + (float)(j % 3) * 0.25f;       vb[k] = -vf[k] - (float)(j % 2) * 0.5f;
            if (j % 3 == 1) { uf[k] = sa[j / 3 % 14]; vf[k] = sb[j / 3 % 14]; }
            if (j % 5 == 2) { ub[k] = sa[j / 5 % 14]; vb[k] = sb[j / 5 % 14]; }
        }
    const uint8_t value[4] = {1, 2, 3, 4};
    hsfb::Sums s;
    hsfb::fb_rows(uf.data(), P * 4, vf.data(), P * 4, ub.data(), P * 4, vb.data(), P * 4, W, H, alpha, beta, value, mask.data(), P, err2.data(), P * 4, &s);
    unsigned long long sum = 0;
    for (size_t k = 0; k < n; k++) sum = sum * 31 + mask[k] + hscolor::float_bits(err2[k]);
    std::printf("%d %d %d %g %g | %llu %llu %llu %llu %llu %u | %llu\n", W, H, pad, (double)alpha, (double)beta, (unsigned long long)s.cls[0],
                (unsigned long long)s.cls[1], (unsigned long long)s.cls[2], (unsigned long long)s.cls[3], (unsigned long long)s.sum_q, s.max_bits, sum);
}

int main()
{
    const int shapes[5][3] = {{5, 3, 0}, {1, 9, 0}, {9, 1, 0}, {7, 5, 3}, {1, 1, 2}};
    for (const auto &sh : shapes) {
        run(sh[0], sh[1], sh[2], 0.01f, 0.5f);
        run(sh[0], sh[1], sh[2], 0.f, 0.f);
        run(sh[0], sh[1], sh[2], 1e6f, 1e30f);
    }
    return 0;
}
"""


def sanitizer_planes(W, H, pad):
    """The planes of SANITIZER_MAIN's run()."""
    sa = np.array([np.nan, 1, np.inf, 0, BIG, 0, 1e9, 0, 0, -0.0, 1e-42, 2, 0.5, -1e9], np.float32)
    sb = np.array([1, np.nan, 0, -np.inf, 0, -BIG, 0, -1e9, 0, -0.0, -1e-42, -0.0, 0.5, 1e9], np.float32)
    n = (W + pad) * (H - 1) + W
    flat = [np.zeros(n + pad, np.float32) for _ in range(4)]
    uf, vf, ub, vb = (p[:(W + pad) * H].reshape(H, W + pad)[:, :W] for p in flat)
    j = np.arange(W * H).reshape(H, W)
    uf[...] = ((j * 7 % 5) - 2).astype(np.float32) * np.float32(0.75)
    vf[...] = ((j * 3 % 5) - 2).astype(np.float32) * np.float32(0.5)
    ub[...] = -uf + (j % 3).astype(np.float32) * np.float32(0.25)
    vb[...] = -vf - (j % 2).astype(np.float32) * np.float32(0.5)
    m = j % 3 == 1
    uf[m], vf[m] = sa[j[m] // 3 % 14], sb[j[m] // 3 % 14]
    m = j % 5 == 2
    ub[m], vb[m] = sa[j[m] // 5 % 14], sb[j[m] // 5 % 14]
    return uf, vf, ub, vb, n


def test_rule_under_sanitizers(hs, tmp_path):
    """The host rule as a stand-alone program under AddressSanitizer and UBSan: special values, 1-pixel-wide and
    1-pixel-high frames and strided rows in exact-size heap blocks; its statistics and checksum are the library's."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    main = tmp_path / "fb_rule_main.cpp"
    main.write_text(SANITIZER_MAIN)
    exe = str(tmp_path / "fb_rule")
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
    assert len(lines) == 15
    for line in lines:
        head, mid, tail = line.split(" | ")
        W, H, pad = (int(x) for x in head.split()[:3])
        alpha, beta = (float(x) for x in head.split()[3:])
        uf, vf, ub, vb, n = sanitizer_planes(W, H, pad)
        mwhole, ewhole = np.full(n + pad, 0xA5, np.uint8), np.full(n + pad, -7.0, np.float32)
        mask = mwhole[:(W + pad) * H].reshape(H, W + pad)[:, :W]
        err2 = ewhole[:(W + pad) * H].reshape(H, W + pad)[:, :W]
        _, _, s = hs.fb_host(uf, vf, ub, vb, mask=mask, err2=err2, stats=True, alpha=alpha, beta=beta, values=(1, 2, 3, 4))
        assert [int(x) for x in mid.split()] == list(stat_tuple(s)), line
        total = 0
        for m, e in zip(mwhole[:n].tolist(), ewhole[:n].view(np.uint32).tolist()):
            total = (total * 31 + m + e) % (1 << 64)
        assert int(tail) == total, line
