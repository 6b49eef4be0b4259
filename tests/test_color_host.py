"""CPU checks of the dense colour picture's rule (csrc/hs_color_rule.h through hsflow_color_flow_host): the polynomial's
accuracy, the rule against the same formula in float64, exact pixels, borders and argument errors.  No GPU is used."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SEGMENTS = (15, 6, 4, 11, 13, 6)  # RY, YG, GC, CB, BM, MR


def wheel():
    """The 55 entries by Middlebury's integer arithmetic."""
    w = []
    ry, yg, gc, cb, bm, mr = SEGMENTS
    w += [(255, 255 * i // ry, 0) for i in range(ry)]
    w += [(255 - 255 * i // yg, 255, 0) for i in range(yg)]
    w += [(0, 255, 255 * i // gc) for i in range(gc)]
    w += [(0, 255 - 255 * i // cb, 255) for i in range(cb)]
    w += [(255 * i // bm, 0, 255) for i in range(bm)]
    w += [(255, 0, 255 - 255 * i // mr) for i in range(mr)]
    assert len(w) == 55
    return np.array(w, np.float64)


def statement64(u, v, max_flow=None):
    """The rule in float64: np.arctan2, np.sqrt, integer wheel, radius divided by m.  Returns (picture as float levels
    already truncated, rad, m)."""
    a, b = u.astype(np.float64), v.astype(np.float64)
    unknown = np.isnan(a) | np.isnan(b) | (np.abs(a) > 1e9) | (np.abs(b) > 1e9)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.sqrt(a * a + b * b)
    if max_flow is None:
        m = r[~unknown].max() if (~unknown).any() else 0.0
        m = m if m > 0 else 1.0
    else:
        m = float(max_flow)
    with np.errstate(invalid="ignore", over="ignore"):
        rad = r / m
        fk = (np.arctan2(-b, -a) / np.pi + 1.0) * 0.5 * 54.0
    fk = np.where(unknown, 0.0, fk)
    k0 = np.minimum(fk.astype(np.int64), 54)
    k1 = np.where(k0 == 54, 0, k0 + 1)
    f = (fk - k0)[..., None]
    w = wheel() / 255.0
    col = (1.0 - f) * w[k0] + f * w[k1]
    radc = np.where(unknown, 0.0, rad)[..., None]
    col = np.where(radc <= 1.0, 1.0 - radc * (1.0 - col), col * 0.75)
    img = np.floor(255.0 * col)
    img[unknown] = 0.0
    return img, rad, m


def fixed32(k0, f, rad):
    """Steps 5-6 of the rule in fp32, operation by operation, for one wheel position: the three bytes."""
    F = np.float32
    w = wheel()
    k1 = 0 if k0 == 54 else k0 + 1
    out = []
    for c in range(3):
        c0, c1 = F(w[k0][c]) / F(255), F(w[k1][c]) / F(255)
        col = F(F(F(1) - F(f)) * c0) + F(F(f) * c1)
        col = F(F(1) - F(rad)) + F(F(rad) * col) if F(rad) <= 1 else col * F(0.75)
        out.append(int(F(255) * F(col)))
    return tuple(out)


def one(hs, u, v, max_flow=None):
    img, m = hs.color_flow_host(np.array([[u]], np.float32), np.array([[v]], np.float32), max_flow=max_flow, return_scale=True)
    return tuple(int(t) for t in img[0, 0]), m


def test_version(hs):
    assert hs._lib.load().hsflow_version() >= 16


def test_polynomial_accuracy(tmp_path):
    """max |p - atan t| <= 4e-6 over 2^22 evenly spaced fp32 t in [0, 1] plus the 4096 floats nearest 0 and nearest 1
    (measured: 1.76e-6), and the unfolding against atan2 on axes and diagonals with every combination of signs."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path / "color_rule")
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "color_rule_main.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, str(1 << 22), "4096"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    worst, worst_atan2 = [float(t) for t in r.stdout.split()]
    print("max |p - atan t| = %.4g, atan2 on the axes: %.4g" % (worst, worst_atan2))
    assert worst <= 4e-6
    assert worst_atan2 <= 4e-6 + 2e-7  # (the polynomial's bound and the rounding of pi, pi/2 and the two subtractions)


def mixed_flow(scale, n=200000, seed=0):
    rng = np.random.default_rng(seed)
    u = (rng.standard_normal(n) * scale).astype(np.float32)
    v = (rng.standard_normal(n) * scale).astype(np.float32)
    idx = rng.permutation(n)[:4000].reshape(4, 1000)
    u[idx[0]] = 0.0
    v[idx[1]] = 0.0
    v[idx[2]] = u[idx[2]]
    u[idx[3]] = 0.0
    v[idx[3]] = 0.0
    v[idx[1][:300]] = -0.0
    u[idx[0][:300]] = -0.0
    return u.reshape(400, 500), v.reshape(400, 500)


@pytest.mark.parametrize("fixed", [False, True], ids=["auto", "fixed"])
@pytest.mark.parametrize("scale", [1e-20, 0.01, 1.0, 50.0, 1e4, 1e8])
def test_against_float64_statement(hs, scale, fixed):
    """Every channel within 1 level of the float64 statement on every pixel whose float64 rad is not within 2^-20 of 1; at
    most 1e-4 of the pixels excluded.  Both bounds follow from the rule: a colour changes by at most 64 levels per wheel
    step and the angle error is about 2e-5 steps, what remains is the final truncation."""
    u, v = mixed_flow(scale, seed=int(np.log10(scale)) + 30)
    _, _, m_auto = statement64(u, v)
    max_flow = float(np.float32(m_auto / 3)) if fixed else None
    got, m = hs.color_flow_host(u, v, max_flow=max_flow, return_scale=True)
    want, rad, m64 = statement64(u, v, max_flow)
    assert abs(m - m64) <= 1e-5 * m64  # (at 1e-20 the squares are denormal: a few 1e-7 of the largest one)
    excluded = np.abs(rad - 1.0) <= 2.0 ** -20
    share = excluded.mean()
    diff = np.abs(got.astype(np.float64) - want)[~excluded]
    print("scale %g %s: max diff %d levels, excluded share %.3g, m %g" % (scale, "fixed" if fixed else "auto", diff.max(), share, m))
    assert share <= 1e-4
    assert diff.max() <= 1
    if fixed:
        # the 0.75 branch is well populated: the largest of 2e5 Rayleigh radii is below 5.7 sigma, and exp(-1.9^2 / 2) = 0.16
        assert (rad > 1).mean() > 0.1


def test_pinned_pixels(hs):
    W = wheel().astype(int)
    for m in (1.0, 0.37, 1e-20, 5e8):
        fixed_m = float(np.float32(m))
        for mf in (None, fixed_m):
            assert one(hs, 0.0, 0.0, mf)[0] == (255, 255, 255)
            assert one(hs, -0.0, 0.0, mf)[0] == (255, 255, 255)
            # (AUTO takes the radius, not the component: at 1e-20 the square is denormal and the root is not m to the bit)
            m_used = fixed_m if mf is not None else float(np.sqrt(np.float32(fixed_m) * np.float32(fixed_m)))
            assert one(hs, fixed_m, 0.0, mf) == ((255, 0, 0), m_used)
            # theta = -0: wheel position 27 exactly; theta = -+pi/2: 13.5 and 40.5.  rad is 1 but for the denormal square
            rad = np.sqrt(np.float32(fixed_m) * np.float32(fixed_m)) / np.float32(m_used)
            assert rad == 1 or m == 1e-20
            assert one(hs, -fixed_m, 0.0, mf)[0] == fixed32(27, 0.0, rad)
            assert one(hs, 0.0, fixed_m, mf)[0] == fixed32(13, 0.5, rad)
            assert one(hs, 0.0, -fixed_m, mf)[0] == fixed32(40, 0.5, rad)
    assert fixed32(27, 0.0, 1.0) == tuple(W[27]) == (0, 209, 255)
    # the seam is Middlebury's: just below the positive u axis the picture shows wheel entry 54, not entry 0
    rgb, _ = one(hs, 1.0, -0.0)
    assert rgb == tuple(W[54]) == (255, 0, 43)
    assert rgb == fixed32(54, 0.0, 1.0)


def test_seam_pixel(hs):
    """Flow (m, -0.0) at scale m is wheel entry 54 itself, (255, 0, 43): the seam is Middlebury's, and a pixel on the scale
    shows the wheel's own levels -- the saturation is formed as (1 - rad) + rad col, exact at rad = 1, where
    fl(1 - fl(1 - fl(43 / 255))) = 0.16862744 would truncate to 42."""
    for m in (1.0, 0.37, 5e8):
        mf = float(np.float32(m))
        for scale in (None, mf):
            assert one(hs, mf, -0.0, scale)[0] == (255, 0, 43)
            assert one(hs, mf, 0.0, scale)[0] == (255, 0, 0)


def test_unknown_flow(hs):
    big = float(np.float32(1e9) * (np.float32(1) + np.float32(2.0 ** -23)))
    assert np.float32(big) > np.float32(1e9)
    for bad in (np.nan, np.inf, -np.inf, big, -big):
        for mf in (None, 2.0):
            assert one(hs, bad, 0.5, mf)[0] == (0, 0, 0)
            assert one(hs, 0.5, bad, mf)[0] == (0, 0, 0)
        u = np.array([[bad, 3.0, 0.0]], np.float32)
        v = np.array([[1.0, 4.0, bad]], np.float32)
        img, m = hs.color_flow_host(u, v, return_scale=True)
        assert m == 5.0 and tuple(img[0, 0]) == (0, 0, 0) and tuple(img[0, 2]) == (0, 0, 0)
        assert tuple(img[0, 1]) == one(hs, 3.0, 4.0, 5.0)[0]
    # exactly 1e9 is known
    rgb, m = one(hs, 1e9, 0.0)
    assert m == float(np.float32(1e9)) and rgb == (255, 0, 0)
    rgb, m = one(hs, -1e9, 1e9)
    assert rgb != (0, 0, 0) and np.isfinite(m) and abs(m - 1e9 * 2 ** 0.5) < 1e3


def test_denormal_flow(hs):
    tiny = float(np.float32(1e-42))
    for mf in (None, 1.0, 1e-30):
        rgb, m = one(hs, tiny, -tiny, mf)
        assert np.isfinite(m) and m > 0
        assert min(rgb) >= 254  # the squares vanish: white
    rgb, m = one(hs, tiny, tiny)
    assert m == 1.0


def test_beyond_the_scale(hs):
    """rad = 2 in FIXED: the 0.75 branch."""
    assert one(hs, 2.0, 0.0, 1.0)[0] == fixed32(0, 0.0, 2.0) == (191, 0, 0)
    assert one(hs, -2.0, 0.0, 1.0)[0] == fixed32(27, 0.0, 2.0)
    assert one(hs, 0.0, 1.0, 0.5)[0] == fixed32(13, 0.5, 2.0)


def test_all_unknown(hs):
    u = np.full((3, 5), np.nan, np.float32)
    v = np.full((3, 5), np.inf, np.float32)
    img, m = hs.color_flow_host(u, v, return_scale=True)
    assert m == 1.0 and not img.any()


def raw(hs, u, v, cp, rgb, stride, width=None, height=None, us=None, vs=None, scale=None):
    L = hs._lib.load()
    h, w = u.shape
    return L.hsflow_color_flow_host(u.ctypes.data, u.strides[0] if us is None else us, v.ctypes.data, v.strides[0] if vs is None else vs,
                                    w if width is None else width, h if height is None else height, ctypes.byref(cp) if cp is not None else None,
                                    rgb.ctypes.data if rgb is not None else None, stride, scale)


@pytest.mark.parametrize("width", [1, 3, 5])
def test_strides_and_canary(hs, width):
    rng = np.random.default_rng(width)
    H = 4
    big_u = rng.standard_normal((H, width + 3)).astype(np.float32)
    big_v = rng.standard_normal((H, width + 2)).astype(np.float32)
    u, v = big_u[:, :width], big_v[:, :width]
    want = hs.color_flow_host(np.ascontiguousarray(u), np.ascontiguousarray(v))
    for pad in (0, 1, 5):
        stride = 3 * width + pad
        buf = np.full(H * stride + 7, 0xA5, np.uint8)
        cp = hs.make_color_params()
        m = ctypes.c_float()
        assert raw(hs, u, v, cp, buf, stride, scale=ctypes.byref(m)) == hs._lib.OK
        rows = buf[:H * stride].reshape(H, stride)
        assert np.array_equal(rows[:, :3 * width].reshape(H, width, 3), want)
        assert (rows[:, 3 * width:] == 0xA5).all() and (buf[H * stride:] == 0xA5).all()
        assert m.value > 0


def test_argument_errors(hs):
    E = hs._lib
    u = np.ones((2, 4), np.float32)
    v = np.ones((2, 4), np.float32)
    rgb = np.zeros((2, 12), np.uint8)
    cp = hs.make_color_params()
    assert cp.struct_size == ctypes.sizeof(hs.HsflowColorParams) == 16 and cp.scale_mode == hs.COLOR_SCALE_AUTO
    assert raw(hs, u, v, cp, rgb, 12) == E.OK
    assert raw(hs, u, v, None, rgb, 12) == E.E_ARG
    assert raw(hs, u, v, cp, None, 12) == E.E_ARG
    L = E.load()
    assert L.hsflow_color_flow_host(None, 16, v.ctypes.data, 16, 4, 2, ctypes.byref(cp), rgb.ctypes.data, 12, None) == E.E_ARG
    assert L.hsflow_color_flow_host(u.ctypes.data, 16, None, 16, 4, 2, ctypes.byref(cp), rgb.ctypes.data, 12, None) == E.E_ARG
    assert raw(hs, u, v, cp, rgb, 11) == E.E_SIZE
    assert raw(hs, u, v, cp, rgb, 12, us=12) == E.E_SIZE
    assert raw(hs, u, v, cp, rgb, 12, width=0) == E.E_SIZE
    assert raw(hs, u, v, cp, rgb, 12, height=-1) == E.E_SIZE
    bad = hs.make_color_params()
    bad.struct_size = 12
    assert raw(hs, u, v, bad, rgb, 12) == E.E_ARG
    bad = hs.make_color_params()
    bad.scale_mode = 2
    assert raw(hs, u, v, bad, rgb, 12) == E.E_ARG
    for mf in (0.0, -1.0, np.inf, np.nan):
        assert raw(hs, u, v, hs.make_color_params(mf), rgb, 12) == E.E_ARG
    assert raw(hs, u, v, hs.make_color_params(1e-45), rgb, 12) == E.OK  # a denormal scale is finite and > 0
    with pytest.raises(hs.HsflowError):
        hs.color_flow_host(u, v, max_flow=-3.0)
    with pytest.raises(ValueError):
        hs.color_flow_host(u, v[:1])
