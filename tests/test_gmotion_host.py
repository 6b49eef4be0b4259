"""CPU checks of the global-motion rule (csrc/hs_gmotion_rule.h through hsflow_gmotion_*_host): the host forms are held to
the NumPy restatement of tests/gmotion_ref.py bit for bit, to float64 least squares within a bound the test works out,
and to hsflow_warp_host for the warp by a model.  No GPU work here."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gmotion_ref as G
from conftest import ROOT

F = np.float32
VALUES = (200, 90, 40, 7)


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def host_fit(hs, u, v, state, gp, pad=0):
    """hsflow_gmotion_fit_host on planes whose rows are `pad` elements longer than the width: (result, mask, ru bits, rv bits),
    after checking that nothing beyond a row's width was written."""
    H, W = u.shape
    uu, _ = G.padded(u, pad, F(7.0))
    vv, _ = G.padded(v, pad, F(-3.0))
    ss = G.padded(state, pad, 0)[0] if state is not None else None
    mask, mw = G.padded(np.zeros((H, W), np.uint8), pad, 0xA5)
    ru, ruw = G.padded(np.zeros((H, W), F), pad, F(123.0))
    rv, rvw = G.padded(np.zeros((H, W), F), pad, F(123.0))
    res = hs.HsflowGmotionResult()
    st = hs._lib.load().hsflow_gmotion_fit_host(ptr(uu), ptr(vv), uu.strides[0], ptr(ss) if ss is not None else None, ss.strides[0] if ss is not None else 0, W, H,
                                                 ctypes.byref(gp), ptr(mask), mask.strides[0], ptr(ru), ptr(rv), ru.strides[0], ctypes.byref(res))
    assert st == 0, hs._lib.load().hsflow_last_error(None)
    assert (mw[:, W:] == 0xA5).all() and (ruw[:, W:] == F(123.0)).all() and (rvw[:, W:] == F(123.0)).all()
    return res, mask.copy(), ru.view(np.uint32).copy(), rv.view(np.uint32).copy()


def same_as_restatement(res, mask, ru, rv, ref):
    assert np.array_equal(np.array(res.p[:], F).view(np.uint32), ref["p"].view(np.uint32)), (list(res.p), ref["p"])
    assert F(res.threshold).view(np.uint32) == F(ref["thr"]).view(np.uint32), (res.threshold, ref["thr"])
    assert res.flags == ref["flags"]
    assert list(res.cls) == ref["cls"]
    assert np.array_equal(mask, ref["mask"])
    assert np.array_equal(ru, ref["ru"]) and np.array_equal(rv, ref["rv"])


# ---- H1. version, structs, defaults, errors ------------------------------------------------------------------------------------

def test_version_structs_defaults(hs):
    L = hs._lib.load()
    assert L.hsflow_version() >= 23
    text = open(os.path.join(ROOT, "include", "hsflow.h")).read()
    assert int(re.search(r"#define HSFLOW_VERSION_MINOR (\d+)", text).group(1)) >= 23
    assert ctypes.sizeof(hs.HsflowGmotionParams) == 40 and ctypes.sizeof(hs.HsflowGmotionResult) == 64
    gp = hs.HsflowGmotionParams()
    L.hsflow_default_gmotion_params(ctypes.byref(gp))
    L.hsflow_default_gmotion_params(None)
    assert gp.struct_size == 40 and gp.model == hs.GMOTION_AFFINE and gp.passes == 3 and gp.threshold_mode == hs.GMOTION_THRESHOLD_FIXED
    assert gp.inlier_px == 1.0 and gp.scale2 == 6.0 and gp.min_thr2 == 0.0625 and list(gp.value) == [255, 0, 0, 0] and list(gp.reserved) == [0, 0]
    for name, val in (("TRANSLATION", 0), ("SIMILARITY", 1), ("AFFINE", 2), ("ZERO", 3), ("THRESHOLD_FIXED", 0), ("THRESHOLD_AUTO", 1), ("INLIER", 0),
                      ("OUTLIER", 1), ("UNTRUSTED", 2), ("UNKNOWN", 3), ("MAX_PASSES", 8), ("MAX_SIDE", 16384)):
        assert int(re.search(r"#define HSFLOW_GMOTION_%s (\d+)" % name, text).group(1)) == val == getattr(hs, "GMOTION_" + name)


def test_every_documented_error(hs):
    L = hs._lib.load()
    E_ARG, E_SIZE = hs._lib.E_ARG, hs._lib.E_SIZE
    W, H = 12, 5
    u, v, state = G.field(W, H, 1)
    mask = np.zeros((H, W), np.uint8)
    ru, rv = np.zeros((H, W), F), np.zeros((H, W), F)
    res = hs.HsflowGmotionResult()

    def call(gp=None, u_=u, v_=v, fs=4 * W, s=state, ss=W, w=W, h=H, m=mask, ms=W, a=ru, b=rv, rs=4 * W, r=res, null_gp=False):
        gp = gp if gp is not None else hs.make_gmotion_params()
        opt = lambda x: ptr(x) if isinstance(x, np.ndarray) else x
        return L.hsflow_gmotion_fit_host(opt(u_), opt(v_), fs, opt(s), ss, w, h, None if null_gp else ctypes.byref(gp), opt(m), ms, opt(a), opt(b), rs,
                                         ctypes.byref(r) if r is not None else None)
    assert call() == 0
    assert call(null_gp=True) == E_ARG
    bad = hs.make_gmotion_params()
    bad.struct_size = 36
    assert call(bad) == E_ARG
    for field_, val in (("model", 3), ("model", -1), ("passes", 0), ("passes", 9), ("threshold_mode", 2), ("inlier_px", 0.0), ("inlier_px", -1.0),
                        ("inlier_px", float("nan")), ("inlier_px", float("inf")), ("inlier_px", 1e-30), ("inlier_px", 1e30)):
        gp = hs.make_gmotion_params()
        setattr(gp, field_, val)
        assert call(gp) == E_ARG, (field_, val)
    for field_, val in (("scale2", 0.0), ("scale2", float("nan")), ("scale2", 2e6), ("min_thr2", 0.0), ("min_thr2", float("inf")), ("min_thr2", -1.0)):
        gp = hs.make_gmotion_params(threshold="auto")
        setattr(gp, field_, val)
        assert call(gp) == E_ARG, (field_, val)
    gp = hs.make_gmotion_params()
    gp.reserved[1] = 1
    assert call(gp) == E_ARG
    assert call(u_=None) == E_ARG and call(v_=None) == E_ARG
    assert call(u_=ctypes.c_void_p(u.ctypes.data + 2)) == E_ARG                       # misaligned flow plane
    assert call(a=ctypes.c_void_p(ru.ctypes.data + 1)) == E_ARG                       # misaligned residual plane
    assert call(b=None) == E_ARG and call(a=None) == E_ARG                            # one residual plane without the other
    assert call(m=None, a=None, b=None, r=None) == E_ARG                              # nothing asked for
    assert call(m=None, a=None, b=None) == 0 and call(a=None, b=None, r=None) == 0 and call(m=None, r=None) == 0
    assert call(a=u) == E_ARG and call(m=state) == E_ARG                              # an output over an input
    assert call(w=0) == E_SIZE and call(h=-1) == E_SIZE
    assert call(w=16385, fs=4 * 16385, ms=16385, rs=4 * 16385, ss=16385) == E_SIZE and call(h=16385) == E_SIZE
    assert call(fs=4 * W - 4) == E_SIZE and call(fs=4 * W + 2) == E_SIZE
    assert call(rs=4 * W - 4) == E_SIZE and call(rs=4 * W + 2) == E_SIZE
    assert call(ms=W - 1) == E_SIZE and call(ss=W - 1) == E_SIZE
    assert b"" != L.hsflow_last_error(None)
    # the warp by a model, compose and invert
    wp = hs.make_warp_params(1)
    src, dst = np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)
    m6 = (ctypes.c_float * 6)(0.5, 0, 0, 0, 0, 0)
    nanm = (ctypes.c_float * 6)(float("nan"), 0, 0, 0, 0, 0)
    warp = lambda model=m6, s=src, d=dst, w=W, ss=W, ds=W: L.hsflow_gmotion_warp_host(model, w, H, ctypes.byref(wp), ptr(s) if s is not None else None, ss, None, 0,
                                                                                        ptr(d) if d is not None else None, ds, None)
    assert warp() == 0
    assert warp(model=None) == E_ARG and warp(model=nanm) == E_ARG and warp(s=None) == E_ARG and warp(d=None) == E_ARG and warp(d=src) == E_ARG
    assert warp(w=0) == E_SIZE and warp(ss=W - 1) == E_SIZE and warp(ds=W - 1) == E_SIZE
    out = (ctypes.c_float * 6)()
    assert L.hsflow_gmotion_compose_host(None, m6, out) == E_ARG and L.hsflow_gmotion_compose_host(m6, nanm, out) == E_ARG
    assert L.hsflow_gmotion_compose_host(m6, m6, None) == E_ARG and L.hsflow_gmotion_invert_host(m6, None) == E_ARG
    singular = (ctypes.c_float * 6)(1, -1, 0, 2, 0, 3)                                 # I + L has a zero row
    assert L.hsflow_gmotion_invert_host(singular, out) == E_ARG
    singular2 = (ctypes.c_float * 6)(0, 1, 2, 0, 1, 0)                                # [[2, 2], [1, 1]]
    assert L.hsflow_gmotion_invert_host(singular2, out) == E_ARG


# ---- H2. bit equality with the restatement ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", G.SHAPES + G.SMALL)
@pytest.mark.parametrize("kind", [G.TRANSLATION, G.SIMILARITY, G.AFFINE])
@pytest.mark.parametrize("mode", [G.FIXED, G.AUTO])
def test_bit_equality(hs, W, H, kind, mode):
    u, v, state = G.field(W, H, seed=100 * W + H)
    for passes in (1, 3):
        for use_state, pad in ((True, 3), (False, 0)):
            s = state if use_state else None
            gp = hs.make_gmotion_params(kind, passes, mode, inlier_px=0.8, scale2=5.0, min_thr2=0.01, values=VALUES)
            ref = G.fit(u, v, s, kind, passes, mode, 0.8, 5.0, 0.01, VALUES)
            same_as_restatement(*host_fit(hs, u, v, s, gp, pad), ref)
            assert sum(ref["cls"]) == W * H
    if W * H >= 40:
        assert ref["cls"][3] >= 10      # the NaN, Inf, > 1e9 and > kMaxFlow pixels are UNKNOWN; +-kMaxFlow itself is not
        at = np.argwhere(np.abs(u) == 2048.0)
        assert len(at) == 2 and all(ref["classes"][y, x] != 3 or not np.isfinite(v[y, x]) or abs(v[y, x]) > 2048 for y, x in at)


def test_a_pixel_exactly_at_the_threshold_is_an_inlier(hs):
    """AUTO, one pass: min_thr2 is set to the r2 of a pixel above the histogram's threshold, which makes it T itself."""
    W, H = 37, 29
    u, v, state = G.field(W, H, seed=5)
    first = G.fit(u, v, state, G.AFFINE, 1, G.AUTO, scale2=1.0, min_thr2=1e-6)
    r2 = G.residual(u, v, first["p"])[2]
    cand = np.argwhere((first["classes"] == 1) & (r2 > first["thr"]) & (r2 < 4 * first["thr"]))
    y, x = cand[0]
    gp = hs.make_gmotion_params("affine", 1, "auto", scale2=1.0, min_thr2=float(r2[y, x]), values=VALUES)
    res, mask, ru, rv = host_fit(hs, u, v, state, gp)
    assert F(res.threshold) == r2[y, x] and mask[y, x] == VALUES[0]
    same_as_restatement(res, mask, ru, rv, G.fit(u, v, state, G.AFFINE, 1, G.AUTO, scale2=1.0, min_thr2=float(r2[y, x]), value=VALUES))
    # FIXED, three passes: a translation whose mean is exact, and pixels exactly inlier_px away on either side
    u = np.full((8, 16), 3.25, F)
    v = np.full((8, 16), -1.5, F)
    u[2, 3:7] += F(1.0)
    u[5, 3:7] -= F(1.0)
    res, mask, _, _ = host_fit(hs, u, v, None, hs.make_gmotion_params("translation", 3, "fixed", inlier_px=1.0))
    assert list(res.p) == [3.25, 0, 0, -1.5, 0, 0] and res.threshold == 1.0 and list(res.cls) == [128, 0, 0, 0] and (mask == 255).all()


# ---- H3. accuracy against float64 least squares ---------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", [G.FIXED, G.AUTO])
def test_accuracy_with_a_planted_block_of_outliers(hs, mode):
    W, H = 120, 80
    Xi, Yi = G.coords(W, H)
    X, Y = np.broadcast_to(Xi * 0.5, (H, W)), np.broadcast_to(Yi * 0.5, (H, W))
    true = np.array([1.25, 0.0125, -0.00625, -0.5, 0.0078125, 0.015625])
    u = (true[0] + true[1] * X + true[2] * Y).astype(F)
    v = (true[3] + true[4] * X + true[5] * Y).astype(F)
    planted = np.zeros((H, W), bool)
    planted[18:62, 27:93] = True                                                      # 44 x 66 = 2904 of 9600 pixels: 30 %
    assert abs(planted.mean() - 0.30) < 0.005
    rng = np.random.default_rng(3)
    u[planted] += (6.0 + rng.random(planted.sum())).astype(F)                         # displaced by at least 6 px in u and 6 in v
    v[planted] -= (6.0 + rng.random(planted.sum())).astype(F)
    px, scale2, min_thr2 = 4.0, 2.0, 0.0625
    # on the CPU first: under the model of pass 0 the threshold of pass 1 separates the two populations, so for AUTO the median lies among the inliers
    first = G.fit(u, v, None, G.AFFINE, 1, mode, px, scale2, min_thr2)
    r2 = G.residual(u, v, first["p"])[2]
    assert r2[~planted].max() <= first["thr"] < r2[planted].min(), (r2[~planted].max(), first["thr"], r2[planted].min())
    res, mask, _, _ = host_fit(hs, u, v, None, hs.make_gmotion_params("affine", 3, mode, px, scale2, min_thr2))
    assert np.array_equal(mask == 255, ~planted) and list(res.cls) == [int((~planted).sum()), int(planted.sum()), 0, 0]
    sel = ~planted
    A = np.stack([np.ones(sel.sum()), X[sel], Y[sel]], axis=1)
    N = np.linalg.inv(A.T @ A)
    p = np.array(res.p[:], np.float64)
    for which, plane in ((0, u), (3, v)):
        theta = np.linalg.lstsq(A, plane[sel].astype(np.float64), rcond=None)[0]
        for cx, cy in ((X[0, 0], Y[0, 0]), (X[0, -1], Y[0, -1]), (X[-1, 0], Y[-1, 0]), (X[-1, -1], Y[-1, -1])):
            z = np.array([1.0, cx, cy])
            quant = np.abs(A @ (N @ z)).sum() / 512.0                                 # every flow moves by at most half a quantisation step
            rounding = 2.0 ** -24 * (abs(theta[0]) + abs(theta[1] * cx) + abs(theta[2] * cy))   # the parameters rounded to fp32
            got = p[which] + p[which + 1] * cx + p[which + 2] * cy
            print("corner", cx, cy, "error", abs(got - z @ theta), "bound", quant + rounding)
            assert abs(got - z @ theta) <= quant + rounding


# ---- H4. degenerate sets and extremes -------------------------------------------------------------------------------------------

def degenerate_fields():
    W, H = 21, 17
    nan = np.full((H, W), np.nan, F)
    base_u, base_v, _ = G.field(W, H, 9, specials=False, with_state=False)
    out = {}
    out["none"] = (nan.copy(), nan.copy(), G.ZERO)
    for name, keep, used in (("one", (slice(4, 5), slice(6, 7)), G.TRANSLATION), ("row", (slice(5, 6), slice(None)), G.SIMILARITY),
                             ("column", (slice(None), slice(10, 11)), G.SIMILARITY)):
        u, v = nan.copy(), nan.copy()
        u[keep], v[keep] = base_u[keep], base_v[keep]
        out[name] = (u, v, used)
    u, v = nan.copy(), nan.copy()
    for k in range(H):
        u[k, k + 2], v[k, k + 2] = base_u[k, k + 2], base_v[k, k + 2]
    out["diagonal"] = (u, v, G.SIMILARITY)
    return out


@pytest.mark.parametrize("name", ["none", "one", "row", "column", "diagonal"])
def test_degenerate_sets_fall_back(hs, name):
    u, v, used = degenerate_fields()[name]
    for mode in (G.FIXED, G.AUTO):
        for passes in (1, 3):
            gp = hs.make_gmotion_params("affine", passes, mode, inlier_px=50.0, scale2=1e5, values=VALUES)
            res, mask, ru, rv = host_fit(hs, u, v, None, gp)
            same_as_restatement(res, mask, ru, rv, G.fit(u, v, None, G.AFFINE, passes, mode, 50.0, 1e5, 0.0625, VALUES))
            assert res.flags == (used << 8 | hs.GMOTION_FLAG_FALLBACK)
            if name == "none":
                assert list(res.p) == [0.0] * 6 and res.cls[3] == u.size
    if name in ("row", "column", "diagonal"):   # asked for as a similarity they are no fallback; as a translation neither
        res = host_fit(hs, u, v, None, hs.make_gmotion_params("similarity", 1, "fixed"))[0]
        assert res.flags == G.SIMILARITY << 8
    if name != "none":
        res = host_fit(hs, u, v, None, hs.make_gmotion_params("translation", 1, "fixed"))[0]
        assert res.flags == G.TRANSLATION << 8


@pytest.mark.parametrize("W,H", [(16384, 4), (4, 16384)])
def test_extreme_fields_against_big_integer_sums(hs, W, H):
    rng = np.random.default_rng(W)
    u = np.where(rng.random((H, W)) < 0.5, F(2048.0), F(-2048.0)).astype(F)
    v = np.where(rng.random((H, W)) < 0.5, F(2048.0), F(-2048.0)).astype(F)
    for kind, passes in ((G.AFFINE, 1), (G.SIMILARITY, 2)):
        gp = hs.make_gmotion_params(kind, passes, "fixed", inlier_px=2500.0, values=VALUES)
        same_as_restatement(*host_fit(hs, u, v, None, gp), G.fit(u, v, None, kind, passes, G.FIXED, 2500.0, value=VALUES))
    # the largest sums the rule can meet: one sign everywhere
    u[:], v[:] = F(2048.0), F(-2048.0)
    s = G.sums_of(u, v, np.ones((H, W), bool))
    assert s[6] == W * H * 2 ** 19 and max(abs(x) for x in s) < 2 ** 63
    res = host_fit(hs, u, v, None, hs.make_gmotion_params("affine", 1, "fixed"))[0]
    assert list(res.p) == [2048.0, 0, 0, -2048.0, 0, 0] and res.cls[0] == W * H


# ---- H5. compose, invert, warp by a model -----------------------------------------------------------------------------------------

def as_matrix(p):
    p = np.asarray(p, np.float64)
    return np.array([[1 + p[1], p[2], p[0]], [p[4], 1 + p[5], p[3]], [0, 0, 1]])


def test_compose_and_invert(hs):
    rng = np.random.default_rng(11)
    for _ in range(50):
        m1 = (rng.normal(0, 1, 6) * [20, 0.3, 0.3, 20, 0.3, 0.3]).astype(F)
        m2 = (rng.normal(0, 1, 6) * [20, 0.3, 0.3, 20, 0.3, 0.3]).astype(F)
        M = as_matrix(m2) @ as_matrix(m1)
        want = np.array([M[0, 2], M[0, 0] - 1, M[0, 1], M[1, 2], M[1, 0], M[1, 1] - 1])
        got = hs.gmotion_compose(m1, m2)
        assert got.dtype == F and np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want) + 1e-12 * np.abs(M).max() + 2.0 ** -149)
        I = np.linalg.inv(as_matrix(m1))
        want = np.array([I[0, 2], I[0, 0] - 1, I[0, 1], I[1, 2], I[1, 0], I[1, 1] - 1])
        inv = hs.gmotion_invert(m1)
        assert np.all(np.abs(inv - want) <= 2.0 ** -23 * np.abs(want) + 1e-11 * np.abs(I).max())
        # compose(m, invert(m)) is the identity within the fp32 rounding of the inverse's parameters carried through m
        back = hs.gmotion_compose(m1, inv)
        slack = 2.0 ** -23 * (np.abs(I).max() + 1) * (np.abs(as_matrix(m1)).max() + 1) * 4
        assert np.all(np.abs(back) <= slack), (back, slack)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("border", ["constant", "replicate"])
def test_warp_by_model_equals_warp_by_its_planes(hs, C, border):
    W, H = 45, 31
    rng = np.random.default_rng(C)
    src = rng.integers(0, 256, (H, W) if C == 1 else (H, W, C), dtype=np.uint8)
    ref = rng.integers(0, 256, src.shape, dtype=np.uint8)
    outside = inside = 0
    for model in ([3.25, 0.05, -0.08, -2.5, 0.08, 0.05], [-30.0, 0, 0, 4.0, 0, 0], [0.3, 0.9, 0.2, 0.1, -0.3, 1.4]):
        mu, mv = G.model_planes(model, W, H)
        for t in (1.0, 0.5, -1.0):
            want, ws = hs.warp_host(mu, mv, src, ref=ref, t=t, border=border, fill=(9, 8, 7), return_stats=True)
            got, gs = hs.gmotion_warp_host(model, src, ref=ref, t=t, border=border, fill=(9, 8, 7), return_stats=True)
            assert np.array_equal(got, want)
            assert bytes(gs) == bytes(ws)
            outside, inside = outside + ws.outside, inside + ws.inside
    assert outside > 0 and inside > 0


# ---- H6. the rule under the sanitizers -----------------------------------------------------------------------------------------

def test_rule_under_address_and_ub_sanitizers(tmp_path):
    """tests/gmotion_host_san.cpp includes the rule header alone and runs the host fit and warp on odd shapes and extreme
    fields; built with -fsanitize=address,undefined and run as a child process."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "gmotion_host_san")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                        "-I", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), os.path.join(ROOT, "tests", "gmotion_host_san.cpp"), "-o", exe],
                       capture_output=True, text=True)
    if r.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|unsupported option|libasan|libubsan|libclang_rt", r.stderr):
        pytest.skip("the compiler has no sanitizer runtime")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "gmotion rule: ok" in r.stdout
