"""The host side of the coarse-to-fine solve: hsflow_pyramid_plan, and the two rules of csrc/hs_pyramid_rule.h on the host
(hsflow_pyramid_down_host, hsflow_pyramid_prolong_host), held to NumPy restatements; the rule header under sanitizers; and
the whole scheme composed from the host rules, hsflow_warp_host and the CPU oracle's solve, which must find a shift that
one solve cannot.  No GPU work: the device side is held to these rules by tests/test_gpu_pyramid.py."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

F = np.float32
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (67, 45), (160, 128)]  # (W, H)


# ---- restatements -----------------------------------------------------------------------------------------------------------

def down_np(img):
    """`down` in int64 NumPy: the 25 taps of every output pixel summed at once."""
    H, W = img.shape
    h, w = (H + 1) // 2, (W + 1) // 2
    k = np.array([1, 4, 6, 4, 1], np.int64)
    ys = np.clip(2 * np.arange(h)[:, None] + np.arange(-2, 3)[None, :], 0, H - 1)  # (h, 5)
    xs = np.clip(2 * np.arange(w)[:, None] + np.arange(-2, 3)[None, :], 0, W - 1)  # (w, 5)
    taps = img.astype(np.int64)[ys[:, None, :, None], xs[None, :, None, :]]      # (h, w, 5, 5)
    total = (taps * k[None, None, :, None] * k[None, None, None, :]).sum(axis=(2, 3))
    return ((total + 128) >> 8).astype(np.uint8)


def prolong_np(c, W, H):
    """`prolong` in fp32 NumPy, every operation an array operation of type float32 and so rounded on its own."""
    c = np.asarray(c, F)

    def axis(a, n, ax):
        i = np.arange(n)
        k0 = i >> 1
        k1 = np.minimum(k0 + 1, a.shape[ax] - 1)
        lo, hi = np.take(a, k0, ax), np.take(a, k1, ax)
        shape = [1, 1]
        shape[ax] = n
        with np.errstate(invalid="ignore", over="ignore"):
            mid = ((lo + hi).astype(F) * F(0.5)).astype(F)
        return np.where((i & 1).astype(bool).reshape(shape), mid, lo)

    with np.errstate(invalid="ignore", over="ignore"):
        return (F(2) * axis(axis(c, W, 1), H, 0)).astype(F)


def padded(rng, W, H, dtype, pad):
    """A random (H, W) array as a view into rows `pad` elements longer, and the whole buffer."""
    if dtype == np.uint8:
        whole = rng.integers(0, 256, (H, W + pad), dtype=np.uint8)
    else:
        whole = (rng.standard_normal((H, W + pad)) * 7).astype(F)
    return whole[:, :W], whole


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the composition every pyramid test shares -------------------------------------------------------------------------------

def warp_step(hs, curr, u0, v0):
    """The warped frame of a step: the warp rule with one channel, t = 1, REPLICATE; an unknown pixel keeps curr's byte."""
    w = hs.warp_host(u0, v0, curr, border="replicate")
    with np.errstate(invalid="ignore"):
        unknown = np.isnan(u0) | np.isnan(v0) | (np.abs(u0) > F(1e9)) | (np.abs(v0) > F(1e9))
    return np.where(unknown, curr, w).astype(np.uint8)


def compose(hs, prev, curr, sizes, warps, median_radius, solve):
    """The scheme of include/hsflow.h from the host rules.  solve(level, step, prev_l, frame) -> (du, dv) float32.
    Returns the per-level lists (prevs, currs, totals) with totals[l] = (u, v) after the level's last step."""
    n = len(sizes)
    prevs, currs = [prev], [curr]
    for l in range(1, n):
        prevs.append(hs.pyramid_down_host(prevs[-1]))
        currs.append(hs.pyramid_down_host(currs[-1]))
        assert prevs[-1].shape == (sizes[l][1], sizes[l][0])
    totals = [None] * n
    u = v = None
    for l in range(n - 1, -1, -1):
        W, H = sizes[l]
        for k in range(warps):
            if l == n - 1 and k == 0:
                u, v = solve(l, k, prevs[l], currs[l])
            else:
                if k == 0:
                    u0, v0 = hs.pyramid_prolong_host(u, W, H), hs.pyramid_prolong_host(v, W, H)
                else:
                    u0, v0 = u, v
                du, dv = solve(l, k, prevs[l], warp_step(hs, currs[l], u0, v0))
                with np.errstate(invalid="ignore", over="ignore"):
                    u, v = (u0 + du).astype(F), (v0 + dv).astype(F)
            if median_radius:
                u, v, _, _ = hs.median_host(u, v, radius=median_radius)
        totals[l] = (u, v)
    return prevs, currs, totals


def interior_epe(u, v, dx, dy, m=16):
    e = np.sqrt((u.astype(np.float64) - dx) ** 2 + (v.astype(np.float64) - dy) ** 2)[m:-m, m:-m]
    return float(e.mean())


# ---- the plan ---------------------------------------------------------------------------------------------------------------

def plan_rule(W, H, levels=0, min_size=32):
    out = [(W, H)]
    while len(out) < (levels or 8):
        w, h = (out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2
        if not levels and min(w, h) < min_size:
            break
        out.append((w, h))
    return out


def test_version_and_defaults(hs):
    assert hs._lib.load().hsflow_version() >= 21
    pp = hs.make_pyramid_params()
    assert ctypes.sizeof(pp) == 20 and pp.struct_size == 20
    assert (pp.levels, pp.min_size, pp.warps, pp.median_radius) == (0, 32, 1, 0)
    hs._lib.load().hsflow_default_pyramid_params(None)


def test_plan(hs):
    assert hs.pyramid_plan(160, 128) == [(160, 128), (80, 64), (40, 32)]
    assert hs.pyramid_plan(161, 127) == [(161, 127), (81, 64), (41, 32)]
    assert len(hs.pyramid_plan(1920, 1080)) == 6
    assert hs.pyramid_plan(1, 1) == [(1, 1)]
    for W, H in [(160, 128), (161, 127), (1920, 1080), (1, 1), (600, 480), (33, 9), (31, 500), (70000, 64)]:
        assert hs.pyramid_plan(W, H) == plan_rule(W, H), (W, H)
        for ms in (1, 8, 100):
            assert hs.pyramid_plan(W, H, min_size=ms) == plan_rule(W, H, min_size=ms), (W, H, ms)
    assert len(hs.pyramid_plan(1 << 20, 1 << 20, min_size=1)) == 8  # the cap
    assert hs.pyramid_plan(33, 9, levels=3) == [(33, 9), (17, 5), (9, 3)]
    assert hs.pyramid_plan(3, 2, levels=3) == [(3, 2), (2, 1), (1, 1)]
    assert hs.pyramid_plan(1, 1, levels=1) == [(1, 1)]


def test_plan_refusals(hs):
    lib = hs._lib.load()
    n = ctypes.c_int(0)
    ws = (ctypes.c_int * 8)()

    def call(W, H, pp, levels=n):
        return lib.hsflow_pyramid_plan(W, H, ctypes.byref(pp) if pp is not None else None, ctypes.byref(levels) if levels is not None else None, ws, None)

    for W, H, lv in [(3, 2, 4), (1, 1, 2), (160, 128, 8)]:  # explicit levels beyond 1 x 1 (160 x 128 reaches it at the 9th)
        st = call(W, H, hs.make_pyramid_params(levels=lv))
        assert st == (hs._lib.E_SIZE if (W, H) != (160, 128) else hs._lib.OK), (W, H, lv)
    assert call(256, 256, hs.make_pyramid_params(levels=8)) == hs._lib.OK and n.value == 8
    assert call(127, 127, hs.make_pyramid_params(levels=8)) == hs._lib.OK  # 127, 64, 32, 16, 8, 4, 2, 1
    assert call(63, 63, hs.make_pyramid_params(levels=8)) == hs._lib.E_SIZE
    for W, H in [(0, 5), (5, 0), (-1, 5)]:
        assert call(W, H, hs.make_pyramid_params()) == hs._lib.E_SIZE
    assert call(64, 64, None) == hs._lib.E_ARG
    assert call(64, 64, hs.make_pyramid_params(), levels=None) == hs._lib.E_ARG
    bad = hs.make_pyramid_params()
    bad.struct_size = 16
    assert call(64, 64, bad) == hs._lib.E_ARG
    for kw in ({"levels": -1}, {"levels": 9}, {"min_size": 0}, {"warps": 0}, {"warps": 9}, {"median_radius": -1}, {"median_radius": 3}):
        assert call(64, 64, hs.make_pyramid_params(**kw)) == hs._lib.E_ARG, kw
        with pytest.raises(hs.HsflowError) as e:
            hs.pyramid_plan(64, 64, **kw)
        assert e.value.status == hs._lib.E_ARG


# ---- down -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SHAPES)
def test_down_against_int64_restatement(hs, W, H):
    rng = np.random.default_rng(100 * W + H)
    for pad in (0, 5):
        img, _ = padded(rng, W, H, np.uint8, pad)
        out, whole = padded(rng, (W + 1) // 2, (H + 1) // 2, np.uint8, pad)
        before = whole.copy()
        got = hs.pyramid_down_host(img, out=out)
        assert got is out and np.array_equal(out, down_np(img)), (W, H, pad)
        assert np.array_equal(whole[:, out.shape[1]:], before[:, out.shape[1]:])  # nothing beyond a row's ceil(W/2) bytes
    for value in (0, 1, 127, 255):
        assert np.all(hs.pyramid_down_host(np.full((H, W), value, np.uint8)) == value)


def test_down_refusals(hs):
    lib = hs._lib.load()
    a, b = np.zeros((4, 6), np.uint8), np.zeros((2, 3), np.uint8)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)
    assert lib.hsflow_pyramid_down_host(p(a), 6, 6, 4, p(b), 3) == hs._lib.OK
    assert lib.hsflow_pyramid_down_host(None, 6, 6, 4, p(b), 3) == hs._lib.E_ARG
    assert lib.hsflow_pyramid_down_host(p(a), 6, 6, 4, None, 3) == hs._lib.E_ARG
    assert lib.hsflow_pyramid_down_host(p(a), 5, 6, 4, p(b), 3) == hs._lib.E_SIZE
    assert lib.hsflow_pyramid_down_host(p(a), 6, 6, 4, p(b), 2) == hs._lib.E_SIZE
    assert lib.hsflow_pyramid_down_host(p(a), 6, 0, 4, p(b), 3) == hs._lib.E_SIZE
    assert lib.hsflow_pyramid_down_host(p(a), 6, 6, 0, p(b), 3) == hs._lib.E_SIZE


# ---- prolong ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("Wc,Hc", SHAPES)
def test_prolong_against_fp32_restatement(hs, Wc, Hc):
    rng = np.random.default_rng(7 + 100 * Wc + Hc)
    for odd in (0, 1):
        W, H = 2 * Wc - odd, 2 * Hc - odd
        for pad in (0, 3):
            c, _ = padded(rng, Wc, Hc, F, pad)
            out, whole = padded(rng, W, H, F, pad)
            before = whole.copy()
            hs.pyramid_prolong_host(c, W, H, out=out)
            assert np.array_equal(bits(out), bits(prolong_np(c, W, H))), (W, H, pad)
            assert np.array_equal(bits(whole[:, W:]), bits(before[:, W:]))
        for value in (F(0), F(-0.0), F(1.5), F(-3e37), F(1e-40)):
            got = hs.pyramid_prolong_host(np.full((Hc, Wc), value, F), W, H)
            assert np.array_equal(bits(got), bits(np.full((H, W), F(2) * value, F))), (W, H, value)


def test_prolong_special_values_stay_single_pixels(hs):
    """Even positions copy: a NaN or an Inf of the coarse plane reaches ONE even fine position, and of the odd ones only
    those next to it."""
    Wc, Hc, r, k = 9, 7, 3, 4
    for W, H in [(18, 14), (17, 13)]:
        for special in (F(np.nan), F(np.inf), F(-np.inf)):
            c = np.arange(Wc * Hc, dtype=F).reshape(Hc, Wc)
            c[r, k] = special
            out = hs.pyramid_prolong_host(c, W, H)
            hit = ~np.isfinite(out)
            want = np.zeros((H, W), bool)
            want[2 * r - 1:2 * r + 2, 2 * k - 1:2 * k + 2] = True
            assert np.array_equal(hit, want)
            assert hit[::2, ::2].sum() == 1 and hit[2 * r, 2 * k]
            assert np.array_equal(bits(out), bits(prolong_np(c, W, H)))
    # opposite infinities side by side: each stays where it is, only the odd position between them is NaN
    c = np.zeros((1, 3), F)
    c[0, 0], c[0, 1] = np.inf, -np.inf
    out = hs.pyramid_prolong_host(c, 6, 1)[0]
    assert out[0] == np.inf and np.isnan(out[1]) and out[2] == -np.inf and out[3] == -np.inf and out[4] == 0 and out[5] == 0
    # the doubling overflows where it must, and nowhere else
    out = hs.pyramid_prolong_host(np.full((1, 1), F(2e38), F), 2, 2)
    assert np.all(np.isinf(out))


def test_prolong_refusals(hs):
    lib = hs._lib.load()
    c, d = np.zeros((2, 3), F), np.zeros((4, 6), F)
    p = lambda x: ctypes.c_void_p(x.ctypes.data)
    assert lib.hsflow_pyramid_prolong_host(p(c), 12, 6, 4, p(d), 24) == hs._lib.OK
    assert lib.hsflow_pyramid_prolong_host(p(c), 12, 5, 3, p(d), 24) == hs._lib.OK
    assert lib.hsflow_pyramid_prolong_host(None, 12, 6, 4, p(d), 24) == hs._lib.E_ARG
    assert lib.hsflow_pyramid_prolong_host(p(c), 12, 6, 4, None, 24) == hs._lib.E_ARG
    assert lib.hsflow_pyramid_prolong_host(p(c), 8, 6, 4, p(d), 24) == hs._lib.E_SIZE
    assert lib.hsflow_pyramid_prolong_host(p(c), 12, 6, 4, p(d), 20) == hs._lib.E_SIZE
    assert lib.hsflow_pyramid_prolong_host(p(c), 14, 6, 4, p(d), 24) == hs._lib.E_SIZE
    assert lib.hsflow_pyramid_prolong_host(p(c), 12, 6, 4, p(d), 26) == hs._lib.E_SIZE
    assert lib.hsflow_pyramid_prolong_host(p(c), 12, 0, 4, p(d), 24) == hs._lib.E_SIZE


# ---- the rule header under sanitizers ----------------------------------------------------------------------------------------

def lcg(seed, n):
    out = np.empty(n, np.uint32)
    x = seed & 0xFFFFFFFF
    for i in range(n):
        x = (x * 1664525 + 1013904223) & 0xFFFFFFFF
        out[i] = x
    return out


def fnv(h, data):
    for b in data.tobytes():
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h


def test_rule_under_sanitizers(hs, tmp_path):
    """tests/pyramid_rule_asan_main.cpp, a stand-alone program that includes csrc/hs_pyramid_rule.h, under AddressSanitizer
    and UBSan: every shape in exact-size heap blocks; what it computes is what the library computes."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    main = os.path.join(ROOT, "tests", "pyramid_rule_asan_main.cpp")
    exe = str(tmp_path / "pyramid_rule")
    base = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    # the runtimes linked into the program where the compiler has them as archives; the environment is left as it is
    for flags in (base + ["-static-libasan", "-static-libubsan"], base):
        if subprocess.run([gxx] + flags + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True).returncode == 0:
            break
    else:
        pytest.skip("the sanitizer runtimes do not link here")
    if subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, timeout=60).returncode != 0:
        pytest.skip("a sanitized program does not start in this environment (the runtime's link-order check)")
    r = subprocess.run([gxx] + flags + ["-Wall", "-Wextra", "-I", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), main, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(SHAPES) + 1
    for line, (W, H) in zip(lines, SHAPES):
        x = lcg(12345 + 1000 * W + H, 2 * W * H)
        img = (x[:W * H] >> 24).astype(np.uint8).reshape(H, W)
        c = (((x[W * H:] >> 16).astype(np.int64) - 32768).astype(F) / F(64)).astype(F).reshape(H, W)
        hd = fnv(2166136261, hs.pyramid_down_host(img))
        hp = 2166136261
        for odd in (0, 1):
            hp = fnv(hp, hs.pyramid_prolong_host(c, 2 * W - odd, 2 * H - odd))
        assert line == "%d %d %08x %08x" % (W, H, hd, hp), (W, H)
    assert lines[-1] == "plan 3 6 1 0"


# ---- the scheme is worth having -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", [(160, 128), (161, 127)])
def test_scheme_finds_a_shift_one_solve_cannot(hs, oracle, W, H):
    """A (5, -3) px shift, lambda 0.003, ITER 100, auto levels, one warp, every increment solved by the CPU oracle: the
    interior mean end-point error is below 1 px and below a quarter of the one-level solve's (the NumPy model of the
    scheme measured 0.247 against 5.48 px, 22 x: the factor 4 is margin)."""
    from opticalflowhs_amd import synth
    dx, dy, lam, iters = 5.0, -3.0, 0.003, 100
    A, B = synth.translating_pair(W, H, seed=1, dx=dx, dy=dy)

    def solve(level, step, prev, frame):
        u, v = oracle.calc_optical_flow_hs(prev, frame, lam, iters, term_type=oracle.TERMCRIT_ITER)
        return np.asarray(u, F), np.asarray(v, F)

    sizes = hs.pyramid_plan(W, H)
    assert len(sizes) == 3
    _, _, totals = compose(hs, A, B, sizes, 1, 0, solve)
    one = interior_epe(*solve(0, 0, A, B), dx, dy)
    pyr = interior_epe(*totals[0], dx, dy)
    print("%dx%d: interior mean EPE one level %.3f px, pyramid %.3f px (%.1f x)" % (W, H, one, pyr, one / pyr))
    assert pyr < 1.0 and pyr < one / 4
