"""hsflow_solve_pyramid on the device, held bit for bit to the scheme composed through public entries: the host rules of
tests/test_pyramid_host.py for the frames, the base flow and the warped frame, a fresh one-pair context's solve for every
increment, an fp32 addition, and hsflow_median_host where asked.  Then the state the call leaves behind, the quality of the
flow, the refusals and the command line."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from opticalflowhs_amd import synth
from test_pyramid_host import F, bits, compose, interior_epe

pytestmark = pytest.mark.gpu

LAM = 0.003
SHIFTS = [(5.0, -3.0), (-2.5, 4.0), (0.75, -0.5)]


def pair_of(W, H, shift=SHIFTS[0], seed=1):
    return synth.translating_pair(W, H, seed=seed, dx=shift[0], dy=shift[1])


def device_solve(hs, params, log=None):
    """The increment of one step as any caller would get it: a fresh one-pair context of the level's size."""
    def solve(level, step, prev, frame):
        H, W = prev.shape
        with hs.HSFlow(W, H, 1, own_stream=True) as c:
            c.set_frames(np.ascontiguousarray(prev), np.ascontiguousarray(frame))
            info = c.solve(params)
            if log is not None:
                log[(level, step)] = info["iterations_done"]
            return c.flow()
    return solve


def assert_same(got, want, what):
    for g, w, name in zip(got, want, "uv"):
        diff = bits(g) != bits(w)
        assert not diff.any(), "%s: %s differs at %d of %d values, first at %s" % (what, name, diff.sum(), diff.size, np.argwhere(diff)[0])


def check_against_composition(hs, ctx, frames, params, levels, warps, median, pairs=1, sweeps=None):
    info = ctx.solve_pyramid(params, levels=levels, warps=warps, median_radius=median)
    sizes = hs.pyramid_plan(ctx.width, ctx.height, levels=levels)
    assert info["sizes"] == sizes and info["levels"] == len(sizes) and info["warps"] == warps and info["median_radius"] == median
    assert info["solves"] == len(sizes) * warps and info["down_launches"] == len(sizes) - 1 and info["step_launches"] == info["solves"] - 1
    for pair in range(pairs):
        log = {}
        prevs, currs, totals = compose(hs, frames[pair][0], frames[pair][1], sizes, warps, median, device_solve(hs, params, log))
        assert_same(ctx.flow(pair), totals[0], "pair %d: the context's flow" % pair)
        for l in range(len(sizes)):
            a, b, u, v = ctx.pyramid_level(l, pair)
            assert np.array_equal(a, prevs[l]) and np.array_equal(b, currs[l]), "pair %d level %d: frames" % (pair, l)
            assert_same((u, v), totals[l], "pair %d level %d: total" % (pair, l))
        if sweeps is not None:
            sweeps.append(([[log[(l, k)] for k in range(warps)] for l in range(len(sizes))], info["sweeps"]))
    return info


# ---- 1. bit for bit against the composition -------------------------------------------------------------------------------------

CASES = []
for _shape, _levels in (((67, 45), 2), ((160, 128), 0), ((161, 127), 0), ((320, 256), 4), ((33, 9), 3)):
    CASES.append((_shape, _levels, 1, 0, 0))
    CASES.append((_shape, _levels, 2, 1, 1))
CASES += [((160, 128), 0, 2, 2, 0), ((67, 45), 2, 1, 2, 1), ((161, 127), 0, 2, 0, 0)]


@pytest.mark.parametrize("shape,levels,warps,median,graph", CASES)
def test_iter_bit_for_bit(hs, gpu_ok, shape, levels, warps, median, graph):
    W, H = shape
    A, B = pair_of(W, H)
    params = hs.make_params(lam=LAM, max_iter=40, term_type=hs.TERM_ITER, use_graph=bool(graph))
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        info = check_against_composition(hs, ctx, [(A, B)], params, levels, warps, median)
        assert info["sweeps"] == [[40] * warps] * info["levels"]
        # the same call again on the kept level contexts: the same bits
        first = ctx.flow()
        ctx.solve_pyramid(params, levels=levels, warps=warps, median_radius=median)
        assert_same(ctx.flow(), first, "second call")


@pytest.mark.parametrize("shape,levels,warps,median,graph", [((160, 128), 0, 1, 0, 0), ((160, 128), 0, 2, 1, 1), ((67, 45), 2, 2, 0, 0), ((161, 127), 0, 1, 2, 0)])
def test_iter_eps_bit_for_bit(hs, gpu_ok, shape, levels, warps, median, graph):
    """ITER|EPS with one pair: every level's solve stops where the same solve on a context of its own stops.  Epsilon 0.02
    under a budget of 40 sweeps: with the CPU oracle the coarse levels of these pairs stop after 13 .. 36 sweeps and the finest
    after 42 .. 51, so some solves stop early and some run the budget."""
    W, H = shape
    A, B = pair_of(W, H)
    params = hs.make_params(lam=LAM, max_iter=40, epsilon=0.02, term_type=hs.TERM_ITER | hs.TERM_EPS, use_graph=bool(graph))
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        sweeps = []
        check_against_composition(hs, ctx, [(A, B)], params, levels, warps, median, sweeps=sweeps)
        want, got = sweeps[0]
        print("sweeps per level and step:", got)
        assert got == want
        flat = [s for level in got for s in level]
        assert min(flat) < 40 and max(flat) == 40, "the epsilon of this test is meant to stop some solves early and not all: %r" % (got,)


def test_three_pairs(hs, gpu_ok):
    W, H = 161, 127
    frames = [pair_of(W, H, shift, seed=k + 1) for k, shift in enumerate(SHIFTS)]
    params = hs.make_params(lam=LAM, max_iter=30, term_type=hs.TERM_ITER)
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        for k, (A, B) in enumerate(frames):
            ctx.set_frames(A, B, pair=k)
        check_against_composition(hs, ctx, frames, params, 0, 2, 1, pairs=3)
        for k, (A, B) in enumerate(frames):
            a, b = ctx.frames(k)
            assert np.array_equal(a, A) and np.array_equal(b, B)


# ---- 2. levels = 1 --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("term", ["iter", "iter_eps"])
def test_one_level_is_solve(hs, gpu_ok, term):
    W, H = 161, 127
    A, B = pair_of(W, H, SHIFTS[2])
    params = hs.make_params(lam=1.0, max_iter=60, epsilon=1e-3, term_type=hs.TERM_ITER if term == "iter" else hs.TERM_ITER | hs.TERM_EPS)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx, hs.HSFlow(W, H, 1, own_stream=True) as ref:
        for c in (ctx, ref):
            c.set_frames(A, B)
        ri = ref.solve(params)
        info = ctx.solve_pyramid(params, levels=1)
        assert info["levels"] == 1 and info["step_launches"] == 0 and info["total_launches"] == 0 and info["down_launches"] == 0
        assert_same(ctx.flow(), ref.flow(), "levels = 1")
        assert ctx.info()["iterations_done"] == ri["iterations_done"] == info["sweeps"][0][0]


# ---- 3. the state afterwards ----------------------------------------------------------------------------------------------------

def test_state_afterwards(hs, gpu_ok):
    W, H = 160, 128
    A, B = pair_of(W, H)
    params = hs.make_params(lam=LAM, max_iter=40, term_type=hs.TERM_ITER)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        ctx.solve(params)  # (derivatives of the caller's frames are in place: the pyramid must invalidate them)
        ctx.solve_pyramid(params, warps=2)
        a, b = ctx.frames()
        assert np.array_equal(a, A) and np.array_equal(b, B)
        with pytest.raises(hs.HsflowError) as e:
            ctx.verify()
        assert e.value.status == hs._lib.E_STATE
        u, v = ctx.flow()
        assert np.array_equal(ctx.warp(src=B, border="replicate"), hs.warp_host(u, v, B, border="replicate"))
        assert np.array_equal(ctx.color(), hs.color_flow_host(u, v))
        ctx.median_apply(0, radius=1)
        mu, mv, _, _ = hs.median_host(u, v, radius=1)
        assert_same(ctx.flow(), (mu, mv), "median_apply on the pyramid's flow")
        # a warm solve starts from the pyramid's flow as from any caller-written flow
        warm = hs.make_params(lam=LAM, max_iter=10, term_type=hs.TERM_ITER, use_previous=True)
        ctx.solve(warm)
        with hs.HSFlow(W, H, 1, own_stream=True) as ref:
            import torch
            ref.set_frames(A, B)
            tu, tv = torch.from_numpy(mu).cuda(), torch.from_numpy(mv).cuda()
            ref.set_flow_rows_from(tu, tv, 0, H)
            ref.solve(warm)
            assert_same(ctx.flow(), ref.flow(), "warm solve from the pyramid's flow")
        # a plain solve with reuse_derivatives right after a pyramid solve recomputes them
        ctx.solve_pyramid(params)
        ctx.solve(hs.make_params(lam=LAM, max_iter=40, term_type=hs.TERM_ITER, reuse_derivatives=True))
        with hs.HSFlow(W, H, 1, own_stream=True) as ref:
            ref.set_frames(A, B)
            ref.solve(params)
            assert_same(ctx.flow(), ref.flow(), "plain solve after a pyramid solve")
        assert ctx.verify().ok
        with pytest.raises(hs.HsflowError) as e:
            ctx.pyramid_level(0)
        assert e.value.status == hs._lib.E_STATE
        # another plan on the same context: that plan's composition
        check_against_composition(hs, ctx, [(A, B)], params, 2, 1, 0)
        check_against_composition(hs, ctx, [(A, B)], params, 0, 1, 0)


# ---- 4. quality on the device ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H,shift", [(160, 128, (5.0, -3.0)), (320, 256, (9.0, 6.0))])
def test_quality(hs, gpu_ok, W, H, shift):
    """Interior mean end-point error below 1 px and below a quarter of the one-level solve's (the CPU model: 0.247 against
    5.48 px, and 0.244 against 10.77 px)."""
    A, B = pair_of(W, H, shift)
    params = hs.make_params(lam=LAM, max_iter=100, term_type=hs.TERM_ITER)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        ctx.solve(params)
        one = interior_epe(*ctx.flow(), *shift)
        ctx.solve_pyramid(params)
        pyr = interior_epe(*ctx.flow(), *shift)
    print("%dx%d shift %s: interior mean EPE one level %.3f px, pyramid %.3f px (%.1f x)" % (W, H, shift, one, pyr, one / pyr))
    assert pyr < 1.0 and pyr < one / 4


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------

def test_refusals(hs, gpu_ok):
    W, H = 48, 32
    A, B = pair_of(W, H, SHIFTS[2])
    L = hs._lib.load()
    good = hs.make_params(lam=LAM, max_iter=20, term_type=hs.TERM_ITER)
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        st = L.hsflow_solve_pyramid(ctx._h, ctypes.byref(good), ctypes.byref(hs.make_pyramid_params()))
        assert st == hs._lib.E_STATE  # frames not set
        for k in range(2):
            ctx.set_frames(A, B, pair=k)
        ctx.solve(good)
        before = [ctx.flow(k) for k in range(2)]

        def refused(status, params=good, pp=None, **kw):
            pp = pp if pp is not None else hs.make_pyramid_params(**kw)
            st = L.hsflow_solve_pyramid(ctx._h, ctypes.byref(params) if params is not None else None, ctypes.byref(pp) if pp is not False else None)
            assert st == status, (st, status, kw)
            for k in range(2):
                assert_same(ctx.flow(k), before[k], "flow after a refusal")

        refused(hs._lib.E_ARG, params=None)
        refused(hs._lib.E_ARG, pp=False)
        short = hs.make_pyramid_params()
        short.struct_size = 16
        refused(hs._lib.E_ARG, pp=short)
        for kw in ({"levels": -1}, {"levels": 9}, {"min_size": 0}, {"warps": 0}, {"warps": 9}, {"median_radius": 3}, {"median_radius": -1}):
            refused(hs._lib.E_ARG, **kw)
        refused(hs._lib.E_ARG, params=hs.make_params(lam=LAM, max_iter=20, term_type=hs.TERM_ITER, mode=hs.MODE_CLASSIC))
        refused(hs._lib.E_ARG, params=hs.make_params(lam=LAM, max_iter=20, term_type=hs.TERM_ITER, use_previous=True))
        refused(hs._lib.E_ARG, params=hs.make_params(lam=LAM, max_iter=20, term_type=hs.TERM_ITER, profile=True))
        refused(hs._lib.E_ARG, params=hs.make_params(lam=LAM, max_iter=20, term_type=hs.TERM_ITER, kernel=hs.KERNEL_PERSIST))
        refused(hs._lib.E_ARG, params=hs.make_params(lam=-1.0, max_iter=20, term_type=hs.TERM_ITER))
        refused(hs._lib.E_SIZE, levels=8)  # 48 x 32 is 1 x 1 at the seventh level
        ctx.set_row_origin(1)
        refused(hs._lib.E_STATE)
        ctx.set_row_origin(0)
        ctx.set_eps_rows(8, 16)
        refused(hs._lib.E_STATE)
        ctx.set_eps_rows(0, 0)
        ctx.set_pair_termination(True)
        refused(hs._lib.E_STATE, params=hs.make_params(lam=LAM, max_iter=20, term_type=hs.TERM_ITER | hs.TERM_EPS))
        ctx.solve_pyramid(good)  # (under ITER the per-pair stop has nothing to decide)
        ctx.set_pair_termination(False)
        n = ctx.pyramid_info()["levels"]
        buf = np.zeros((H, W), F)
        ptr = ctypes.c_void_p(buf.ctypes.data)
        assert L.hsflow_pyramid_get_level(ctx._h, 0, 0, None, 0, None, 0, ptr, 4 * W, ptr, 4 * W) == hs._lib.OK
        assert L.hsflow_pyramid_get_level(ctx._h, 0, 0, None, 0, None, 0, None, 0, None, 0) == hs._lib.OK
        assert L.hsflow_pyramid_get_level(ctx._h, n, 0, None, 0, None, 0, ptr, 4 * W, None, 0) == hs._lib.E_ARG
        assert L.hsflow_pyramid_get_level(ctx._h, -1, 0, None, 0, None, 0, ptr, 4 * W, None, 0) == hs._lib.E_ARG
        assert L.hsflow_pyramid_get_level(ctx._h, 0, 2, None, 0, None, 0, ptr, 4 * W, None, 0) == hs._lib.E_ARG
        assert L.hsflow_pyramid_get_level(ctx._h, 0, 0, None, 0, None, 0, ptr, 4 * W - 4, None, 0) == hs._lib.E_SIZE
        assert L.hsflow_pyramid_get_level(ctx._h, 0, 0, None, 0, None, 0, None, 0, ptr, 4 * W + 2) == hs._lib.E_SIZE
        assert L.hsflow_pyramid_get_level(ctx._h, 0, 0, ptr, W - 1, None, 0, None, 0, None, 0) == hs._lib.E_SIZE
        with pytest.raises(ValueError):
            ctx.pyramid_level(n)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        with pytest.raises(hs.HsflowError) as e:
            ctx.pyramid_info()
        assert e.value.status == hs._lib.E_STATE


# ---- 6. command line -------------------------------------------------------------------------------------------------------------

def _cli(args, extra_env=None, ok=True):
    cli = os.path.join(ROOT, "opticalflowhs_amd", "hsflow_cli")
    if not os.path.exists(cli):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "opticalflowhs_amd", "csrc"), "-s", "host"])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "opticalflowhs_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    for name in ("HSFLOW_RENDER_DEVICE", "HSFLOW_JPEG_DEVICE", "HSFLOW_PICTURE", "HSFLOW_COLOR_MAX", "HSFLOW_MEDIAN", "HSFLOW_PYRAMID", "HSFLOW_VERIFY"):
        env.pop(name, None)
    env.update(extra_env or {})
    r = subprocess.run([cli] + args, env=env, capture_output=True, text=True, timeout=120)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r


def test_cli(hs, gpu_ok, tmp_path):
    W, H = 160, 128
    A, B = pair_of(W, H)
    tint = np.array([1.0, 0.8, 0.6])
    frames = [np.clip(np.rint(g[..., None] * tint), 0, 255).astype(np.uint8) for g in (A, B)]
    names = [str(tmp_path / ("frame%d.ppm" % k)) for k in range(2)]
    head = b"P6\n%d %d\n255\n" % (W, H)
    for name, f in zip(names, frames):
        with open(name, "wb") as fh:
            fh.write(head + f.tobytes())
    args = lambda out: ["-cv", "-hd", names[0], names[1], out, ".003", "60"]
    pictures = {}
    for value, kw in (("auto", {}), ("2,2,1", {"levels": 2, "warps": 2, "median_radius": 1}), (None, None)):
        with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
            ctx.set_frames_bgr(np.ascontiguousarray(frames[0][..., ::-1]), np.ascontiguousarray(frames[1][..., ::-1]), blur=True)
            if kw is None:
                ctx.solve(lam=0.003, max_iter=60)
            else:
                ctx.solve_pyramid(lam=0.003, max_iter=60, **kw)
            want = head + np.ascontiguousarray(ctx.color()).tobytes()
        for route in ({}, {"HSFLOW_RENDER_DEVICE": "1"}):
            out = str(tmp_path / "out.ppm")
            _cli(args(out), dict(route, HSFLOW_PICTURE="color", **({"HSFLOW_PYRAMID": value} if value else {})))
            assert open(out, "rb").read() == want, (value, route)
        pictures[value] = want
    assert len(set(pictures.values())) == 3
    for bad in ("0", "9", "x", "auto,", "auto,0", "auto,9", "2,1,3", "2,1,1,", "3;2", "autox"):
        r = _cli(args(str(tmp_path / "bad.ppm")), {"HSFLOW_PYRAMID": bad}, ok=False)
        assert r.returncode == 1 and "HSFLOW_PYRAMID" in r.stdout, bad
    for route in (["-cv", "-cam"], ["-cl", "-cam", "x", "3", "5", "1", "GPU"], ["-cl", "-hd", names[0], names[1], "o.ppm", "3", "5", "1", "GPU"]):
        r = _cli(route, {"HSFLOW_PYRAMID": "auto"}, ok=False)
        assert r.returncode == 1 and "HSFLOW_PYRAMID" in r.stdout
