"""The strip kernel's set-up and trapezoid at the edges of the tile grid: every explicit shape below must leave the bits of
KERNEL_SIMPLE on the same context -- ITER and ITER|EPS (an epsilon no sweep undercuts, and one that stops the solve
early), from zero flow and from the flow a short solve left behind.

Frame sizes, the smallest that show each edge of the grid (regions are 256 columns x wavefronts * rows-per-lane rows):
  300 x 90   one tile column whose side lanes are mirrored; with few sweeps per launch the top and the bottom tile are
             the same workgroup
  256 x 200, 470 x 200   two and three tile rows (a top, an interior and a bottom tile); two tile columns put the corners
             of a region's halo inside the image
  259 x 161  W % 4 != 0 and an odd height: reversed strips (odd rows per lane) at both borders
Textured frames (synth.translating_pair), so the flow is nowhere near the denormals the scaled state keeps differently.
The early epsilon: the CPU oracle stops these solves after 16 - 22 of 47 sweeps at 0.03 (cold and warm), and the pairs of
the batched case after 8, 22 and 45; the tests assert on the SIMPLE reference that the stop is early, not that count.
"""
import numpy as np
import pytest

from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
MAX_IT = 47                 # two launches of 20 and a tail of 7; six of 7 and a tail of 5; fifteen of 3 and a tail of 2; 32 + 15
EPS_NEVER = float(np.float32(1e-6))
EPS_EARLY = 0.03
SIZES = [(300, 90), (256, 200), (470, 200), (259, 161)]
# (sweeps per launch, rows per lane, threads): 5 rows with 16 and 12 wavefronts; 4 rows for the even-rows phase
# and the most sweeps a launch can have (32), where the trapezoid's tables are at their clamps
SHAPES = [(20, 5, 1024), (7, 5, 1024), (3, 5, 1024), (20, 5, 768), (7, 5, 768), (3, 5, 768), (12, 4, 1024), (32, 5, 1024)]
MODES = [("iter", ITER, EPS_NEVER), ("itereps", ITER | EPS, EPS_NEVER), ("early", ITER | EPS, EPS_EARLY)]

_frames = {}
_refs = {}


def frames(W, H):
    if (W, H) not in _frames:
        _frames[(W, H)] = synth.translating_pair(W, H, seed=3)
    return _frames[(W, H)]


def solve_all(hs, ctx, **kw):
    """The six solves of one kernel shape on ctx: {(mode, warm): (u, v, iterations_done)}."""
    out = {}
    for name, tt, eps in MODES:
        for warm in (False, True):
            if warm:  # the warm start: the flow a short solve leaves on the device
                ctx.solve(lam=2.0, max_iter=3, term_type=ITER, kernel=hs.KERNEL_SIMPLE)
            info = ctx.solve(lam=1.0, max_iter=MAX_IT, term_type=tt, epsilon=eps, use_previous=warm, **kw)
            u, v = ctx.flow()
            out[(name, warm)] = (u, v, info["iterations_done"], info)
    return out


def reference(hs, W, H, origin):
    """KERNEL_SIMPLE's six solves of a frame size, computed once and shared."""
    key = (W, H, origin)
    if key not in _refs:
        A, B = frames(W, H)
        with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
            ctx.set_row_origin(origin)
            ctx.set_frames(A, B)
            ref = solve_all(hs, ctx, kernel=hs.KERNEL_SIMPLE)
        for (name, warm), (u, v, done, _) in ref.items():
            assert np.isfinite(u).all() and np.isfinite(v).all()
            if name == "early":
                assert 1 < done < MAX_IT, (key, warm, done)  # the early epsilon does stop early
            else:
                assert done == MAX_IT, (key, name, warm, done)
            u.setflags(write=False)
            v.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def check_shape(hs, W, H, origin, T, R, nt):
    ref = reference(hs, W, H, origin)
    A, B = frames(W, H)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_row_origin(origin)
        ctx.set_frames(A, B)
        got = solve_all(hs, ctx, kernel=hs.KERNEL_STRIP, strip_rows=R, fuse_steps=T, threads=nt)
    for key, (u, v, done, info) in got.items():
        ru, rv, rdone, _ = ref[key]
        what = (W, H, origin, T, R, nt) + key
        assert info["kernel"] == hs.KERNEL_STRIP and info["fuse_steps"] == T and info["groups_per_thread"] == R \
            and info["threads"] == nt, (what, info)  # the shape asked for is the shape that ran
        assert done == rdone, (what, done, rdone)
        assert np.array_equal(u, ru) and np.array_equal(v, rv), (what, int((u != ru).sum()), int((v != rv).sum()))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%d_R%d_%d" % s)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_strip_shapes_match_simple_bits(hs, gpu_ok, size, shape):
    check_shape(hs, size[0], size[1], 0, *shape)


@pytest.mark.parametrize("shape", [(20, 5, 1024), (7, 5, 768), (12, 4, 1024)], ids=lambda s: "T%d_R%d_%d" % s)
def test_row_origin_one(hs, gpu_ok, shape):
    """A slab whose row 0 is row 1 of its frame: "above row 0" is still the slab's border (reflected), the checkerboard
    phase is the other one, and with 5 rows per lane the reversed strip sits at the top."""
    check_shape(hs, 256, 200, 1, *shape)
    r0, r1 = reference(hs, 256, 200, 0), reference(hs, 256, 200, 1)
    assert not np.array_equal(r0[("iter", False)][0], r1[("iter", False)][0])  # the origin did change the summation order


@pytest.mark.parametrize("T", [20, 7])
def test_batched_pairs_stop_on_their_own(hs, gpu_ok, T):
    """Three pairs in one context, each stopping on its own Eps: the launches over the pairs still running (the pair list)
    go through the same set-up.  Flow and per-pair results against KERNEL_SIMPLE on the same context."""
    W, H = 300, 90
    pairs = [synth.translating_pair(W, H, seed=5, dx=0.75, dy=-0.5), synth.translating_pair(W, H, seed=6, dx=0.15, dy=-0.1),
             synth.translating_pair(W, H, seed=7, dx=1.5, dy=1.0)]
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        for i, (A, B) in enumerate(pairs):
            ctx.set_frames(A, B, pair=i)
        ctx.set_pair_termination(True)
        res = {}
        for name, kw in (("simple", dict(kernel=hs.KERNEL_SIMPLE)),
                         ("strip", dict(kernel=hs.KERNEL_STRIP, strip_rows=5, fuse_steps=T, threads=1024))):
            info = ctx.solve(lam=1.0, max_iter=MAX_IT, term_type=ITER | EPS, epsilon=EPS_EARLY, **kw)
            pr = ctx.pair_results()
            res[name] = (info, pr, [ctx.flow(pair=i) for i in range(3)])
        info, pr, fl = res["strip"]
        assert info["kernel"] == hs.KERNEL_STRIP and info["fuse_steps"] == T and info["groups_per_thread"] == 5, info
        _, pr0, fl0 = res["simple"]
        done0 = [r["iterations_done"] for r in pr0]
        assert len(set((d - 1) // T for d in done0)) >= 2 and max(done0) <= MAX_IT, done0  # the pairs stop in different launches
        for i in range(3):
            assert pr[i]["iterations_done"] == pr0[i]["iterations_done"] and pr[i]["status"] == pr0[i]["status"], (i, pr[i], pr0[i])
            assert pr[i]["last_eps"] == pr0[i]["last_eps"], (i, pr[i], pr0[i])
            assert np.array_equal(fl[i][0], fl0[i][0]) and np.array_equal(fl[i][1], fl0[i][1]), i
