"""The strip kernel's sweep loop laid out for the wavefronts that never drop a row (guards hinted, one cross-sum object per
interior boundary in the loop's copy of the sweep, the copy behind the loop marked): every case must leave the bits of
KERNEL_SIMPLE on the same context, and where ITER|EPS is on, its iterations_done.

What can go wrong is bookkeeping, not arithmetic: a cross sum that is undefined where its boundary is no longer needed must
never be read, in any row count, launch length or Eps mode; and the exchange's double buffer must start at buffer 0 in every
launch and every persistent phase whatever the length of the one before (the cases were written when the exchange addresses
were carried from sweep to sweep -- measured and dropped, DESIGN 4.1 -- and pin that rule for whoever tries again).

Frame sizes, the smallest that still have halo and core wavefronts, reversed strips (5 rows per lane) and side tiles:
  300 x 100  six tiles at 20 sweeps per launch and 5 rows per lane (two tile columns, three tile rows), seed 1
  262 x 37   W % 4 != 0 (lanes that load reflected scalars), one tile row, too low for the derivative pass to be fused, seed 2
Textured frames (synth.translating_pair).  The early epsilon, 0.03, stops KERNEL_SIMPLE inside the budget on both (asserted on
the reference, not assumed).
"""
import numpy as np
import pytest

from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS_NEVER = float(np.float32(1e-6))
EPS_EARLY = 0.03
SIZES = [(300, 100, 1), (262, 37, 2)]  # width, height, seed
SIZE_IDS = ["%dx%d" % (w, h) for w, h, _ in SIZES]

_frames = {}


def frames(W, H, seed):
    if (W, H, seed) not in _frames:
        _frames[(W, H, seed)] = synth.translating_pair(W, H, seed=seed)
    return _frames[(W, H, seed)]


def context(hs, W, H, seed, origin=0):
    ctx = hs.HSFlow(W, H, 1, own_stream=True)
    if origin:
        ctx.set_row_origin(origin)
    ctx.set_frames(*frames(W, H, seed))
    return ctx


def run(hs, ctx, kernel_kw, warm, asynchronous=False, **solve_kw):
    """One solve; a warm one starts from the flow a short KERNEL_SIMPLE solve leaves on the device."""
    if warm:
        ctx.solve(lam=2.0, max_iter=3, term_type=ITER, kernel=hs.KERNEL_SIMPLE)
    kw = dict(solve_kw, use_previous=warm, **kernel_kw)
    if asynchronous:
        ctx.solve_async(**kw)
        ctx.synchronize()
        info = ctx.info()
    else:
        info = ctx.solve(**kw)
    u, v = ctx.flow()
    return u, v, info


def check(hs, ctx, what, strip_kw, warm=False, asynchronous=False, early=None, **solve_kw):
    """KERNEL_SIMPLE (synchronous) and the strip kernel on the same context: same bits, and under ITER|EPS the same count."""
    ru, rv, ri = run(hs, ctx, dict(kernel=hs.KERNEL_SIMPLE), warm, **solve_kw)
    assert np.isfinite(ru).all() and np.isfinite(rv).all(), what
    if early is not None:
        if early:
            assert 1 < ri["iterations_done"] < solve_kw["max_iter"], (what, ri["iterations_done"])  # the epsilon does stop the solve early
        else:
            assert ri["iterations_done"] == solve_kw["max_iter"], (what, ri["iterations_done"])
    u, v, i = run(hs, ctx, dict(strip_kw, kernel=strip_kw.get("kernel", hs.KERNEL_STRIP)), warm, asynchronous, **solve_kw)
    assert i["kernel"] == hs.KERNEL_STRIP, (what, i)
    for k, name in (("fuse_steps", "fuse_steps"), ("strip_rows", "groups_per_thread"), ("threads", "threads")):
        if strip_kw.get(k):  # the shape asked for is the shape that ran (a solve shorter than a launch is one launch of its length)
            want = min(strip_kw[k], solve_kw["max_iter"]) if k == "fuse_steps" else strip_kw[k]
            assert i[name] == want, (what, name, i)
    if solve_kw["term_type"] & EPS:
        assert i["iterations_done"] == ri["iterations_done"], (what, i["iterations_done"], ri["iterations_done"])
    assert np.array_equal(u, ru) and np.array_equal(v, rv), (what, int((u != ru).sum()), int((v != rv).sum()))
    return i


# ---- buffer parity across launches: launches of 3, 3, 1 (fuse_steps 3, 7 sweeps), of 1 each, of 2 with a tail of 1, of 20, 20, 5
@pytest.mark.parametrize("max_iter", [7, 45])
@pytest.mark.parametrize("T", [1, 2, 3, 20])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_buffer_parity_across_launches(hs, gpu_ok, size, T, max_iter):
    W, H, seed = size
    shape = dict(strip_rows=5, fuse_steps=T, threads=1024)
    with context(hs, W, H, seed) as ctx:
        for warm in (False, True):
            what = (size, T, max_iter, warm)
            check(hs, ctx, what + ("iter",), shape, warm, lam=1.0, max_iter=max_iter, term_type=ITER)
            # ITER|EPS with an epsilon no sweep undercuts: witness launches, the last one witness + measured last sweep
            check(hs, ctx, what + ("itereps",), shape, warm, early=False, lam=1.0, max_iter=max_iter, term_type=ITER | EPS,
                  epsilon=EPS_NEVER)


# ---- row counts and widths: rows per lane x threads as the planner allows them (sweeps per launch: what leaves the tile a core)
ROW_SHAPES = [(1, 1024, 3), (2, 1024, 7), (3, 1024, 7), (4, 1024, 12), (5, 1024, 20), (5, 768, 20), (6, 768, 20), (6, 512, 7),
              (4, 768, 7), (4, 512, 7), (3, 512, 7), (5, 512, 7)]


@pytest.mark.parametrize("rows", ROW_SHAPES, ids=lambda s: "R%d_%d_T%d" % s)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_row_counts_and_widths(hs, gpu_ok, size, rows):
    W, H, seed = size
    R, nt, T = rows
    shape = dict(strip_rows=R, fuse_steps=T, threads=nt)
    max_iter = 2 * T + 3  # two full launches and an odd tail
    with context(hs, W, H, seed) as ctx:
        check(hs, ctx, (size, rows, "iter"), shape, lam=1.0, max_iter=max_iter, term_type=ITER)
        check(hs, ctx, (size, rows, "itereps"), shape, early=False, lam=1.0, max_iter=max_iter, term_type=ITER | EPS, epsilon=EPS_NEVER)
        check(hs, ctx, (size, rows, "early"), shape, warm=True, early=True, lam=1.0, max_iter=47, term_type=ITER | EPS, epsilon=EPS_EARLY)


# ---- row origin 1: the other checkerboard phase; with 5 rows per lane the reversed strip sits at the top
@pytest.mark.parametrize("rows", [(5, 1024, 20), (4, 1024, 12)], ids=lambda s: "R%d_%d_T%d" % s)
def test_row_origin_one(hs, gpu_ok, rows):
    W, H, seed = SIZES[0]
    R, nt, T = rows
    shape = dict(strip_rows=R, fuse_steps=T, threads=nt)
    flows = []
    for origin in (0, 1):
        with context(hs, W, H, seed, origin) as ctx:
            if origin:
                check(hs, ctx, (rows, "iter"), shape, lam=1.0, max_iter=2 * T + 5, term_type=ITER)
                check(hs, ctx, (rows, "itereps"), shape, warm=True, early=False, lam=1.0, max_iter=2 * T + 5, term_type=ITER | EPS,
                      epsilon=EPS_NEVER)
            ctx.solve(lam=1.0, max_iter=2 * T + 5, term_type=ITER, kernel=hs.KERNEL_SIMPLE)
            flows.append(ctx.flow()[0])
    assert not np.array_equal(flows[0], flows[1])  # the origin did change the summation order


# ---- Eps modes, cold and warm, the derivative pass fused into the first launch and as a kernel of its own
@pytest.mark.parametrize("separate_deriv", [False, True], ids=["fused", "separate"])
@pytest.mark.parametrize("T", [20, 7])
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_eps_modes(hs, gpu_ok, size, T, separate_deriv):
    W, H, seed = size
    shape = dict(strip_rows=5, fuse_steps=T, threads=1024, profile=separate_deriv)
    fusable = H >= 16 * 5 and W >= 256  # the image is at least as large as one region
    with context(hs, W, H, seed) as ctx:
        for warm in (False, True):
            what = (size, T, separate_deriv, warm)
            i = check(hs, ctx, what + ("iter",), shape, warm, lam=1.0, max_iter=47, term_type=ITER)
            assert bool(i["deriv_fused"]) == (fusable and not separate_deriv), (what, i)
            check(hs, ctx, what + ("never",), shape, warm, early=False, lam=1.0, max_iter=47, term_type=ITER | EPS, epsilon=EPS_NEVER)
            check(hs, ctx, what + ("early",), shape, warm, early=True, lam=1.0, max_iter=47, term_type=ITER | EPS, epsilon=EPS_EARLY)
            if separate_deriv:
                continue  # (a profiled solve is synchronous)
            check(hs, ctx, what + ("async never",), shape, warm, asynchronous=True, early=False, lam=1.0, max_iter=47,
                  term_type=ITER | EPS, epsilon=EPS_NEVER)
            check(hs, ctx, what + ("async early",), shape, warm, asynchronous=True, early=True, lam=1.0, max_iter=47,
                  term_type=ITER | EPS, epsilon=EPS_EARLY)


# ---- the persistent launch: every phase starts at buffer 0, whatever the length of the one before
@pytest.mark.parametrize("sweeps,T", [(25, 5), (24, 8)], ids=["25_T5", "24_T8"])
def test_persistent_phases(hs, gpu_ok, sweeps, T):
    W, H, seed = SIZES[0]
    with context(hs, W, H, seed) as ctx:
        ctx.solve(lam=1.0, max_iter=sweeps, term_type=ITER, kernel=hs.KERNEL_SIMPLE)
        su, sv = ctx.flow()
        ctx.solve(lam=1.0, max_iter=sweeps, term_type=ITER, kernel=hs.KERNEL_STRIP, fuse_steps=T, strip_rows=5, threads=1024)
        u0, v0 = ctx.flow()
        assert np.array_equal(u0, su) and np.array_equal(v0, sv)
        for sync, graph, tt in ((True, False, ITER), (False, True, ITER), (False, False, ITER | EPS), (False, True, ITER | EPS)):
            kw = dict(lam=1.0, max_iter=sweeps, term_type=tt, epsilon=EPS_NEVER, kernel=hs.KERNEL_PERSIST, fuse_steps=T, strip_rows=5,
                      threads=1024, use_graph=graph)
            if sync:
                i = ctx.solve(**kw)
            else:
                ctx.solve_async(**kw)
                ctx.synchronize()
                i = ctx.info()
            u, v = ctx.flow()
            assert i["persistent"] == -(-sweeps // T) and i["jacobi_launches"] == 1 and i["kernel"] == hs.KERNEL_STRIP, i
            assert i["iterations_done"] == sweeps and i["eps_rerun"] == 0, i
            assert np.array_equal(u, u0) and np.array_equal(v, v0), (sweeps, T, sync, graph, tt)


# ---- 12 wavefronts: the buffers of a slot lie side by side whatever the number of slots
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_twelve_wavefronts_with_eps(hs, gpu_ok, size):
    W, H, seed = size
    seed = 3 - seed  # (the other seed)
    shape = dict(strip_rows=5, fuse_steps=9, threads=768)
    with context(hs, W, H, seed) as ctx:
        for warm in (False, True):
            check(hs, ctx, (size, warm, "never"), shape, warm, early=False, lam=1.0, max_iter=30, term_type=ITER | EPS, epsilon=EPS_NEVER)
            check(hs, ctx, (size, warm, "early"), shape, warm, early=True, lam=1.0, max_iter=47, term_type=ITER | EPS, epsilon=EPS_EARLY)
            check(hs, ctx, (size, warm, "async"), shape, warm, asynchronous=True, early=False, lam=1.0, max_iter=30,
                  term_type=ITER | EPS, epsilon=EPS_NEVER)
