"""Contexts that hold several image pairs (hsflow_create's n_pairs) against the same pairs solved one by one.

The reference for every pair of a batch is that pair alone in an HSFlow(W, H, 1) context -- itself pinned to the CPU
oracle by tests/test_gpu_parity.py -- and a batch pair must equal it BIT FOR BIT: under ITER termination the pairs of a
context are independent.  A sample of pairs is also checked against the oracle directly, so that a batch and a single
pair cannot both be wrong in the same way.  Neighbouring pairs differ sharply (constant 255, textured, constant 0,
textured, ...): the planes lie back to back without guard rows, so a read across a pair boundary changes bits.

Under EPS termination the pairs of a batch share ONE stopping sweep (include/hsflow.h, hsflow_solve): the Eps of a
sweep is the maximum over all pairs, so the batch stops at the first sweep whose maximum is below epsilon.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
RMS_TOL = 1e-4


def rms(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return float(np.sqrt(np.mean(d * d)))


def batch_frames(W, H, N, seed):
    """constant 255, textured, constant 0, textured, ...: every textured pair sits between two flat ones."""
    out = []
    for i in range(N):
        if i % 2:
            out.append(synth.random_pair(W, H, seed=seed + i))
        else:
            A = np.full((H, W), 255 if i % 4 == 0 else 0, np.uint8)
            out.append((A, A.copy()))
    return out


def load(ctx, pairs):
    for i, (A, B) in enumerate(pairs):
        ctx.set_frames(A, B, pair=i)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


class Singles(object):
    """One single-pair context per pair: the reference solves."""

    def __init__(self, hs, W, H, pairs):
        self.ctxs = []
        for A, B in pairs:
            c = hs.HSFlow(W, H, 1, own_stream=True)
            c.set_frames(A, B)
            self.ctxs.append(c)

    def solve(self, **kw):
        out = []
        for c in self.ctxs:
            c.solve(**kw)
            out.append(c.flow())
        return out

    def close(self):
        for c in self.ctxs:
            c.close()


# (name, parameters, sweeps): explicit sweeps per launch leave a tail launch (sweeps % fuse_steps != 0)
def cv_configs(hs):
    S, F, T, D, A = hs.KERNEL_SIMPLE, hs.KERNEL_FUSED, hs.KERNEL_STRIP, hs.KERNEL_FOLD, hs.KERNEL_AUTO
    cfg = [("simple", dict(kernel=S), 13), ("simple_graph", dict(kernel=S, use_graph=True), 13),
           ("fused", dict(kernel=F), 45), ("fused_3", dict(kernel=F, fuse_steps=3, tile_w=32, tile_h=16, threads=256), 13),
           ("fused_5_graph", dict(kernel=F, fuse_steps=5, tile_w=64, tile_h=24, threads=512, use_graph=True), 13),
           ("fused_7", dict(kernel=F, fuse_steps=7, threads=1024), 13),
           ("strip", dict(kernel=T), 45), ("strip_graph", dict(kernel=T, use_graph=True), 45),
           ("fold", dict(kernel=D), 45), ("fold_graph", dict(kernel=D, use_graph=True), 45),
           ("auto", dict(kernel=A), 45), ("auto_graph", dict(kernel=A, use_graph=True), 45)]
    # (fuse_steps, strip_rows, threads) of test_kernel_variants_are_bit_identical
    for t, r, nt in ((1, 1, 256), (2, 2, 192), (3, 3, 1024), (7, 6, 768), (8, 3, 640), (12, 8, 512)):
        cfg.append(("strip_%d_%d_%d" % (t, r, nt), dict(kernel=T, fuse_steps=t, strip_rows=r, threads=nt), 13))
    for t, r, nt in ((2, 2, 128), (5, 5, 768), (8, 3, 320), (11, 4, 448)):
        cfg.append(("fold_%d_%d_%d" % (t, r, nt), dict(kernel=D, fuse_steps=t, strip_rows=r, threads=nt), 13))
    return cfg


# (W, H, N); the last shape's strip plan has more than 256 workgroups, a number that is no multiple of the 8 XCDs
CV_SHAPES = [(1, 1, 4), (9, 1, 5), (1, 9, 3), (2, 2, 6), (7, 130, 3), (131, 6, 4), (256, 80, 3), (258, 81, 2),
             (333, 150, 5), (600, 480, 8), (700, 300, 23)]


@pytest.mark.parametrize("shape", CV_SHAPES, ids=["%dx%dx%d" % s for s in CV_SHAPES])
def test_every_cv_kernel_on_batches_equals_single_pairs(hs, oracle, gpu_ok, shape):
    W, H, N = shape
    lam = 0.5
    pairs = batch_frames(W, H, N, seed=100 * W + H)
    if shape == CV_SHAPES[-1]:
        tiles = hs.plan_query(W, H, N, lam=lam, max_iter=45, term_type=ITER, kernel=hs.KERNEL_STRIP)["tiles"]
        assert tiles > 256 and tiles % 8, tiles
    ran = skipped = tails = 0
    singles = Singles(hs, W, H, pairs)
    try:
        with hs.HSFlow(W, H, N, own_stream=True) as ctx:
            load(ctx, pairs)
            for name, kw, it in cv_configs(hs):
                try:
                    info = ctx.solve(lam=lam, max_iter=it, term_type=ITER, **kw)
                except hs.HsflowError as e:   # a plan the library refuses for this shape (e.g. a halo wider than the frame)
                    assert e.status == hs._lib.E_SIZE, (name, e)
                    skipped += 1
                    continue
                ran += 1
                assert info["iterations_done"] == it and info["n_pairs"] == N, (name, info)
                if info["kernel"] != hs.KERNEL_SIMPLE and it % info["fuse_steps"]:
                    tails += 1
                want = singles.solve(lam=lam, max_iter=it, term_type=ITER, **kw)
                for i in range(N):
                    assert same(ctx.flow(pair=i), want[i]), (name, shape, i, info)
                if name == "auto":
                    # the oracle on the textured pairs (at most three of them: the oracle is CPU time)
                    for i in range(1, min(N, 6), 2):
                        uo, vo = oracle.calc_optical_flow_hs(pairs[i][0], pairs[i][1], lam, it, term_type=ITER, threads=0)
                        u, v = ctx.flow(pair=i)
                        assert rms(u, uo) <= RMS_TOL and rms(v, vo) <= RMS_TOL, (shape, i, rms(u, uo), rms(v, vo))
                    # the flat pairs stay exactly at rest
                    for i in range(0, N, 2):
                        u, v = ctx.flow(pair=i)
                        assert not u.any() and not v.any(), (shape, i)
                    auto = [ctx.flow(pair=i) for i in range(N)]
        assert ran >= 0.75 * (ran + skipped) and tails >= 5, (ran, skipped, tails)
        # the same pairs in another order: every pair's flow stays what it was
        perm = np.random.default_rng(W * H + N).permutation(N)
        if N > 1 and np.array_equal(perm, np.arange(N)):
            perm = np.roll(perm, 1)
        with hs.HSFlow(W, H, N, own_stream=True) as ctx:
            load(ctx, [pairs[j] for j in perm])
            ctx.solve(lam=lam, max_iter=45, term_type=ITER, kernel=hs.KERNEL_AUTO)
            for k, j in enumerate(perm):
                assert same(ctx.flow(pair=k), auto[j]), (shape, k, j)
    finally:
        singles.close()


@pytest.mark.parametrize("shape", [(256, 96), (264, 80), (300, 257), (1024, 333)])
def test_derivative_pass_in_the_first_launch_on_batches(hs, oracle, gpu_ok, shape):
    """k_jacobi_strip_deriv / k_jacobi_fold_deriv on batches: the derivative plane of every pair equals the oracle's,
    and the flow equals the profile=True solve (never fused: a derivative kernel of its own) and the single-pair solve."""
    W, H = shape
    N = 3
    pairs = batch_frames(W, H, N, seed=7 * W + H)
    # textured, flat, textured: the first and the last pair of the context are textured too
    pairs = [pairs[1], pairs[0], synth.random_pair(W, H, seed=W + 3)]
    derivs = [oracle.derivatives(A, B) for A, B in pairs]
    fused = 0
    singles = Singles(hs, W, H, pairs)
    try:
        with hs.HSFlow(W, H, N, own_stream=True) as ctx:
            load(ctx, pairs)
            for it, R, graph, kern in ((1, 5, False, hs.KERNEL_STRIP), (7, 4, True, hs.KERNEL_STRIP), (20, 0, True, hs.KERNEL_STRIP),
                                       (9, 2, False, hs.KERNEL_STRIP), (13, 6, True, hs.KERNEL_STRIP), (10, 0, False, hs.KERNEL_AUTO),
                                       (1, 1, False, hs.KERNEL_FOLD), (13, 2, True, hs.KERNEL_FOLD), (8, 3, False, hs.KERNEL_FOLD),
                                       (17, 5, True, hs.KERNEL_FOLD), (30, 0, False, hs.KERNEL_FOLD)):
                kw = dict(lam=0.5, max_iter=it, term_type=ITER, kernel=kern, strip_rows=R)
                ctx.solve(lam=2.0, max_iter=2, term_type=ITER, kernel=hs.KERNEL_SIMPLE)   # a derivative plane to overwrite
                i1 = ctx.solve(use_graph=graph, **kw)
                got = [ctx.flow(pair=i) for i in range(N)]
                fold = i1["kernel"] == hs.KERNEL_FOLD
                rows = (i1["threads"] // 64) * i1["groups_per_thread"] * (2 if fold else 1)
                fusable = W >= (128 if fold else 256) and H >= rows and i1["groups_per_thread"] <= 6
                assert i1["deriv_fused"] == (1 if fusable else 0), (shape, it, R, kern, i1)
                fused += i1["deriv_fused"]
                for i in range(N):
                    d = ctx.derivatives(pair=i)
                    assert all(np.array_equal(d[k], derivs[i][k]) for k in range(3)), (shape, it, R, kern, i)
                i2 = ctx.solve(profile=True, **kw)
                assert i2["deriv_fused"] == 0 and i2["iterations_done"] == it
                want = singles.solve(**kw)
                for i in range(N):
                    assert same(got[i], ctx.flow(pair=i)), (shape, it, R, kern, i)
                    assert same(got[i], want[i]), (shape, it, R, kern, i)
    finally:
        singles.close()
    assert fused >= 6, fused


# ---- ITER|EPS on batches: one stopping sweep for all pairs --------------------------------------------------------

LAM, EPSILON, BUDGET = 0.002, 1e-3, 200


def eps_pairs():
    """48x40 pairs whose own stopping sweeps (lambda 0.002, epsilon 1e-3) differ: identical frames stop after sweep 1, a
    nearly flat pair after a few, a random pair after ~40, the golden pair after ~150, a translating texture not within
    the budget of 200."""
    d = np.load(os.path.join(GOLDEN, "eps_48x40_l0.002_e1e-3.npz"))
    flat = np.full((40, 48), 100, np.uint8)
    flat[12:20, 16:26] = 102
    return {"same": (d["A"], d["A"].copy()), "flat": (flat, np.roll(flat, 1, axis=1)), "random": synth.random_pair(48, 40, seed=3),
            "golden": (d["A"], d["B"]), "moving": synth.translating_pair(48, 40, seed=9),
            "same2": (synth.random_pair(48, 40, seed=8)[0],) * 2}


EPS_BATCHES = {"stops_golden": ["flat", "golden", "same", "random"], "budget": ["random", "moving", "golden", "flat"],
               "all_same": ["same", "same2", "same"], "stops_random": ["same", "flat", "random"]}


def single_probe(hs, pair, n, rows=None, warm=0, **kw):
    with hs.HSFlow(48, 40, 1, own_stream=True) as c:
        c.set_frames(*pair)
        if rows:
            c.set_eps_rows(*rows)
        if warm:
            c.solve(lam=LAM, max_iter=warm, term_type=ITER)
        return c.solve_probe(lam=LAM, max_iter=n, use_previous=bool(warm), **kw)


def single_iter(hs, pair, n, warm=0):
    with hs.HSFlow(48, 40, 1, own_stream=True) as c:
        c.set_frames(*pair)
        if warm:
            c.solve(lam=LAM, max_iter=warm, term_type=ITER)
        c.solve(lam=LAM, max_iter=n, term_type=ITER, use_previous=bool(warm))
        return c.flow()


def stop_of(emax, budget):
    hit = np.nonzero(emax.astype(np.float64) < EPSILON)[0]
    return int(hit[0]) + 1 if len(hit) and hit[0] < budget else budget


@pytest.mark.parametrize("kernel", ["strip", "fold", "simple", "auto"])
def test_batch_eps_is_the_maximum_over_pairs_and_stops_every_pair_at_once(hs, gpu_ok, kernel):
    k = {"strip": hs.KERNEL_STRIP, "fold": hs.KERNEL_FOLD, "simple": hs.KERNEL_SIMPLE, "auto": hs.KERNEL_AUTO}[kernel]
    P = eps_pairs()
    e = {name: single_probe(hs, P[name], BUDGET, kernel=k) for name in P}
    own = {name: stop_of(e[name], BUDGET) for name in P}
    assert own["same"] == 1 and 1 < own["flat"] < own["random"] < own["golden"] < BUDGET == own["moving"], own
    seen = set()
    for bname, names in EPS_BATCHES.items():
        pairs = [P[n] for n in names]
        emax = np.maximum.reduce([e[n] for n in names])
        n = stop_of(emax, BUDGET)
        seen.add(n)
        assert n >= max(own[x] for x in names), (bname, n)   # no pair stops the batch before its own stopping sweep
        with hs.HSFlow(48, 40, len(pairs), own_stream=True) as ctx:
            load(ctx, pairs)
            assert np.array_equal(ctx.solve_probe(lam=LAM, max_iter=BUDGET, kernel=k), emax), bname
            info = ctx.solve(lam=LAM, max_iter=BUDGET, epsilon=EPSILON, term_type=ITER | EPS, kernel=k)
            assert info["iterations_done"] == n and info["last_eps"] == emax[n - 1], (bname, n, info, emax[n - 1])
            if n == BUDGET and kernel == "auto":
                assert info["eps_rerun"] == 0, info   # the moving pair's witness proves "no early stop" for the batch
            for i, name in enumerate(names):
                assert same(ctx.flow(pair=i), single_iter(hs, P[name], n)), (bname, i, name, n)
            if bname in ("stops_golden", "stops_random", "all_same"):   # EPS alone: every pair converges
                info = ctx.solve(lam=LAM, max_iter=0, epsilon=EPSILON, term_type=EPS, kernel=k)
                assert info["iterations_done"] == n and info["last_eps"] == emax[n - 1], (bname, info)
                for i, name in enumerate(names):
                    assert same(ctx.flow(pair=i), single_iter(hs, P[name], n)), (bname, "eps only", i)
    assert 1 in seen and BUDGET in seen and len(seen) == len(EPS_BATCHES), seen


@pytest.mark.parametrize("kernel", ["strip", "simple"])
def test_batch_eps_over_a_row_window(hs, gpu_ok, kernel):
    """hsflow_set_eps_rows applies to every pair of the batch: Eps = max over pairs of each pair's window."""
    k = hs.KERNEL_STRIP if kernel == "strip" else hs.KERNEL_SIMPLE
    P = eps_pairs()
    names = EPS_BATCHES["stops_golden"] + ["moving"]
    for rows in ((8, 20), (0, 1), (39, 1)):
        # (the moving texture alone would not stop; over one row at the border it may: its own sweep decides it)
        e = [single_probe(hs, P[n], BUDGET, rows=rows, kernel=k) for n in names]
        emax = np.maximum.reduce(e)
        n = stop_of(emax, BUDGET)
        with hs.HSFlow(48, 40, len(names), own_stream=True) as ctx:
            load(ctx, [P[x] for x in names])
            ctx.set_eps_rows(*rows)
            assert np.array_equal(ctx.solve_probe(lam=LAM, max_iter=BUDGET, kernel=k), emax), rows
            info = ctx.solve(lam=LAM, max_iter=BUDGET, epsilon=EPSILON, term_type=ITER | EPS, kernel=k)
            assert info["iterations_done"] == n and info["last_eps"] == emax[n - 1], (rows, n, info)
            for i, name in enumerate(names):
                assert same(ctx.flow(pair=i), single_iter(hs, P[name], n)), (rows, i, name)


def test_batch_iter_eps_async_graph_and_warm_start(hs, gpu_ok):
    P = eps_pairs()
    for bname in ("stops_golden", "budget", "all_same", "stops_random"):
        names = EPS_BATCHES[bname]
        pairs = [P[n] for n in names]
        emax = np.maximum.reduce([single_probe(hs, p, BUDGET) for p in pairs])
        n = stop_of(emax, BUDGET)
        want = [single_iter(hs, p, n) for p in pairs]
        with hs.HSFlow(48, 40, len(pairs), own_stream=True) as ctx:
            load(ctx, pairs)
            kw = dict(lam=LAM, max_iter=BUDGET, epsilon=EPSILON, term_type=ITER | EPS)
            for how in ("async", "graph", "async_graph"):
                if how.startswith("async"):
                    ctx.solve_async(use_graph=how.endswith("graph"), **kw)
                    ctx.synchronize()   # settles the owed early-stop check
                    info = ctx.info()
                else:
                    info = ctx.solve(use_graph=True, **kw)
                assert info["iterations_done"] == n and info["last_eps"] == emax[n - 1], (bname, how, n, info)
                for i in range(len(pairs)):
                    assert same(ctx.flow(pair=i), want[i]), (bname, how, i)
            # warm start: 5 sweeps, then ITER|EPS from that flow
            warm = 5
            ew = np.maximum.reduce([single_probe(hs, p, BUDGET - warm, warm=warm) for p in pairs])
            nw = stop_of(ew, BUDGET - warm)
            ctx.solve(lam=LAM, max_iter=warm, term_type=ITER)
            info = ctx.solve(lam=LAM, max_iter=BUDGET - warm, epsilon=EPSILON, term_type=ITER | EPS, use_previous=True)
            assert info["iterations_done"] == nw and info["last_eps"] == ew[nw - 1], (bname, nw, info)
            for i, p in enumerate(pairs):
                assert same(ctx.flow(pair=i), single_iter(hs, p, nw, warm=warm)), (bname, "warm", i)


# ---- classic mode on batches ------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(37, 29, 2), (61, 23, 3), (258, 64, 5), (333, 131, 4), (7, 130, 3)])
def test_classic_mode_on_batches_is_the_oracle_bit_for_bit(hs, oracle, gpu_ok, shape):
    W, H, N = shape
    alpha, it = 4.0, 13
    pairs = batch_frames(W, H, N, seed=3 * W + H)
    want = [oracle.classic_flow(A, B, alpha, it) for A, B in pairs]
    shipped = [oracle.classic_flow(A, B, alpha, it, update_v=False)[0] for A, B in pairs]
    derivs = [oracle.classic_derivatives(A, B) for A, B in pairs]
    variants = [dict(kernel=hs.KERNEL_SIMPLE), dict(kernel=hs.KERNEL_FUSED), dict(kernel=hs.KERNEL_FUSED, fuse_steps=3),
                dict(kernel=hs.KERNEL_STRIP), dict(kernel=hs.KERNEL_AUTO, use_graph=True)] + \
        [dict(kernel=hs.KERNEL_STRIP, strip_rows=r, fuse_steps=5) for r in range(2, 9)]
    ran = 0
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        load(ctx, pairs)
        for kw in variants:
            try:
                ctx.solve(mode=hs.MODE_CLASSIC, alpha=alpha, max_iter=it, term_type=ITER, **kw)
            except hs.HsflowError as e:   # no aligned strip shape for this height with the requested rows
                assert e.status == hs._lib.E_SIZE and kw.get("strip_rows"), (shape, kw, e)
                continue
            ran += 1
            for i in range(N):
                assert same(ctx.flow(pair=i), want[i]), (shape, kw, i)
                d = ctx.derivatives(pair=i)
                assert all(np.array_equal(d[k], derivs[i][k]) for k in range(3)), (shape, kw, i)
            ctx.solve(mode=hs.MODE_CLASSIC_AS_SHIPPED, alpha=alpha, max_iter=it, term_type=ITER, **kw)
            for i in range(N):
                u, v = ctx.flow(pair=i)
                assert np.array_equal(u, shipped[i]) and not v.any(), (shape, kw, i)
    assert ran >= 6, ran


# ---- writes of one pair stay inside it --------------------------------------------------------------------------

def test_writes_to_one_pair_leave_the_others_alone(hs, oracle, gpu_ok):
    import torch
    W, H, N = 61, 37, 4
    pairs = batch_frames(W, H, N, seed=500)
    rng = np.random.default_rng(5)
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        load(ctx, pairs)
        ctx.solve(lam=0.5, max_iter=10, term_type=ITER)
        flows = [ctx.flow(pair=j) for j in range(N)]
        derivs = [ctx.derivatives(pair=j) for j in range(N)]

        def others_unchanged(i, what):
            for j in range(N):
                if j == i:
                    continue
                assert same(ctx.frames(pair=j), pairs[j]), (what, i, j)
                assert same(ctx.flow(pair=j), flows[j]), (what, i, j)

        for i in (0, 2, 3, 1):
            A, B = synth.random_pair(W, H, seed=600 + i)
            ctx.set_frames(A, B, pair=i)
            assert same(ctx.frames(pair=i), (A, B))
            others_unchanged(i, "host")
            # device frames with a row pitch
            A, B = synth.random_pair(W, H, seed=610 + i)
            ta = torch.zeros((H, W + 13), dtype=torch.uint8, device="cuda")
            tb = torch.zeros((H, W + 13), dtype=torch.uint8, device="cuda")
            ta[:, :W] = torch.from_numpy(A).cuda()
            tb[:, :W] = torch.from_numpy(B).cuda()
            torch.cuda.synchronize()
            ctx.set_frames(ta[:, :W], tb[:, :W], pair=i)
            ctx.synchronize()
            assert same(ctx.frames(pair=i), (A, B))
            others_unchanged(i, "device")
            for blur in (True, False):
                ca, cb = (rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(2))
                ctx.set_frames_bgr(ca, cb, blur=blur, pair=i)
                ga, gb = oracle.bgr2gray(ca), oracle.bgr2gray(cb)
                if blur:
                    ga, gb = oracle.box_blur3(ga), oracle.box_blur3(gb)
                assert same(ctx.frames(pair=i), (ga, gb)), blur
                others_unchanged(i, "bgr")
            ga, gb = synth.random_pair(W, H, seed=620 + i)
            ctx.set_frames_gray_blur(ga, gb, pair=i)
            assert same(ctx.frames(pair=i), (oracle.box_blur3(ga), oracle.box_blur3(gb)))
            others_unchanged(i, "gray_blur")
            nxt = synth.random_pair(W, H, seed=630 + i)[1]
            prev = ctx.frames(pair=i)[1]
            ctx.push_frame(nxt, pair=i)
            assert same(ctx.frames(pair=i), (prev, nxt))
            others_unchanged(i, "push")
            # device row copies of the flow, out and in
            ud = torch.empty((6, W), dtype=torch.float32, device="cuda")
            vd = torch.empty((6, W), dtype=torch.float32, device="cuda")
            ctx.flow_rows_to(ud, vd, H - 6, 6, pair=i)
            ctx.synchronize()
            u, v = ctx.flow(pair=i)
            assert np.array_equal(ud.cpu().numpy(), u[H - 6:]) and np.array_equal(vd.cpu().numpy(), v[H - 6:])
            zu, ov = torch.zeros_like(ud), torch.ones_like(vd)
            torch.cuda.synchronize()
            ctx.set_flow_rows_from(zu, ov, H - 6, 6, pair=i)   # the pair's last rows: pair i+1's first follow in memory
            ctx.synchronize()
            u2, v2 = ctx.flow(pair=i)
            assert not u2[H - 6:].any() and np.all(v2[H - 6:] == 1) and np.array_equal(u2[:H - 6], u[:H - 6])
            others_unchanged(i, "flow rows")
            flows[i] = (u2, v2)
            pairs[i] = ctx.frames(pair=i)
            # the derivatives of the new frames: a reuse_derivatives solve must not reuse the stale plane
            ctx.solve(lam=0.5, max_iter=10, term_type=ITER, reuse_derivatives=True)
            for j in range(N):
                d = ctx.derivatives(pair=j)
                want = oracle.derivatives(*pairs[j]) if j == i else derivs[j]
                assert all(np.array_equal(d[k], want[k]) for k in range(3)), (i, j)
            derivs[i] = ctx.derivatives(pair=i)
            with hs.HSFlow(W, H, 1, own_stream=True) as one:
                one.set_frames(*pairs[i])
                one.solve(lam=0.5, max_iter=10, term_type=ITER)
                assert same(ctx.flow(pair=i), one.flow()), i
            for j in range(N):
                if j != i:
                    assert same(ctx.flow(pair=j), flows[j]), (i, j)
            flows[i] = ctx.flow(pair=i)


# ---- more pairs than a 16-bit grid dimension -----------------------------------------------------------------------

def test_more_pairs_than_a_grid_dimension_holds(hs, oracle, gpu_ok):
    """70 000 pairs of 4x4 in one context: more layers than the device takes in grid z (the per-pixel kernels put one
    layer of workgroups per pair) and more workgroups than 65 535 for the tiled kernels.  Every launch must stay valid
    and every sampled pair equal its single-pair solve -- around pairs 65 535 / 65 536 above all."""
    W, H, N = 4, 4, 70000
    kinds = [synth.random_pair(W, H, seed=900 + s) for s in range(5)]
    kinds.insert(2, (np.full((H, W), 255, np.uint8),) * 2)
    kinds.append((np.zeros((H, W), np.uint8),) * 2)
    K = len(kinds)   # 7 kinds, pair i is kind i % 7: neighbours always differ
    rng = np.random.default_rng(3)
    sample = sorted({0, 1, 2, 65534, 65535, 65536, 65537, N - 2, N - 1} | set(int(x) for x in rng.integers(0, N, 16)))
    derivs = [oracle.derivatives(A, B) for A, B in kinds]
    ran = 0
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for i in range(N):
            ctx.set_frames(*kinds[i % K], pair=i)
        for name, kw in (("simple", dict(kernel=hs.KERNEL_SIMPLE)), ("fused", dict(kernel=hs.KERNEL_FUSED)),
                         ("strip", dict(kernel=hs.KERNEL_STRIP)), ("auto", dict(kernel=hs.KERNEL_AUTO))):
            try:
                info = ctx.solve(lam=0.5, max_iter=6, term_type=ITER, **kw)
            except hs.HsflowError as e:
                assert e.status == hs._lib.E_SIZE, (name, e)
                continue
            ran += 1
            assert info["iterations_done"] == 6, (name, info)
            want = []
            for A, B in kinds:
                with hs.HSFlow(W, H, 1, own_stream=True) as one:
                    one.set_frames(A, B)
                    one.solve(lam=0.5, max_iter=6, term_type=ITER, **kw)
                    want.append(one.flow())
            for i in sample:
                assert same(ctx.flow(pair=i), want[i % K]), (name, i)
                d = ctx.derivatives(pair=i)
                assert all(np.array_equal(d[k], derivs[i % K][k]) for k in range(3)), (name, i)
        # classic mode: derivatives, planes and the one-sweep kernel all take one grid layer per pair
        ctx.solve(mode=hs.MODE_CLASSIC, alpha=4.0, max_iter=5, term_type=ITER, kernel=hs.KERNEL_SIMPLE)
        cw = [oracle.classic_flow(A, B, 4.0, 5) for A, B in kinds]
        for i in sample:
            assert same(ctx.flow(pair=i), cw[i % K]), ("classic", i)
    assert ran >= 3, ran
