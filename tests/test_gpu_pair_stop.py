"""hsflow_set_pair_termination: under EPS termination every pair of a batched context stops on its own Eps, as
cvCalcOpticalFlowHS called pair by pair does (OpticalFlowOpenCV.cpp:29,94).

The yardstick of pair i is that pair alone in an HSFlow(W, H, 1) context with the same parameters: flow bit for bit
(`same` of tests/test_gpu_batch.py), iterations_done and last_eps equal.  Behind it stands the CPU oracle, run pair by
pair on these inputs (lambda 0.002, epsilon 1e-3, budget 200): its own stopping sweeps are the table ORACLE below.  At
every stop Eps lies at least 1e-6 either side of epsilon (the closest: 512x160 `smooth`, 1.00112e-3 before the stop,
0.97823e-3 at it), an order of magnitude above the 1e-7 by which the GPU's Eps and the oracle's differ, so the stopping
sweep must equal the oracle's for every pair, with no allowance.
"""
import ctypes
import math

import numpy as np
import pytest

from opticalflowhs_amd import synth
from test_gpu_batch import BUDGET, EPS_BATCHES, EPSILON, LAM, eps_pairs, load, same, single_iter, single_probe, stop_of

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2

# the oracle's own stopping sweep of every pair, solved alone
ORACLE = {(48, 40): {"same": 1, "same2": 1, "flat": 6, "random": 41, "golden": 152, "moving": 200},
          (512, 160): {"same": 1, "same2": 1, "flat": 6, "random": 47, "smooth": 164, "moving": 200},
          (600, 480): {"same": 1, "same2": 1, "flat": 6, "random": 49, "smooth": 166, "moving": 200}}
SIZES = sorted(ORACLE)


def sized_pairs(W, H):
    """The set of tests/test_gpu_batch.py's eps_pairs() at a larger size, `smooth` in the place of `golden`."""
    flat = np.full((H, W), 100, np.uint8)
    flat[H // 3:H // 3 + 8, W // 3:W // 3 + 10] = 102
    smooth = synth.smooth_random_pair(W, H, seed=5)
    return {"same": (smooth[0], smooth[0].copy()), "flat": (flat, np.roll(flat, 1, axis=1)), "random": synth.random_pair(W, H, seed=3),
            "smooth": smooth, "moving": synth.translating_pair(W, H, seed=9), "same2": (synth.random_pair(W, H, seed=8)[0],) * 2}


def pairs_of(size):
    return eps_pairs() if size == (48, 40) else sized_pairs(*size)


def batches_of(size):
    if size == (48, 40):
        return EPS_BATCHES
    return {b: [("smooth" if n == "golden" else n) for n in names] for b, names in EPS_BATCHES.items()}


def kernel_of(hs, name):
    return {"strip": hs.KERNEL_STRIP, "fold": hs.KERNEL_FOLD, "simple": hs.KERNEL_SIMPLE, "fused": hs.KERNEL_FUSED, "auto": hs.KERNEL_AUTO}[name]


class Ones(object):
    """One single-pair context per pair, with the same row origin and Eps rows: the yardstick."""

    def __init__(self, hs, size, pairs, rows=None, origin=0):
        self.ctxs = []
        for A, B in pairs:
            c = hs.HSFlow(size[0], size[1], 1, own_stream=True)
            c.set_frames(A, B)
            if origin:
                c.set_row_origin(origin)
            if rows:
                c.set_eps_rows(*rows)
            self.ctxs.append(c)

    def solve(self, **kw):
        """[(flow, info)] of every pair"""
        out = []
        for c in self.ctxs:
            info = c.solve(**kw)
            out.append((c.flow(), info))
        return out

    def close(self):
        for c in self.ctxs:
            c.close()


def wait_solve(ctx):
    ctx._check(ctx._lib.hsflow_wait_solve(ctx._h))


def set_async_reduce(ctx, on):
    ctx._check(ctx._lib.hsflow_set_async_reduce(ctx._h, 1 if on else 0))


def check_pairs(ctx, want, what, counts=None):
    """Every pair of ctx against its one-pair solve: flow bit for bit, iterations_done and last_eps equal; hsflow_info
    by its rule.  Returns the pair results."""
    res = ctx.pair_results()
    assert [r["pair"] for r in res] == list(range(len(want))), what
    for i, (flow, info) in enumerate(want):
        r = res[i]
        print(what, "pair", i, "iterations", r["iterations_done"], "one-pair", info["iterations_done"], "last_eps", r["last_eps"],
              info["last_eps"], "sweeps", r["sweeps_executed"], "rerun", r["eps_rerun"])
        assert r["status"] == 0, (what, i, r)
        assert r["iterations_done"] == info["iterations_done"], (what, i, r, info)
        assert r["last_eps"] == info["last_eps"], (what, i, r, info)
        if counts is not None:
            assert r["iterations_done"] == counts[i], (what, i, r, counts)
        assert same(ctx.flow(pair=i), flow), (what, i)
    info = ctx.info()
    most = max(r["iterations_done"] for r in res)
    first = [r for r in res if r["iterations_done"] == most][0]
    assert info["iterations_done"] == most and info["last_eps"] == first["last_eps"], (what, info, res)
    assert info["eps_rerun"] == (1 if any(r["eps_rerun"] for r in res) else 0), (what, info, res)
    return res


def check_work_bound(res, info, budget, kernel, what):
    """A proven pair ran the budget; a pair that took the exact pass ran at most the witness pass (if one ran)
    + ceil(k / T) * T + k sweeps for a stop at sweep k.  Whether a witness pass ran is read off what ran: the strip or
    the folded kernel, and every pair with at least the budget behind it."""
    T = 32 if info["kernel"] == 1 else info["fuse_steps"]   # 1: HSFLOW_KERNEL_SIMPLE (HSFLOW_PAIR_STOP_SIMPLE_CHUNK)
    witness = info["kernel"] in (3, 4) and all(r["sweeps_executed"] >= budget for r in res)   # STRIP, FOLD
    for r in res:
        k = r["iterations_done"]
        assert r["eps_rerun"] in ((0, 1) if witness else (0,)), (what, r)
        if witness and not r["eps_rerun"]:
            assert r["sweeps_executed"] == budget and k == budget, (what, r)
        else:
            bound = budget * (1 if witness else 0) + int(math.ceil(k / float(T))) * T + k
            assert 0 < r["sweeps_executed"] <= bound, (what, r, T, bound)
            if k < budget and witness:
                assert r["eps_rerun"] == 1, (what, r)


@pytest.mark.parametrize("kernel", ["strip", "fold", "simple", "fused", "auto"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_every_pair_of_a_batch_stops_on_its_own_eps(hs, gpu_ok, size, kernel):
    k = kernel_of(hs, kernel)
    P = pairs_of(size)
    kw = dict(lam=LAM, max_iter=BUDGET, epsilon=EPSILON, term_type=ITER | EPS, kernel=k)
    for bname, names in batches_of(size).items():
        pairs = [P[n] for n in names]
        counts = [ORACLE[size][n] for n in names]
        ones = Ones(hs, size, pairs)
        try:
            want = ones.solve(**kw)
            with hs.HSFlow(size[0], size[1], len(pairs), own_stream=True) as ctx:
                load(ctx, pairs)
                ctx.set_pair_termination(True)
                info = ctx.solve(**kw)
                res = check_pairs(ctx, want, (size, kernel, bname, "solve"), counts)
                check_work_bound(res, info, BUDGET, kernel, (size, kernel, bname))
                if kernel in ("simple", "fused"):
                    continue   # (asynchronous ITER|EPS is the strip / fold kernels')
                info = ctx.solve(use_graph=True, **kw)
                check_pairs(ctx, want, (size, kernel, bname, "graph"), counts)
                for graph in (False, True):
                    ctx.solve_async(use_graph=graph, **kw)
                    ctx.synchronize()
                    res = check_pairs(ctx, want, (size, kernel, bname, "async", graph), counts)
                    check_work_bound(res, ctx.info(), BUDGET, kernel, (size, kernel, bname, "async"))
                # a repeat that takes the owed check over, then the marker route
                ctx.solve_async(use_graph=True, **kw)
                ctx.solve_async(use_graph=True, **kw)
                ctx.synchronize()
                check_pairs(ctx, want, (size, kernel, bname, "repeat"), counts)
                set_async_reduce(ctx, True)
                for graph in (False, True):
                    ctx.solve_async(use_graph=graph, **kw)
                    wait_solve(ctx)
                    check_pairs(ctx, want, (size, kernel, bname, "async_reduce", graph), counts)
                set_async_reduce(ctx, False)
        finally:
            ones.close()


@pytest.mark.parametrize("kernel", ["strip", "fold", "auto"])
def test_a_batch_in_which_no_pair_stops_costs_the_same_launches(hs, gpu_ok, kernel):
    """Two moving pairs: nothing stops, nothing is re-run, and the launches are those of the batch that stops as one
    (the kernels that run a witness pass; the simple and the LDS-tile kernel measure every pair by itself)."""
    size = (512, 160)
    P = pairs_of(size)
    pairs = [P["moving"], synth.translating_pair(size[0], size[1], seed=11)]
    kw = dict(lam=LAM, max_iter=BUDGET, epsilon=EPSILON, term_type=ITER | EPS, kernel=kernel_of(hs, kernel))
    with hs.HSFlow(size[0], size[1], 2, own_stream=True) as ctx:
        load(ctx, pairs)
        off = ctx.solve(**kw)
        flows = [ctx.flow(pair=i) for i in range(2)]
        ctx.set_pair_termination(True)
        on = ctx.solve(**kw)
        assert on["eps_rerun"] == 0 and off["eps_rerun"] == 0 and on["jacobi_launches"] == off["jacobi_launches"], (on, off)
        assert on["iterations_done"] == BUDGET
        for i, r in enumerate(ctx.pair_results()):
            assert r["sweeps_executed"] == BUDGET and r["iterations_done"] == BUDGET and r["eps_rerun"] == 0, r
            assert same(ctx.flow(pair=i), flows[i]), i


@pytest.mark.parametrize("kernel", ["strip", "fold", "simple", "fused", "auto"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_warm_start_and_eps_alone(hs, gpu_ok, size, kernel):
    k = kernel_of(hs, kernel)
    P = pairs_of(size)
    warm = 5
    for bname, names in batches_of(size).items():
        pairs = [P[n] for n in names]
        with hs.HSFlow(size[0], size[1], len(pairs), own_stream=True) as ctx:
            load(ctx, pairs)
            ctx.set_pair_termination(True)
            # a warm start of 5 ITER sweeps, then ITER|EPS from that flow
            ones = Ones(hs, size, pairs)
            try:
                ones.solve(lam=LAM, max_iter=warm, term_type=ITER, kernel=k)
                ctx.solve(lam=LAM, max_iter=warm, term_type=ITER, kernel=k)
                kw = dict(lam=LAM, max_iter=BUDGET - warm, epsilon=EPSILON, term_type=ITER | EPS, use_previous=True, kernel=k)
                want = ones.solve(**kw)
                ctx.solve(**kw)
                counts = None
                if size == (48, 40):
                    counts = [stop_of(single_probe(hs, p, BUDGET - warm, warm=warm, kernel=k), BUDGET - warm) for p in pairs]
                check_pairs(ctx, want, (size, kernel, bname, "warm"), counts)
                if kernel not in ("simple", "fused"):
                    ones.solve(lam=LAM, max_iter=warm, term_type=ITER, kernel=k)
                    ctx.solve(lam=LAM, max_iter=warm, term_type=ITER, kernel=k)
                    ctx.solve_async(**kw)
                    ctx.synchronize()
                    check_pairs(ctx, ones.solve(**kw), (size, kernel, bname, "warm async"), counts)
                # EPS alone, on the batches in which every pair converges
                if bname != "budget":
                    kw = dict(lam=LAM, max_iter=0, epsilon=EPSILON, term_type=EPS, kernel=k)
                    want = ones.solve(**kw)
                    ctx.solve(**kw)
                    check_pairs(ctx, want, (size, kernel, bname, "eps alone"), [ORACLE[size][n] for n in names])
            finally:
                ones.close()


@pytest.mark.parametrize("kernel", ["strip", "fold", "simple", "fused", "auto"])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
def test_row_windows_and_row_origin(hs, gpu_ok, size, kernel):
    """Eps over a row window (the strip and the simple kernel take one; AUTO then picks the strip kernel), and a context
    that sits at an odd row of a larger frame (every kernel)."""
    k = kernel_of(hs, kernel)
    P = pairs_of(size)
    H = size[1]
    names = batches_of(size)["stops_golden"] + ["moving"]
    pairs = [P[n] for n in names]
    kw = dict(lam=LAM, max_iter=BUDGET, epsilon=EPSILON, term_type=ITER | EPS, kernel=k)
    cases = [(None, 1)]
    if kernel in ("strip", "simple", "auto"):
        cases += [((8, 20), 0), ((0, 1), 0), ((H - 1, 1), 0), ((8, 20), 3)]
    for rows, origin in cases:
        ones = Ones(hs, size, pairs, rows=rows, origin=origin)
        try:
            want = ones.solve(**kw)
            with hs.HSFlow(size[0], size[1], len(pairs), own_stream=True) as ctx:
                load(ctx, pairs)
                if origin:
                    ctx.set_row_origin(origin)
                if rows:
                    ctx.set_eps_rows(*rows)
                ctx.set_pair_termination(True)
                ctx.solve(**kw)
                check_pairs(ctx, want, (size, kernel, rows, origin))
                if kernel not in ("simple", "fused"):
                    ctx.solve_async(use_graph=True, **kw)
                    ctx.synchronize()
                    check_pairs(ctx, want, (size, kernel, rows, origin, "async"))
            assert len(set(i["iterations_done"] for _, i in want)) >= 3, (rows, origin)   # the pairs do stop apart
        finally:
            ones.close()


def test_a_stalled_pair_keeps_its_flow_and_the_others_stop(hs, gpu_ok):
    """EPS alone with an epsilon below the limit cycle: the stall rule runs per pair."""
    P = eps_pairs()
    kw = dict(lam=LAM, max_iter=0, epsilon=1e-30, term_type=EPS)
    with hs.HSFlow(48, 40, 1, own_stream=True) as one:
        one.set_frames(*P["golden"])
        with pytest.raises(hs.HsflowError) as e:
            one.solve(**kw)
        assert e.value.status == hs._lib.E_NOTERM
        want, winfo = one.flow(), one.info()
    with hs.HSFlow(48, 40, 3, own_stream=True) as ctx:
        load(ctx, [P["same"], P["golden"], P["same2"]])
        ctx.set_pair_termination(True)
        with pytest.raises(hs.HsflowError) as e:
            ctx.solve(**kw)
        assert e.value.status == hs._lib.E_NOTERM and "pair 1" in str(e.value)
        res = ctx.pair_results()
        assert [r["status"] for r in res] == [0, hs._lib.E_NOTERM, 0], res
        assert res[0]["iterations_done"] == 1 and res[2]["iterations_done"] == 1, res
        assert res[1]["iterations_done"] == winfo["iterations_done"] and res[1]["last_eps"] == winfo["last_eps"], (res, winfo)
        assert same(ctx.flow(pair=1), want)
        for i in (0, 2):
            u, v = ctx.flow(pair=i)
            assert not u.any() and not v.any(), i


# ---- hsflow_solve_probe_pairs ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["strip", "fold", "simple", "fused", "auto"])
def test_probe_pairs_columns_are_the_single_probes_and_rows_give_the_batch(hs, gpu_ok, kernel):
    k = kernel_of(hs, kernel)
    P = eps_pairs()
    e = {name: single_probe(hs, P[name], BUDGET, kernel=k) for name in P}
    for bname, names in EPS_BATCHES.items():
        for on in (False, True):   # independent of the switch
            with hs.HSFlow(48, 40, len(names), own_stream=True) as ctx:
                load(ctx, [P[n] for n in names])
                ctx.set_pair_termination(on)
                batch = ctx.solve_probe(lam=LAM, max_iter=BUDGET, kernel=k)
                got = ctx.solve_probe_pairs(lam=LAM, max_iter=BUDGET, kernel=k)
                assert got.shape == (BUDGET, len(names))
                for i, n in enumerate(names):
                    assert np.array_equal(got[:, i], e[n]), (bname, i, n)
                    assert same(ctx.flow(pair=i), single_iter(hs, P[n], BUDGET)), (bname, i)
                assert np.array_equal(got.max(axis=1), batch), bname
    # a tail launch (13 sweeps at 5 per launch), a row window, a warm start
    if kernel in ("strip", "simple"):
        names = EPS_BATCHES["budget"]
        with hs.HSFlow(48, 40, len(names), own_stream=True) as ctx:
            load(ctx, [P[n] for n in names])
            ctx.set_eps_rows(8, 20)
            ctx.solve(lam=LAM, max_iter=5, term_type=ITER)
            got = ctx.solve_probe_pairs(lam=LAM, max_iter=13, kernel=k, fuse_steps=5 if kernel == "strip" else 0, use_previous=True)
            for i, n in enumerate(names):
                want = single_probe(hs, P[n], 13, rows=(8, 20), warm=5, kernel=k, fuse_steps=5 if kernel == "strip" else 0)
                assert np.array_equal(got[:, i], want), (i, n)


@pytest.mark.parametrize("kernel", ["strip", "fold", "auto"])
def test_probe_pairs_over_more_workgroups_than_xcds(hs, gpu_ok, kernel):
    """11 pairs of 512x160: the words of a pair lie scattered over the launch by the XCD tile permutation."""
    k = kernel_of(hs, kernel)
    W, H, n = 512, 160, 60
    P = sized_pairs(W, H)
    names = ["flat", "random", "same", "smooth", "moving", "random", "same2", "flat", "moving", "smooth", "random"]
    singles = {}
    for name in set(names):
        with hs.HSFlow(W, H, 1, own_stream=True) as c:
            c.set_frames(*P[name])
            singles[name] = c.solve_probe(lam=LAM, max_iter=n, kernel=k)
    with hs.HSFlow(W, H, len(names), own_stream=True) as ctx:
        load(ctx, [P[x] for x in names])
        batch = ctx.solve_probe(lam=LAM, max_iter=n, kernel=k)
        info = ctx.info()
        assert info["tiles"] > 8 and info["tiles"] % len(names) == 0, info
        got = ctx.solve_probe_pairs(lam=LAM, max_iter=n, kernel=k)
        for i, name in enumerate(names):
            assert np.array_equal(got[:, i], singles[name]), (i, name)
        assert np.array_equal(got.max(axis=1), batch)


def test_probe_pairs_with_more_pairs_than_a_grid_dimension(hs, gpu_ok):
    """70 000 pairs of 4x4, as test_more_pairs_than_a_grid_dimension_holds."""
    W, H, N, n = 4, 4, 70000, 6
    kinds = [synth.random_pair(W, H, seed=900 + s) for s in range(5)]
    kinds.insert(2, (np.full((H, W), 255, np.uint8),) * 2)
    kinds.append((np.zeros((H, W), np.uint8),) * 2)
    K = len(kinds)
    singles = []
    for A, B in kinds:
        with hs.HSFlow(W, H, 1, own_stream=True) as one:
            one.set_frames(A, B)
            singles.append(one.solve_probe(lam=0.5, max_iter=n, kernel=hs.KERNEL_STRIP))
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for i in range(N):
            ctx.set_frames(*kinds[i % K], pair=i)
        batch = ctx.solve_probe(lam=0.5, max_iter=n, kernel=hs.KERNEL_STRIP)
        assert ctx.info()["tiles"] > 65535
        got = ctx.solve_probe_pairs(lam=0.5, max_iter=n, kernel=hs.KERNEL_STRIP)
        assert got.shape == (n, N)
        want = np.stack([singles[i % K] for i in range(N)], axis=1)
        assert np.array_equal(got, want), np.nonzero((got != want).any(axis=0))[0][:10]
        assert np.array_equal(got.max(axis=1), batch)


# ---- the switch off ---------------------------------------------------------------------------------------------------

def test_switched_off_again_the_batch_stops_as_one(hs, gpu_ok):
    """test_batch_eps_is_the_maximum_over_pairs_and_stops_every_pair_at_once's "stops_golden" case after a toggle."""
    P = eps_pairs()
    names = EPS_BATCHES["stops_golden"]
    e = {n: single_probe(hs, P[n], BUDGET) for n in names}
    emax = np.maximum.reduce([e[n] for n in names])
    n = stop_of(emax, BUDGET)
    kw = dict(lam=LAM, max_iter=BUDGET, epsilon=EPSILON, term_type=ITER | EPS)
    with hs.HSFlow(48, 40, len(names), own_stream=True) as ctx:
        load(ctx, [P[x] for x in names])
        with pytest.raises(hs.HsflowError) as err:   # before the first solve
            ctx.pair_results()
        assert err.value.status == hs._lib.E_STATE
        ctx.set_pair_termination(True)
        ctx.solve(**kw)
        assert len(set(r["iterations_done"] for r in ctx.pair_results())) == len(names)
        ctx.set_pair_termination(False)
        for how in ("solve", "async"):
            if how == "solve":
                info = ctx.solve(**kw)
            else:
                ctx.solve_async(**kw)
                ctx.synchronize()
                info = ctx.info()
            assert info["iterations_done"] == n and info["last_eps"] == emax[n - 1], (how, info)
            for i, name in enumerate(names):
                assert same(ctx.flow(pair=i), single_iter(hs, P[name], n)), (how, i)
            for i, r in enumerate(ctx.pair_results()):   # the batch's values for every pair
                assert r["pair"] == i and r["status"] == 0 and r["iterations_done"] == n and r["last_eps"] == emax[n - 1], r
                assert r["eps_rerun"] == info["eps_rerun"] and r["sweeps_executed"] >= n, (r, info)
        # ITER alone: nothing to stop on, whatever the switch says
        ctx.set_pair_termination(True)
        info = ctx.solve(lam=LAM, max_iter=17, term_type=ITER)
        assert info["iterations_done"] == 17
        for i, r in enumerate(ctx.pair_results()):
            assert r["iterations_done"] == 17 and r["sweeps_executed"] == 17 and r["status"] == 0, r
            assert same(ctx.flow(pair=i), single_iter(hs, P[names[i]], 17)), i
        # bad arguments on a live context
        r = hs.HsflowPairResult()
        r.struct_size = ctypes.sizeof(r)
        f = ctx._lib.hsflow_get_pair_result
        assert f(ctx._h, len(names), ctypes.byref(r)) == hs._lib.E_ARG and f(ctx._h, -1, ctypes.byref(r)) == hs._lib.E_ARG
        assert f(ctx._h, 0, None) == hs._lib.E_ARG
        r.struct_size -= 4
        assert f(ctx._h, 0, ctypes.byref(r)) == hs._lib.E_ARG
    with hs.HSFlow(48, 40, 1, own_stream=True) as one:   # a one-pair context accepts the switch; nothing changes
        one.set_frames(*P["golden"])
        a = one.solve(**kw)
        fa = one.flow()
        one.set_pair_termination(True)
        b = one.solve(**kw)
        assert a == b and same(one.flow(), fa)
        assert one.pair_results()[0]["iterations_done"] == a["iterations_done"] == ORACLE[(48, 40)]["golden"]


# ---- hsflow_verify, hsflow_take_verdict, refusals, consumers ------------------------------------------------------------

@pytest.mark.parametrize("kernel", ["strip", "fold", "simple", "fused", "auto"])
def test_verify_finds_every_pairs_own_stopping_sweep(hs, gpu_ok, kernel):
    import torch
    k = kernel_of(hs, kernel)
    for size in SIZES:
        P = pairs_of(size)
        kw = dict(lam=LAM, max_iter=BUDGET, epsilon=EPSILON, term_type=ITER | EPS, kernel=k)
        for bname, names in batches_of(size).items():
            counts = [ORACLE[size][n] for n in names]
            with hs.HSFlow(size[0], size[1], len(names), own_stream=True) as ctx:
                load(ctx, [P[n] for n in names])
                ctx.set_pair_termination(True)
                for how in ("solve", "async"):
                    if how == "async" and kernel in ("simple", "fused"):
                        continue
                    if how == "solve":
                        ctx.solve(**kw)
                    else:
                        ctx.solve_async(use_graph=True, **kw)
                    r = ctx.verify()
                    assert r.ok == 1 and r.pair == -1 and r.iterations_done == r.iterations_ref == max(counts), (size, bname, how, r.ok, r.pair)
                    for i, c in enumerate(counts):
                        r = ctx.verify(pair=i)
                        assert r.ok == 1 and r.pair == i and r.iterations_done == c and r.iterations_ref == c, (size, bname, how, i, c)
                if bname != "stops_golden":
                    continue
                # one stopped pair's flow corrupted: verify names that pair
                bad = names.index("flat")
                z = torch.full((2, size[0]), 0.25, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                ctx.set_flow_rows_from(z, z, 3, 2, pair=bad)
                r = ctx.verify()
                assert r.ok == 0 and r.pair == bad and r.u.failing > 0, (r.ok, r.pair)
                for i in range(len(names)):
                    assert ctx.verify(pair=i).ok == (0 if i == bad else 1), i


def test_take_verdict_is_proven_iff_every_pair_is(hs, gpu_ok):
    size = (512, 160)
    P = pairs_of(size)
    kw = dict(lam=LAM, max_iter=BUDGET, epsilon=EPSILON, term_type=ITER | EPS)
    other = synth.translating_pair(size[0], size[1], seed=11)
    for pairs, proven in (([P["moving"], other], True), ([P["moving"], P["flat"]], False)):
        with hs.HSFlow(size[0], size[1], 2, own_stream=True) as ctx:
            load(ctx, pairs)
            ctx.set_pair_termination(True)
            ctx.solve_async(**kw)
            assert ctx.take_verdict() is proven
            assert ctx.info()["iterations_done"] == BUDGET   # nothing is re-run: the flow of the budget stands


def test_refusal_and_consumers_of_a_pair_that_stopped_early(hs, gpu_ok):
    import torch
    size = (512, 160)
    P = pairs_of(size)
    names = ["moving", "flat", "random", "same"]
    pairs = [P[n] for n in names]
    kw = dict(lam=LAM, max_iter=BUDGET, epsilon=EPSILON, term_type=ITER | EPS)
    ones = Ones(hs, size, pairs)
    try:
        ones.solve(**kw)
        with hs.HSFlow(size[0], size[1], len(pairs), own_stream=True) as ctx:
            load(ctx, pairs)
            ctx.set_pair_termination(True)
            with pytest.raises(hs.HsflowError) as e:
                ctx.solve(kernel=hs.KERNEL_PERSIST, **kw)
            assert e.value.status == hs._lib.E_ARG and "pair" in str(e.value) and "PERSIST" in str(e.value), e.value
            for how in ("solve", "async"):
                if how == "solve":
                    ctx.solve(**kw)
                else:
                    ctx.solve_async(use_graph=True, **kw)   # every consumer settles the owed check itself
                for i, one in enumerate(ones.ctxs):
                    assert np.array_equal(ctx.render(pair=i), one.render()), (how, i)
                    assert np.array_equal(ctx.render(route="cl", pair=i), one.render(route="cl")), (how, i)
                    du, dv, stride = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
                    ctx._check(ctx._lib.hsflow_flow_view_device(ctx._h, i, ctypes.byref(du), ctypes.byref(dv), ctypes.byref(stride)))
                    a, b = hs.HsflowPlaneDiff(), hs.HsflowPlaneDiff()
                    one._check(one._lib.hsflow_compare_flow_device(one._h, 0, du, stride.value, dv, stride.value, ctypes.byref(a), ctypes.byref(b)))
                    assert a.differing == 0 and b.differing == 0, (how, i, a.as_dict(), b.as_dict())
                    u, v = one.flow()
                    tu, tv = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
                    torch.cuda.synchronize()
                    a, b = ctx.compare_flow(tu, tv, pair=i)
                    assert a.differing == 0 and b.differing == 0, (how, i)
                    ud, vd = torch.empty_like(tu), torch.empty_like(tv)
                    ctx.flow_rows_to(ud, vd, 0, size[1], pair=i)
                    ctx.synchronize()
                    assert np.array_equal(ud.cpu().numpy(), u) and np.array_equal(vd.cpu().numpy(), v), (how, i)
            # set_flow_device, then a warm start from it: every pair continues from ITS final flow
            z = torch.zeros((4, size[0]), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ctx.set_flow_rows_from(z, z, 10, 4, pair=1)
            ones.ctxs[1].set_flow_rows_from(z, z, 10, 4)
            warm = dict(lam=LAM, max_iter=7, term_type=ITER, use_previous=True)
            ctx.solve(**warm)
            for i, one in enumerate(ones.ctxs):
                one.solve(**warm)
                assert same(ctx.flow(pair=i), one.flow()), ("warm", i)
    finally:
        ones.close()


PERSIST_AUTO_CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
import opticalflowhs_amd as hs
from opticalflowhs_amd import synth
kw = dict(lam=0.002, max_iter=200, epsilon=1e-3, term_type=3, kernel=hs.KERNEL_AUTO)
found = 0
for W, H, N in ((1280, 720, 2), (1600, 900, 2), (1024, 768, 2), (960, 540, 4)):
    moving = synth.translating_pair(W, H, seed=9)
    flat = np.full((H, W), 100, np.uint8)
    flat[H // 3:H // 3 + 8, W // 3:W // 3 + 10] = 102
    pairs = [moving, (flat, np.roll(flat, 1, axis=1))] + [synth.translating_pair(W, H, seed=11 + i) for i in range(N - 2)]
    with hs.HSFlow(W, H, N, own_stream=True) as ctx:
        for i, (A, B) in enumerate(pairs):
            ctx.set_frames(A, B, pair=i)
        ctx.solve_async(**kw)          # the batch that stops as one: AUTO may take the persistent launch
        ctx.synchronize()
        if ctx.info()["persistent"] == 0:
            continue
        found += 1
        ctx.set_pair_termination(True)
        ctx.solve_async(**kw)
        ctx.synchronize()
        info = ctx.info()
        assert info["persistent"] == 0, info
        res = ctx.pair_results()
        for i, (A, B) in enumerate(pairs):
            with hs.HSFlow(W, H, 1, own_stream=True) as one:
                one.set_frames(A, B)
                oi = one.solve(lam=0.002, max_iter=200, epsilon=1e-3, term_type=3, kernel=hs.KERNEL_STRIP)
                u, v = one.flow()
            gu, gv = ctx.flow(pair=i)
            assert res[i]["iterations_done"] == oi["iterations_done"] and res[i]["last_eps"] == oi["last_eps"], (i, res[i], oi)
            assert np.array_equal(gu, u) and np.array_equal(gv, v), i
        assert res[1]["iterations_done"] < 200 == res[0]["iterations_done"], res
print("PERSIST-AUTO-SHAPES", found)
'''


def test_auto_does_not_take_the_persistent_launch_under_the_switch(hs, gpu_ok):
    """HSFLOW_PERSIST_AUTO=1 lets AUTO take the one persistent launch; a batch whose pairs stop each on its own must not
    get it (the launch holds every pair to its last phase).  The variable is read once per process: a child process."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, HSFLOW_PERSIST_AUTO="1")
    r = subprocess.run([sys.executable, "-c", PERSIST_AUTO_CHILD % ROOT], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    shapes = [int(line.split()[1]) for line in r.stdout.splitlines() if line.startswith("PERSIST-AUTO-SHAPES")]
    assert shapes and shapes[0] >= 1, r.stdout[-2000:]   # at least one shape where AUTO does take it with the switch off
