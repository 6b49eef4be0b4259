"""The stopping rule of an ITER|EPS solve, walked along: ties, launch boundaries, and the ends of the float range.

Everything here is measured against a sequence built from FLOWS only, never from the library's Eps code: the one-sweep
kernel stepped one sweep per call, the flow read back after every sweep, and E_k = max |flow_k - flow_(k-1)| taken in
numpy float32.  (The kernels form the change as fma(4, old, -new) on their scaled state, which is the fp32 subtraction of
the unscaled flows exactly, so a kernel's Eps must equal E_k bit for bit.)  Before the sequence is used it is tied to the
CPU oracle: the stepped flows under the project's RMS bar, E_k under the 4e-7 * fmax bar of tests/test_gpu_blocks.py.
Those two are the only tolerances in this file.  The rule is strict and decided in double: a solve stops after the
first sweep k with float(E_k) < epsilon, else at the budget -- plain Python over the sequence (`expected_stop`).

Frames: synth.translating_pair at 258x81 and 333x150 (the smallest shapes in the suite that give the strip kernel two
tile columns and the folded kernel three) and the golden 48x40 pair (a single tile).  The persistent launch refuses all
three (it wants a width that is a multiple of 4, at least 256, and a core tile as high as a phase is long): it runs on a
translating pair at 260x84, the nearest shape it takes, with 5 sweeps per phase and 5 rows per lane."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN
from opticalflowhs_amd import synth
from test_gpu_parity import RMS_TOL, _report, rms, write_report  # noqa: F401  (write_report: the parity report, written again with this module's counts)

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
INF = float("inf")

# name -> (parameters by name of the kernel constant, runs synchronously, runs asynchronously under ITER|EPS)
FORMS = {
    "simple": (dict(kernel="KERNEL_SIMPLE"), True, False),
    "fused": (dict(kernel="KERNEL_FUSED"), True, False),
    "fused_T5": (dict(kernel="KERNEL_FUSED", fuse_steps=5), True, False),
    "strip_T20_R5": (dict(kernel="KERNEL_STRIP", fuse_steps=20, strip_rows=5), True, True),
    "strip_T7_R5_768": (dict(kernel="KERNEL_STRIP", fuse_steps=7, strip_rows=5, threads=768), True, True),   # odd R, reversed strips
    "strip_T12_R4": (dict(kernel="KERNEL_STRIP", fuse_steps=12, strip_rows=4), True, True),                 # even R, E0 template
    "strip_T7_R2": (dict(kernel="KERNEL_STRIP", fuse_steps=7, strip_rows=2), True, True),
    "fold": (dict(kernel="KERNEL_FOLD"), True, True),
    "fold_T5_R3": (dict(kernel="KERNEL_FOLD", fuse_steps=5, strip_rows=3), True, True),
    "auto": (dict(kernel="KERNEL_AUTO"), True, True),
    "persist": (dict(kernel="KERNEL_PERSIST", fuse_steps=5, strip_rows=5), False, True),                      # asynchronous only
}
WITNESSING = [f for f in FORMS if FORMS[f][2]]
PLAIN_FRAMES = ("t258x81", "t333x150", "golden48x40")
CASES = [(fr, fo) for fo in FORMS for fr in (("t260x84",) if fo == "persist" else PLAIN_FRAMES)]


def form_kw(hs, form):
    kw = dict(FORMS[form][0])
    kw["kernel"] = getattr(hs, kw["kernel"])
    return kw


def modes(form, graph=True):
    _, sync, asyn = FORMS[form]
    return (["sync"] if sync else []) + (["async"] if asyn else []) + (["graph"] if graph and sync else []) + (["async_graph"] if graph and not sync else [])


def frame_of(name):
    """(A, B, lambda, budget): budgets that leave a full launch, a second one and a shorter tail at 5, 7, 12 and 20 sweeps per launch."""
    if name == "golden48x40":
        d = np.load(os.path.join(GOLDEN, "eps_48x40_l0.002_e1e-3.npz"))
        return np.ascontiguousarray(d["A"]), np.ascontiguousarray(d["B"]), 0.002, 44
    W, H, seed, n = {"t258x81": (258, 81, 3, 47), "t333x150": (333, 150, 5, 53), "t260x84": (260, 84, 4, 47)}[name]
    A, B = synth.translating_pair(W, H, seed=seed)
    return np.ascontiguousarray(A), np.ascontiguousarray(B), 0.7, n


class Ref(object):
    pass


_refs = {}


def reference(hs, oracle, name):
    """The stepped sequence of one frame pair (computed once, shared, never written again)."""
    if name in _refs:
        return _refs[name]
    r = Ref()
    r.name = name
    r.A, r.B, r.lam, r.n = frame_of(name)
    r.H, r.W = r.A.shape
    zero = np.zeros((r.H, r.W), np.float32)
    r.flows = [(zero, zero)]
    with hs.HSFlow(r.W, r.H, 1, own_stream=True) as ctx:
        ctx.set_frames(r.A, r.B)
        for k in range(r.n):
            i = ctx.solve(lam=r.lam, max_iter=1, term_type=ITER, kernel=hs.KERNEL_SIMPLE, use_previous=k > 0)
            assert i["iterations_done"] == 1 and i["kernel"] == hs.KERNEL_SIMPLE
            r.flows.append(ctx.flow())
    r.E = np.array([max(np.abs(r.flows[k][0] - r.flows[k - 1][0]).max(), np.abs(r.flows[k][1] - r.flows[k - 1][1]).max())
                    for k in range(1, r.n + 1)], np.float32)
    assert r.E.dtype == np.float32 and np.isfinite(r.E).all() and (r.E > 0).all()
    # ... tied to the CPU oracle, stepped the same way
    uo, vo = zero, zero
    Eo = []
    for k in range(1, r.n + 1):
        u1, v1 = oracle.calc_optical_flow_hs(r.A, r.B, r.lam, 1, term_type=ITER, use_previous=k > 1, velx=uo, vely=vo)
        Eo.append(max(float(np.abs(u1 - uo).max()), float(np.abs(v1 - vo).max())))
        uo, vo = u1, v1
        assert rms(r.flows[k][0], uo) <= RMS_TOL and rms(r.flows[k][1], vo) <= RMS_TOL, (name, k)
    fmax = max(1.0, float(np.abs(uo).max()), float(np.abs(vo).max()))
    assert np.all(np.abs(r.E - np.array(Eo)) <= 4e-7 * fmax), (name, np.abs(r.E - np.array(Eo)).max(), fmax)
    for f in r.flows:
        f[0].setflags(write=False)
        f[1].setflags(write=False)
    r.E.setflags(write=False)
    _refs[name] = r
    return r


def expected_stop(E, eps, first=0):
    """Sweeps an ITER|EPS solve runs that starts after sweep `first` with the rest of the budget: up to the first k with float(E_k) < eps."""
    for k in range(first + 1, len(E) + 1):
        if float(E[k - 1]) < eps:
            return k - first
    return len(E) - first


def up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def down(x):
    return float(np.nextafter(np.float32(x), np.float32(0)))


def run(ctx, how, **kw):
    """One solve; the report as the caller of that mode gets it (an asynchronous solve's through info(), which measures last_eps on demand)."""
    if how in ("sync", "graph"):
        return ctx.solve(use_graph=how == "graph", **kw)
    ctx.solve_async(use_graph=how == "async_graph", **kw)
    ctx.synchronize()
    return ctx.info()


def clean(r):
    return (r.ok == 1 and r.iterations_ref == r.iterations_done and r.u.differing == 0 and r.v.differing == 0 and r.deriv_differing == 0
            and r.u.failing == 0 and r.v.failing == 0)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def warm(ctx, ref, k):
    """The reference flow after k sweeps becomes the context's flow."""
    import torch
    ud, vd = (torch.from_numpy(np.array(x)).cuda() for x in ref.flows[k])
    torch.cuda.synchronize()
    ctx.set_flow_rows_from(ud, vd, 0, ref.H)
    ctx.synchronize()


def tally(checked, off):
    t = _report.setdefault("_stop_rule_exact", {"stops_checked": 0, "off_the_expected_sweep": 0})
    t["stops_checked"] += checked
    t["off_the_expected_sweep"] += off


def check_solve(ctx, ref, info, want_n, first=0, what=None, verify=True):
    """count, flow, last_eps and verify() of a solve that started after sweep `first`."""
    tally(1, int(info["iterations_done"] != want_n))
    assert info["iterations_done"] == want_n, (what, info["iterations_done"], want_n)
    assert same(ctx.flow(), ref.flows[first + want_n]), what
    assert np.float32(info["last_eps"]) == ref.E[first + want_n - 1], (what, info["last_eps"], ref.E[first + want_n - 1])
    if verify:
        assert clean(ctx.verify()), what


def refuses_async_eps(hs, ctx, ref, kw):
    with pytest.raises(hs.HsflowError) as e:
        ctx.solve_async(lam=ref.lam, max_iter=ref.n, term_type=ITER | EPS, epsilon=1e-3, **kw)
    assert e.value.status == hs._lib.E_ARG


@pytest.mark.parametrize("frame,form", CASES)
def test_every_sweeps_eps_is_the_fp32_change_of_the_flow(hs, oracle, gpu_ok, frame, form):
    ref = reference(hs, oracle, frame)
    kw = form_kw(hs, form)
    n, lam = ref.n, ref.lam
    tiny = FLT_MIN   # no sweep's change is below it: the budget runs out
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        for first in (0, 5):                                  # cold, and a warm start after 5 sweeps
            if first:
                warm(ctx, ref, first)
            e = ctx.solve_probe(lam=lam, max_iter=n - first, term_type=ITER, use_previous=first > 0, **kw)
            assert e.dtype == np.float32 and np.array_equal(e, ref.E[first:]), (frame, form, first, np.flatnonzero(e != ref.E[first:])[:4])
            assert same(ctx.flow(), ref.flows[n])
            for how in modes(form, graph=False):              # WitnessLast (synchronous) / measured on demand (asynchronous)
                if first:
                    warm(ctx, ref, first)
                i = run(ctx, how, lam=lam, max_iter=n - first, term_type=ITER | EPS, epsilon=tiny, use_previous=first > 0, **kw)
                check_solve(ctx, ref, i, n - first, first, (frame, form, how, first), verify=False)
        if not FORMS[form][2]:
            refuses_async_eps(hs, ctx, ref, kw)
        # over a row window that cuts a tile row: the strip and the simple kernel only, the others refuse a window
        y0, y1 = 7, ref.H - 9
        Ew = np.array([max(np.abs(ref.flows[k][0][y0:y1] - ref.flows[k - 1][0][y0:y1]).max(),
                           np.abs(ref.flows[k][1][y0:y1] - ref.flows[k - 1][1][y0:y1]).max()) for k in range(1, n + 1)], np.float32)
        ctx.set_eps_rows(y0, y1 - y0)
        if kw["kernel"] in (hs.KERNEL_STRIP, hs.KERNEL_SIMPLE):
            e = ctx.solve_probe(lam=lam, max_iter=n, term_type=ITER, **kw)
            assert np.array_equal(e, Ew), (frame, form, "window", np.flatnonzero(e != Ew)[:4])
            i = ctx.solve(lam=lam, max_iter=n, term_type=ITER | EPS, epsilon=tiny, **kw)
            assert i["iterations_done"] == n and np.float32(i["last_eps"]) == Ew[-1] and same(ctx.flow(), ref.flows[n]), (frame, form, i)
        elif kw["kernel"] in (hs.KERNEL_FOLD, hs.KERNEL_FUSED):
            with pytest.raises(hs.HsflowError) as err:
                ctx.solve_probe(lam=lam, max_iter=n, term_type=ITER, **kw)
            assert err.value.status == hs._lib.E_ARG


def tie_sweeps(T, n):
    """Sweep 1, the last sweep of the first launch, the first of the second, one inside the tail launch, the budget's last."""
    launches = -(-n // T)
    tail0 = (launches - 1) * T                               # sweeps before the tail launch
    return sorted({1, min(T, n), min(T + 1, n), tail0 + max(1, (n - tail0 + 1) // 2), n})


@pytest.mark.parametrize("frame,form", CASES)
def test_ties_stop_where_the_strict_rule_says(hs, oracle, gpu_ok, frame, form):
    ref = reference(hs, oracle, frame)
    kw = form_kw(hs, form)
    n, lam, E = ref.n, ref.lam, ref.E
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        # the launch boundaries of this form on this frame, from the solve's own report
        i0 = run(ctx, modes(form)[0], lam=lam, max_iter=n, term_type=ITER, **kw)
        T = i0["fuse_steps"]
        assert 1 <= T <= n and i0["iterations_done"] == n
        if form != "persist":                                # (the plan query stands for a synchronous solve, which the persistent launch refuses under EPS)
            pq = hs.plan_query(ref.W, ref.H, 1, lam=lam, max_iter=n, term_type=ITER | EPS, epsilon=float(E[0]), **kw)
            assert pq["fuse_steps"] == T and pq["jacobi_launches"] == -(-n // T), (pq, T)
        ks = tie_sweeps(T, n)
        assert ks[0] == 1 and ks[-1] == n and (T == 1 or n <= T or T in ks and T + 1 in ks), (T, ks)
        quarter = ks[len(ks) // 2]
        for how in modes(form):
            for k in ks:
                ek = float(E[k - 1])
                cases = [ek, up(ek), down(ek)]
                if k == quarter:                             # a double strictly between two floats: E_k < eps, the stop is at k
                    q = ek + (up(ek) - ek) * 0.25
                    assert ek < q < up(ek) and float(np.float32(q)) == ek
                    cases.append(q)
                for eps in cases:
                    want = expected_stop(E, eps)
                    i = run(ctx, how, lam=lam, max_iter=n, term_type=ITER | EPS, epsilon=eps, **kw)
                    assert i["fuse_steps"] == T, (i, T)
                    check_solve(ctx, ref, i, want, 0, (frame, form, how, k, eps.hex()))
            # once more from a warm start after 5 sweeps: a tie in the second launch of THAT solve
            first = 5
            k = min(first + T + 1, n)
            for eps in (float(E[k - 1]), up(E[k - 1])):
                warm(ctx, ref, first)
                i = run(ctx, how, lam=lam, max_iter=n - first, term_type=ITER | EPS, epsilon=eps, use_previous=True, **kw)
                check_solve(ctx, ref, i, expected_stop(E, eps, first), first, (frame, form, how, "warm", k, eps.hex()), verify=False)
        # what the ties are there for: the strict rule put a stop on both sides of one of them
        assert expected_stop(E, up(E[0])) == 1 and expected_stop(E, float(E[0])) > 1


LARGE = [INF, 1e39, FLT_MAX, 2.0 ** 127, 2.0 ** 126, 2.0 ** 100, 1e30]
SMALL = [FLT_MIN, 1e-40, 5e-324, 0.0, -1.0, float("nan")]


def oracle_stop(oracle, A, B, lam, n, eps):
    with np.errstate(over="ignore"):                         # (the oracle's front end rounds epsilon through fp32, as cvTermCriteria does)
        return oracle.calc_optical_flow_hs(A, B, lam, n, eps, ITER | EPS, return_info=True)[2]


_oracle_seen = set()


def oracle_agrees(oracle, ref):
    """The expectation of the two lists, on the oracle itself (once per frame)."""
    if ref.name in _oracle_seen:
        return
    for eps in LARGE:
        assert oracle_stop(oracle, ref.A, ref.B, ref.lam, ref.n, eps) == 1 == expected_stop(ref.E, eps), eps
    for eps in SMALL:
        assert oracle_stop(oracle, ref.A, ref.B, ref.lam, ref.n, eps) == ref.n == expected_stop(ref.E, eps), eps
    _oracle_seen.add(ref.name)


@pytest.mark.parametrize("form", list(FORMS))
def test_epsilon_at_the_ends_of_the_float_range(hs, oracle, gpu_ok, form):
    ref = reference(hs, oracle, "t260x84" if form == "persist" else "t258x81")
    oracle_agrees(oracle, ref)
    kw = form_kw(hs, form)
    n, lam = ref.n, ref.lam
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        for how in modes(form, graph=False):
            run(ctx, how, lam=lam, max_iter=n, term_type=ITER, **kw)
            plain = ctx.flow()
            assert same(plain, ref.flows[n])
            for eps in LARGE:
                i = run(ctx, how, lam=lam, max_iter=n, term_type=ITER | EPS, epsilon=eps, **kw)
                check_solve(ctx, ref, i, 1, 0, (form, how, eps))
            for eps in SMALL:
                i = run(ctx, how, lam=lam, max_iter=n, term_type=ITER | EPS, epsilon=eps, **kw)
                check_solve(ctx, ref, i, n, 0, (form, how, eps))
                assert same(ctx.flow(), plain)
                # no sweep's change is below FLT_MIN on this pair: the witness pass (where one runs) holds, nothing is re-run;
                # a NaN gets no witness pass at all
                assert i["eps_rerun"] == 0, (form, how, eps, i)
        # EPS alone: a finite epsilon above every change stops at sweep 1; one that can never stop is refused before anything is launched
        if FORMS[form][1]:
            for eps in (FLT_MAX, 1e30):
                i = ctx.solve(lam=lam, max_iter=0, term_type=EPS, epsilon=eps, **kw)
                check_solve(ctx, ref, i, 1, 0, (form, "EPS alone", eps))
            for eps in (INF, 0.0, -1.0, float("nan")):
                with pytest.raises(hs.HsflowError) as err:
                    ctx.solve(lam=lam, max_iter=0, term_type=EPS, epsilon=eps, **kw)
                assert err.value.status == hs._lib.E_NOTERM, (form, eps)
                assert same(ctx.flow(), ref.flows[1])        # (nothing ran)


@pytest.mark.parametrize("per_pair", [False, True])
def test_epsilon_at_the_ends_on_a_three_pair_context(hs, oracle, gpu_ok, per_pair):
    names = ("t258x81", "t333x150")
    ref = reference(hs, oracle, names[0])
    oracle_agrees(oracle, ref)
    n, lam, W, H = ref.n, ref.lam, ref.W, ref.H
    pairs = [(ref.A, ref.B)] + [synth.translating_pair(W, H, seed=s) for s in (11, 12)]
    want = {}
    with hs.HSFlow(W, H, 1, own_stream=True) as one:         # every pair's flow after 1 and after n sweeps, by the one-sweep kernel
        for p, (A, B) in enumerate(pairs):
            one.set_frames(A, B)
            for k in (1, n):
                one.solve(lam=lam, max_iter=k, term_type=ITER, kernel=hs.KERNEL_SIMPLE)
                want[p, k] = one.flow()
    assert same(want[0, 1], ref.flows[1]) and same(want[0, n], ref.flows[n])
    for eps in LARGE[:1] + SMALL[:1]:                         # (the other pairs stop where pair 0 does)
        for p in (1, 2):
            assert oracle_stop(oracle, pairs[p][0], pairs[p][1], lam, n, eps) == (1 if eps > 1 else n)
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        for p, (A, B) in enumerate(pairs):
            ctx.set_frames(A, B, pair=p)
        ctx.set_pair_termination(per_pair)
        for form in ("simple", "strip_T20_R5", "fold", "auto"):
            kw = form_kw(hs, form)
            for how in modes(form, graph=False):
                for eps, k in [(e, 1) for e in LARGE] + [(e, n) for e in SMALL]:
                    i = run(ctx, how, lam=lam, max_iter=n, term_type=ITER | EPS, epsilon=eps, **kw)
                    tally(1, int(i["iterations_done"] != k))
                    assert i["iterations_done"] == k, (form, how, eps, i)
                    res = ctx.pair_results()
                    assert [r["iterations_done"] for r in res] == [k] * 3 and [r["status"] for r in res] == [0] * 3, (form, how, eps, res)
                    for p in range(3):
                        assert same(ctx.flow(pair=p), want[p, k]), (form, how, eps, p)
                    assert clean(ctx.verify()), (form, how, eps)


@pytest.mark.parametrize("frame,depth,lanes", [("t333x150", 3, 2), ("t258x81", 3, 3)])
def test_epsilon_at_the_ends_through_the_pair_pipeline(hs, oracle, gpu_ok, frame, depth, lanes):
    """submit_device on shared streams; with three lanes the pipeline picks its own launch shape at 258x81."""
    import torch
    ref = reference(hs, oracle, frame)
    oracle_agrees(oracle, ref)
    a, b = torch.from_numpy(ref.A).cuda(), torch.from_numpy(ref.B).cuda()
    torch.cuda.synchronize()
    with hs.PairPipeline(ref.W, ref.H, depth=depth, lanes=lanes) as pl:
        tickets = []
        for eps, k in [(e, 1) for e in LARGE] + [(e, ref.n) for e in SMALL]:
            tickets.append((pl.submit_device(a, b, lam=ref.lam, max_iter=ref.n, term_type=ITER | EPS, epsilon=eps), eps, k))
            if len(tickets) < depth:
                continue
            t, e0, k0 = tickets.pop(0)                        # the oldest pair in flight
            i = pl.info(t)
            tally(1, int(i["iterations_done"] != k0))
            assert i["iterations_done"] == k0 and np.float32(i["last_eps"]) == ref.E[k0 - 1], (frame, e0, i)
            assert same([x.cpu().numpy() for x in pl.flow_device(t)], ref.flows[k0]), (frame, e0)
            assert clean(pl.verify(t)), (frame, e0)
        for t, e0, k0 in tickets:
            i = pl.info(t)
            tally(1, int(i["iterations_done"] != k0))
            assert i["iterations_done"] == k0 and same([x.cpu().numpy() for x in pl.flow_device(t)], ref.flows[k0]), (frame, e0, i)


def test_epsilon_at_the_ends_through_the_one_shot_and_the_row_slabs(hs, oracle, gpu_ok):
    ref = reference(hs, oracle, "t333x150")
    oracle_agrees(oracle, ref)
    n, lam, W, H = ref.n, ref.lam, ref.W, ref.H
    L = hs._lib.load()
    for eps, k in [(e, 1) for e in LARGE] + [(e, n) for e in SMALL]:
        u, v = np.full((H, W), 7.0, np.float32), np.full((H, W), 7.0, np.float32)
        st = L.hsflow_calc_optical_flow_hs_8u32f(ref.A.ctypes.data, ref.B.ctypes.data, W, W, H, 0, u.ctypes.data, v.ctypes.data, W * 4,
                                                 lam, ITER | EPS, n, ctypes.c_double(eps))
        assert st == 0, (eps, L.hsflow_last_error(None))
        tally(1, int(not same((u, v), ref.flows[k])))
        assert same((u, v), ref.flows[k]), ("one shot", eps)
    for eps in (FLT_MAX, 1e30):                               # EPS alone through the same entry
        u, v = np.zeros((H, W), np.float32), np.zeros((H, W), np.float32)
        assert L.hsflow_calc_optical_flow_hs_8u32f(ref.A.ctypes.data, ref.B.ctypes.data, W, W, H, 0, u.ctypes.data, v.ctypes.data, W * 4,
                                                   lam, EPS, 0, ctypes.c_double(eps)) == 0
        assert same((u, v), ref.flows[1]), ("one shot, EPS alone", eps)
    for eps in (INF, 0.0, -1.0, float("nan")):
        assert L.hsflow_calc_optical_flow_hs_8u32f(ref.A.ctypes.data, ref.B.ctypes.data, W, W, H, 0, u.ctypes.data, v.ctypes.data, W * 4,
                                                   lam, EPS, 0, ctypes.c_double(eps)) == hs._lib.E_NOTERM, eps
    L.hsflow_release_cached()
    with hs.SlabFrame(W, H, devices=(0, 0), halo=12) as s:
        s.set_frames(ref.A, ref.B)
        for eps, k in [(e, 1) for e in LARGE] + [(e, n) for e in SMALL]:
            s.solve(lam=lam, max_iter=n, term_type=ITER | EPS, epsilon=eps)
            tally(1, int(s.iterations_done() != k))
            assert s.iterations_done() == k, ("slabs", eps, s.iterations_done())
            assert same(s.flow(), ref.flows[k]), ("slabs", eps)


def largest_fuse_steps(hs, W, H, n, lam, kernel):
    """The largest fuse_steps the planner admits: the bound in the code, then what the plan query makes of it and of one more."""
    import re
    from conftest import ROOT
    m = re.search(r"constexpr\s+int\s+kMaxFuse\s*=\s*(\d+)\s*;", open(os.path.join(ROOT, "opticalflowhs_amd", "csrc", "hs_context.hip.h")).read())
    assert m
    bound = int(m.group(1))
    got = [hs.plan_query(W, H, 1, lam=lam, max_iter=n, term_type=ITER | EPS, epsilon=1.0, kernel=kernel, fuse_steps=T)["fuse_steps"] for T in (bound, bound + 1)]
    assert got == [bound, bound], (got, bound)
    return bound


@pytest.mark.parametrize("kernel", ["KERNEL_STRIP", "KERNEL_FOLD"])
def test_mid_range_epsilon_never_proves_anything(hs, oracle, gpu_ok, kernel):
    """Thresholds that leave the float range part-way through a launch: the longest launch the planner admits."""
    ref = reference(hs, oracle, "t333x150")
    n, lam = ref.n, ref.lam
    k = getattr(hs, kernel)
    T = largest_fuse_steps(hs, ref.W, ref.H, n, lam, k)
    assert T < n
    edge = math.ldexp(1.0, 127 - 2 * T)
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        for how in ("sync", "async"):
            for eps in (edge * 0.5, edge, edge * 2, 2.0 ** 89, 2.0 ** 126):
                assert expected_stop(ref.E, eps) == 1
                i = run(ctx, how, lam=lam, max_iter=n, term_type=ITER | EPS, epsilon=eps, kernel=k, fuse_steps=T)
                assert i["fuse_steps"] == T and i["kernel"] == k, i
                check_solve(ctx, ref, i, 1, 0, (kernel, how, eps))
