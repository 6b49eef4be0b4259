"""Warm starts (use_previous) from flow the CALLER wrote, across the float range: tests/warm_flows.py has the inputs.

The method of tests/test_gpu_stop_rule.py: the one-sweep kernel, stepped one sweep per call from the uploaded flow, gives
flows[k]; E_k = max |flow_k - flow_(k-1)| in numpy float32.  That sequence is tied to the CPU oracle once per (frame,
rung) -- RMS of u and of v at most RMS_TOL * max(1, fin), E_k within 4e-7 * max(1, fin), fin the largest |starting
value|: the sweep map is affine, so rounding error scales with the state -- and everything else is compared with it bit
for bit.  "Bit for bit" is the rule of hs_verify_rule.h (hs.compare_planes): differing values pass only where both are
finite and below HSFLOW_VERIFY_TINY; on the two lowest rungs the exempt elements are counted and must stay under 1 % of
the plane.  lambda = 1, 47 sweeps (two launches of 20 and a tail of 7; 32 + 15; ...), then 6 more from the solve's own
result, compared with flows[53].

hsflow_verify refuses a solve that continued from an earlier flow (the starting flow is gone), so the device-side check
after each solve is the same comparison kernel (compare_flow) against the stepped flow, uploaded.

The strip and folded kernels keep 4^k * flow inside a launch.  Without a cap on the launch length that state leaves the
float range on the rungs from 1e24 up (test_warm_flow_host.py has the model); the solve measures flow planes a caller
wrote and shortens its launches ("caller-written flow").  Seen on an MI355X before that cap existed, both frames
alike: every element NaN after 47 sweeps at 1e24 and 1e26 with 32 sweeps per launch (20 and fewer: fine), at 1e30 with 20
and 32, at 1e36 with every strip and fold form down to 5 sweeps per launch -- the model's sweeps 26, 22, 15 and 5; a third
of the plane wrong on the mixed rung; the batch's 1e30 pair "stopped" at sweep 20.  The one-sweep and the LDS-tile kernel
were right throughout, and so were all kernels on the NaN / Inf rungs.  The classic strip kernel's hoisted-reciprocal
division (its default shape at 333x131) returned NaN everywhere at 1e36 (hs_kernels_classic_strip.hip.h has the cause).
"""
import ctypes

import numpy as np
import pytest

import warm_flows as wf
from opticalflowhs_amd import synth
from test_gpu_parity import RMS_TOL, _report, check_stop, rms, write_report  # noqa: F401  (write_report: the parity report, written again with this module's figures)
from test_gpu_stop_rule import down, expected_stop, run, up

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
LAM = 1.0
N, N2 = 47, 53

FORMS = {
    "fused_T5": dict(kernel="KERNEL_FUSED", fuse_steps=5),
    "strip_T20_R5": dict(kernel="KERNEL_STRIP", fuse_steps=20, strip_rows=5, threads=1024),
    "strip_T7_R5_768": dict(kernel="KERNEL_STRIP", fuse_steps=7, strip_rows=5, threads=768),
    "strip_T12_R4": dict(kernel="KERNEL_STRIP", fuse_steps=12, strip_rows=4, threads=1024),
    "strip_T32_R5": dict(kernel="KERNEL_STRIP", fuse_steps=32, strip_rows=5, threads=1024),
    "fold": dict(kernel="KERNEL_FOLD"),
    "fold_T5_R3": dict(kernel="KERNEL_FOLD", fuse_steps=5, strip_rows=3),
    "auto": dict(kernel="KERNEL_AUTO"),
    "strip_T20_R5_graph": dict(kernel="KERNEL_STRIP", fuse_steps=20, strip_rows=5, threads=1024, use_graph=True),
    "fold_graph": dict(kernel="KERNEL_FOLD", use_graph=True),
}
SIMPLE = dict(kernel="KERNEL_SIMPLE")
PERSIST = dict(kernel="KERNEL_PERSIST", fuse_steps=5, strip_rows=5)
EPS_FORMS = {"strip_T20_R5": FORMS["strip_T20_R5"], "fold": FORMS["fold"], "auto": FORMS["auto"], "simple": SIMPLE}
EPS_RUNGS = ("S20", "S1e+18", "S1e+30")


def form_kw(hs, kw):
    kw = dict(kw)
    kw["kernel"] = getattr(hs, kw["kernel"])
    return kw


def upload(ctx, u0, v0, how="plane", pair=0):
    """The starting flow through hsflow_set_flow_device: the whole plane in one call, or in ranges of 7 rows from a pitched tensor."""
    import torch
    H, W = u0.shape
    if how == "plane":
        ud, vd = torch.from_numpy(np.array(u0)).cuda(), torch.from_numpy(np.array(v0)).cuda()
        torch.cuda.synchronize()
        ctx.set_flow_rows_from(ud, vd, 0, H, pair=pair)
    else:
        ud = torch.full((H, W + 10), 7.0, dtype=torch.float32, device="cuda")
        vd = torch.full((H, W + 10), 7.0, dtype=torch.float32, device="cuda")
        ud[:, :W] = torch.from_numpy(np.array(u0)).cuda()
        vd[:, :W] = torch.from_numpy(np.array(v0)).cuda()
        torch.cuda.synchronize()
        for r in range(0, H, 7):
            n = min(7, H - r)
            ctx.set_flow_rows_from(ud[r:r + n, :W], vd[r:r + n, :W], r, n, pair=pair)
    ctx.synchronize()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Ref(object):
    pass


_refs = {}


def reference(hs, oracle, frame, rung):
    """The stepped sequence of one starting flow (computed once, shared, never written again) and how far it lies from the oracle's."""
    key = (frame, rung)
    if key in _refs:
        return _refs[key]
    r = Ref()
    r.frame, r.rung = frame, rung
    r.A, r.B = wf.frames(frame)
    r.H, r.W = r.A.shape
    r.u0, r.v0 = wf.start_flow(frame, rung)
    r.finite = rung in wf.FINITE_RUNGS
    r.flows = [(r.u0, r.v0)]
    with hs.HSFlow(r.W, r.H, 1, own_stream=True) as ctx:
        ctx.set_frames(r.A, r.B)
        upload(ctx, r.u0, r.v0)
        got = ctx.flow()
        assert np.array_equal(bits(got[0]), bits(r.u0)) and np.array_equal(bits(got[1]), bits(r.v0)), key   # the planes hold the caller's bits
        for k in range(N2):
            i = ctx.solve(lam=LAM, max_iter=1, term_type=ITER, kernel=hs.KERNEL_SIMPLE, use_previous=True)
            assert i["iterations_done"] == 1 and i["kernel"] == hs.KERNEL_SIMPLE
            r.flows.append(ctx.flow())
    for f in r.flows[1:]:
        f[0].setflags(write=False)
        f[1].setflags(write=False)
    if r.finite:
        r.fin = wf.fin_of(r.u0, r.v0)
        with np.errstate(over="ignore"):
            r.E = np.array([max(np.abs(r.flows[k][0] - r.flows[k - 1][0]).max(), np.abs(r.flows[k][1] - r.flows[k - 1][1]).max())
                            for k in range(1, N2 + 1)], np.float32)
        r.E.setflags(write=False)
        # the oracle, stepped the same way
        uo, vo = r.u0, r.v0
        worst_rms, worst_e = 0.0, 0.0
        r.oracle_finite = True
        for k in range(1, N + 1):
            with np.errstate(all="ignore"):
                u1, v1 = oracle.calc_optical_flow_hs(r.A, r.B, LAM, 1, term_type=ITER, use_previous=True, velx=uo, vely=vo)
                eo = max(float(np.abs(u1 - uo).max()), float(np.abs(v1 - vo).max()))
            uo, vo = u1, v1
            r.oracle_finite = r.oracle_finite and bool(np.isfinite(uo).all() and np.isfinite(vo).all())
            if np.isfinite(r.flows[k][0]).all() and np.isfinite(r.flows[k][1]).all():
                worst_rms = max(worst_rms, rms(r.flows[k][0], uo), rms(r.flows[k][1], vo))
                worst_e = max(worst_e, abs(float(r.E[k - 1]) - eo))
            else:
                worst_rms = worst_e = float("inf")
        r.worst_rms, r.worst_e = worst_rms, worst_e
    _refs[key] = r
    return r


def same_by_rule(hs, got, want, what):
    """hs_verify_rule.h over both planes: nothing failing; returns the number of exempt (differing, both tiny) elements."""
    exempt = 0
    for g, w in zip(got, want):
        d = hs.compare_planes(g, w)
        assert d.failing == 0, (what, d.failing, d.first_failing, d.max_abs_diff, d.max_ulp, d.nonfinite)
        exempt += d.differing
    return exempt


def device_clean(ctx, want, what):
    """The comparison kernel of hsflow_verify against the stepped flow: nothing failing."""
    import torch
    ud, vd = torch.from_numpy(np.array(want[0])).cuda(), torch.from_numpy(np.array(want[1])).cuda()
    torch.cuda.synchronize()
    du, dv = ctx.compare_flow(ud, vd)
    assert du.failing == 0 and dv.failing == 0, (what, du.failing, dv.failing)


def count_exempt(ref, form, exempt):
    t = _report.setdefault("_warm_flow_exempt_tiny", {})
    t["%s/%s/%s" % (ref.frame, ref.rung, form)] = int(exempt)
    if ref.rung in ("S1e-38", "S1e-30"):
        assert exempt < 0.01 * 2 * ref.W * ref.H, (ref.frame, ref.rung, form, exempt)


@pytest.mark.parametrize("rung", wf.FINITE_RUNGS)
@pytest.mark.parametrize("frame", list(wf.FRAMES))
def test_stepped_sequence_against_the_oracle(hs, oracle, gpu_ok, frame, rung):
    """KERNEL_SIMPLE from a caller-written flow against cvCalcOpticalFlowHS(usePrevious): the project's bar, scaled by the state."""
    ref = reference(hs, oracle, frame, rung)
    scale = max(1.0, ref.fin)
    _report["warm_flow_%s_%s" % (frame, rung)] = {"fin": ref.fin, "rms": ref.worst_rms, "rms_over_fin": ref.worst_rms / ref.fin,
                                                  "rms_over_max_1_fin": ref.worst_rms / scale, "eps_abs_diff_over_max_1_fin": ref.worst_e / scale}
    assert ref.oracle_finite, (frame, rung)
    assert all(np.isfinite(f[0]).all() and np.isfinite(f[1]).all() for f in ref.flows), (frame, rung)
    assert np.isfinite(ref.E).all() and (ref.E > 0).all()
    assert ref.worst_rms <= RMS_TOL * scale, (frame, rung, ref.worst_rms, scale)
    assert ref.worst_e <= 4e-7 * scale, (frame, rung, ref.worst_e, scale)


def warm_solves(hs, ctx, ref, form, kw, how="sync"):
    """47 sweeps from the uploaded flow, then 6 more from the result: both against the stepped sequence."""
    what = (ref.frame, ref.rung, form, how)
    i = run(ctx, how, lam=LAM, max_iter=N, term_type=ITER, use_previous=True, **kw)
    assert i["iterations_done"] == N, (what, i)
    if kw["kernel"] != hs.KERNEL_AUTO:       # the kernel asked for ran (the persistent launch reports the strip kernel)
        assert i["kernel"] == (hs.KERNEL_STRIP if kw["kernel"] == hs.KERNEL_PERSIST else kw["kernel"]), (what, i)
    exempt = same_by_rule(hs, ctx.flow(), ref.flows[N], what)
    device_clean(ctx, ref.flows[N], what)
    i = run(ctx, how, lam=LAM, max_iter=N2 - N, term_type=ITER, use_previous=True, **kw)
    assert i["iterations_done"] == N2 - N, (what, i)
    exempt = max(exempt, same_by_rule(hs, ctx.flow(), ref.flows[N2], what + ("second",)))
    count_exempt(ref, form, exempt)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("rung", wf.FINITE_RUNGS)
@pytest.mark.parametrize("frame", list(wf.FRAMES))
def test_warm_solve_leaves_the_stepped_bits(hs, oracle, gpu_ok, frame, rung, form):
    ref = reference(hs, oracle, frame, rung)
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        upload(ctx, ref.u0, ref.v0)
        kw = form_kw(hs, FORMS[form])
        warm_solves(hs, ctx, ref, form, kw, how="graph" if kw.pop("use_graph", False) else "sync")


@pytest.mark.parametrize("rung", ("S20", "S1e+18", "S1e+30"))
def test_persistent_launch_from_a_written_flow(hs, oracle, gpu_ok, rung):
    ref = reference(hs, oracle, "t260x84", rung)
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        upload(ctx, ref.u0, ref.v0)
        warm_solves(hs, ctx, ref, "persist", form_kw(hs, PERSIST), how="async")


@pytest.mark.parametrize("rung", wf.FINITE_RUNGS)
@pytest.mark.parametrize("frame", list(wf.FRAMES))
def test_upload_in_row_ranges_from_a_pitched_tensor(hs, oracle, gpu_ok, frame, rung):
    ref = reference(hs, oracle, frame, rung)
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        upload(ctx, ref.u0, ref.v0, how="rows7")
        got = ctx.flow()
        assert np.array_equal(bits(got[0]), bits(ref.u0)) and np.array_equal(bits(got[1]), bits(ref.v0))
        warm_solves(hs, ctx, ref, "strip_T20_R5_rows7", form_kw(hs, FORMS["strip_T20_R5"]))


@pytest.mark.parametrize("rung", ("S20", "S1e+30"))
@pytest.mark.parametrize("frame", list(wf.FRAMES))
def test_one_shot_with_use_previous(hs, oracle, gpu_ok, frame, rung):
    ref = reference(hs, oracle, frame, rung)
    H, W = ref.H, ref.W
    velx, vely = np.full((H, W + 8), 7.0, np.float32), np.full((H, W + 8), 7.0, np.float32)
    velx[:, :W], vely[:, :W] = ref.u0, ref.v0
    L = hs._lib.load()
    try:
        st = L.hsflow_calc_optical_flow_hs_8u32f(ref.A.ctypes.data, ref.B.ctypes.data, W, W, H, 1, velx.ctypes.data, vely.ctypes.data, (W + 8) * 4,
                                                 LAM, ITER, N, ctypes.c_double(0.0))
        assert st == 0, L.hsflow_last_error(None)
    finally:
        L.hsflow_release_cached()
    same_by_rule(hs, (velx[:, :W], vely[:, :W]), ref.flows[N], (frame, rung, "one shot"))
    assert np.all(velx[:, W:] == 7.0) and np.all(vely[:, W:] == 7.0)


@pytest.mark.parametrize("form", list(EPS_FORMS))
@pytest.mark.parametrize("rung", EPS_RUNGS)
@pytest.mark.parametrize("frame", list(wf.FRAMES))
def test_iter_eps_stops_where_the_stepped_sequence_says(hs, oracle, gpu_ok, frame, rung, form):
    ref = reference(hs, oracle, frame, rung)
    kw = form_kw(hs, EPS_FORMS[form])
    E = ref.E[:N]
    epsilons = [up(E[20]), down(E[20]), float(E.min()) * 0.5]
    assert expected_stop(E, epsilons[2]) == N and expected_stop(E, epsilons[0]) < N
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        for how in (("sync",) if form == "simple" else ("sync", "async")):
            for eps in epsilons:
                want = expected_stop(E, eps)
                what = (frame, rung, form, how, eps)
                upload(ctx, ref.u0, ref.v0)
                i = run(ctx, how, lam=LAM, max_iter=N, term_type=ITER | EPS, epsilon=eps, use_previous=True, **kw)
                assert i["iterations_done"] == want, (what, i["iterations_done"], want)
                same_by_rule(hs, ctx.flow(), ref.flows[want], what)
                assert np.float32(i["last_eps"]) == E[want - 1], (what, i["last_eps"], E[want - 1])


_oracle_nonfinite = {}


def oracle_nonfinite(oracle, ref, n):
    key = (ref.frame, ref.rung, n)
    if key not in _oracle_nonfinite:
        with np.errstate(all="ignore"):
            _oracle_nonfinite[key] = oracle.calc_optical_flow_hs(ref.A, ref.B, LAM, n, term_type=ITER, use_previous=True, velx=ref.u0, vely=ref.v0)
    return _oracle_nonfinite[key]


@pytest.mark.parametrize("form", ["simple"] + list(FORMS))
@pytest.mark.parametrize("rung", wf.NONFINITE)
@pytest.mark.parametrize("frame", list(wf.FRAMES))
def test_nonfinite_values_spread_one_pixel_per_sweep(hs, oracle, gpu_ok, frame, rung, form):
    ref = reference(hs, oracle, frame, rung)
    kw = form_kw(hs, SIMPLE if form == "simple" else FORMS[form])
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        for n in (7, N):
            upload(ctx, ref.u0, ref.v0)
            i = ctx.solve(lam=LAM, max_iter=n, term_type=ITER, use_previous=True, **kw)
            assert i["iterations_done"] == n and (kw["kernel"] == hs.KERNEL_AUTO or i["kernel"] == kw["kernel"]), i   # the kernel asked for ran
            for g, o, s in zip(ctx.flow(), oracle_nonfinite(oracle, ref, n), ref.flows[n]):
                what = (frame, rung, form, n)
                assert np.array_equal(~np.isfinite(g), ~np.isfinite(o)), what
                assert (~np.isfinite(g)).any() and np.isfinite(g).any(), what
                assert np.array_equal(np.isnan(g), np.isnan(s)) and np.array_equal(np.isfinite(g), np.isfinite(s)), what
                fin = np.isfinite(s)
                assert np.array_equal(bits(g)[fin], bits(s)[fin]), (what, int((bits(g)[fin] != bits(s)[fin]).sum()))


@pytest.mark.parametrize("form", list(EPS_FORMS))
def test_eps_ignores_nan_and_the_solve_still_stops(hs, oracle, gpu_ok, form):
    ref = reference(hs, oracle, "t300x90", "nan")
    kw = form_kw(hs, EPS_FORMS[form])
    with np.errstate(all="ignore"):
        uo, vo, n_o, _ = oracle.calc_optical_flow_hs(ref.A, ref.B, LAM, 30, 0.5, ITER | EPS, use_previous=True, velx=ref.u0, vely=ref.v0, return_info=True)
    assert 1 < n_o < 30
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        for how in (("sync",) if form == "simple" else ("sync", "async")):
            upload(ctx, ref.u0, ref.v0)
            i = run(ctx, how, lam=LAM, max_iter=30, term_type=ITER | EPS, epsilon=0.5, use_previous=True, **kw)
            assert np.isfinite(i["last_eps"]), (form, how, i)
            u, v = ctx.flow()
            if i["iterations_done"] == n_o:              # (else check_stop compares at the GPU's count, and fails on the NaN it meets)
                mu, mv = ~np.isfinite(uo), ~np.isfinite(vo)
                assert np.array_equal(~np.isfinite(u), mu) and np.array_equal(~np.isfinite(v), mv), (form, how)
                got, want = (np.where(mu, 0, u), np.where(mv, 0, v)), (np.where(mu, 0, uo), np.where(mv, 0, vo))
            else:
                got, want = (u, v), (uo, vo)
            check_stop("warm_flow_nan_eps_%s_%s" % (form, how), oracle, ref.A, ref.B, LAM, got, i["iterations_done"], want, n_o, u0=ref.u0, v0=ref.v0)


@pytest.mark.parametrize("kernel,T", [("KERNEL_STRIP", 32), ("KERNEL_FOLD", 24)])
@pytest.mark.parametrize("size", [(300, 90), (259, 161)], ids=lambda s: "%dx%d" % s)
def test_lambda_change_without_a_caller_write(hs, gpu_ok, size, kernel, T):
    """A solve with lambda = 3e38 leaves flow as large as the frames make it (synth.random_pair with seed 8, the frames of
    test_scaled_state_matches_canonical_arithmetic_down_to_denormals: several hundred pixels; nothing near 1e19 on these
    frames); the next solve continues from it with lambda = 1, and no caller wrote anything."""
    frame = size
    W, H = size
    A, B = synth.random_pair(W, H, seed=8)
    res = []
    for kw in (dict(kernel=hs.KERNEL_SIMPLE), dict(kernel=getattr(hs, kernel), fuse_steps=T)):
        with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
            ctx.set_frames(A, B)
            ctx.solve(lam=3e38, max_iter=70, term_type=ITER, **kw)
            first = ctx.flow()
            i = ctx.solve(lam=1.0, max_iter=N, term_type=ITER, use_previous=True, **kw)
            assert i["kernel"] == kw["kernel"] and i["iterations_done"] == N
            res.append((first, ctx.flow()))
    assert max(np.abs(res[0][0][0][np.isfinite(res[0][0][0])]).max(), np.abs(res[0][0][1][np.isfinite(res[0][0][1])]).max()) > 100
    for stage in (0, 1):
        for s, g in zip(res[0][stage], res[1][stage]):
            fin = np.isfinite(s)
            assert np.array_equal(np.isfinite(g), fin), (frame, kernel, stage)
            assert np.array_equal(bits(g)[fin], bits(s)[fin]), (frame, kernel, stage, int((bits(g)[fin] != bits(s)[fin]).sum()))


CLASSIC_KERNELS = {"simple": dict(kernel="KERNEL_SIMPLE"), "fused": dict(kernel="KERNEL_FUSED"), "strip": dict(kernel="KERNEL_STRIP"),
                   "strip_R5": dict(kernel="KERNEL_STRIP", strip_rows=5), "strip_R8": dict(kernel="KERNEL_STRIP", strip_rows=8)}


@pytest.mark.parametrize("kern", list(CLASSIC_KERNELS))
@pytest.mark.parametrize("rung", ("S1", "S1e+06", "S1e+18", "S1e+31", "S1e+36", "nan"))   # 1e31: numerators on both sides of 2^96 x denominator
@pytest.mark.parametrize("alpha", [15.0, 0.3])
def test_classic_mode_from_a_written_flow(hs, oracle, gpu_ok, alpha, rung, kern):
    """The classic kernels (the strip kernel's hand-made division among them) on large numerators, bit for bit against the
    oracle (test_warm_flow_host.py: the classic oracle stays finite on every one of these rungs)."""
    frame = "t333x131"
    A, B = wf.frames(frame)
    u0, v0 = wf.start_flow(frame, rung)
    with np.errstate(all="ignore"):
        uo, vo = oracle.classic_flow(A, B, alpha, 13, use_previous=True, u0=u0, v0=v0)
    kw = form_kw(hs, CLASSIC_KERNELS[kern])
    with hs.HSFlow(A.shape[1], A.shape[0], 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        upload(ctx, u0, v0)
        i = ctx.solve(mode=hs.MODE_CLASSIC, alpha=alpha, max_iter=13, term_type=ITER, use_previous=True, reuse_derivatives=False, **kw)
        assert i["kernel"] == kw["kernel"] and i["iterations_done"] == 13, i
        u, v = ctx.flow()
    assert np.array_equal(u, uo, equal_nan=True) and np.array_equal(v, vo, equal_nan=True), \
        (alpha, rung, kern, int((bits(u) != bits(uo)).sum()), int((bits(v) != bits(vo)).sum()))
    assert np.isnan(uo).any() == (rung == "nan")


@pytest.mark.parametrize("per_pair", [False, True])
@pytest.mark.parametrize("form", ["strip_T20_R5", "fold"])
def test_batch_pairs_do_not_touch_their_neighbours(hs, oracle, gpu_ok, form, per_pair):
    """Rungs 1, 1e30 and NaN side by side in one context: every pair is its single-pair solve, bit for bit."""
    frame, rungs = "t300x90", ("S1", "S1e+30", "nan")
    refs = [reference(hs, oracle, frame, r) for r in rungs]
    kw = form_kw(hs, FORMS[form])
    A, B = wf.frames(frame)
    H, W = A.shape
    solves = [dict(max_iter=N, term_type=ITER)] + ([dict(max_iter=N, term_type=ITER | EPS, epsilon=0.5)] if per_pair else [])
    single = {}
    with hs.HSFlow(W, H, 1, own_stream=True) as one:
        one.set_frames(A, B)
        for p, ref in enumerate(refs):
            for s, sk in enumerate(solves):
                upload(one, ref.u0, ref.v0)
                i = one.solve(lam=LAM, use_previous=True, **sk, **kw)
                single[p, s] = (i["iterations_done"], one.flow())
    done = [single[p, len(solves) - 1][0] for p in range(3)]
    if per_pair:
        assert 1 < done[0] < N and done[1] == N and 1 < done[2] < N, done   # the large pair runs on while its neighbours stop
    with hs.HSFlow(W, H, 3, own_stream=True) as ctx:
        for p in range(3):
            ctx.set_frames(A, B, pair=p)
        ctx.set_pair_termination(per_pair)
        for s, sk in enumerate(solves):
            for p, ref in enumerate(refs):
                upload(ctx, ref.u0, ref.v0, pair=p)
            ctx.solve(lam=LAM, use_previous=True, **sk, **kw)
            res = ctx.pair_results() if per_pair else None
            for p, ref in enumerate(refs):
                what = (form, per_pair, s, p)
                n1, (u1, v1) = single[p, s]
                if res is not None and s == 1:
                    assert res[p]["iterations_done"] == n1 and res[p]["status"] == 0, (what, res[p], n1)
                u, v = ctx.flow(pair=p)
                assert np.array_equal(np.isnan(u), np.isnan(u1)) and np.array_equal(np.isnan(v), np.isnan(v1)), what
                ok = ~np.isnan(u1), ~np.isnan(v1)
                assert np.array_equal(bits(u)[ok[0]], bits(u1)[ok[0]]) and np.array_equal(bits(v)[ok[1]], bits(v1)[ok[1]]), what
                if s == 0 and ref.finite:
                    same_by_rule(hs, (u, v), ref.flows[N], what)


@pytest.mark.parametrize("form", ["strip_T20_R5", "fold", "auto"])
def test_beyond_the_ladder_the_one_sweep_kernel_takes_the_solve(hs, oracle, gpu_ok, form):
    """S = 1e37 (largest value 4.4e37): not one sweep of 4^k * flow fits the float range any more, the canonical arithmetic
    still does (test_warm_flow_host.py).  The solve must say that KERNEL_SIMPLE ran, and an asynchronous ITER|EPS solve is
    complete when the call returns."""
    frame = "t300x90"
    A, B = wf.frames(frame)
    H, W = A.shape
    u0, v0 = wf.scaled(frame, 1e37)
    fin = wf.fin_of(u0, v0)
    with np.errstate(all="ignore"):
        uo, vo = oracle.calc_optical_flow_hs(A, B, LAM, N, term_type=ITER, use_previous=True, velx=u0, vely=v0)
    kw = form_kw(hs, FORMS[form])
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        upload(ctx, u0, v0)
        ctx.solve(lam=LAM, max_iter=N, term_type=ITER, use_previous=True, kernel=hs.KERNEL_SIMPLE)
        want = ctx.flow()
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
        assert rms(want[0], uo) <= RMS_TOL * fin and rms(want[1], vo) <= RMS_TOL * fin, (rms(want[0], uo) / fin, rms(want[1], vo) / fin)
        for how, tt in (("sync", ITER), ("async", ITER), ("sync", ITER | EPS), ("async", ITER | EPS)):
            upload(ctx, u0, v0)
            i = run(ctx, how, lam=LAM, max_iter=N, term_type=tt, epsilon=1e-3, use_previous=True, **kw)
            assert i["kernel"] == hs.KERNEL_SIMPLE and i["fuse_steps"] == 1 and i["iterations_done"] == N, (form, how, tt, i)
            got = ctx.flow()
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (form, how, tt)


@pytest.mark.parametrize("rung", wf.NONFINITE)
def test_nonfinite_values_through_the_persistent_launch(hs, oracle, gpu_ok, rung):
    ref = reference(hs, oracle, "t260x84", rung)
    kw = form_kw(hs, PERSIST)
    with hs.HSFlow(ref.W, ref.H, 1, own_stream=True) as ctx:
        ctx.set_frames(ref.A, ref.B)
        for n in (7, N):
            upload(ctx, ref.u0, ref.v0)
            i = run(ctx, "async", lam=LAM, max_iter=n, term_type=ITER, use_previous=True, **kw)
            assert i["iterations_done"] == n and i["kernel"] == hs.KERNEL_STRIP and i["persistent"] > 0, i
            for g, o, s in zip(ctx.flow(), oracle_nonfinite(oracle, ref, n), ref.flows[n]):
                assert np.array_equal(~np.isfinite(g), ~np.isfinite(o)), (rung, n)
                assert np.array_equal(np.isnan(g), np.isnan(s)) and np.array_equal(np.isfinite(g), np.isfinite(s)), (rung, n)
                fin = np.isfinite(s)
                assert np.array_equal(bits(g)[fin], bits(s)[fin]), (rung, n)


def test_what_the_context_knows_about_its_planes(hs, oracle, gpu_ok):
    """The transitions of the "tame" state, seen through info.fuse_steps (a capped launch is shorter than the 32 sweeps asked
    for) and checked against the stepped sequences: a caller's write is measured; a small measurement, and a solve from
    zero, make the planes the solver's own again; HSFLOW_FLOW_SOLVER_MADE keeps what was known; a classic solve is not
    trusted."""
    frame = "t300x90"
    big, one = reference(hs, oracle, frame, "S1e+30"), reference(hs, oracle, frame, "S1")
    kw = dict(kernel=hs.KERNEL_STRIP, fuse_steps=32, strip_rows=5, threads=1024)
    import torch
    with hs.HSFlow(big.W, big.H, 1, own_stream=True) as ctx:
        ctx.set_frames(big.A, big.B)

        def warm(n, ref, k):
            i = ctx.solve(lam=LAM, max_iter=n, term_type=ITER, use_previous=True, **kw)
            same_by_rule(hs, ctx.flow(), ref.flows[k], (ref.rung, k))
            return i["fuse_steps"]

        upload(ctx, big.u0, big.v0)
        assert warm(N, big, N) < 32                    # a caller's large values: measured, capped
        assert warm(N2 - N, big, N2) == N2 - N          # still 1.6e29: measured again (6 sweeps fit)
        ctx.solve(lam=LAM, max_iter=N, term_type=ITER, **kw)
        cold = ctx.flow()
        assert ctx.solve(lam=LAM, max_iter=N, term_type=ITER, use_previous=True, **kw)["fuse_steps"] == 32   # from zero: the solver's own
        upload(ctx, one.u0, one.v0)
        assert warm(N, one, N) == 32                   # a caller's small values: measured, nothing to cap
        assert warm(N2 - N, one, N2) == N2 - N
        # rows the caller vouches for (this context's own flow, copied out and written back): nothing changes
        ud, vd = (torch.empty((big.H, big.W), dtype=torch.float32, device="cuda") for _ in range(2))
        ctx.flow_rows_to(ud, vd, 0, big.H)
        ctx.synchronize()
        ctx.set_flow_rows_from(ud[-16:], vd[-16:], big.H - 16, 16, solver_made=True)
        ctx.synchronize()
        same_by_rule(hs, ctx.flow(), one.flows[N2], "written back")
        with pytest.raises(hs.HsflowError) as e:
            ctx._check(ctx._lib.hsflow_set_flow_device_ex(ctx._h, 0, 0, 16, ud.data_ptr(), big.W * 4, vd.data_ptr(), big.W * 4, 2))
        assert e.value.status == hs._lib.E_ARG
        # a classic solve from 4.4e18, then a CV warm solve with full-length launches: the bits of the one-sweep kernel
        res = []
        for k in (dict(kernel=hs.KERNEL_SIMPLE), kw):
            u18, v18 = wf.start_flow(frame, "S1e+18")
            upload(ctx, u18, v18)
            ctx.solve(mode=hs.MODE_CLASSIC, alpha=15.0, max_iter=5, term_type=ITER, use_previous=True, kernel=hs.KERNEL_FUSED)
            ctx.solve(lam=LAM, max_iter=N, term_type=ITER, use_previous=True, **k)
            res.append(ctx.flow())
        assert np.isfinite(res[0][0]).all() and np.abs(res[0][0]).max() > 1e15
        same_by_rule(hs, res[1], res[0], "classic, then CV")
    assert np.isfinite(cold[0]).all()
