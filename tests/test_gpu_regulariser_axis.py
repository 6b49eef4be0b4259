"""Cold solves along the whole range of the regularisation weight: lambda from a denormal to FLT_MAX in CV mode, alpha from
where alpha^2 is zero to where it is Inf in classic mode.  tests/regulariser_axis.py has frames, rungs, the float64
reference and the bar; tests/test_regulariser_axis_host.py shows what is taken for granted here.

CV mode.  Every kernel shares sweep_coefs (v_rsq_f32, alpha split as s * s) and the host's coeff = max(1 / lambda, FLT_MIN),
so kernel against kernel cannot see a mistake in either.  Here every form is held against an all-float64 iteration:
max(rms_u, rms_v) <= 4 x d_oracle, d_oracle the distance of the C oracle from the same float64 flow on the same rung and pair
(about 1e-8 of the largest flow everywhere), besides the project's own 1e-4 RMS against the C oracle.  Every measured ratio
goes into the parity report (test_gpu_parity.write_report, key "regulariser_axis").  47 sweeps: 20 + 20 + 7, 32 + 15, 24 + 23, or 5 x 8 + 7 under the cap on
the launch length.

At lambda = FLT_MAX the original (both restatements) returns NaN: alpha = fl32(1 / fl32(1 / lambda)) of a flat pixel is Inf.
The library's al = be = 0 on such a pixel stays finite and float64-close; that behaviour is asserted, not the NaN.

Kernel against kernel is bit for bit by the rule of hs_verify_rule.h (differing values pass only where both are below
1e-30).  On the rungs 1e-20 and below every value of the flow is below 1e-30, so that comparison says nothing and is not
made: the float64 bar is the check there.  From 1e-10 up every element has the same bits in every form on the noise pairs
and on texture131x67, whose flow stays above 1e-28.  texture300x90 lets the flow decay across 150 static columns down to
denormals, where the strip kernels' scaled state keeps bits the canonical arithmetic loses: there at most
ra.DENORMAL_DIFFER elements may differ -- what the host model of the two arithmetics shows at any launch length -- and only
below 1e-37, inside the static half (same_bits).

The persistent launch takes frames at least one region large whose width is a multiple of 4: it runs on the 300x90 pairs
and must refuse the 131x67 ones.
"""
import numpy as np
import pytest

import regulariser_axis as ra
from test_gpu_parity import RMS_TOL, _report as _parity_report, rms, write_report  # noqa: F401  (write_report: the parity report, written again with this module's figures)
from test_gpu_stop_rule import run
from test_gpu_warm_flow import bits, same_by_rule

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
N = ra.SWEEPS

FORMS = {
    "simple": dict(kernel="KERNEL_SIMPLE"),
    "fused": dict(kernel="KERNEL_FUSED"),
    "strip": dict(kernel="KERNEL_STRIP"),
    "strip_T32": dict(kernel="KERNEL_STRIP", fuse_steps=32),
    "strip_R5_1024": dict(kernel="KERNEL_STRIP", strip_rows=5, threads=1024),
    "fold": dict(kernel="KERNEL_FOLD"),
    "fold_T24": dict(kernel="KERNEL_FOLD", fuse_steps=24),
    "persist": dict(kernel="KERNEL_PERSIST", fuse_steps=5, strip_rows=5),
    "auto_graph": dict(kernel="KERNEL_AUTO", use_graph=True),
}
OTHER_FORMS = [f for f in FORMS if f != "simple"]
STRIP_LIKE = ("strip", "strip_T32", "strip_R5_1024", "fold", "fold_T24", "auto_graph")
EPS_FORMS = {"simple": ("sync",), "strip": ("sync", "async"), "fold": ("sync", "async"), "auto_graph": ("graph", "async_graph")}

_report = _parity_report.setdefault("regulariser_axis", {})     # written with the parity report, as test_gpu_warm_flow.py's figures are


def form_kw(hs, form):
    kw = dict(FORMS[form])
    kw["kernel"] = getattr(hs, kw["kernel"])
    graph = kw.pop("use_graph", False)
    how = "async" if form == "persist" else "graph" if graph else "sync"
    return kw, how


def runs_here(form, pair):
    return form != "persist" or ra.size_of(pair)[0] == 300


def refused(hs, pair, form, lam):
    A, B = ra.frames(pair)
    kw, _ = form_kw(hs, form)
    with hs.HSFlow(A.shape[1], A.shape[0], 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        with pytest.raises(hs.HsflowError) as e:
            ctx.solve_async(lam=lam, max_iter=N, term_type=ITER, **kw)
        assert e.value.status == hs._lib.E_SIZE, (pair, form, e.value.status)


_solved = {}


def solved(hs, pair, rung, form, sweeps=N):
    """(u, v, info) of one cold ITER solve (once per pair, rung, form and sweep count; shared, never written again)."""
    key = (pair, rung, form, sweeps)
    if key not in _solved:
        A, B = ra.frames(pair)
        kw, how = form_kw(hs, form)
        with hs.HSFlow(A.shape[1], A.shape[0], 1, own_stream=True) as ctx:
            ctx.set_frames(A, B)
            i = run(ctx, how, lam=ra.CV_RUNGS[rung], max_iter=sweeps, term_type=ITER, **kw)
            u, v = ctx.flow()
        assert i["iterations_done"] == sweeps, (key, i)
        if form != "auto_graph":       # the kernel asked for ran (the persistent launch reports the strip kernel)
            assert i["kernel"] == (hs.KERNEL_STRIP if form == "persist" else kw["kernel"]), (key, i)
        if form == "persist":
            assert i["persistent"] > 0, (key, i)
        u.setflags(write=False)
        v.setflags(write=False)
        _solved[key] = (u, v, i)
    return _solved[key]


def same_bits(pair, rung, form, got, want):
    """Kernel against kernel from lambda = 1e-10 up: the same bits in every element.  On texture300x90 alone, whose flow
    decays to denormals inside the static half, at most ra.DENORMAL_DIFFER elements of the two planes together may differ
    (the host model's count), each with both values finite and below ra.DENORMAL_BELOW, each in the static half."""
    differing = 0
    for g, w in zip(got, want):
        assert np.isfinite(g).all() and np.isfinite(w).all(), (pair, rung, form)
        d = bits(g) != bits(w)
        differing += int(d.sum())
        if pair == ra.DECAYS_TO_DENORMALS and d.any():
            assert max(np.abs(g[d]).max(), np.abs(w[d]).max()) < ra.DENORMAL_BELOW, (pair, rung, form, np.abs(g[d]).max(), np.abs(w[d]).max())
            assert np.argwhere(d)[:, 1].max() < g.shape[1] // 2, (pair, rung, form, np.argwhere(d)[:4])
    _report.setdefault("differing_denormals", {})["%s/%s/%s" % (rung, pair, form)] = differing
    assert differing <= (ra.DENORMAL_DIFFER if pair == ra.DECAYS_TO_DENORMALS else 0), (pair, rung, form, differing)


def check_bar(oracle, pair, rung, form, flow):
    """Finite, within FACTOR x d_oracle of the float64 flow, and (where the oracle has an answer) within the project's RMS_TOL of it."""
    r, bar = ra.reference(oracle, pair, rung), ra.bar_reference(oracle, pair, rung)
    u, v = flow
    assert np.isfinite(u).all() and np.isfinite(v).all(), (pair, rung, form)
    d = ra.distance((u, v), r.f64)
    ratio = d / bar.d_oracle
    _report.setdefault("ratio_to_d_oracle", {})["%s/%s/%s" % (rung, pair, form)] = ratio
    worst = _report.setdefault("worst_ratio_per_rung", {})
    worst[rung] = max(worst.get(rung, 0.0), ratio)
    print("%s %s %s: %.3g from float64 = %.3f x d_oracle %.3g (largest flow %.3g)" % (rung, pair, form, d, ratio, bar.d_oracle, r.fmax))
    assert d <= ra.FACTOR * bar.d_oracle, (pair, rung, form, d, bar.d_oracle, ratio)
    if r.oracle_finite:
        ru, rv = rms(u, r.oracle[0]), rms(v, r.oracle[1])
        assert ru <= RMS_TOL and rv <= RMS_TOL, (pair, rung, form, ru, rv)


@pytest.mark.parametrize("rung", ra.FINITE_RUNGS)
@pytest.mark.parametrize("form", list(FORMS))
def test_against_float64(hs, oracle, gpu_ok, form, rung):
    for pair in ra.PAIRS:
        if not runs_here(form, pair):
            if rung == "1e-3":
                refused(hs, pair, form, ra.CV_RUNGS[rung])
            continue
        u, v, _ = solved(hs, pair, rung, form)
        if rung == "1e-40":      # 1 / lambda = Inf, s = 0: the bar is exact
            assert np.isfinite(u).all() and np.isfinite(v).all() and not u.any() and not v.any(), (pair, form)
        else:
            check_bar(oracle, pair, rung, form, (u, v))


@pytest.mark.parametrize("rung", ra.KERNEL_RUNGS)
@pytest.mark.parametrize("form", OTHER_FORMS)
def test_every_form_leaves_the_bits_of_the_one_sweep_kernel(hs, gpu_ok, form, rung):
    """(The rungs 1e-20 and below are not here: all their values lie below 1e-30, which the rule exempts wholesale.)"""
    for pair in ra.PAIRS:
        if not runs_here(form, pair):
            continue
        want = solved(hs, pair, rung, "simple")
        got = solved(hs, pair, rung, form)
        assert max(np.abs(want[0]).max(), np.abs(want[1]).max()) > 1e-6
        same_bits(pair, rung, form, got[:2], want[:2])


@pytest.mark.parametrize("form", list(FORMS))
def test_launch_lengths_along_the_axis(hs, gpu_ok, form):
    """32 (24 for the folded kernel's form) sweeps per launch are honoured up to the last lambda with 1 / lambda >= 1e-20f; one
    float further, and on every rung above, a strip or fold launch has at most 8."""
    for pair in ra.PAIRS:
        if not runs_here(form, pair):
            continue
        for rung in ra.CV_RUNGS:
            i = solved(hs, pair, rung, form)[2]
            assert i["iterations_done"] == N, (pair, rung, form, i)
            if rung in ra.ABOVE_CAP:
                if form in STRIP_LIKE:
                    assert 1 <= i["fuse_steps"] <= 8, (pair, rung, form, i["fuse_steps"])
            elif "fuse_steps" in FORMS[form]:
                assert i["fuse_steps"] == FORMS[form]["fuse_steps"], (pair, rung, form, i["fuse_steps"])


@pytest.mark.parametrize("form", list(FORMS))
def test_flt_max_stays_finite_where_the_original_yields_nan(hs, oracle, gpu_ok, form):
    for pair in ra.PAIRS:
        if not runs_here(form, pair):
            continue
        assert not ra.reference(oracle, pair, "flt_max").oracle_finite
        u, v, _ = solved(hs, pair, "flt_max", form)
        check_bar(oracle, pair, "flt_max", form, (u, v))
        if form != "simple":
            same_bits(pair, "flt_max", form, (u, v), solved(hs, pair, "flt_max", "simple")[:2])


@pytest.mark.parametrize("rung", ra.EPS_RUNGS)
@pytest.mark.parametrize("form", list(EPS_FORMS))
def test_iter_eps_stops_where_the_oracles_sequence_says(hs, oracle, gpu_ok, form, rung):
    """epsilon halfway (geometrically) between the oracle's E_(k-1) and E_k, at least 0.05 % from either: the solve stops after
    sweep k, by witness launches or by the exact pass it falls back to (eps_rerun says which)."""
    lam = ra.CV_RUNGS[rung]
    kw, _ = form_kw(hs, form)
    for pair in ra.PAIRS:
        k, eps = ra.eps_stop(ra.oracle_eps(oracle, pair, rung))
        want = solved(hs, pair, rung, "simple", sweeps=k)
        A, B = ra.frames(pair)
        with hs.HSFlow(A.shape[1], A.shape[0], 1, own_stream=True) as ctx:
            ctx.set_frames(A, B)
            for how in EPS_FORMS[form]:
                what = (pair, rung, form, how, k, eps)
                i = run(ctx, how, lam=lam, max_iter=N, term_type=ITER | EPS, epsilon=eps, **kw)
                assert i["iterations_done"] == k, (what, i["iterations_done"], i["last_eps"])
                assert i["eps_rerun"] in (0, 1), (what, i)
                assert i["last_eps"] < eps, (what, i["last_eps"])
                _report.setdefault("eps_rerun", {})["%s/%s/%s/%s" % (rung, pair, form, how)] = int(i["eps_rerun"])
                if rung in ra.KERNEL_RUNGS:
                    same_bits(pair, rung, form + "_eps_" + how, ctx.flow(), want[:2])
                else:       # 1e-30, 1e-20: every value lies below 1e-30, where the rule of hs_verify_rule.h lets launch shapes differ
                    same_by_rule(hs, ctx.flow(), want[:2], what)


@pytest.mark.parametrize("size", ra.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("form", ["strip_T32", "fold_T24"])
def test_three_pairs_three_lambdas_on_one_context(hs, gpu_ok, form, size):
    """lambda = 1e-30, 1 and 3e38 one after another, cold each time, on a context of three pairs: every pair is its
    single-pair solve on a fresh context bit for bit.  The solve at 3e38 leaves planes the planner does not call tame; the cold solve after it
    makes them the solver's own again, so a warm solve may have its 32 sweeps per launch without a measurement."""
    names = ["noise%dx%d" % size, "texture%dx%d" % size, "noise%dx%d" % size]
    kw, _ = form_kw(hs, form)
    lams = (("1e-30", ra.CV_RUNGS["1e-30"]), ("one", 1.0), ("3e38", ra.CV_RUNGS["3e38"]))
    single = {}      # every reference from a context that has solved nothing else
    for name in set(names):
        A, B = ra.frames(name)
        for rung, lam in lams:
            if rung in ra.CV_RUNGS:
                single[name, rung] = solved(hs, name, rung, form)[:2]
            else:
                with hs.HSFlow(size[0], size[1], 1, own_stream=True) as one:
                    one.set_frames(A, B)
                    one.solve(lam=lam, max_iter=N, term_type=ITER, **kw)
                    single[name, rung] = one.flow()
    with hs.HSFlow(size[0], size[1], 3, own_stream=True) as ctx:
        for p, name in enumerate(names):
            A, B = ra.frames(name)
            ctx.set_frames(A, B, pair=p)
        for rung, lam in lams:
            i = ctx.solve(lam=lam, max_iter=N, term_type=ITER, **kw)
            assert i["iterations_done"] == N and i["kernel"] == kw["kernel"], (form, size, rung, i)
            assert (i["fuse_steps"] <= 8) == (rung == "3e38"), (form, size, rung, i["fuse_steps"])
            for p, name in enumerate(names):
                u, v = ctx.flow(pair=p)
                u1, v1 = single[name, rung]
                assert np.isfinite(u).all() and np.isfinite(v).all()
                assert np.array_equal(bits(u), bits(u1)) and np.array_equal(bits(v), bits(v1)), (form, size, rung, p)
        cold = ctx.solve(lam=1.0, max_iter=N, term_type=ITER, **kw)
        warm = ctx.solve(lam=1.0, max_iter=N, term_type=ITER, use_previous=True, **kw)
        assert cold["fuse_steps"] == warm["fuse_steps"] == FORMS[form]["fuse_steps"], (form, size, cold["fuse_steps"], warm["fuse_steps"])


# ---- classic mode -------------------------------------------------------------------------------------------------------

CLASSIC_PLAIN = {"simple": dict(kernel="KERNEL_SIMPLE"), "fused": dict(kernel="KERNEL_FUSED")}
# the shapes of tests/test_gpu_frontend.py: default, 6, 4, 2 divide with the hoisted reciprocal; 5, 8, 7 with the complete packed division
CLASSIC_STRIP = {"strip": dict(), "strip_R6": dict(strip_rows=6), "strip_R4": dict(strip_rows=4), "strip_R2_T3": dict(strip_rows=2, fuse_steps=3),
                 "strip_R5": dict(strip_rows=5), "strip_R8_T5": dict(strip_rows=8, fuse_steps=5), "strip_R7": dict(strip_rows=7)}

_classic = {}


def classic_oracle(oracle, pair, rung):
    key = (pair, rung)
    if key not in _classic:
        A, B = ra.frames(pair)
        with np.errstate(all="ignore"):
            _classic[key] = oracle.classic_flow(A, B, ra.ALPHA_RUNGS[rung], N)
    return _classic[key]


def classic_check(hs, oracle, pair, rung, kern, kw):
    A, B = ra.frames(pair)
    uo, vo = classic_oracle(oracle, pair, rung)
    with hs.HSFlow(A.shape[1], A.shape[0], 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        i = ctx.solve(mode=hs.MODE_CLASSIC, alpha=ra.ALPHA_RUNGS[rung], max_iter=N, term_type=ITER, **kw)
        u, v = ctx.flow()
    assert i["kernel"] == kw["kernel"] and i["iterations_done"] == N, (pair, rung, kern, i)
    assert np.array_equal(np.isnan(u), np.isnan(uo)) and np.array_equal(np.isnan(v), np.isnan(vo)), \
        (pair, rung, kern, int(np.isnan(u).sum()), int(np.isnan(uo).sum()))
    assert np.array_equal(u, uo, equal_nan=True) and np.array_equal(v, vo, equal_nan=True), \
        (pair, rung, kern, int((bits(u) != bits(uo)).sum()), int((bits(v) != bits(vo)).sum()))
    _report.setdefault("classic_nan_elements", {})["%s/%s" % (rung, pair)] = int(np.isnan(uo).sum())


@pytest.mark.parametrize("rung", list(ra.ALPHA_RUNGS))
@pytest.mark.parametrize("kern", list(CLASSIC_PLAIN))
def test_classic_one_sweep_and_lds_tile_kernel_on_every_alpha(hs, oracle, gpu_ok, kern, rung):
    """alpha^2 a denormal (1e-19: the It = 255 patch divides to Inf, NaN spreads), zero (1e-23: 0 / 0 besides), Inf (2e19:
    everything divides to zero) and the ordinary rungs: the oracle's bits and the oracle's NaN."""
    kw = dict(CLASSIC_PLAIN[kern])
    kw["kernel"] = getattr(hs, kw["kernel"])
    for pair in ra.PAIRS:
        classic_check(hs, oracle, pair, rung, kern, kw)
    uo, _ = classic_oracle(oracle, ra.PAIRS[0], rung)
    assert np.isnan(uo).any() == (rung in ("1e-19", "1e-23"))


@pytest.mark.parametrize("rung", ra.ALPHA_IN_GATE)
@pytest.mark.parametrize("kern", list(CLASSIC_STRIP))
def test_classic_strip_kernel_at_both_ends_of_its_gate(hs, oracle, gpu_ok, kern, rung):
    kw = dict(CLASSIC_STRIP[kern], kernel=hs.KERNEL_STRIP)
    for pair in ra.PAIRS:
        classic_check(hs, oracle, pair, rung, kern, kw)


@pytest.mark.parametrize("rung,inside", [("below_2^-20", "2^-20"), ("above_2^20", "2^20")])
def test_one_float_outside_the_gate_the_strip_kernel_is_refused(hs, oracle, gpu_ok, rung, inside):
    """... and AUTO falls back to the LDS-tile kernel there, where one float further in it takes the strip kernel on the same frames."""
    alpha = ra.ALPHA_RUNGS[rung]
    for pair in ra.PAIRS:
        A, B = ra.frames(pair)
        uo, vo = classic_oracle(oracle, pair, rung)
        with hs.HSFlow(A.shape[1], A.shape[0], 1, own_stream=True) as ctx:
            ctx.set_frames(A, B)
            i = ctx.solve(mode=hs.MODE_CLASSIC, alpha=ra.ALPHA_RUNGS[inside], max_iter=N, term_type=ITER)
            assert i["kernel"] == hs.KERNEL_STRIP and i["iterations_done"] == N, (pair, inside, i)
            ui, vi = ctx.flow()
            assert np.array_equal(ui, classic_oracle(oracle, pair, inside)[0]) and np.array_equal(vi, classic_oracle(oracle, pair, inside)[1]), (pair, inside)
            for kw in CLASSIC_STRIP.values():
                with pytest.raises(hs.HsflowError) as e:
                    ctx.solve(mode=hs.MODE_CLASSIC, alpha=alpha, max_iter=N, term_type=ITER, kernel=hs.KERNEL_STRIP, **kw)
                assert e.value.status == hs._lib.E_ARG, (pair, rung, kw, e.value.status)
            i = ctx.solve(mode=hs.MODE_CLASSIC, alpha=alpha, max_iter=N, term_type=ITER)      # AUTO: the LDS-tile kernel takes it
            u, v = ctx.flow()
        assert i["kernel"] == hs.KERNEL_FUSED and i["iterations_done"] == N, (pair, rung, i)
        assert np.array_equal(u, uo) and np.array_equal(v, vo) and np.isfinite(u).all(), (pair, rung)
