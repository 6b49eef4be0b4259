"""The references alone along the lambda and alpha range (tests/regulariser_axis.py): what test_gpu_regulariser_axis.py
takes for granted.  CPU only.

* Both restatements of cvCalcOpticalFlowHS are finite and agree bit for bit on every rung up to the largest lambda whose
  Ilambda = fl32(1 / lambda) still has a finite fp32 reciprocal; one float further -- FLT_MAX included -- a flat pixel's
  alpha = fl32(1 / Ilambda) is Inf, 0 * Inf is NaN, and the NaN spreads a pixel per sweep.  The C oracle and the NumPy one
  agree on that too (same NaN mask): the header of oracle/hs_cv_oracle.c pins Ilambda and alpha as fp32 stores, so the NaN
  is the original's, not a restatement's.
* The bar of the GPU tests is one the arithmetic meets: a NumPy model of the kernels' fp32 arithmetic lies at most
  4 x d_oracle from the float64 reference on every rung and pair (measured here: 1.2 - 2.1).
* The strip kernels' scaled state stays finite, and equal to the canonical arithmetic, at the edge of the launch cap of
  prepare_solve (hs_solve.hip.h): 32 sweeps per launch on the last lambda with 1/lambda >= 1e-20f, 8 at 3e38 and FLT_MAX.
* The oracle's Eps sequence gives the ITER|EPS test a stopping sweep on every rung above 1e-38.
* The classic oracle is finite wherever alpha^2 is a positive number no smaller than 255 / FLT_MAX; below that (the rung
  1e-19, alpha^2 a denormal) Et / alpha^2 of a flat pixel is Inf and NaN follows, by Kernels.cl's own arithmetic.
"""
import numpy as np
import pytest

import regulariser_axis as ra
from oracle import hs_numpy

ITER = 1


def both(oracle, pair, lam):
    A, B = ra.frames(pair)
    with np.errstate(all="ignore"):
        c = oracle.calc_optical_flow_hs(A, B, lam, ra.SWEEPS, term_type=ITER)
        n = hs_numpy.calc_optical_flow_hs(A, B, lam, ra.SWEEPS, term_type=ITER)
    return c, n


def test_the_rungs_stand_where_the_host_code_decides():
    one = np.float32(1.0)
    assert one / np.float32(ra.CAP_IN) >= np.float32(1e-20) > one / np.float32(ra.CV_RUNGS["cap_out"])
    assert 9e19 < ra.CAP_IN < 1.1e20
    assert one / np.float32(ra.NORMAL_IN) >= np.float32(ra.FLT_MIN) > one / np.float32(ra.CV_RUNGS["normal_out"]) > 0
    assert 8.4e37 < ra.NORMAL_IN < 8.6e37
    assert ra.CV_RUNGS["3e38"] < ra.LARGEST_FINITE < ra.FLT_MAX
    assert 0 < ra.CV_RUNGS["1e-40"] < ra.FLT_MIN and np.isinf(ra.inv32(ra.CV_RUNGS["1e-40"]))
    lams = [ra.CV_RUNGS[r] for r in ra.CV_RUNGS]
    assert lams == sorted(lams) and len(set(lams)) == len(lams)
    assert all(float(np.float32(x)) == x for x in lams)
    # classic: the gate of prepare_classic is 2^-40 <= fl32(alpha * alpha) <= 2^40
    for r in ra.ALPHA_RUNGS:
        assert (2.0 ** -40 <= ra.alpha2(r) <= 2.0 ** 40) == (r in ra.ALPHA_IN_GATE), r
    assert 0 < ra.alpha2("1e-19") < ra.FLT_MIN and ra.alpha2("1e-23") == 0 and np.isfinite(ra.alpha2("1e19")) and np.isinf(ra.alpha2("2e19"))


def test_the_frames_hold_what_the_rungs_need():
    for pair in ra.PAIRS:
        A, B = ra.frames(pair)
        W, H = ra.size_of(pair)
        assert A.shape == (H, W)
        ix, iy, it = hs_numpy.derivatives(A, B)
        for which, want in (("hot", 255), ("still", 0)):
            ys, xs = ra.flat_inner(pair, which)
            assert ys.stop - ys.start >= 12 and xs.stop - xs.start >= 12
            assert ys.start > 8 and xs.start > 8 and ys.stop < H - 8 and xs.stop < W - 8     # clear of the borders
            assert not ix[ys, xs].any() and not iy[ys, xs].any() and (it[ys, xs] == want).all(), (pair, which)
        if pair.startswith("texture"):
            assert np.array_equal(A[:, 40:W // 2], B[:, 40:W // 2]) and not np.array_equal(A[:, W // 2:], B[:, W // 2:])


@pytest.mark.parametrize("rung", ra.FINITE_RUNGS)
def test_both_oracles_are_finite_and_agree(oracle, rung):
    for pair in ra.PAIRS:
        (uc, vc), (un, vn) = both(oracle, pair, ra.CV_RUNGS[rung])
        assert np.isfinite(uc).all() and np.isfinite(vc).all() and np.isfinite(un).all() and np.isfinite(vn).all(), (pair, rung)
        assert np.array_equal(uc, un) and np.array_equal(vc, vn), (pair, rung)
        if rung == "1e-40":          # 1 / denormal = Inf, alpha = 0: nothing ever moves
            assert not uc.any() and not vc.any(), pair
        else:
            assert uc.any() and vc.any(), (pair, rung)
        assert reference_is_shared(oracle, pair, rung, (uc, vc))


def reference_is_shared(oracle, pair, rung, flow):
    r = ra.reference(oracle, pair, rung)
    return np.array_equal(r.oracle[0], flow[0]) and np.array_equal(r.oracle[1], flow[1]) and r.oracle_finite


_nan_counts = {}


@pytest.mark.parametrize("lam", ["one_float_up", "flt_max"])
def test_beyond_the_largest_finite_lambda_both_oracles_yield_nan(oracle, lam):
    """Recorded (u and v alike, C and NumPy alike, one float above the largest finite lambda and FLT_MAX alike): NaN elements
    per plane after 47 sweeps -- noise300x90 10233 of 27000, texture300x90 25372, noise131x67 8268 of 8777, texture131x67 8731
    (every pixel with Ix = Iy = 0 starts one; the smooth texture has many more of them than the two patches)."""
    x = ra.up(ra.LARGEST_FINITE) if lam == "one_float_up" else ra.FLT_MAX
    for pair in ra.PAIRS:
        (uc, vc), (un, vn) = both(oracle, pair, x)
        _nan_counts[pair, lam] = int(np.isnan(uc).sum())
        assert np.isnan(uc).any() and np.isnan(vc).any(), (pair, lam)
        # the two restatements agree: same NaN elements, same bits elsewhere
        assert np.array_equal(uc, un, equal_nan=True) and np.array_equal(vc, vn, equal_nan=True), (pair, lam)
        assert not np.isinf(uc).any() and not np.isinf(vc).any()
        # the NaN starts on the flat pixels and walks a pixel per sweep: 47 sweeps do not fill a plane
        ys, xs = ra.flat_inner(pair, "hot")
        assert np.isnan(uc[ys, xs]).all() and np.isfinite(uc).any()
    assert _nan_counts["noise300x90", lam] == 10233 and _nan_counts["noise131x67", lam] == 8268
    print("NaN elements per plane:", _nan_counts)


@pytest.mark.parametrize("rung", ra.BAR_RUNGS)
def test_the_model_of_the_gpu_arithmetic_meets_the_bar(oracle, rung):
    for pair in ra.PAIRS:
        r = ra.reference(oracle, pair, rung)
        m = ra.model_flow(r.A, r.B, r.lam)
        assert np.isfinite(m[0]).all() and np.isfinite(m[1]).all(), (pair, rung)
        d = ra.distance(m, r.f64)
        print("%s %s: d_oracle %.3g (%.3g of the largest flow %.3g), model %.3g = %.2f x d_oracle" % (pair, rung, r.d_oracle, r.d_oracle / r.fmax, r.fmax, d, d / r.d_oracle))
        assert r.d_oracle > 0 and r.fmax > 0
        assert d <= ra.FACTOR * r.d_oracle, (pair, rung, d, r.d_oracle)
        assert r.d_oracle <= 1e-6 * r.fmax, (pair, rung)     # the bar is a tight one on every rung: relative to the flow, fp32 rounding


def test_the_model_is_zero_and_finite_at_the_ends(oracle):
    for pair in ra.PAIRS:
        A, B = ra.frames(pair)
        u, v = ra.model_flow(A, B, ra.CV_RUNGS["1e-40"])
        assert not u.any() and not v.any()
        # FLT_MAX: coeff = FLT_MIN, al = be = 0 on a flat pixel -- finite, and float64-close by the bar of the neighbouring rung
        u, v = ra.model_flow(A, B, ra.FLT_MAX)
        assert np.isfinite(u).all() and np.isfinite(v).all()
        d = ra.distance((u, v), ra.reference(oracle, pair, "flt_max").f64)
        assert d <= ra.FACTOR * ra.bar_reference(oracle, pair, "flt_max").d_oracle, (pair, d)


@pytest.mark.parametrize("rung,T", [("cap_in", 32), ("3e38", 8), ("flt_max", 8)])
def test_scaled_state_is_finite_at_the_edge_of_the_launch_cap(rung, T):
    """If 32 sweeps per launch overflowed on the last lambda that is allowed them, the threshold of prepare_solve would be
    wrong.  It is not: on a flat pixel with |It| = 255 the largest number formed is 4^33 * 255 / sqrt(1e-20) = 1.9e32."""
    lam = ra.CV_RUNGS[rung]
    for pair in ra.PAIRS:
        A, B = ra.frames(pair)
        u, v, finite = ra.scaled_model_flow(A, B, lam, T)
        assert finite, (pair, rung, T)
        cu, cv = ra.model_flow(A, B, lam)
        # equal bit for bit -- powers of 4 commute with every rounding -- except where the canonical value is (or was formed
        # from) a denormal, which the scaled state carries with all its bits: the project's one exemption, met
        # here only where the texture's flow has decayed to nothing (texture300x90: 3 and 2 elements, all below 1e-37)
        for s, c in ((u, cu), (v, cv)):
            differ = s != c
            assert (np.abs(s[differ]) < ra.DENORMAL_BELOW).all() and (np.abs(c[differ]) < ra.DENORMAL_BELOW).all(), (pair, rung, T, int(differ.sum()))
            assert differ.sum() <= 3 and (pair == ra.DECAYS_TO_DENORMALS or not differ.any()), (pair, rung, T, int(differ.sum()))
        al, be, ga = ra.gpu_coefs(A, B, lam)
        ys, xs = ra.flat_inner(pair, "hot")
        assert not al[ys, xs].any() and not be[ys, xs].any()
        assert float(np.abs(ga).max()) == float(ga[ys, xs].max()) and 0.99 <= float(ga[ys, xs].max()) * np.sqrt(max(1.0 / lam, ra.FLT_MIN)) / 255 <= 1.01


_denormal_differ = {}


@pytest.mark.parametrize("rung", ra.KERNEL_RUNGS + ("flt_max",))
def test_where_scaled_and_canonical_arithmetic_part_on_the_decaying_texture(rung):
    """The bar of the GPU tests' kernel-against-kernel comparison on texture300x90 (ra.DENORMAL_DIFFER, ra.DENORMAL_BELOW): at
    every launch length the forms run with, after 47 sweeps and after the 40 of the ITER|EPS test, the two arithmetics differ
    in at most 5 elements of u and v together, all below 1e-37 (the largest 5.0e-39), all in the static half.  The last rung
    run checks that the constant is the largest count met, not merely above it."""
    lam = ra.CV_RUNGS[rung]
    A, B = ra.frames(ra.DECAYS_TO_DENORMALS)
    for sweeps in (ra.SWEEPS, 40):
        cu, cv = ra.model_flow(A, B, lam, sweeps)
        for T in ra.LAUNCH_LENGTHS:
            if rung in ra.ABOVE_CAP and T > 8:
                continue
            u, v, finite = ra.scaled_model_flow(A, B, lam, T, sweeps)
            assert finite
            n = 0
            for s, c in ((u, cu), (v, cv)):
                differ = s != c
                n += int(differ.sum())
                if differ.any():
                    assert max(np.abs(s[differ]).max(), np.abs(c[differ]).max()) < ra.DENORMAL_BELOW, (rung, sweeps, T)
                    assert np.argwhere(differ)[:, 1].max() < A.shape[1] // 2, (rung, sweeps, T)
            assert n <= ra.DENORMAL_DIFFER, (rung, sweeps, T, n)
            _denormal_differ[rung, sweeps, T] = n
    if len({k[0] for k in _denormal_differ}) == len(ra.KERNEL_RUNGS) + 1:
        assert max(_denormal_differ.values()) == ra.DENORMAL_DIFFER


def test_without_the_cap_a_long_launch_would_leave_the_float_range():
    """The cap is needed where it matters most: 32 sweeps per launch at FLT_MAX carry 4^k * 255 / sqrt(FLT_MIN) past FLT_MAX."""
    A, B = ra.frames("noise131x67")
    assert not ra.scaled_model_flow(A, B, ra.FLT_MAX, 32)[2]


@pytest.mark.parametrize("rung", ra.EPS_RUNGS)
def test_the_oracles_eps_sequence_gives_a_stop(oracle, rung):
    for pair in ra.PAIRS:
        E = ra.oracle_eps(oracle, pair, rung)
        assert len(E) == ra.SWEEPS and np.isfinite(E).all()
        stop = ra.eps_stop(E)
        assert stop is not None, (pair, rung, E[:5], E[-5:])
        k, eps = stop
        assert 2 <= k <= 40 and E[k - 1] < eps < E[:k - 1].min() and eps > 1e-30


@pytest.mark.parametrize("rung", list(ra.ALPHA_RUNGS))
def test_classic_oracle_along_alpha(oracle, rung):
    """Where alpha^2 is a positive number the flow is finite and float64-close -- as long as Et / alpha^2 of a flat pixel stays
    inside fp32: 255 / alpha^2 <= FLT_MAX, alpha^2 >= 7.5e-37.  The rung 1e-19 (alpha^2 = 1e-38, a denormal) lies below that:
    the It = 255 patch divides to Inf, Ex * Inf = 0 * Inf is NaN, and the average carries it on, in the oracle as in a kernel
    that follows Kernels.cl.  alpha^2 = 0 adds 0 / 0 on the It = 0 patch; alpha^2 = Inf divides everything to zero."""
    alpha = ra.ALPHA_RUNGS[rung]
    a2 = ra.alpha2(rung)
    for pair in ra.PAIRS:
        A, B = ra.frames(pair)
        with np.errstate(all="ignore"):
            u, v = oracle.classic_flow(A, B, alpha, ra.SWEEPS)
        nans = int(np.isnan(u).sum() + np.isnan(v).sum())
        if a2 > 0 and np.isfinite(a2) and 255.0 / a2 <= ra.FLT_MAX:
            assert nans == 0 and np.isfinite(u).all() and np.isfinite(v).all(), (pair, rung, nans)
            fu, fv = ra.f64_classic_flow(A, B, alpha)
            fmax = float(max(np.abs(fu).max(), np.abs(fv).max()))
            assert ra.distance((u, v), (fu, fv)) <= 1e-5 * max(fmax, 1e-30), (pair, rung, ra.distance((u, v), (fu, fv)), fmax)
        elif np.isfinite(a2):
            assert rung in ("1e-19", "1e-23") and nans > 0 and not np.isinf(u).any() and not np.isinf(v).any(), (pair, rung)
            ys, xs = ra.flat_inner(pair, "hot")
            assert np.isnan(u[ys, xs]).all()
            if a2 > 0:        # nothing but that overflow makes one: the first sweep's NaN are the flat pixels with |Et| / alpha^2 > FLT_MAX
                first = np.isnan(oracle.classic_flow(A, B, alpha, 1)[0])
                ex, ey, et = oracle.classic_derivatives(A, B)
                assert first.any() and np.array_equal(first, (ex == 0) & (ey == 0) & (np.abs(et).astype(np.float64) / a2 > ra.FLT_MAX)), (pair, rung)
        else:
            assert not u.any() and not v.any(), (pair, rung)
