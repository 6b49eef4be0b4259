"""The reference alone on caller-written starting flows (tests/warm_flows.py): what test_gpu_warm_flow.py takes for granted.

CPU only.  Both restatements of cvCalcOpticalFlowHS (oracle/hs_cv_oracle.c, oracle/hs_numpy.py) stay finite on every rung
of the ladder and agree bit for bit; non-finite starting values spread alike in both; and the model that places the rungs:
a kernel that keeps 4^k * flow after k sweeps of a launch leaves the float range at sweep 26, 22, 15 and 5 of a launch on
the rungs 1e24, 1e26, 1e30 and 1e36, and never on a rung at or below 1e19.
"""
import numpy as np
import pytest

import warm_flows as wf
from oracle import hs_numpy

ITER, EPS = 1, 2
SWEEPS = 47


def both(oracle, A, B, lam, n, u0, v0, **kw):
    with np.errstate(all="ignore"):
        a = oracle.calc_optical_flow_hs(A, B, lam, n, use_previous=True, velx=u0, vely=v0, **kw)
        b = hs_numpy.calc_optical_flow_hs(A, B, lam, n, use_previous=True, velx=u0, vely=v0, **kw)
    return a, b


@pytest.mark.parametrize("rung", wf.FINITE_RUNGS)
@pytest.mark.parametrize("frame", list(wf.FRAMES))
def test_both_oracles_stay_finite_and_agree(oracle, frame, rung):
    A, B = wf.frames(frame)
    u0, v0 = wf.start_flow(frame, rung)
    assert np.isfinite(u0).all() and np.isfinite(v0).all()
    for lam in (0.7, 1.0):
        (uc, vc), (un, vn) = both(oracle, A, B, lam, SWEEPS, u0, v0, term_type=ITER)
        assert np.isfinite(uc).all() and np.isfinite(vc).all(), (frame, rung, lam)
        assert np.array_equal(uc, un) and np.array_equal(vc, vn), (frame, rung, lam)


def test_one_rung_above_the_ladder_is_still_finite(oracle):
    """S = 1e37: where no strip launch fits any more (test_gpu_warm_flow.py) the reference still has an answer."""
    A, B = wf.frames("t300x90")
    u0, v0 = wf.scaled("t300x90", 1e37)
    (uc, vc), (un, vn) = both(oracle, A, B, 1.0, SWEEPS, u0, v0, term_type=ITER)
    assert np.isfinite(uc).all() and np.isfinite(vc).all() and np.array_equal(uc, un) and np.array_equal(vc, vn)


def test_lowest_rung_holds_denormals_and_mixed_rung_both_scales():
    tiny = float(np.finfo(np.float32).tiny)
    for frame in wf.FRAMES:
        u0, _ = wf.start_flow(frame, "S1e-38")
        a = np.abs(u0)
        assert ((a > 0) & (a < tiny)).any() and (a >= tiny).any()
        um, _ = wf.start_flow(frame, "mixed")
        assert np.abs(um[20:41, 60:141]).max() > 1e30 and np.abs(um[:20]).max() < 10 and np.abs(um[:, 141:]).max() < 10
        assert abs(wf.fin_of(*wf.start_flow(frame, "S1")) - 4.41) < 0.3, frame
    assert abs(wf.fin_of(*wf.start_flow("t300x90", "S1")) - 4.41) < 0.01


@pytest.mark.parametrize("rung", wf.NONFINITE)
@pytest.mark.parametrize("frame", list(wf.FRAMES))
def test_nonfinite_values_spread_alike_in_both_oracles(oracle, frame, rung):
    A, B = wf.frames(frame)
    u0, v0 = wf.start_flow(frame, rung)
    for n in (7, SWEEPS):
        (uc, vc), (un, vn) = both(oracle, A, B, 1.0, n, u0, v0, term_type=ITER)
        mu, mv = ~np.isfinite(uc), ~np.isfinite(vc)
        assert np.array_equal(mu, ~np.isfinite(un)) and np.array_equal(mv, ~np.isfinite(vn)), (frame, rung, n)
        assert np.array_equal(uc[~mu], un[~mu]) and np.array_equal(vc[~mv], vn[~mv]), (frame, rung, n)
        assert mu.any() and not mu.all()
    if frame == "t300x90" and rung in ("nan", "inf"):
        # one pixel per sweep, and the average leaves the centre out: after 7 sweeps the 64 pixels of the diamond of radius 7
        # that lie an odd distance away, clipped by no border; the NaN and the Inf of the two rungs together give 128
        (uc, vc), _ = both(oracle, A, B, 1.0, 7, u0, v0, term_type=ITER)
        assert int((~np.isfinite(uc)).sum()) == 64 and int((~np.isfinite(vc)).sum()) == 64
        u2, v2 = np.array(wf.start_flow(frame, "nan")[0]), np.array(wf.start_flow(frame, "inf")[1])
        (uc, vc), (un, vn) = both(oracle, A, B, 1.0, 7, u2, v2, term_type=ITER)
        assert int((~np.isfinite(uc)).sum()) == 128 and int((~np.isfinite(vc)).sum()) == 128
        assert not np.isinf(uc).any() and not np.isinf(vc).any()
        assert np.array_equal(~np.isfinite(uc), ~np.isfinite(un)) and np.array_equal(~np.isfinite(vc), ~np.isfinite(vn))


def test_eps_ignores_nan(oracle):
    """The reference's `if (t > Eps)` never takes a NaN: an ITER|EPS solve stops although the flow holds NaN."""
    A, B = wf.frames("t300x90")
    u0, v0 = wf.start_flow("t300x90", "nan")
    with np.errstate(all="ignore"):
        rc = oracle.calc_optical_flow_hs(A, B, 1.0, 30, 0.5, ITER | EPS, use_previous=True, velx=u0, vely=v0, return_info=True)
        rn = hs_numpy.calc_optical_flow_hs(A, B, 1.0, 30, 0.5, ITER | EPS, use_previous=True, velx=u0, vely=v0, return_info=True)
    assert rc[2] == 15 and abs(rc[3] - 0.4817) < 1e-4 and np.isnan(rc[0]).any(), rc[2:]
    assert rn[2] == rc[2]


def overflow_sweep(frame, S, T=32):
    """The first sweep k of a launch at which 4^k * max|flow_k| leaves the float range (None: never within T sweeps)."""
    A, B = wf.frames(frame)
    u, v = wf.scaled(frame, S)
    for k in range(1, T + 1):
        with np.errstate(all="ignore"):
            u, v = hs_numpy.calc_optical_flow_hs(A, B, 1.0, 1, term_type=ITER, use_previous=True, velx=u, vely=v)
        assert np.isfinite(u).all() and np.isfinite(v).all(), (S, k)
        if 4.0 ** k * wf.fin_of(u, v) > wf.FLT_MAX:
            return k
    return None


def test_where_a_scaled_launch_leaves_the_float_range():
    """Why the rungs stand where they do (300x90, lambda 1)."""
    assert [overflow_sweep("t300x90", S) for S in (1e24, 1e26, 1e30, 1e36)] == [26, 22, 15, 5]
    for S in (1e-38, 1.0, 20.0, 1e6, 1e18, 1e19):
        assert overflow_sweep("t300x90", S) is None, S


CLASSIC_RUNGS = ("S1", "S1e+06", "S1e+18", "S1e+31", "S1e+36")


@pytest.mark.parametrize("alpha", [15.0, 0.3])
def test_classic_oracle_is_finite_on_its_rungs(oracle, alpha):
    """The classic update divides by alpha^2 + Ex^2 + Ey^2 and multiplies the numerator by a derivative first."""
    A, B = wf.frames("t333x131")
    for rung in CLASSIC_RUNGS:
        u0, v0 = wf.start_flow("t333x131", rung)
        with np.errstate(all="ignore"):
            u, v = oracle.classic_flow(A, B, alpha, 13, use_previous=True, u0=u0, v0=v0)
        assert np.isfinite(u).all() and np.isfinite(v).all(), (alpha, rung)
