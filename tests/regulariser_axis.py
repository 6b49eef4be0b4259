"""Cold solves along the whole range of the regularisation weight (test_regulariser_axis_host.py, test_gpu_regulariser_axis.py):
frames, rungs, the float64 reference, the model of the GPU arithmetic and the bars -- one definition.

Frames: 300x90 (two strip tile columns, several fold tiles) and 131x67 (one tile, W % 4 != 0), each as a "noise" pair
(synth.random_pair: flow in the hundreds at a large lambda) and a "texture" pair (synth.translating_pair whose left half does
not move: flow decays into a static half).  Every pair carries two flat 16x16 patches (their inner 14x14 pixels have
Ix = Iy = 0): A = 0, B = 255 (It = 255; columns 20..35) and A = B = 77 (It = 0; columns W-40..W-25).

The float64 reference iterates the same Jacobi scheme with nothing stored in fp32: exact derivatives,
ilambda = 1 / float64(float32(lambda)), alpha = 1 / (ilambda + Ix^2 + Iy^2), 4-neighbour mean with replicate border.

The bar, per rung and pair: d_oracle = max(rms_u, rms_v) of the C oracle against that reference -- what the original's own
mix of double evaluation and fp32 stores costs.  A kernel may lie 4 x d_oracle from the reference: the model of the GPU's
arithmetic below (fp32 throughout, alpha split as s * s, canonical pair sums, correctly rounded 1/sqrt) lies 1.2 - 2.1 x
d_oracle away on these frames (test_regulariser_axis_host.py asserts <= 4), and v_rsq_f32 is good to 1 ulp where the model
rounds correctly.  Everything is computed once, shared between the tests and never written again.
"""
import types

import numpy as np

from opticalflowhs_amd import synth
from oracle import hs_numpy

ITER, EPS = 1, 2
SWEEPS = 47
F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)
FACTOR = 4.0           # the bar: FACTOR * d_oracle
TINY = 1e-30           # HSFLOW_VERIFY_TINY

SIZES = ((300, 90), (131, 67))
PAIRS = tuple("%s%dx%d" % (k, w, h) for (w, h) in SIZES for k in ("noise", "texture"))
PATCH = 16
PATCH_ROWS = {"hot": 10, "still": 38}           # first row of the It = 255 and the It = 0 patch


def patch_cols(W):
    return {"hot": 20, "still": W - 40}


_frames = {}


def size_of(pair):
    """(W, H) of "noise300x90" ..."""
    w, h = pair[len("noise") if pair.startswith("noise") else len("texture"):].split("x")
    return int(w), int(h)


def frames(pair):
    if pair not in _frames:
        W, H = size_of(pair)
        if pair.startswith("noise"):
            A, B = synth.random_pair(W, H, seed=8)
        else:
            A, B = synth.translating_pair(W, H, seed=3)
            A, B = np.array(A), np.array(B)
            B[:, :W // 2] = A[:, :W // 2]
        A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
        c = patch_cols(W)
        r = PATCH_ROWS
        A[r["hot"]:r["hot"] + PATCH, c["hot"]:c["hot"] + PATCH] = 0
        B[r["hot"]:r["hot"] + PATCH, c["hot"]:c["hot"] + PATCH] = 255
        A[r["still"]:r["still"] + PATCH, c["still"]:c["still"] + PATCH] = 77
        B[r["still"]:r["still"] + PATCH, c["still"]:c["still"] + PATCH] = 77
        A.setflags(write=False)
        B.setflags(write=False)
        _frames[pair] = (A, B)
    return _frames[pair]


def flat_inner(pair, which):
    """Slices of the pixels of a patch whose 3x3 neighbourhood lies inside it."""
    W, _ = size_of(pair)
    r, c = PATCH_ROWS[which], patch_cols(W)[which]
    return slice(r + 1, r + PATCH - 1), slice(c + 1, c + PATCH - 1)


# ---- rungs ------------------------------------------------------------------------------------------------------------

def f32(x):
    return float(np.float32(x))


def inv32(x):
    """fl32(1 / fl32(x)), the host's and the oracle's Ilambda."""
    with np.errstate(all="ignore"):
        return np.float32(1.0) / np.float32(x)


def last_float_where(pred, lo, hi):
    """The largest float32 in [lo, hi] for which pred holds (pred holds at lo, fails at hi, and flips once)."""
    a, b = int(np.float32(lo).view(np.uint32)), int(np.float32(hi).view(np.uint32))
    assert pred(float(np.uint32(a).view(np.float32))) and not pred(float(np.uint32(b).view(np.float32)))
    while b - a > 1:
        m = (a + b) // 2
        if pred(float(np.uint32(m).view(np.float32))):
            a = m
        else:
            b = m
    return float(np.uint32(a).view(np.float32))


def up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def down(x):
    return float(np.nextafter(np.float32(x), np.float32(0)))


CAP_IN = last_float_where(lambda x: inv32(x) >= np.float32(1e-20), 1e10, 1e30)     # the last lambda with coeff >= 1e-20f
NORMAL_IN = last_float_where(lambda x: inv32(x) >= np.float32(FLT_MIN), 1e30, 3e38)  # the last with 1/lambda a normal number
# The largest lambda at which the original's alpha = fl32(1 / fl32(1 / lambda)) of a flat pixel is a number: one float
# further 1/lambda rounds to the denormal 2^-128, whose reciprocal is 2^128.  test_regulariser_axis_host.py holds both oracles
# against it on every pair (finite here, NaN one float up).
LARGEST_FINITE = last_float_where(lambda x: bool(np.isfinite(inv32(inv32(x)))), 3e38, FLT_MAX)

CV_RUNGS = {
    "1e-40": f32(1e-40), "1e-38": f32(1e-38), "1e-30": f32(1e-30), "1e-20": f32(1e-20), "1e-10": f32(1e-10), "1e-3": f32(1e-3),
    "1e4": f32(1e4), "1e10": f32(1e10), "cap_in": CAP_IN, "cap_out": up(CAP_IN), "1e30": f32(1e30),
    "normal_in": NORMAL_IN, "normal_out": up(NORMAL_IN), "3e38": f32(3e38), "largest_finite": LARGEST_FINITE, "flt_max": FLT_MAX,
}
FINITE_RUNGS = tuple(r for r in CV_RUNGS if r != "flt_max")      # both oracles finite
BAR_RUNGS = tuple(r for r in FINITE_RUNGS if r != "1e-40")       # ... and the flow not identically zero
KERNEL_RUNGS = tuple(r for r in BAR_RUNGS if r not in ("1e-38", "1e-30", "1e-20"))   # kernel against kernel says something (values above 1e-30)
ABOVE_CAP = tuple(r for r in CV_RUNGS if CV_RUNGS[r] > CAP_IN)
EPS_RUNGS = tuple(r for r in BAR_RUNGS if r != "1e-38")          # the oracle's Eps sequence must give a stop on each of these

# Kernel against kernel: the one pair whose flow reaches the denormals (the others hold nothing below 1e-28 from 1e-10 up), the
# most elements of its two planes together at which scaled_model_flow and model_flow differ -- over every KERNEL_RUNG and
# FLT_MAX, 47 and 40 sweeps, 5, 8, 13, 24 and 32 sweeps per launch: test_regulariser_axis_host.py -- and the size below which
# all of them lie (the largest is 5.0e-39).
DECAYS_TO_DENORMALS = "texture300x90"
DENORMAL_DIFFER = 5
DENORMAL_BELOW = 1e-37
LAUNCH_LENGTHS = (5, 8, 13, 24, 32)     # what the forms of test_gpu_regulariser_axis.py run with

ALPHA_RUNGS = {
    "2^-20": 2.0 ** -20, "below_2^-20": down(2.0 ** -20), "2^20": 2.0 ** 20, "above_2^20": up(2.0 ** 20), "1e-3": f32(1e-3), "1e3": f32(1e3),
    "1e-19": f32(1e-19), "1e-23": f32(1e-23), "1e19": f32(1e19), "2e19": f32(2e19),
}
ALPHA_IN_GATE = ("2^-20", "2^20", "1e-3", "1e3")
ALPHA_JUST_OUT = ("below_2^-20", "above_2^20")


def alpha2(rung):
    with np.errstate(all="ignore"):
        return float(np.float32(ALPHA_RUNGS[rung]) * np.float32(ALPHA_RUNGS[rung]))


# ---- float64 reference ------------------------------------------------------------------------------------------------

def rms(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.sqrt(np.mean(d * d)))


def distance(got, want):
    return max(rms(got[0], want[0]), rms(got[1], want[1]))


def _mean4_f64(p):
    q = np.pad(p, 1, mode="edge")
    return (q[1:-1, :-2] + q[1:-1, 2:] + q[:-2, 1:-1] + q[2:, 1:-1]) * 0.25


def f64_flow(A, B, lam, sweeps=SWEEPS):
    """CV mode, all float64."""
    ix, iy, it = (d.astype(np.float64) for d in hs_numpy.derivatives(A, B))
    ilambda = np.float64(1.0) / np.float64(np.float32(lam))
    alpha = 1.0 / (ilambda + ix * ix + iy * iy)
    u = np.zeros(A.shape, np.float64)
    v = np.zeros(A.shape, np.float64)
    for _ in range(sweeps):
        ub, vb = _mean4_f64(u), _mean4_f64(v)
        t = (ix * ub + iy * vb + it) * alpha
        u, v = ub - ix * t, vb - iy * t
    return u, v


def _tex(p, di, dj):
    """p(i + di, j + dj) with clamp-to-edge, i the column."""
    H, W = p.shape
    q = np.pad(p, 1, mode="edge")
    return q[1 + dj:1 + dj + H, 1 + di:1 + di + W]


def f64_classic_flow(A, B, alpha, sweeps=SWEEPS):
    """Classic mode with the formulae of oracle/hs_classic_oracle.c, all float64 (alpha^2 from the fp32 alpha, in double)."""
    a, b = A.astype(np.float64), B.astype(np.float64)
    a00, a10, a01, a11 = _tex(a, 0, 0), _tex(a, 1, 0), _tex(a, 0, 1), _tex(a, 1, 1)
    b00, b10, b01, b11 = _tex(b, 0, 0), _tex(b, 1, 0), _tex(b, 0, 1), _tex(b, 1, 1)
    ex = 0.25 * (a10 - a00 + a11 - a01 + b10 - b00 + b11 - b01)
    ey = 0.25 * (a01 - a00 + a11 - a10 + b01 - b00 + b11 - b10)
    et = 0.25 * (b00 - a00 + b10 - a10 + b01 - a01 + b11 - a11)
    a2 = np.float64(np.float32(alpha)) ** 2
    u = np.zeros(A.shape, np.float64)
    v = np.zeros(A.shape, np.float64)
    for _ in range(sweeps):
        ua = (_tex(u, -1, 0) + _tex(u, 1, 0) + _tex(u, 0, -1) + _tex(u, 0, 1)) / 6.0 + \
             (_tex(u, -1, -1) + _tex(u, 1, -1) + _tex(u, -1, 1) + _tex(u, 1, 1)) / 12.0
        va = (_tex(v, -1, 0) + _tex(v, 1, 0) + _tex(v, 0, -1) + _tex(v, 0, 1)) / 6.0 + \
             (_tex(v, -1, -1) + _tex(v, 1, -1) + _tex(v, -1, 1) + _tex(v, 1, 1)) / 12.0
        t = (ex * ua + ey * va + et) / (a2 + ex * ex + ey * ey)
        u, v = ua - ex * t, va - ey * t
    return u, v


# ---- the GPU's arithmetic in NumPy --------------------------------------------------------------------------------------

def _fma(a, b, c):
    """fl32(a * b + c) of float32 arrays: the product is exact in double, the sum rounds there once more (a double rounding
    about once in 2^29 -- and alike at every power-of-4 scale, which is all test (3) needs)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def gpu_coefs(A, B, lam):
    """sweep_coefs (hs_kernels.hip.h) with the host's coeff = max(fl32(1/lambda), FLT_MIN), 1/sqrt correctly rounded."""
    ix, iy, it = hs_numpy.derivatives(A, B)
    coeff = max(inv32(lam), np.float32(FLT_MIN))
    with np.errstate(all="ignore"):
        arg = np.float32(coeff) + (ix * ix + iy * iy)
        s = (1.0 / np.sqrt(arg.astype(np.float64))).astype(np.float32)
    return ix * s, iy * s, it * s


def _pair_sums(p, par):
    """update_cv's canonical 4-neighbour sum: even pixel (D + R) + (U + L), odd pixel (D + L) + (U + R)."""
    q = np.pad(p, 1, mode="edge")
    L, R, U, D = q[1:-1, :-2], q[1:-1, 2:], q[:-2, 1:-1], q[2:, 1:-1]
    return np.where(par, (D + L) + (U + R), (D + R) + (U + L))


def _parity(shape):
    y, x = np.indices(shape)
    return ((x + y) & 1).astype(bool)


def model_flow(A, B, lam, sweeps=SWEEPS):
    """The canonical fp32 arithmetic of every kernel (update_cv)."""
    al, be, ga = gpu_coefs(A, B, lam)
    par = _parity(A.shape)
    u = np.zeros(A.shape, np.float32)
    v = np.zeros(A.shape, np.float32)
    quarter = np.float32(0.25)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            ub, vb = _pair_sums(u, par) * quarter, _pair_sums(v, par) * quarter
            q = _fma(al, ub, _fma(be, vb, ga))
            u, v = _fma(-al, q, ub), _fma(-be, q, vb)
    return u, v


def scaled_model_flow(A, B, lam, T, sweeps=SWEEPS):
    """The strip kernels' scaled state (hs_kernels_strip.hip.h): inside a launch of up to T sweeps the planes hold 4^k * flow,
    the neighbour sum is the average at the next scale and the constant term is multiplied by 4 per sweep (once more behind
    the last sweep, as strip_row_update does).  Returns (u, v, every intermediate value was finite)."""
    al, be, ga = gpu_coefs(A, B, lam)
    par = _parity(A.shape)
    u = np.zeros(A.shape, np.float32)
    v = np.zeros(A.shape, np.float32)
    four = np.float32(4.0)
    finite = True
    done = 0
    with np.errstate(all="ignore"):
        while done < sweeps:
            n = min(T, sweeps - done)
            g = ga * four
            for _ in range(n):
                ub, vb = _pair_sums(u, par), _pair_sums(v, par)
                t = _fma(be, vb, g)
                q = _fma(al, ub, t)
                u, v = _fma(-al, q, ub), _fma(-be, q, vb)
                g = g * four
                finite = finite and all(bool(np.isfinite(x).all()) for x in (ub, vb, t, q, u, v, g))
            back = np.float32(4.0 ** -n)
            u, v = u * back, v * back
            done += n
    return u, v, finite


# ---- shared results ---------------------------------------------------------------------------------------------------

_refs = {}


def reference(oracle, pair, rung):
    """C oracle, float64 reference and d_oracle of one rung and pair (computed once)."""
    key = (pair, rung)
    if key not in _refs:
        r = types.SimpleNamespace()
        r.pair, r.rung, r.lam = pair, rung, CV_RUNGS[rung]
        r.A, r.B = frames(pair)
        r.H, r.W = r.A.shape
        with np.errstate(all="ignore"):
            r.oracle = oracle.calc_optical_flow_hs(r.A, r.B, r.lam, SWEEPS, term_type=ITER)
        r.f64 = f64_flow(r.A, r.B, r.lam)
        for p in r.oracle + r.f64:
            p.setflags(write=False)
        r.oracle_finite = bool(np.isfinite(r.oracle[0]).all() and np.isfinite(r.oracle[1]).all())
        r.d_oracle = distance(r.oracle, r.f64) if r.oracle_finite else float("nan")
        r.fmax = float(max(np.abs(r.f64[0]).max(), np.abs(r.f64[1]).max()))
        _refs[key] = r
    return _refs[key]


def bar_reference(oracle, pair, rung):
    """The reference whose d_oracle is the bar of a rung: its own, or at FLT_MAX (where the oracle yields NaN) that of the
    neighbouring finite rung, against the float64 flow of FLT_MAX itself."""
    return reference(oracle, pair, "largest_finite" if rung == "flt_max" else rung)


_eps = {}


def oracle_eps(oracle, pair, rung):
    """E_1 .. E_47 of the oracle, stepped one sweep per call (as tests/test_gpu_stop_rule.py does): float64 array."""
    key = (pair, rung)
    if key not in _eps:
        A, B = frames(pair)
        lam = CV_RUNGS[rung]
        u = np.zeros(A.shape, np.float32)
        v = np.zeros(A.shape, np.float32)
        E = []
        with np.errstate(all="ignore"):
            for k in range(SWEEPS):
                u1, v1 = oracle.calc_optical_flow_hs(A, B, lam, 1, term_type=ITER, use_previous=k > 0, velx=u, vely=v)
                E.append(max(float(np.abs(u1 - u).max()), float(np.abs(v1 - v).max())))
                u, v = u1, v1
        E = np.array(E, np.float64)
        E.setflags(write=False)
        _eps[key] = E
    return _eps[key]


def eps_stop(E):
    """(k, epsilon): the latest k <= 40 with E_k < E_(k-1) * (1 - 1e-3) and E_k >= 1e-30 at which an ITER|EPS solve with
    epsilon = sqrt(E_(k-1) * E_k) stops first -- E_(k-1) is the smallest change before sweep k, so no earlier sweep lies below
    epsilon either.  None where the sequence has no such k."""
    for k in range(40, 1, -1):
        e0, e1 = E[k - 2], E[k - 1]
        if e1 < e0 * (1 - 1e-3) and e1 >= 1e-30 and e0 <= E[:k - 1].min():
            return k, float(np.sqrt(e0 * e1))
    return None
