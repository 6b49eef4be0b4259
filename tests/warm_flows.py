"""Caller-written starting flows for the warm-start tests (test_warm_flow_host.py, test_gpu_warm_flow.py): one definition.

Frames: synth.translating_pair at 300x90 (one strip tile column whose side lanes are mirrored) and at 259x161 (W % 4 != 0,
an odd height, several fold columns), both with seed 3 -- the smallest shapes tests/test_gpu_strip_trims.py uses for those
edges.  Base flow: default_rng(1).standard_normal((H, W)) as float32, drawn for u first and then for v.  A rung of the ladder
is S * base; the largest |base| is about 4.4, so a rung's largest input is about 4.4 * S.  The lowest rung puts denormals
into the planes, the highest is the last at which the four-neighbour sum stays inside fp32 (at 3e37 it does not).
"""
import numpy as np

from opticalflowhs_amd import synth

FRAMES = {"t300x90": (300, 90, 3), "t259x161": (259, 161, 3)}
# the nearest shape the persistent launch takes (tests/test_gpu_stop_rule.py), and one the classic strip kernel runs at
EXTRA_FRAMES = {"t260x84": (260, 84, 4), "t333x131": (333, 131, 3)}
LADDER = (1e-38, 1e-30, 1e-10, 1.0, 20.0, 1e6, 1e18, 1e24, 1e26, 1e30, 1e36)
NONFINITE = ("nan", "inf", "corners")
FINITE_RUNGS = tuple("S%g" % s for s in LADDER) + ("mixed",)
RUNGS = FINITE_RUNGS + NONFINITE
FLT_MAX = float(np.finfo(np.float32).max)

_frames = {}
_base = {}


def size_of(name):
    """(W, H, seed) of a frame pair."""
    return FRAMES[name] if name in FRAMES else EXTRA_FRAMES[name]


def frames(name):
    if name not in _frames:
        W, H, seed = size_of(name)
        A, B = synth.translating_pair(W, H, seed=seed)
        A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
        A.setflags(write=False)
        B.setflags(write=False)
        _frames[name] = (A, B)
    return _frames[name]


def base_flow(name):
    if name not in _base:
        W, H, _ = size_of(name)
        rng = np.random.default_rng(1)
        u = rng.standard_normal((H, W)).astype(np.float32)
        v = rng.standard_normal((H, W)).astype(np.float32)
        u.setflags(write=False)
        v.setflags(write=False)
        _base[name] = (u, v)
    return _base[name]


def scaled(name, S):
    """S * base in float32 (the product is taken in double and rounded once)."""
    u, v = base_flow(name)
    return (u.astype(np.float64) * S).astype(np.float32), (v.astype(np.float64) * S).astype(np.float32)


def start_flow(name, rung):
    """(u0, v0) of a rung: "S<value>" for the ladder, "mixed", "nan", "inf" or "corners"."""
    W, H, _ = size_of(name)
    if rung.startswith("S"):
        u, v = scaled(name, float(rung[1:]))
    elif rung == "mixed":          # 1e30 inside rows 20-40, columns 60-140; 1 elsewhere
        u, v = scaled(name, 1.0)
        bu, bv = scaled(name, 1e30)
        u[20:41, 60:141] = bu[20:41, 60:141]
        v[20:41, 60:141] = bv[20:41, 60:141]
    else:
        u, v = scaled(name, 1.0)
        if rung == "nan":
            u[40, 100] = np.nan
        elif rung == "inf":
            v[10, 250] = np.inf   # column W - 9 at 259 wide
        elif rung == "corners":    # corner pixels and mirrored halos
            u[0, 0] = -np.inf
            v[H - 1, W - 1] = np.nan
        else:
            raise KeyError(rung)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


def fin_of(u0, v0):
    """The largest absolute value of a (finite) starting flow."""
    return float(max(np.abs(u0).max(), np.abs(v0).max()))
