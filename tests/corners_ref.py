"""An independent NumPy restatement of the corner rule (include/hsflow.h, "which points to follow"), written from the
header's text: edge padding, shifted-slice sums, math.isqrt, a stable sort.  Nothing here is taken from
csrc/hs_corners_rule.h.  Also the test planes that the host and the GPU tests share."""
import math
import struct

import numpy as np

MIN_EIGEN, HARRIS = 0, 1
OVERFLOW, TRUNCATED = 1, 2
NAN_BITS = 0x7FC00000
RECORD = np.dtype([("x", "<u2"), ("y", "<u2"), ("index", "<u4"), ("score", "<i8")])
SHAPES = ((67, 19), (130, 35))


def params(kind=MIN_EIGEN, block_r=1, nms_r=3, quality_q16=655, border=0, fg=(1, 255), max_candidates=65536, min_score=1):
    return dict(kind=kind, block_r=block_r, nms_r=nms_r, quality_q16=quality_q16, border=border, fg=fg, max_candidates=max_candidates, min_score=min_score)


# ---- planes -------------------------------------------------------------------------------------------------------------------

def noise(W, H, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, 256, (H, W), dtype=np.uint8)


def sines(W, H):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    t = np.sin(x * 0.71 + y * 0.13) + np.sin(x * 0.23 - y * 0.57) + np.sin((x + 2 * y) * 0.31) + np.sin(x * y * 0.011)
    return np.clip(np.rint(127.5 + 31.0 * t), 0, 255).astype(np.uint8)


def checker(W, H, cell=8, lo=0, hi=255, ox=0, oy=0):
    y, x = np.mgrid[0:H, 0:W]
    return np.where((((x + ox) // cell) + ((y + oy) // cell)) % 2 == 0, lo, hi).astype(np.uint8)


def plane(name, W, H):
    return {"noise": lambda: noise(W, H), "sines": lambda: sines(W, H), "checker": lambda: checker(W, H)}[name]()


# ---- the rule -----------------------------------------------------------------------------------------------------------------

def box(a, r):
    """The sum over the (2 r + 1)^2 window whose coordinates are clamped to the frame: the window of the edge-padded plane."""
    H, W = a.shape
    q = np.pad(a, r, mode="edge")
    out = np.zeros_like(a)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out += q[dy:dy + H, dx:dx + W]
    return out


def scores(g, kind, block_r):
    p = np.pad(g.astype(np.int64), 1, mode="edge")
    ix = (p[:-2, 2:] + 2 * p[1:-1, 2:] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[1:-1, :-2] + p[2:, :-2])
    iy = (p[2:, :-2] + 2 * p[2:, 1:-1] + p[2:, 2:]) - (p[:-2, :-2] + 2 * p[:-2, 1:-1] + p[:-2, 2:])
    A, B, C = box(ix * ix, block_r), box(ix * iy, block_r), box(iy * iy, block_r)
    if kind == HARRIS:
        return 25 * (A * C - B * B) - (A + C) ** 2
    D = (A - C) ** 2 + 4 * B * B
    root = np.empty_like(D)
    for k, d in enumerate(D.ravel().tolist()):
        r = math.isqrt(d)
        root.flat[k] = r if r * r == d else r + 1
    return (A + C) - root


def corners(g, mask=None, capacity=1024, **kw):
    """{"result": dict, "records": structured array of the n_written corners, "xy": float32 (capacity, 2), "survivors":
    the indices of all survivors, "S": the score plane}."""
    p = params(**kw)
    H, W = g.shape
    S = scores(g, p["kind"], p["block_r"])
    ok = np.ones((H, W), bool) if mask is None else (mask >= p["fg"][0]) & (mask <= p["fg"][1])
    b = p["border"]
    y, x = np.mgrid[0:H, 0:W]
    ok &= (x >= b) & (y >= b) & (x < W - b) & (y < H - b)
    smax = max(0, int(S[ok].max())) if ok.any() else 0
    T = max(p["min_score"], (smax >> 16) * p["quality_q16"])
    strong = ok & (S >= T)
    r = p["nms_r"]
    far = np.iinfo(np.int64).min
    q = np.pad(S, r, mode="constant", constant_values=far)
    lost = np.zeros((H, W), bool)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            nb = q[r + dy:r + dy + H, r + dx:r + dx + W]
            lost |= nb > S
            if dy < 0 or (dy == 0 and dx < 0):
                lost |= nb == S
    survivors = np.flatnonzero((strong & ~lost).ravel())
    cand = survivors[:p["max_candidates"]]
    order = np.argsort(-S.ravel()[cand], kind="stable")
    ranked = cand[order]
    n_written = min(len(ranked), capacity)
    rec = np.zeros(n_written, RECORD)
    rec["index"] = ranked[:n_written]
    rec["x"], rec["y"] = ranked[:n_written] % W, ranked[:n_written] // W
    rec["score"] = S.ravel()[ranked[:n_written]]
    xy = np.full((capacity, 2), NAN_BITS, np.uint32).view(np.float32)
    xy[:n_written, 0], xy[:n_written, 1] = rec["x"], rec["y"]
    flags = (OVERFLOW if len(cand) > capacity else 0) | (TRUNCATED if len(survivors) > p["max_candidates"] else 0)
    result = dict(n_survivors=len(survivors), n_candidates=len(cand), n_written=n_written, flags=flags, smax=smax, threshold=T,
                  allowed_px=int(ok.sum()), strong_px=int(strong.sum()))
    return dict(result=result, records=rec, xy=xy, survivors=survivors, S=S)


def result_bytes(d):
    return struct.pack("<4I2q2Q2Q", d["n_survivors"], d["n_candidates"], d["n_written"], d["flags"], d["smax"], d["threshold"], d["allowed_px"], d["strong_px"], 0, 0)
