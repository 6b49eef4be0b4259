"""What the global-motion tests share: a NumPy restatement of csrc/hs_gmotion_rule.h and the fields the fits are tried on.
The restatement sums Python integers, solves in float64 in the rule's order, and does every fp32 step as its own array
operation.  No GPU work here."""
import numpy as np

F = np.float32
K_MAX_FLOW = F(2048.0)
K_UNKNOWN = F(1e9)
K_BIN_BASE = (127 - 32) << 2
K_REL = 2.0 ** -36
NAN_BITS = 0x7fc00000
TRANSLATION, SIMILARITY, AFFINE, ZERO = 0, 1, 2, 3
FIXED, AUTO = 0, 1
SHAPES = [(13, 7), (260, 37), (1027, 9), (96, 64)]           # (W, H): narrower than a wavefront, just wider than a 256-column tile, many tiles, whole tiles
SMALL = [(1, 1), (1, 40), (40, 1)]


def coords(W, H):
    """Doubled centred integer coordinates (1, W) and (H, 1), int64."""
    return (2 * np.arange(W, dtype=np.int64) - (W - 1))[None, :], (2 * np.arange(H, dtype=np.int64) - (H - 1))[:, None]


def model_planes(p, W, H):
    """(mu, mv), float32 (H, W), in the rule's order."""
    p = np.asarray(p, F)
    Xi, Yi = coords(W, H)
    X, Y = Xi.astype(F) * F(0.5), Yi.astype(F) * F(0.5)
    ax, ay = p[1] * X, p[2] * Y
    s0 = p[0] + ax
    mu = s0 + ay
    bx, by = p[4] * X, p[5] * Y
    s1 = p[3] + bx
    mv = s1 + by
    return np.broadcast_to(mu, (H, W)).astype(F), np.broadcast_to(mv, (H, W)).astype(F)


def usable(u, v, state):
    """(unknown, untrusted) boolean planes."""
    with np.errstate(invalid="ignore"):
        unknown = np.isnan(u) | np.isnan(v) | (np.abs(u) > K_UNKNOWN) | (np.abs(v) > K_UNKNOWN) | (np.abs(u) > K_MAX_FLOW) | (np.abs(v) > K_MAX_FLOW)
    untrusted = ~unknown & (state == 0) if state is not None else np.zeros_like(unknown)
    return unknown, untrusted


def residual(u, v, p):
    H, W = u.shape
    mu, mv = model_planes(p, W, H)
    with np.errstate(invalid="ignore", over="ignore"):
        ru = u - mu
        rv = v - mv
        uu = ru * ru
        vv = rv * rv
        r2 = uu + vv
    return ru, rv, r2


def sums_of(u, v, sel):
    """The twelve sums over the pixels `sel`, Python integers."""
    H, W = u.shape
    Xi, Yi = coords(W, H)
    Xi, Yi = np.broadcast_to(Xi, (H, W))[sel], np.broadcast_to(Yi, (H, W))[sel]
    with np.errstate(invalid="ignore", over="ignore"):
        su = u[sel] * F(256.0)
        sv = v[sel] * F(256.0)
    qu, qv = np.rint(su).astype(np.int64), np.rint(sv).astype(np.int64)
    tot = lambda a: int(sum(int(x) for x in a))
    return [len(Xi), tot(Xi), tot(Yi), tot(Xi * Xi), tot(Xi * Yi), tot(Yi * Yi), tot(qu), tot(qu * Xi), tot(qu * Yi), tot(qv), tot(qv * Xi), tot(qv * Yi)]


def solve(s, kind):
    """(p float32[6], flags) from the sums, float64 in the rule's order."""
    D = np.float64
    n, Sx, Sy, Sxx, Sxy, Syy, Su, Sux, Suy, Sv, Svx, Svy = [D(float(x)) for x in s]
    with np.errstate(all="ignore"):
        nxx, nyy = n * Sxx, n * Syy
        A, B, C = nxx - Sx * Sx, n * Sxy - Sx * Sy, nyy - Sy * Sy
        Eu, Fu, Ev, Fv = n * Sux - Sx * Su, n * Suy - Sy * Su, n * Svx - Sx * Sv, n * Svy - Sy * Sv
        AC = A * C
        Dt = AC - B * B
        spread_x, spread_y = A > nxx * D(K_REL), C > nyy * D(K_REL)
        q = [D(0.0)] * 6
        used = ZERO
        if kind == AFFINE and s[0] >= 3 and spread_x and spread_y and Dt > AC * D(K_REL):
            used = AFFINE
            q[1] = (Eu * C - Fu * B) / Dt
            q[2] = (Fu * A - Eu * B) / Dt
            q[4] = (Ev * C - Fv * B) / Dt
            q[5] = (Fv * A - Ev * B) / Dt
            q[0] = (Su - q[1] * Sx - q[2] * Sy) / n
            q[3] = (Sv - q[4] * Sx - q[5] * Sy) / n
        elif kind >= SIMILARITY and s[0] >= 2 and (spread_x or spread_y):
            used = SIMILARITY
            den = A + C
            a, b = (Eu + Fv) / den, (Ev - Fu) / den
            q[1], q[2], q[4], q[5] = a, -b, b, a
            q[0] = (Su - a * Sx + b * Sy) / n
            q[3] = (Sv - b * Sx - a * Sy) / n
        elif s[0] >= 1:
            used = TRANSLATION
            q[0], q[3] = Su / n, Sv / n
        p = np.array([q[0] / D(256.0), q[1] / D(128.0), q[2] / D(128.0), q[3] / D(256.0), q[4] / D(128.0), q[5] / D(128.0)], np.float64).astype(F)
    return p, used << 8 | (1 if used != kind else 0)


def bins_of(r2):
    return np.clip((r2.view(np.uint32) >> 21).astype(np.int64) - K_BIN_BASE, 0, 255)


def bin_upper(k):
    return np.array([(k + K_BIN_BASE + 1) << 21], np.uint32).view(F)[0]


def auto_threshold(r2, use, scale2, min_thr2):
    hist = np.bincount(bins_of(r2[use]), minlength=256)
    total = int(hist.sum())
    if total == 0:
        return F(min_thr2)
    k = min(int(np.searchsorted(np.cumsum(hist), (total + 1) // 2)), 255)
    t = F(scale2) * bin_upper(k)
    return t if t > F(min_thr2) else F(min_thr2)


def fit(u, v, state, kind, passes, mode, inlier_px=1.0, scale2=6.0, min_thr2=0.0625, value=(255, 0, 0, 0)):
    """The whole rule: dict(p, thr, flags, cls, mask, ru, rv) with ru, rv as uint32 bit planes."""
    unknown, untrusted = usable(u, v, state)
    use = ~unknown & ~untrusted
    p = np.zeros(6, F)
    thr = F(inlier_px) * F(inlier_px)
    flags = 0
    for j in range(passes + 1):
        if j > 0 and mode == AUTO:
            thr = auto_threshold(residual(u, v, p)[2], use, scale2, min_thr2)
        if j == passes:
            break
        sel = use if j == 0 else use & (residual(u, v, p)[2] <= thr)
        p, flags = solve(sums_of(u, v, sel), kind)
    ru, rv, r2 = residual(u, v, p)
    cls = np.where(unknown, 3, np.where(untrusted, 2, np.where(r2 <= thr, 0, 1))).astype(np.int64)
    rub, rvb = ru.view(np.uint32).copy(), rv.view(np.uint32).copy()
    rub[unknown | np.isnan(ru)] = NAN_BITS
    rvb[unknown | np.isnan(rv)] = NAN_BITS
    return {"p": p, "thr": thr, "flags": flags, "cls": [int((cls == k).sum()) for k in range(4)], "mask": np.asarray(value, np.uint8)[cls], "ru": rub,
            "rv": rvb, "classes": cls}


def field(W, H, seed, specials=True, with_state=True):
    """(u, v, state): a planted affine motion plus Gaussian noise, a block of outliers, and the values the rule has a word
    about -- NaN, +-Inf, just above 1e9, at and just above kMaxFlow, -0.0, quantisation ties -- at random pixels; a state
    plane with zeros."""
    rng = np.random.default_rng(seed)
    Xi, Yi = coords(W, H)
    X, Y = Xi * 0.5, Yi * 0.5
    u = (1.5 + 0.03 * X - 0.02 * Y + rng.normal(0.0, 0.3, (H, W))).astype(F)
    v = (-0.75 + 0.015 * X + 0.025 * Y + rng.normal(0.0, 0.3, (H, W))).astype(F)
    u[:max(H // 3, 1), :max(W // 3, 1)] += F(6.0)
    v[:max(H // 3, 1), :max(W // 3, 1)] -= F(5.0)
    n = W * H
    if specials and n >= 40:
        vals = [np.nan, np.inf, -np.inf, np.nextafter(F(1e9), F(np.inf)), -np.nextafter(F(1e9), F(np.inf)), 2048.0, -2048.0, np.nextafter(F(2048.0), F(np.inf)),
                -np.nextafter(F(2048.0), F(np.inf)), -0.0, 0.5 / 256, 1.5 / 256, -2.5 / 256, (300 + 0.5) / 256, -(1001 + 0.5) / 256, 1e-42, 3e38]
        where = rng.choice(n, size=2 * len(vals), replace=False)
        for k, val in enumerate(vals):
            u.flat[where[2 * k]] = F(val)
            v.flat[where[2 * k + 1]] = F(val)
    state = None
    if with_state:
        state = np.where(rng.random((H, W)) < 0.1, 0, rng.integers(1, 256, (H, W))).astype(np.uint8)
    return u, v, state


def padded(a, pad, fill):
    """A copy of the plane a inside rows that are `pad` elements longer: (the view of the plane, the whole array)."""
    whole = np.full((a.shape[0], a.shape[1] + pad), fill, a.dtype)
    whole[:, :a.shape[1]] = a
    return whole[:, :a.shape[1]], whole
