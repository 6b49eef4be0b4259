"""A NumPy restatement of the linking rule (opticalflowhs_amd/csrc/hs_link_rule.h) and the cases the link tests share.

The restatement shares no code with the library: the landing pixel is hsinterp::target written again in fp32 NumPy, the
votes are np.unique over the keys.  It returns the exact bytes of the four outputs."""
import numpy as np

F = np.float32
KNOWN_MAX = F(1e9)        # hscolor::kUnknown: a magnitude above it is no flow

SHAPES = [(67, 19), (130, 37), (64, 16), (1, 1), (300, 260)]


def target(u, v, W, H):
    """(landed, qx, qy) per pixel at t = 1: every operation rounded to fp32 on its own, the frame test on the floats."""
    u, v = np.asarray(u, F), np.asarray(v, F)
    with np.errstate(invalid="ignore", over="ignore"):
        known = ~(np.isnan(u) | np.isnan(v) | (np.abs(u) > KNOWN_MAX) | (np.abs(v) > KNOWN_MAX))
        us, vs = np.where(known, u, F(0)), np.where(known, v, F(0))
        xs = np.arange(W, dtype=np.int64)[None, :].astype(F)
        ys = np.arange(H, dtype=np.int64)[:, None].astype(F)
        da, db = (us * F(1)).astype(F), (vs * F(1)).astype(F)
        hx = ((xs + da).astype(F) + F(0.5)).astype(F)
        hy = ((ys + db).astype(F) + F(0.5)).astype(F)
        inside = (hx >= F(0)) & (hx < F(W)) & (hy >= F(0)) & (hy < F(H))
        qx = np.floor(np.where(inside, hx, F(0))).astype(np.int64)
        qy = np.floor(np.where(inside, hy, F(0))).astype(np.int64)
    landed = known & inside & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
    return landed, qx, qy


def link(A, B, u, v, cap_a, cap_b, link_capacity):
    """(links bytes of the records written, side_a bytes, side_b bytes, result bytes, dict of the header)."""
    A, B = np.asarray(A, np.int64), np.asarray(B, np.int64)
    H, W = A.shape
    landed, qx, qy = target(u, v, W, H)
    fg = A > 0
    over = fg & (A > cap_a)
    live = fg & ~over
    gone = live & ~landed
    b = np.where(landed, B[qy, qx], 0)
    matched = live & landed & (b > 0) & (b <= cap_b)
    unmatched = live & landed & ~matched
    keys, counts = np.unique((A[matched] - 1) * cap_b + (b[matched] - 1), return_counts=True)
    la, lb = keys // cap_b + 1, keys % cap_b + 1
    n_links = len(keys)
    n_written = min(n_links, link_capacity)
    links = np.zeros((n_written, 4), np.uint32)
    links[:, 0], links[:, 1], links[:, 2] = la[:n_written], lb[:n_written], counts[:n_written]

    def side(n, mine, other, gone_px, unmatched_px):
        out = np.zeros((n, 8), np.uint32)
        out[:, 0] = gone_px + unmatched_px
        out[:, 4], out[:, 5] = gone_px, unmatched_px
        for k in np.unique(mine):
            sel = mine == k
            px = counts[sel]
            top = px.max()
            out[k - 1, 0] += px.sum()
            out[k - 1, 1] = len(px)
            out[k - 1, 2] = other[sel][px == top].min()
            out[k - 1, 3] = top
        return out

    gone_a = np.bincount(A[gone], minlength=cap_a + 1)[1:cap_a + 1]
    unm_a = np.bincount(A[unmatched], minlength=cap_a + 1)[1:cap_a + 1]
    sa = side(cap_a, la, lb, gone_a, unm_a)
    sb = side(cap_b, lb, la, np.zeros(cap_b, np.int64), np.zeros(cap_b, np.int64))
    mutual = sum(1 for a in range(1, cap_a + 1) if sa[a - 1, 2] and sb[sa[a - 1, 2] - 1, 2] == a)
    head = dict(n_links=n_links, n_written=n_written, flags=1 if n_links > link_capacity else 0, n_mutual=mutual, voted_px=int(counts.sum()),
                gone_px=int(gone.sum()), unmatched_px=int(unmatched.sum()), over_a_px=int(over.sum()))
    res = np.zeros(1, np.dtype([("w", np.uint32, 4), ("q", np.uint64, 6)]))
    res["w"][0] = [head["n_links"], head["n_written"], head["flags"], head["n_mutual"]]
    res["q"][0][:4] = [head["voted_px"], head["gone_px"], head["unmatched_px"], head["over_a_px"]]
    return links.tobytes(), sa.tobytes(), sb.tobytes(), res.tobytes(), head


# ---- label planes -------------------------------------------------------------------------------------------------------

def labels_of(name, W, H, seed=0):
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.RandomState(1000 + seed)
    if name == "one":
        return np.ones((H, W), np.int32)
    if name == "checker":                      # many labels in cells of 5 x 3 pixels, some background, some negative
        lab = ((y // 3) * ((W + 4) // 5) + x // 5 + 1).astype(np.int32)
        lab[(x + y) % 7 == 0] = 0
        lab[(x * 3 + y) % 11 == 0] = -3
        return lab
    if name == "random5000":
        lab = rng.randint(-2, 5001, size=(H, W)).astype(np.int32)
        return lab
    if name == "random60":
        return rng.randint(0, 61, size=(H, W)).astype(np.int32)
    if name == "rects":
        lab = np.zeros((H, W), np.int32)
        for k in range(1, 9):
            x0, y0 = rng.randint(0, max(W - 1, 1)), rng.randint(0, max(H - 1, 1))
            lab[y0:y0 + 1 + rng.randint(0, H // 2 + 1), x0:x0 + 1 + rng.randint(0, W // 2 + 1)] = k
        return lab
    if name == "halves":                       # a split or a merge against "one"
        return np.where(x * 2 < W, 1, 2).astype(np.int32)
    raise KeyError(name)


def flow_of(name, W, H, seed=0):
    y, x = np.mgrid[0:H, 0:W]
    rng = np.random.RandomState(2000 + seed)
    if name == "zero":
        return np.zeros((H, W), F), np.zeros((H, W), F)
    if name == "shift":
        return np.full((H, W), 3, F), np.full((H, W), -2, F)
    if name == "halfpixel":                    # exactly +-0.5 and +-1.5: the tie of the landing rule
        u = np.where(x % 2 == 0, F(0.5), F(-0.5)).astype(F) + np.where(y % 3 == 0, F(1), F(0)).astype(F)
        v = np.where(y % 2 == 0, F(-0.5), F(0.5)).astype(F)
        return u, v
    if name == "random":
        return (rng.rand(H, W).astype(F) - F(0.5)) * F(12), (rng.rand(H, W).astype(F) - F(0.5)) * F(8)
    if name == "sprinkled":                    # the extreme values among a random field
        u, v = flow_of("random", W, H, seed)
        u, v = u.copy(), v.copy()
        special = [np.nan, np.inf, -np.inf, 1e10, -1e10, 1e9, 3e38, -0.0, 1e-40, 2.0 ** 31, -(2.0 ** 31), float(W), -1.0, 0.49999997]
        n = W * H
        idx = rng.permutation(n)[:max(1, min(n, 40))]
        for k, i in enumerate(idx):
            (u if k % 2 == 0 else v).flat[i] = F(special[k % len(special)])
        return u, v
    raise KeyError(name)


# (labels of A, labels of B, flow, cap_a, cap_b): every path of the rule and of the kernels' vote
CASES = [
    ("one", "one", "zero", 1, 1),
    ("one", "one", "random", 64, 64),
    ("one", "halves", "shift", 4, 4),              # a split
    ("halves", "one", "sprinkled", 4, 4),          # a merge
    ("checker", "checker", "shift", 7, 9),         # caps below the label count: over_a and unmatched
    ("checker", "random60", "halfpixel", 64, 64),
    ("random5000", "random5000", "sprinkled", 5000, 3000),
    ("random60", "rects", "random", 60, 8),
    ("rects", "random60", "sprinkled", 16, 16),
    ("rects", "rects", "halfpixel", 17, 17),
]


def planes(case, W, H):
    a, b, f, cap_a, cap_b = case
    u, v = flow_of(f, W, H, seed=W + H)
    return labels_of(a, W, H, seed=1), labels_of(b, W, H, seed=2), u, v, cap_a, cap_b
