"""A NumPy / Python restatement of the labelling rule of include/hsflow.h (hsflow_regions*), written from the header's
prose and not from csrc/hs_regions_rule.h: the adjacency comes from the predicate as whole-plane float32 arithmetic, the
regions from a breadth-first search started at the pixels in raster order -- which meets the roots in ascending order by
construction -- and every sum is a Python integer.  With it the masks and flow fields a labelling kernel gets wrong."""
import functools
from collections import deque

import numpy as np

F = np.float32
SHAPES = [(13, 7), (260, 37), (1027, 9), (96, 64), (1, 1), (1, 40), (40, 1)]
OVERFLOW = 1


def known(u, v):
    """The fit's test of a flow: no NaN, no magnitude above 1e9, no component above 2048 px."""
    with np.errstate(invalid="ignore"):
        return ~(np.isnan(u) | np.isnan(v) | (np.abs(u) > F(1e9)) | (np.abs(v) > F(1e9)) | (np.abs(u) > F(2048.0)) | (np.abs(v) > F(2048.0)))


def quant(a):
    """rint(fl(a * 256)), ties to even, as Python integers."""
    return np.rint(a.astype(F) * F(256.0)).astype(np.int64)


def edges(fg, u, v, join_px, dy, dx):
    """A boolean plane: pixel (y, x) and pixel (y + dy, x + dx) are joined (False where the neighbour is outside)."""
    H, W = fg.shape
    out = np.zeros((H, W), bool)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys >= ye or xs >= xe:
        return out
    a = (slice(ys, ye), slice(xs, xe))
    b = (slice(ys + dy, ye + dy), slice(xs + dx, xe + dx))
    ok = fg[a] & fg[b]
    if F(join_px) > 0:
        thr = F(join_px) * F(join_px)
        with np.errstate(invalid="ignore", over="ignore"):
            du = (u[a] - u[b]).astype(F)
            dv = (v[a] - v[b]).astype(F)
            d2 = ((du * du).astype(F) + (dv * dv).astype(F)).astype(F)
            k = known(u, v)
            ok = ok & k[a] & k[b] & (d2 <= thr)
    out[a] = ok
    return out


def partition(mask, u, v, connectivity, join_px, fg_lo=1, fg_hi=255, shape=None):
    """(root plane, -1 for background; list of (root, [pixel indices])) by breadth-first search in raster order."""
    if mask is not None:
        H, W = mask.shape
        fg = (mask >= fg_lo) & (mask <= fg_hi)
    else:
        H, W = shape if u is None else u.shape
        fg = np.ones((H, W), bool)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    fwd = {s: edges(fg, u, v, join_px, s[0], s[1]) for s in steps}
    nbr = [[] for _ in range(H * W)]
    for (dy, dx), e in fwd.items():
        ys, xs = np.nonzero(e)
        for y, x in zip(ys.tolist(), xs.tolist()):
            i, j = y * W + x, (y + dy) * W + x + dx
            nbr[i].append(j)
            nbr[j].append(i)
    root = np.full(H * W, -1, np.int64)
    flat = fg.reshape(-1)
    comps = []
    for i in np.nonzero(flat)[0].tolist():
        if root[i] >= 0:
            continue
        root[i] = i
        members = [i]
        todo = deque([i])
        while todo:
            p = todo.popleft()
            for q in nbr[p]:
                if root[q] < 0:
                    root[q] = i
                    members.append(q)
                    todo.append(q)
        comps.append((i, members))
    return root.reshape(H, W), comps


def label(mask, u, v, connectivity=8, min_area=1, join_px=0.0, capacity=0, fg=(1, 255), shape=None):
    """What hsflow_regions* must give: {"labels": int32 plane, "records": list of dicts (min(n_regions, capacity) of them),
    "result": dict}."""
    roots, comps = partition(mask, u, v, connectivity, join_px, fg[0], fg[1], shape)
    H, W = roots.shape
    labels = np.zeros((H, W), np.int32)
    have_flow = u is not None
    kn = known(u, v) if have_flow else np.zeros((H, W), bool)
    qu = quant(np.where(kn, u, F(0))) if have_flow else None
    qv = quant(np.where(kn, v, F(0))) if have_flow else None
    records, n_regions, n_dropped, dropped_px, fg_px = [], 0, 0, 0, 0
    largest = (0, 0)
    for r, members in comps:
        fg_px += len(members)
        if len(members) < min_area:
            n_dropped += 1
            dropped_px += len(members)
            continue
        n_regions += 1
        if len(members) > largest[0]:
            largest = (len(members), n_regions)
        ys = [m // W for m in members]
        xs = [m % W for m in members]
        for y, x in zip(ys, xs):
            labels[y, x] = n_regions
        if n_regions <= capacity:
            flow = [(y, x) for y, x in zip(ys, xs) if kn[y, x]]
            records.append({"root": r, "area": len(members), "x0": min(xs), "y0": min(ys), "x1": max(xs), "y1": max(ys), "sum_x": sum(xs), "sum_y": sum(ys),
                            "n_flow": len(flow), "reserved0": 0, "sum_qu": sum(int(qu[y, x]) for y, x in flow), "sum_qv": sum(int(qv[y, x]) for y, x in flow),
                            "reserved1": 0})
    unknown = int(((roots >= 0) & ~kn).sum()) if have_flow else 0
    result = {"n_regions": n_regions, "n_written": min(n_regions, capacity), "n_dropped": n_dropped, "flags": OVERFLOW if n_regions > capacity else 0,
              "fg_px": fg_px, "dropped_px": dropped_px, "unknown_flow_px": unknown, "largest_area": largest[0], "largest_label": largest[1]}
    return {"labels": labels, "records": records, "result": result}


def same_partition(a, b):
    """Two label planes (0 = background) cut the plane into the same sets."""
    if not np.array_equal(a == 0, b == 0):
        return False
    pairs = set(zip(a.reshape(-1).tolist(), b.reshape(-1).tolist()))
    return len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs))


# ---- the masks -----------------------------------------------------------------------------------------------------------------

def _empty(W, H):
    return np.zeros((H, W), np.uint8)


def _full(W, H):
    return np.full((H, W), 255, np.uint8)


def _checker(W, H):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy + xx) & 1) == 0).astype(np.uint8) * 200


def _diagonals(W, H):
    """One-pixel diagonals: a long one from the corner, and short ones across the corners of tiles of 64 x 16 and of 256
    columns, in both directions."""
    m = np.zeros((H, W), np.uint8)
    for k in range(min(W, H)):
        m[k, k] = 1
    for cx in (64, 128, 256, 1024):
        for cy in (16, 32):
            for (y, x) in ((cy - 1, cx - 1), (cy, cx), (cy - 1, cx + 3), (cy, cx + 2), (cy - 2, cx + 4)):
                if 0 <= y < H and 0 <= x < W:
                    m[y, x] = 255
            for (y, x) in ((cy + 2, cx), (cy + 3, cx - 1)):  # the other diagonal, across the column seam alone
                if 0 <= y < H and 0 <= x < W:
                    m[y, x] = 255
    return m


def _comb(W, H):
    """Teeth on every other column hanging from nothing, joined by a spine along the LAST row: they meet only at the end."""
    m = np.zeros((H, W), np.uint8)
    m[:, ::2] = 255
    m[H - 1, :] = 255
    return m


def _u_shape(W, H):
    """Two arms down the first and the last column that meet only in the last row."""
    m = np.zeros((H, W), np.uint8)
    m[:, 0] = 255
    m[:, W - 1] = 255
    m[H - 1, :] = 255
    if W > 4 and H > 2:
        m[0, 2:W - 2] = 77  # a bar of its own between the arms
    return m


def _spiral(W, H):
    """A rectangular spiral, one pixel wide with one pixel between the turns: walk ahead while the cell two ahead is free."""
    m = np.zeros((H, W), np.uint8)
    x = y = d = turns = 0
    m[0, 0] = 255
    steps = ((1, 0), (0, 1), (-1, 0), (0, -1))
    while turns < 2:
        dx, dy = steps[d]
        nx, ny, fx, fy = x + dx, y + dy, x + 2 * dx, y + 2 * dy
        if 0 <= nx < W and 0 <= ny < H and not m[ny, nx] and not (0 <= fx < W and 0 <= fy < H and m[fy, fx]):
            x, y, turns = nx, ny, 0
            m[y, x] = 255
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def _serpentine(W, H):
    """Every other row full, joined at alternating ends: one long snake that crosses every column seam in every row."""
    m = np.zeros((H, W), np.uint8)
    m[::2, :] = 9
    for k, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if k % 2 == 0 else 0] = 9
    return m


def _vsnake(W, H):
    """The same along the columns: crosses every row seam in every other column."""
    return np.array(_serpentine(H, W).T, order="C", copy=True).reshape(H, W).copy()


def _random(density):
    def make(W, H):
        rng = np.random.RandomState(int(density * 100) * 100003 + 7 * W + H)
        return (rng.random_sample((H, W)) < density).astype(np.uint8) * (1 + rng.randint(0, 255, (H, W))).astype(np.uint8)
    return make


MASKS = {"empty": _empty, "full": _full, "checker": _checker, "diagonals": _diagonals, "comb": _comb, "u": _u_shape, "spiral": _spiral,
         "serpentine": _serpentine, "vsnake": _vsnake, "random30": _random(0.3), "random59": _random(0.59), "random80": _random(0.8)}


# ---- the flow fields for join_px -----------------------------------------------------------------------------------------------

JOIN_PX = 0.5


def _two_blocks(W, H):
    """Two blocks that translate differently and touch along column 64 (a tile seam) or, in a narrow frame, the middle."""
    cut = 64 if W > 64 else W // 2
    u = np.full((H, W), 1.25, F)
    v = np.full((H, W), -0.5, F)
    u[:, cut:] = F(3.0)
    v[:, cut:] = F(0.75)
    return u, v


def _ramp(W, H):
    """u grows by exactly 0.5 = JOIN_PX per column (equality joins) except every seventh step, which is 2^-13 more (every
    value is exact in fp32 at these widths); v the same per row, every third step."""
    assert W <= 2048 and H <= 2048
    xs, ys = np.arange(W), np.arange(H)
    u = np.zeros((H, W), F)
    v = np.zeros((H, W), F)
    u[:, :] = (0.5 * xs + (xs // 7) * 2.0 ** -13).astype(F)[None, :]
    v[:, :] = (0.5 * ys + (ys // 3) * 2.0 ** -13).astype(F)[:, None]
    return u, v


def _sprinkled(W, H):
    """A gentle field with NaN, infinities and 3000-px pixels sprinkled in."""
    rng = np.random.RandomState(31 * W + H)
    u = (0.2 * rng.standard_normal((H, W))).astype(F)
    v = (0.2 * rng.standard_normal((H, W))).astype(F)
    bad = rng.random_sample((H, W))
    u[bad < 0.03] = np.nan
    v[(bad >= 0.03) & (bad < 0.06)] = F(3000.0)
    u[(bad >= 0.06) & (bad < 0.08)] = F(-2048.5)
    v[(bad >= 0.08) & (bad < 0.09)] = np.inf
    return u, v


FLOWS = {"two_blocks": _two_blocks, "ramp": _ramp, "sprinkled": _sprinkled}


@functools.lru_cache(maxsize=None)
def mask_of(name, W, H):
    m = MASKS[name](W, H)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def flow_of(name, W, H):
    u, v = FLOWS[name](W, H)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


def cases():
    """(case name, mask name or None, flow name or None, join_px): every mask alone, every flow with a full and a random
    mask under JOIN_PX, and one flow under join_px 0 (its sums alone)."""
    out = [(m, m, None, 0.0) for m in MASKS]
    for f in FLOWS:
        out.append((f + "-nomask", None, f, JOIN_PX))
        out.append((f + "-random80", "random80", f, JOIN_PX))
    out.append(("sprinkled-join0", "random59", "sprinkled", 0.0))
    return out


@functools.lru_cache(maxsize=None)
def planes(case, W, H):
    """(mask or None, u or None, v or None, join_px) of a case, read-only and shared."""
    for name, m, f, j in cases():
        if name == case:
            mask = mask_of(m, W, H) if m else None
            u, v = flow_of(f, W, H) if f else (None, None)
            return mask, u, v, j
    raise KeyError(case)


@functools.lru_cache(maxsize=None)
def want(case, W, H, connectivity, min_area=1, capacity=0):
    """The restatement's answer for a case, computed once."""
    mask, u, v, j = planes(case, W, H)
    return label(mask, u, v, connectivity, min_area, j, capacity, shape=(H, W))
