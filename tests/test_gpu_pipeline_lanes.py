"""Pair pipeline on SHARED streams (hsflow_pipeline_create_lanes with lanes < depth): the form bench.py's headline runs
(hsflow_pipeline_submit_device, 6 slots on 2 streams).  Seeded random schedules of submits, waits, info and flow_device
calls run against a model of the slots' state (include/hsflow.h, pair_pipeline.cpp) that says which calls must succeed;
every flow and report that comes back must be the synchronous solve of the same pair on a plain context, bit for bit.
Also pinned: the launch shape the pipeline picks by itself with three or more lanes (stream_shape, pair_pipeline.cpp)."""
import collections

import numpy as np
import pytest

from opticalflowhs_amd import synth

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
EPS6 = float(np.float32(1e-6))
RMS_TOL = 1e-4
OK, E_ARG, E_STATE = 0, 1, 5
SHAPE = ("kernel", "fuse_steps", "groups_per_thread", "threads", "tiles")

PARAMS = {
    "P1": dict(lam=1.0, max_iter=100, term_type=ITER | EPS, epsilon=EPS6, use_graph=True),  # the headline's call
    "P2": dict(lam=1.0, max_iter=37, term_type=ITER),                                       # 20 + a tail launch of 17
    "P3": dict(lam=1e-3, max_iter=400, term_type=ITER | EPS, epsilon=1e-4),                 # the patch pair stops early
    "P4": dict(lam=1.0, max_iter=7, term_type=ITER | EPS, epsilon=EPS6),                    # fewer sweeps than one launch
}
KINDS = ("t1", "t2", "random", "patch", "same")
FLAT_KINDS = ("patch", "same")  # where flow decays below 1e-30: the only pairs the exemption may cover


def make_frames(kind, W, H):
    if kind in ("t1", "t2"):
        return synth.translating_pair(W, H, seed=int(kind[1]))   # bench.py's two seed pairs
    if kind == "random":
        return synth.random_pair(W, H, seed=3)
    if kind == "patch":                                          # a flat frame with a patch one grey level brighter
        a = np.full((H, W), 90, np.uint8)
        b = a.copy()
        rows, cols = slice(H // 4, H // 4 + min(80, H // 2)), slice(W // 5, W // 5 + min(300, W // 2))
        a[rows, cols], b[rows, cols] = 120, 121
        return a, b
    a, _ = synth.random_pair(W, H, seed=5)                       # identical frames: Eps = 0 after the first sweep
    return a, a.copy()


def override_shape(hs, W, H, lanes, p):
    """(kernel, fuse_steps, rows per lane, threads) that stream_shape must give a pair, or None where it must stay off."""
    if (lanes < 3 or p.mode != hs.MODE_CV or p.kernel != hs.KERNEL_AUTO or p.fuse_steps or p.strip_rows or p.threads or p.tile_w
            or p.tile_h or not (p.term_type & ITER) or p.max_iter <= 0 or W * H > 1500000 or W < 256 or H < 80):
        return None
    T = min(20, p.max_iter)
    cw, ch = 256 - 2 * ((T + 3) // 4 * 4), 80 - 2 * T
    tiles16 = -(-W // cw) * -(-H // ch)
    return (hs.KERNEL_STRIP, T, 5, 1024 if tiles16 >= 50 else 768)


def shape_of(info):
    return tuple(info[f] for f in SHAPE)


def flows_match(got, want):
    """Bit equality, or equality above 1e-30 (the caller has checked that the exemption applies)."""
    return bool(((got == want) | ((got.abs() < 1e-30) & (want.abs() < 1e-30))).all())


class Reference(object):
    """The synchronous solve of every (pair kind, parameter set) on a plain context: flow (device tensors) and report.  Where
    the pipeline takes its own launch shape, also the synchronous solve with that shape asked for explicitly (`shaped`):
    whether the witness pass of an ITER|EPS solve proves "no early stop" (eps_rerun = 0) depends on the shape."""

    def __init__(self, hs, W, H, frames, lanes):
        import torch
        self.flow, self.info, self.shaped = {}, {}, {}
        dev = lambda f: tuple(torch.from_numpy(x).cuda() for x in f)
        with hs.HSFlow(W, H, own_stream=True) as ctx:
            for k in KINDS:
                ctx.set_frames(*frames[k])
                for pn, kw in PARAMS.items():
                    self.info[(k, pn)] = ctx.solve(**kw)
                    self.flow[(k, pn)] = dev(ctx.flow())
                    ov = override_shape(hs, W, H, lanes, hs.make_params(**kw))
                    if ov is not None:
                        i = ctx.solve(**dict(kw, kernel=ov[0], fuse_steps=ov[1], strip_rows=ov[2], threads=ov[3]))
                        self.shaped[(k, pn)] = (i, dev(ctx.flow()))
        for pn in ("P1", "P3", "P4"):
            i = self.info[("same", pn)]
            assert i["iterations_done"] == 1 and i["eps_rerun"] == 1, (pn, i)
        i = self.info[("patch", "P3")]
        assert 1 < i["iterations_done"] < 400 and i["eps_rerun"] == 1, i   # the rerun path with a flow that differs from the budget's
        i = self.info[("t1", "P1")]
        assert i["iterations_done"] == 100 and i["eps_rerun"] == 0, i


def run_schedule(hs, pl, W, H, depth, lanes, ref, frames, seed, host, n_ops=90):
    """A seeded random schedule on `pl`; returns the tally of what it did."""
    import torch
    rng = np.random.default_rng(seed)
    combos = [(k, pn) for k in KINDS for pn in PARAMS]
    first = [combos[i] for i in rng.permutation(len(combos))]       # every combination at least once
    params = {pn: hs.make_params(**kw) for pn, kw in PARAMS.items()}
    dev = {k: (torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for k, (a, b) in frames.items()}
    host_ref = {key: (u.cpu().numpy(), v.cpu().numpy()) for key, (u, v) in ref.flow.items()} if host else None
    torch.cuda.synchronize()
    what, src, outs = [], {}, {}
    finished, just = set(), []
    tally = collections.Counter()

    def finish(t):
        if t < len(what) and t not in finished:
            finished.add(t)
            just.append(t)

    def check_flow(t, u, v, where):
        k, pn = what[t]
        ur, vr = ref.flow[(k, pn)]
        if (k, pn) in ref.shaped:   # the pipeline's own shape: the same launches as on a plain context, the same bits
            us, vs = ref.shaped[(k, pn)][1]
            assert torch.equal(u, us) and torch.equal(v, vs), (where, t, k, pn)
        if torch.equal(u, ur) and torch.equal(v, vr):
            return
        # the one exemption: a flat synthetic pair, solved in another launch shape, differs below 1e-30 only
        assert k in FLAT_KINDS, (where, t, k, pn)
        got = shape_of(pl.info(t))
        assert got != shape_of(ref.info[(k, pn)]), (where, t, k, pn, got)
        assert flows_match(u, ur) and flows_match(v, vr), (where, t, k, pn)
        tally["exempt"] += 1

    def check_info(t, info, idle):
        k, pn = what[t]
        r = ref.info[(k, pn)]
        assert info["iterations_done"] == r["iterations_done"], (t, k, pn, info, r)
        ov = override_shape(hs, W, H, lanes, params[pn])
        if ov is None:   # no override, no CU share: the asynchronous solve must plan exactly as the synchronous one did
            assert shape_of(info) == shape_of(r), (t, k, pn, shape_of(info), shape_of(r))
        else:
            assert shape_of(info)[:4] == ov, (t, k, pn, shape_of(info), ov)
            r = ref.shaped[(k, pn)][0]
            assert shape_of(info) == shape_of(r), (t, k, pn, shape_of(info), shape_of(r))
        assert info["eps_rerun"] == r["eps_rerun"], (t, k, pn, info, r)
        if idle:         # (while the slot runs the next pair the report keeps what settling measured: no last_eps)
            assert info["last_eps"] == r["last_eps"], (t, k, pn, info["last_eps"], r["last_eps"])
        tally["info"] += 1

    def after_call():
        # every ticket a call just waited for: its host outputs are final, and its source buffers may be reused now
        for t in just:
            if host:
                u, v, big = outs[t]
                ur, vr = host_ref[what[t]]
                if not (np.array_equal(u, ur) and np.array_equal(v, vr)):
                    check_flow(t, torch.from_numpy(np.ascontiguousarray(u)).cuda(), torch.from_numpy(np.ascontiguousarray(v)).cuda(), "host")
                if big is not None:
                    assert np.isnan(big[:, :, W:]).all(), t   # padding columns untouched
                for a in src.pop(t):
                    a.fill(0)
            else:
                for a in src.pop(t):
                    a.fill_(0)
        if just and not host:
            torch.cuda.synchronize()
        del just[:]

    def expect(status, fn, *a):
        if status == OK:
            return fn(*a)
        with pytest.raises(hs.HsflowError) as e:
            fn(*a)
        assert e.value.status == status, (fn.__name__, a, e.value)
        tally["%s %d" % (fn.__name__, status)] += 1
        return None

    def submit():
        t = len(what)
        k, pn = first[t] if t < len(first) else combos[rng.integers(len(combos))]
        if host:
            a, b = hs.pinned_empty((H, W), np.uint8), hs.pinned_empty((H, W), np.uint8)
            a[...], b[...] = frames[k]
            big = None
            if t % 4 == 3:   # pageable, row stride > width
                big = np.full((2, H, W + 7), np.nan, np.float32)
                u, v = big[0, :, :W], big[1, :, :W]
            else:
                u, v = hs.pinned_empty((H, W), np.float32), hs.pinned_empty((H, W), np.float32)
                u.fill(np.nan)
                v.fill(np.nan)
            got = pl.submit(a, b, u, v, params=params[pn])
            outs[t] = (u, v, big)
        else:
            a, b = dev[k][0].clone(), dev[k][1].clone()   # this pair's own buffers: zeroed once a call waited for it
            torch.cuda.synchronize()                      # (complete when submit is called)
            got = pl.submit_device(a, b, params=params[pn])
        assert got == t
        src[t] = (a, b)
        what.append((k, pn))
        if t >= depth:
            finish(t - depth)                             # the slot's previous pair was waited for inside submit
        tally["submit"] += 1

    def wait(t):
        if t >= len(what):
            return expect(E_ARG, pl.wait, t)
        pl.wait(t)
        finish(t)

    def info(t):
        n = len(what)
        if t >= n:
            return expect(E_ARG, pl.info, t)
        finish(t)
        if t + depth < n and t + depth in finished:       # the slot's next pair has finished: that report is gone
            return expect(E_STATE, pl.info, t)
        check_info(t, pl.info(t), idle=t + depth >= n)

    def flow_device(t, copy):
        n = len(what)
        if t >= n:
            return expect(E_ARG, pl.flow_device, t, copy)
        finish(t)
        if t + depth < n:                                 # the slot has taken another pair: its planes are not t's
            return expect(E_STATE, pl.flow_device, t, copy)
        u, v = pl.flow_device(t, copy=copy)
        check_flow(t, u, v, "flow_device")
        tally["flow"] += 1

    def drain():
        pl.drain()
        for t in range(len(what)):
            finish(t)

    def pick():
        n = len(what)
        return int(rng.integers(max(0, n - 2 * depth - 1), n))

    for _ in range(n_ops):
        r = rng.random()
        if not what or r < 0.45:
            submit()
        elif r < 0.60:
            info(pick())
        elif r < 0.77:
            flow_device(pick(), bool(rng.integers(2)))
        elif r < 0.86:
            wait(pick())
        elif r < 0.93:                                    # out of order on one lane: the later pair first
            t = pick()
            wait(t + lanes)
            after_call()
            wait(t)
        elif r < 0.96:
            drain()
        else:                                             # a ticket that was never issued
            [wait, info, lambda t: flow_device(t, True)][int(rng.integers(3))](len(what) + int(rng.integers(3)))
        after_call()
    drain()
    after_call()
    n = len(what)
    assert n >= 3 * depth, (n, depth)                    # every slot went round at least three times
    # long after their frames were released: the last pair of every slot is still there, unchanged
    for t in range(n - depth, n):
        u, v = pl.flow_device(t, copy=False)
        check_flow(t, u, v, "after drain")
        check_info(t, pl.info(t), idle=True)
    if host:
        for t, (u, v, big) in outs.items():
            ur, vr = host_ref[what[t]]
            assert np.array_equal(u, ur) and np.array_equal(v, vr) or what[t][0] in FLAT_KINDS, t
    tally["reruns"] = sum(ref.info[what[t]]["eps_rerun"] for t in range(n))
    return tally


CONFIGS = [  # depth, lanes, W, H, entry point, schedule seed
    pytest.param(6, 2, 1920, 1080, "device", 61, id="headline-6x2-1080p"),
    pytest.param(4, 1, 640, 480, "device", 62, id="one-lane-4x1-640x480"),
    pytest.param(5, 3, 640, 480, "device", 63, id="own-shape-5x3-640x480"),
    pytest.param(8, 3, 424, 240, "device", 64, id="own-shape-8x3-424x240"),
    pytest.param(4, 2, 600, 480, "host", 65, id="host-4x2-600x480"),
]


@pytest.mark.parametrize("depth,lanes,W,H,entry,seed", CONFIGS)
def test_shared_lane_schedule_equals_the_synchronous_solve(hs, oracle, gpu_ok, depth, lanes, W, H, entry, seed):
    frames = {k: make_frames(k, W, H) for k in KINDS}
    ref = Reference(hs, W, H, frames, lanes)
    with hs.PairPipeline(W, H, depth=depth, lanes=lanes) as pl:
        tally = run_schedule(hs, pl, W, H, depth, lanes, ref, frames, seed, host=entry == "host")
    # the schedule did what it is there for: stale tickets refused, rerun pairs, flows read back
    assert tally["flow_device %d" % E_STATE] > 0 and tally["info %d" % E_STATE] > 0, tally
    assert tally["reruns"] > 0 and tally["flow"] > 5 and tally["info"] > 5, tally
    if lanes < 3:
        assert tally["exempt"] == 0, tally
    # the reference itself against the CPU oracle, on a textured and on the early-stopping pair
    for k, pn in (("t1", "P1"), ("patch", "P3")):
        kw = PARAMS[pn]
        uo, vo, n_o, _ = oracle.calc_optical_flow_hs(*frames[k], kw["lam"], kw["max_iter"], kw.get("epsilon", 1e-6), kw["term_type"],
                                                     threads=0, return_info=True)
        u, v = (x.cpu().numpy().astype(np.float64) for x in ref.flow[(k, pn)])
        assert np.sqrt(np.mean((u - uo) ** 2)) <= RMS_TOL and np.sqrt(np.mean((v - vo) ** 2)) <= RMS_TOL, (k, pn)
        assert abs(n_o - ref.info[(k, pn)]["iterations_done"]) <= 1, (k, pn, n_o, ref.info[(k, pn)]["iterations_done"])


OVERRIDE_CASES = [  # W, H, lanes, what the caller set, threads of the pipeline's own shape (None: the override stays off)
    pytest.param(255, 120, 3, {}, None, id="w255"),
    pytest.param(256, 120, 3, {}, 768, id="w256"),
    pytest.param(320, 79, 3, {}, None, id="h79"),
    pytest.param(320, 80, 3, {}, 768, id="h80"),
    pytest.param(1080, 360, 3, {}, 768, id="45tiles"),
    pytest.param(1080, 400, 3, {}, 1024, id="50tiles"),
    pytest.param(1500, 1000, 3, {}, 1024, id="1.5Mpix"),
    pytest.param(1501, 1000, 3, {}, None, id="above-1.5Mpix"),
    pytest.param(640, 480, 3, dict(kernel=3), None, id="kernel"),
    pytest.param(640, 480, 3, dict(fuse_steps=10), None, id="fuse_steps"),
    pytest.param(640, 480, 3, dict(strip_rows=4), None, id="strip_rows"),
    pytest.param(640, 480, 3, dict(threads=512), None, id="threads"),
    pytest.param(640, 480, 3, dict(mode=1, alpha=15.0), None, id="classic"),
    pytest.param(640, 480, 2, {}, None, id="two-lanes"),
]


@pytest.mark.parametrize("W,H,lanes,extra,threads", OVERRIDE_CASES)
def test_pipeline_launch_shape_override_is_pinned(hs, gpu_ok, W, H, lanes, extra, threads):
    """stream_shape: with >= 3 lanes, a pair that left its shape to the planner on a frame of 256 x 80 .. 1.5 Mpixel runs the strip
    kernel with min(20, max_iter) sweeps per launch, 5 rows per lane, 768 / 1024 threads (>= 50 tiles of 16 wavefronts: 1024);
    anywhere else the planner's shape stands.  Either way the flow is the plain context's, bit for bit."""
    import torch
    runs = [dict(lam=1.0, max_iter=30, term_type=ITER | EPS, epsilon=EPS6, use_graph=True), dict(lam=0.5, max_iter=25, term_type=ITER)]
    if extra.get("mode") == hs.MODE_CLASSIC:
        runs = runs[1:]          # (the classic mode terminates on ITER only)
    runs = [dict(kw, **extra) for kw in runs]
    pairs = [synth.translating_pair(W, H, seed=1), synth.random_pair(W, H, seed=3)]
    dev = [(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()) for a, b in pairs]
    torch.cuda.synchronize()
    with hs.HSFlow(W, H, own_stream=True) as ctx, hs.PairPipeline(W, H, depth=3, lanes=lanes) as pl:
        for kw in runs:
            p = hs.make_params(**kw)
            want = override_shape(hs, W, H, lanes, p)
            assert (want is None) == (threads is None) and (want is None or want[3] == threads), (want, threads)
            for (A, B), (a, b) in zip(pairs, dev):
                ctx.set_frames(A, B)
                r = ctx.solve(p)
                ur, vr = (torch.from_numpy(x).cuda() for x in ctx.flow())
                t = pl.submit_device(a, b, params=p)
                u, v = pl.flow_device(t)
                i = pl.info(t)
                assert i["iterations_done"] == r["iterations_done"], (kw, i, r)
                if threads is None:
                    assert shape_of(i) == shape_of(r) and i["eps_rerun"] == r["eps_rerun"], (kw, i, r)
                else:
                    assert shape_of(i)[:4] == (hs.KERNEL_STRIP, min(20, p.max_iter), 5, threads), (kw, shape_of(i))
                assert torch.equal(u, ur) and torch.equal(v, vr), kw
                if threads is not None:   # the same shape asked for explicitly on a plain context: the same launches, the same bits
                    x = ctx.solve(**dict(kw, kernel=hs.KERNEL_STRIP, fuse_steps=min(20, p.max_iter), strip_rows=5, threads=threads))
                    assert shape_of(x) == shape_of(i) and x["eps_rerun"] == i["eps_rerun"], (kw, x, i)
                    ux, vx = (torch.from_numpy(y).cuda() for y in ctx.flow())
                    assert torch.equal(ux, u) and torch.equal(vx, v), kw
