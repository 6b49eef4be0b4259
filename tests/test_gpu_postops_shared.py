"""What the operators on a solved flow share on the host side (opticalflowhs_amd/csrc/hs_postops.hip.h: the synchronous
bracket, the staging planes, the statistics scratch, the device batches' prologue and chunk walk; the pipeline's guard and
wait in pair_pipeline.cpp): render, colour, warp, forward-backward check and median on ONE context, interleaved, against
their host twins -- pictures and masks byte for byte, fp32 planes bit for bit, records exactly.  Two sizes: 70 x 9, whose
packed rows are not word-aligned (the kernels' narrow path), and 72 x 9 (the wide path); two pairs per context."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from opticalflowhs_amd import synth
from test_gpu_fb import dev_stats, put_flow, same_bits
from test_gpu_render import yardstick
from test_fb_host import fields as fb_fields, stat_tuple as fb_tuple
from test_gpu_warp import stat_tuple as warp_tuple
from test_median_host import field as median_field, stat_tuple as median_tuple

pytestmark = pytest.mark.gpu

ITER, EPS = 1, 2
OK = 0
ENV_MAX = "HSFLOW_JPEG_BATCH_MAX"
SIZES = [(70, 9), (72, 9)]
RENDER = dict(step=2, threshold=0.05, scale=4.0)
MEDIAN = dict(radius=1, mode="filter", min_votes=2)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cuda(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def frames(W, H):
    """The frames of the two pairs: a translating pair, and the same pair backwards."""
    A, B = synth.translating_pair(W, H, seed=3, dx=1.5, dy=-0.75)
    return [(A, B), (B, A)]


def pictures(W, H, seed):
    """A source and a reference picture for the warp, one channel and three."""
    rng = np.random.default_rng(seed)
    return {c: tuple(rng.integers(0, 256, (H, W) if c == 1 else (H, W, 3), dtype=np.uint8) for _ in range(2)) for c in (1, 3)}


# ---- 1. the synchronous forms interleaved on one context, an ITER|EPS check owed ------------------------------------------

class Twins(object):
    """The host twins of the five synchronous forms from the flows (u, v) of the two pairs, computed once; `check_*` runs
    one form on the context and compares."""

    def __init__(self, hs, W, H, flows):
        self.hs = hs
        (u0, v0), (u1, v1) = flows
        self.src, self.ref = pictures(W, H, 5)[1]
        self.state = median_field(W, H, 9)[2]
        self.render = yardstick(u0, v0, "cv", **RENDER)
        self.color, self.scale = hs.color_flow_host(u1, v1, return_scale=True)
        pic, st = hs.warp_host(u0, v0, self.src, ref=self.ref, return_stats=True)
        self.warp = (pic, warp_tuple(st))
        mask, err2, st = hs.fb_host(u0, v0, u1, v1, mask=True, err2=True, stats=True)
        self.fb = (mask, bits(err2), fb_tuple(st))
        uo, vo, so, st = hs.median_host(u1, v1, self.state, state_out=True, stats=True, passes=2, **MEDIAN)
        self.median = (bits(uo), bits(vo), so, median_tuple(st))

    def check_render(self, ctx):
        assert np.array_equal(ctx.render("cv", pair=0, **RENDER), self.render)

    def check_color(self, ctx):
        pic, scale = ctx.color(pair=1, return_scale=True)
        assert np.array_equal(pic, self.color) and scale == self.scale

    def check_warp(self, ctx):
        pic, st = ctx.warp(self.src, ref=self.ref, pair=0, return_stats=True)
        assert np.array_equal(pic, self.warp[0]) and warp_tuple(st) == self.warp[1]

    def check_fb(self, ctx):
        mask, err2, st = ctx.fb(0, 1, mask=True, err2=True, stats=True)
        assert np.array_equal(mask, self.fb[0]) and np.array_equal(bits(err2), self.fb[1]) and fb_tuple(st) == self.fb[2]

    def check_median(self, ctx):
        uo, vo, so, st = ctx.median(1, self.state, state_out=True, stats=True, passes=2, **MEDIAN)
        assert np.array_equal(bits(uo), self.median[0]) and np.array_equal(bits(vo), self.median[1])
        assert np.array_equal(so, self.median[2]) and median_tuple(st) == self.median[3]

    def sequence(self):
        return [self.check_render, self.check_color, self.check_warp, self.check_fb, self.check_median]


@pytest.mark.parametrize("W,H", SIZES)
def test_interleaved_behind_an_owed_check(hs, gpu_ok, W, H):
    """Every form settles the owed check of the asynchronous solve in front of it, names the flow only then, waits for its
    own work and leaves the context as the solve left it."""
    L = hs._lib.load()
    kw = dict(lam=1.0, max_iter=60, term_type=ITER | EPS, epsilon=0.05)   # (Eps of sweep 60 is 0.0102 at both sizes: the stop fires)
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        assert L.hsflow_set_async_reduce(ctx._h, 1) == OK
        for p, (A, B) in enumerate(frames(W, H)):
            ctx.set_frames(A, B, pair=p)
        info = ctx.solve(**kw)
        assert 1 < info["iterations_done"] < 60, info                # so the owed check of the asynchronous solve ends in a re-run
        flows = [ctx.flow(p) for p in range(2)]                       # taken once: every twin is computed from these
        assert all(np.abs(f).max() > 0.1 for uv in flows for f in uv)
        twins = Twins(hs, W, H, flows)
        print("solve:", {k: info[k] for k in ("iterations_done", "last_eps", "eps_rerun", "kernel")})
        for order in (twins.sequence(), twins.sequence()[::-1]):
            ctx.solve_async(**kw)                                     # the same solve again: its ITER|EPS check is owed
            for check in order:
                check(ctx)
        for p in range(2):
            u, v = ctx.flow(p)
            assert same_bits(u, flows[p][0]) and same_bits(v, flows[p][1]), p
        after = ctx.info()
        print("after:", {k: after[k] for k in ("iterations_done", "last_eps", "eps_rerun", "kernel")})
        for k in ("iterations_done", "last_eps", "kernel", "width", "height", "n_pairs"):
            assert after[k] == info[k], (k, after[k], info[k])


# ---- 2. staging growth ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SIZES)
def test_staging_grows(hs, gpu_ok, W, H):
    """The synchronous warp with one channel, then with three: its staging pictures grow.  The check with the mask alone,
    then with err2: a second staging plane appears.  The later calls are still the host twin's."""
    uf, vf, ub, vb = fb_fields(W, H, 7 * W + H)
    pics = pictures(W, H, 11)
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        put_flow(ctx, uf, vf, pair=0)
        put_flow(ctx, ub, vb, pair=1)
        for channels in (1, 3, 1):
            src, ref = pics[channels]
            want, wst = hs.warp_host(ub, vb, src, ref=ref, return_stats=True)
            got, gst = ctx.warp(src, ref=ref, pair=1, return_stats=True)
            assert np.array_equal(got, want) and warp_tuple(gst) == warp_tuple(wst), channels
        wm, we, ws = hs.fb_host(uf, vf, ub, vb, mask=True, err2=True, stats=True)
        gm, ge, gs = ctx.fb(0, 1, mask=True, err2=False, stats=False)
        assert np.array_equal(gm, wm) and ge is None and gs is None
        gm, ge, gs = ctx.fb(0, 1, mask=True, err2=True, stats=True)
        assert np.array_equal(gm, wm) and np.array_equal(bits(ge), bits(we)) and fb_tuple(gs) == fb_tuple(ws)
        u, v = ctx.flow(1)
        assert same_bits(u, ub) and same_bits(v, vb)


# ---- 3. chunking through the shared loop ----------------------------------------------------------------------------------

def batch_results(W, H):
    """warp_batch_device, fb_batch_device and median_batch_device over both pairs of a context, with statistics: every
    plane and every record as bytes, by name.  Runs in this process and, with another chunk size in the environment, in a
    child."""
    import torch
    import opticalflowhs_amd as hs
    uf, vf, ub, vb = fb_fields(W, H, 3 * W + H)
    states = np.stack([median_field(W, H, 40 + p)[2] for p in range(2)])
    src, ref = (np.stack([pictures(W, H, 20 + p)[1][k] for p in range(2)]) for k in range(2))
    out = {}
    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        put_flow(ctx, uf, vf, pair=0)
        put_flow(ctx, ub, vb, pair=1)
        warped, wrec = torch.zeros((2, H, W), dtype=torch.uint8, device="cuda"), dev_stats(2)
        ctx.warp_batch_device(out=warped, src=cuda(src), ref=cuda(ref), stats=wrec)
        mask, err2, frec = torch.zeros((2, H, W), dtype=torch.uint8, device="cuda"), torch.zeros((2, H, W), dtype=torch.float32, device="cuda"), dev_stats(2)
        ctx.fb_batch_device([0, 1], [1, 0], mask=mask, err2=err2, stats=frec)
        uo, vo = (torch.zeros((2, H, W), dtype=torch.float32, device="cuda") for _ in range(2))
        so, mrec = torch.zeros((2, H, W), dtype=torch.uint8, device="cuda"), dev_stats(2)
        ctx.median_batch_device(0, 2, state=cuda(states), u_out=uo, v_out=vo, state_out=so, stats=mrec, **MEDIAN)
        ctx.synchronize()
        for name, t in (("warped", warped), ("wrec", wrec), ("mask", mask), ("err2", err2), ("frec", frec), ("uo", uo), ("vo", vo), ("so", so), ("mrec", mrec)):
            out[name] = np.frombuffer(t.cpu().numpy().tobytes(), np.uint8)
        u, v = ctx.flow(1)
        assert same_bits(u, ub) and same_bits(v, vb)
    return out


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import test_gpu_postops_shared as t
np.savez(sys.argv[1], **t.batch_results(int(sys.argv[2]), int(sys.argv[3])))
print("CHILD-OK")
"""


@pytest.mark.parametrize("W,H", SIZES)
def test_chunks_of_one_equal_the_default(hs, gpu_ok, tmp_path, W, H):
    """HSFLOW_JPEG_BATCH_MAX=1 in a fresh process: two chunks of one pair through the shared loop give the planes and
    records of the default, one chunk of two."""
    assert not os.environ.get(ENV_MAX)
    want = batch_results(W, H)
    assert want["warped"].any() and want["mask"].any() and want["so"].any() and all(want[k][:128].any() for k in ("wrec", "frec", "mrec"))
    path = str(tmp_path / "chunks.npz")
    env = dict(os.environ)
    env[ENV_MAX] = "1"
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), path, str(W), str(H)], capture_output=True, text=True,
                       timeout=300, cwd=ROOT, env=env)
    assert r.returncode == 0 and "CHILD-OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    got = np.load(path)
    assert sorted(got.files) == sorted(want)
    for name in want:
        assert np.array_equal(got[name], want[name]), name


# ---- 4. pipeline ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W,H", SIZES)
def test_pipeline_device_forms(hs, gpu_ok, W, H):
    """Depth 2, two tickets (a pair and the same pair backwards): the device forms of warp, check and median_apply behind
    wait() give what the same calls give on a plain context with the same frames."""
    import torch
    kw = dict(lam=1.0, max_iter=30, term_type=ITER)
    pairs = frames(W, H)
    dev = [tuple(cuda(f) for f in AB) for AB in pairs]
    src, ref = (cuda(p) for p in pictures(W, H, 13)[1])
    state = cuda(median_field(W, H, 17)[2])
    mkw = dict(passes=2, state_out=True, stats=True, **MEDIAN)

    def fresh():
        return torch.zeros((H, W), dtype=torch.uint8, device="cuda")

    with hs.HSFlow(W, H, 2, own_stream=True) as ctx:
        for p, (A, B) in enumerate(pairs):
            ctx.set_frames(A, B, pair=p)
        ctx.solve(**kw)
        w_pic, w_rec = ctx.warp(src, ref=ref, out=fresh(), pair=0, return_stats=True)
        w_mask, w_err2, w_frec = ctx.fb(0, 1, mask=True, err2=True, stats=True, device=True)
        w_so, w_mrec = ctx.median_apply(1, state, **mkw)
        ctx.synchronize()
        want = dict(pic=w_pic.cpu().numpy(), wrec=warp_tuple(hs.warp_stats_from(w_rec)), mask=w_mask.cpu().numpy(), err2=bits(w_err2.cpu().numpy()),
                    frec=fb_tuple(hs.fb_stats_from(w_frec)), so=w_so.cpu().numpy(), mrec=median_tuple(hs.median_stats_from(w_mrec)),
                    flow=[tuple(bits(f) for f in ctx.flow(p)) for p in range(2)])
    assert want["pic"].any() and want["mask"].any() and np.abs(want["flow"][0][0].view(np.float32)).max() > 0.1
    with hs.PairPipeline(W, H, depth=2) as pl:
        t = [pl.submit_device(a, b, **kw) for a, b in dev]
        assert t == [0, 1]
        for ticket in t:
            pl.wait(ticket)
        pic, rec = pl.warp(t[0], src, ref=ref, out=fresh(), return_stats=True)       # complete on return, each of them
        assert np.array_equal(pic.cpu().numpy(), want["pic"]) and warp_tuple(hs.warp_stats_from(rec)) == want["wrec"]
        mask, err2, rec = pl.fb(t[0], t[1], mask=True, err2=True, stats=True, device=True)
        assert np.array_equal(mask.cpu().numpy(), want["mask"]) and np.array_equal(bits(err2.cpu().numpy()), want["err2"])
        assert fb_tuple(hs.fb_stats_from(rec)) == want["frec"]
        so, rec = pl.median_apply(t[1], state, **mkw)
        assert np.array_equal(so.cpu().numpy(), want["so"]) and median_tuple(hs.median_stats_from(rec)) == want["mrec"]
        for p in range(2):                                            # pair 1's flow replaced, pair 0's as solved
            u, v = pl.flow_device(t[p])
            assert np.array_equal(bits(u.cpu().numpy()), want["flow"][p][0]) and np.array_equal(bits(v.cpu().numpy()), want["flow"][p][1]), p
