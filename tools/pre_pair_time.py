#!/usr/bin/env python3
"""What the pre-processing of a pair costs, this tree against a built tree of the parent commit (--parent-root) or of a
kernel variant (--variant-root): alone, in front of every pair of a resident stream, and from host buffers.

  A. the pre-processing alone: hsflow_set_frames_device_ex(BGR8_BLUR) on one context, HIP events on its stream around blocks
     of --reps calls (5 blocks after a warm-up; the figure includes what the host needs to enqueue the launches);
  B. the resident stream bench.py measures -- 6 slots on 2 streams, ITER|EPS, 100 sweeps -- fed with frames="bgr_blur", and
     with frames="gray" on frames blurred beforehand (the form without pre-processing): a host clock around --pairs
     submissions and the drain behind them, per block;
  C. the same stream shape fed from page-locked host buffers (PairPipeline.submit: upload into the staging, the
     pre-processing launch, solve, download), frames="gray_blur" and "bgr_blur", the same clock.

Every configuration runs in a fresh child process under a time limit of its own; the configurations of one size
alternate, and the first child that fails ends the run.  --root DIR takes the package from another tree.  The JSON ends
with the comparisons the figures are taken for, each with its verdict (`compare`).
usage: tools/pre_pair_time.py [--out profiles/frames_in_time.json] [--reps 400] [--pairs 300] [--rounds 2]
                              [--parent-root DIR] [--variant-root LABEL=DIR]"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SIZES = [(1920, 1080), (600, 480)]
BLOCKS = 5


def host_clock(go, pairs):
    """ms per pair of BLOCKS blocks of go(pairs) -- submissions and the drain behind them -- after a warm-up."""
    go(60)
    blocks = []
    for _ in range(BLOCKS):
        t0 = time.perf_counter()
        go(pairs)
        blocks.append((time.perf_counter() - t0) / pairs * 1e3)
    return blocks


def child(args):
    sys.path.insert(0, os.path.abspath(args.root or ROOT))
    import numpy as np
    import torch
    import opticalflowhs_amd as hs
    W, H = args.width, args.height
    from opticalflowhs_amd import synth
    # bench.py's two seed pairs, as colour frames whose three channels are the gray frame (BGR->gray then returns it exactly)
    gray = [f for sd in (1, 2) for f in synth.translating_pair(W, H, seed=sd)]
    bgr = [torch.from_numpy(np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))).cuda() for g in gray]
    if not args.frames.startswith("bgr"):
        bgr = [torch.from_numpy(g).cuda() for g in gray]
    out = {"what": args.child, "frames": args.frames, "width": W, "height": H,
           "version": hs._lib.load().hsflow_version()}
    if args.child == "pre":
        s = torch.cuda.Stream()
        with hs.HSFlow(W, H, 1, stream=s.cuda_stream) as ctx:
            def go(n):
                for k in range(n):
                    ctx.set_frames_device(bgr[(2 * k) & 3], bgr[(2 * k + 1) & 3], frames=args.frames)
            go(100)
            ctx.synchronize()
            blocks = []
            for _ in range(BLOCKS):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                go(args.reps)
                e1.record(s)
                e1.synchronize()
                blocks.append(e0.elapsed_time(e1) / args.reps)
            ctx.synchronize()
        out.update(unit="ms per pair (events around %d calls)" % args.reps, blocks=blocks)
    elif args.child == "host":
        src = [hs.pinned_empty(tuple(t.shape), np.uint8) for t in bgr]
        for h, t in zip(src, bgr):
            h[...] = t.cpu().numpy()
        outs = [(hs.pinned_empty((H, W), np.float32), hs.pinned_empty((H, W), np.float32)) for _ in range(7)]
        p = hs.make_params(lam=1.0, max_iter=100, term_type=hs.TERM_ITER | hs.TERM_EPS, epsilon=float(np.float32(1e-6)), use_graph=True)
        with hs.PairPipeline(W, H, depth=6, lanes=2) as pl:
            def go(n):
                for k in range(n):
                    pl.submit(src[(2 * k) & 3], src[(2 * k + 1) & 3], outs[k % 7][0], outs[k % 7][1], params=p, frames=args.frames)
                pl.drain()
            blocks = host_clock(go, args.pairs)
            info = pl.info(pl.submit(src[0], src[1], outs[0][0], outs[0][1], params=p, frames=args.frames))
            out.update(unit="ms per pair (host clock around %d submissions from page-locked buffers and the drain)" % args.pairs, blocks=blocks,
                       iterations_done=info["iterations_done"], eps_rerun=info["eps_rerun"], kernel=info["kernel"])
    else:
        if args.frames == "gray":   # blurred beforehand: what the stream was fed before there was a device route
            with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
                src = []
                for g in gray:
                    ctx.set_frames_gray_blur(g, g)
                    src.append(torch.from_numpy(ctx.frames()[0]).cuda())
        else:
            src = bgr
        torch.cuda.synchronize()
        p = hs.make_params(lam=1.0, max_iter=100, term_type=hs.TERM_ITER | hs.TERM_EPS, epsilon=float(np.float32(1e-6)), use_graph=True)
        kw = {} if args.frames == "gray" else {"frames": args.frames}
        with hs.PairPipeline(W, H, depth=6, lanes=2) as pl:
            def go(n):
                for k in range(n):
                    pl.submit_device(src[(2 * k) & 3], src[(2 * k + 1) & 3], params=p, **kw)
                pl.drain()
            blocks = host_clock(go, args.pairs)
            info = pl.info(pl.submit_device(src[0], src[1], params=p, **kw))
            out.update(unit="ms per pair (host clock around %d submissions and the drain)" % args.pairs, blocks=blocks,
                       iterations_done=info["iterations_done"], eps_rerun=info["eps_rerun"], kernel=info["kernel"], copies_elided=pl.copies_elided())
    print("RESULT " + json.dumps(out), flush=True)


def read_clocks():
    try:
        r = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60)
        return [line.strip() for line in r.stdout.splitlines() if "clk" in line.lower() and "GPU[0]" in line] or "not readable"
    except Exception as e:  # noqa: BLE001 -- a figure that could not be read is recorded as such
        return "not readable: %s" % e


def compare(runs):
    """What has to hold, evaluated: per size and figure, all blocks of all rounds of a configuration pooled.  `a` is not
    slower than `b` when median(a) <= median(b) + the larger of the two spreads (max - min of the pooled blocks)."""
    def pool(what, frames, W, build):
        b = sorted(x for r in runs if (r["what"], r["frames"], r["width"], r["build"]) == (what, frames, W, build) for x in r["blocks"])
        return {"median": b[len(b) // 2], "spread": b[-1] - b[0], "blocks": len(b)} if b else None
    out = []
    for W, H in SIZES:
        for other in sorted({r["build"] for r in runs} - {"this"}):
            for what, frames in sorted({(r["what"], r["frames"]) for r in runs}):
                a, b = pool(what, frames, W, "this"), pool(what, frames, W, other)
                if a and b:
                    out.append({"size": "%dx%d" % (W, H), "figure": what, "frames": frames, "a": "this tree", "b": other, "a_ms": a, "b_ms": b,
                                "a_not_slower_than_b": a["median"] <= b["median"] + max(a["spread"], b["spread"]),
                                "b_not_slower_than_a": b["median"] <= a["median"] + max(a["spread"], b["spread"])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_in_time.json"))
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--pairs", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--root", default=None)
    ap.add_argument("--commit", default=None, help="what to record as the commit where the tree is not a git checkout")
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit, built: every figure is measured on it too")
    ap.add_argument("--variant-root", default=None, metavar="LABEL=DIR",
                    help="a built tree of a kernel variant: pre alone and the bgr_blur stream are measured on it too")
    ap.add_argument("--limit", type=int, default=240, help="seconds a child may take")
    ap.add_argument("--child", choices=["pre", "stream", "host"])
    ap.add_argument("--frames", default="bgr_blur")
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    args = ap.parse_args()
    if args.child:
        return child(args)
    commit = args.commit
    if not commit:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
        except OSError:
            commit = "unknown"
    steps = []
    vlabel, vroot = args.variant_root.split("=", 1) if args.variant_root else (None, None)
    labels = {root: name for root, name in ((args.parent_root, "parent"), (vroot, vlabel)) if root}
    labels[None] = "this"
    both = [None] + ([args.parent_root] if args.parent_root else [])
    groups = [[("pre", "bgr_blur", True)], [("stream", "bgr_blur", True), ("stream", "gray", False)],
              [("host", "gray_blur", False), ("host", "bgr_blur", False)]]   # (figure, frames, on the variant as well)
    for W, H in SIZES:
        for group in groups:
            for _ in range(args.rounds):   # alternating: this tree, the parent, this tree, the parent ...
                steps += [(what, frames, W, H, root) for what, frames, v in group for root in both + ([vroot] if v and vroot else [])]
    results = {"commit": commit, "clocks_before": read_clocks(), "runs": []}
    for what, frames, W, H, root in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--frames", frames, "--width", str(W), "--height", str(H),
               "--reps", str(args.reps), "--pairs", str(args.pairs)] + (["--root", root] if root else [])
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)   # a child killed at its limit raises: the run ends
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit("step %r failed (%d): nothing further is started" % (cmd[3:], r.returncode))
        res = json.loads(line[0][7:])
        res["build"] = labels[root]
        b = sorted(res["blocks"])
        res["median"], res["spread"] = b[len(b) // 2], b[-1] - b[0]
        print("%-6s %-9s %4dx%-4d %-6s median %.4f ms  (blocks %s)" % (what, frames, W, H, res["build"], res["median"],
                                                                     " ".join("%.4f" % x for x in res["blocks"])), flush=True)
        results["runs"].append(res)
        results["clocks_after"] = read_clocks()
        results["comparisons"] = compare(results["runs"])
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
