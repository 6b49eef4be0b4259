#!/usr/bin/env python3
"""What labelling the moving regions of a pair (hsflow_regions_device / _batch_device) costs beside today's
routes.  One size, 1920x1080, on a context of 8 pairs that all hold the flow of the benchmark's pair (the translating
texture of seed 1, lambda 1, 100 iterations).  Per CALL, device events around --reps calls back to back, the C entries
called with arguments prepared once; labels, 64 records and the header are asked for:
  gmotion       one pair, the foreground mask of hsflow_gmotion_fit (values {0, 255, 0, 0}) of that flow, 8-connectivity;
  full          one pair, every pixel foreground: ONE region, every count on one root;
  random59      one pair, a seeded random mask of density 0.59, 4-connectivity: the percolation threshold;
  gmotion x8    the 8 pairs by one hsflow_regions_batch_device (ms per CALL, not per pair);
  copy          (a) a device-to-device copy of the mask plus the label plane;
  host          (b) the route it replaces: mask and flow read back, hsflow_regions_host, the records in hand; a host clock
                around one round, and its labels, records and header equal the device's byte for byte.
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported, and after
a session that failed nothing more is started.
   usage: tools/regions_time.py [--reps 50] [--sessions 3] [--out profiles/regions_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
W, H, PAIRS, CAPACITY = 1920, 1080, 8, 64
MASKS = (("gmotion", 8), ("full", 8), ("random59", 4))
ROWS = [m for m, _ in MASKS] + ["gmotion x8", "copy"] + ["host " + m for m, _ in MASKS]


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n & 1 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def run_child(reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opticalflowhs_amd as hs
    from opticalflowhs_amd import synth
    L = hs._lib.load()
    s = torch.cuda.Stream()

    def events(fn, n=reps):
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(n):
            fn()
        e1.record(s)
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    A, B = synth.translating_pair(W, H, seed=1)
    with hs.HSFlow(W, H, 1) as one:
        one.set_frames(np.ascontiguousarray(A, np.uint8), np.ascontiguousarray(B, np.uint8))
        one.solve(lam=1.0, max_iter=100)
        u, v = one.flow(0)
    gp = hs.make_gmotion_params(values=(0, 255, 0, 0))
    _, gmask, _, _ = hs.global_motion_host(u, v, mask=True, params=gp)
    rng = np.random.RandomState(59)
    masks = {"gmotion": gmask, "full": np.full((H, W), 255, np.uint8), "random59": (rng.random_sample((H, W)) < 0.59).astype(np.uint8) * 255}
    res = {}
    with hs.HSFlow(W, H, PAIRS, stream=s.cuda_stream) as ctx:
        ud, vd = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
        torch.cuda.synchronize()
        for k in range(PAIRS):
            ctx.set_flow_rows_from(ud, vd, 0, H, pair=k)
        ctx.synchronize()
        new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
        labels, recs, heads = new((PAIRS, H, W), torch.int32), new((PAIRS, CAPACITY * 64), torch.uint8), new((PAIRS * 64,), torch.uint8)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        plist = lambda t: (ctypes.c_void_p * PAIRS)(*[t[k].data_ptr() for k in range(PAIRS)])
        for name, conn in MASKS:
            rp = hs.make_regions_params(connectivity=conn)
            dm = torch.from_numpy(masks[name]).cuda()
            torch.cuda.synchronize()

            def one_pair():
                assert L.hsflow_regions_device(ctx._h, 0, P(dm), W, ctypes.byref(rp), P(labels[0]), 4 * W, P(recs[0]), CAPACITY, P(heads)) == 0
            res[name] = events(one_pair)
            ctx.synchronize()
            head = hs.regions_result_from(heads)
            dev = (labels[0].cpu().numpy(), bytes(recs[0].cpu().numpy())[:head.n_written * 64], bytes(head))
            t0 = time.perf_counter()
            hm = dm.cpu().numpy()
            hu, hv = ctx.flow(0)
            hres, hlab, hrec = hs.regions_host(hm, hu, hv, labels=True, records=True, capacity=CAPACITY, params=rp)
            res["host " + name] = (time.perf_counter() - t0) * 1e3
            assert np.array_equal(hlab, dev[0]) and bytes(hrec)[:hres.n_written * 64] == dev[1] and bytes(hres) == dev[2], name
            res["regions " + name] = int(head.n_regions)
            if name == "gmotion":
                ml, ll, rl = (ctypes.c_void_p * PAIRS)(*[dm.data_ptr()] * PAIRS), plist(labels), plist(recs)

                def batch():
                    assert L.hsflow_regions_batch_device(ctx._h, 0, PAIRS, ml, W, ctypes.byref(rp), ll, 4 * W, rl, CAPACITY, P(heads)) == 0
                res["gmotion x8"] = events(batch)
                ctx.synchronize()
                assert bytes(heads.cpu().numpy()) == dev[2] * PAIRS
                a8, b8, a32, b32 = new((H, W), torch.uint8), new((H, W), torch.uint8), new((H, W), torch.int32), new((H, W), torch.int32)

                def copy():
                    b8.copy_(a8)
                    b32.copy_(a32)
                with torch.cuda.stream(s):
                    res["copy"] = events(copy)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "regions_time.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return run_child(args.reps)
    sessions = []
    for k in range(args.sessions):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)], capture_output=True, text=True, timeout=280)
        lines = [t for t in r.stdout.splitlines() if t.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("session %d failed (status %d); nothing more is started" % (k + 1, r.returncode))
        sessions.append(json.loads(lines[-1][7:]))
    first = sessions[0]
    text = ["the moving regions of a pair (hsflow_regions_device, _batch_device), %dx%d, labels + %d records + header: ms per CALL; medians of %d sessions,"
            % (W, H, CAPACITY, args.sessions),
            "each %d calls back to back between device events (host: a host clock around one round of read-back and hsflow_regions_host; its outputs equal the"
            % args.reps,
            "device's byte for byte).  regions kept: " + ", ".join("%s %d" % (m, first["regions " + m]) for m, _ in MASKS)]
    med = {}
    for row in ROWS:
        vals = [s[row] for s in sessions]
        med[row] = median(vals)
        text.append("  %-16s %9.4f   (sessions: %s)" % (row, med[row], ", ".join("%.4f" % t for t in vals)))
    text.append("  gmotion / copy %.1f; full / gmotion %.2f; random59 / gmotion %.2f; gmotion x8 per pair / gmotion %.2f; host gmotion / gmotion %.0f"
                % (med["gmotion"] / med["copy"], med["full"] / med["gmotion"], med["random59"] / med["gmotion"], med["gmotion x8"] / PAIRS / med["gmotion"],
                   med["host gmotion"] / med["gmotion"]))
    text = "\n".join(text) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
