#!/usr/bin/env python3
"""What finding the points to follow (hsflow_corners_device / _batch_device / _planes_device) costs beside a
traffic floor and the route it replaces.  Per CALL, device events around --reps calls back to back after 10 warm-up calls,
the C entries called with arguments prepared once; records, xy and the header are asked for, capacity 1024, the default
parameters unless a row says otherwise:
  1080p         the prev frame of the benchmark's pair (the translating texture of seed 1) as the context holds it, 1920x1080;
  1080p x8      8 pairs of that frame by one hsflow_corners_batch_device (ms per CALL, not per pair);
  600x480       the same texture at 600 x 480;
  noise cap     a 1920x1080 frame of uniform noise, nms_r 1, quality 0: more survivors than the cap of 65536 candidates --
                what the exact ranking costs at its worst;
  floor ...     (a) the traffic floor of the size: a device-to-device copy of the gray plane plus one write (a fill) and one
                read (a maximum) of an int64 score plane, three launches;
  host ...      (b) the route the operator replaces: the frame read back, hsflow_corners_host, xy uploaded; a host clock
                around one round (taken once per session), and its records, xy and header equal the device's byte for byte.
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported with every
session's figure beside them (the spread), and after a session that failed nothing more is started.
   usage: tools/corners_time.py [--reps 30] [--sessions 3] [--out profiles/corners_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
PAIRS, CAPACITY = 8, 1024
ROWS = ["1080p", "1080p x8", "600x480", "noise cap", "floor 1080p", "floor 600x480", "host 1080p", "host 600x480", "host noise cap"]


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
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")

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

    res = {}
    recs, xys, heads = new((PAIRS, CAPACITY * 16), torch.uint8), new((PAIRS, CAPACITY, 2), torch.float32), new((PAIRS * 64,), torch.uint8)

    def against_host(name, gray, prm, ctx):
        """The host route, clocked once, and its outputs against what the device left in recs[0], xys[0], heads."""
        ctx.synchronize()
        head = hs.corners_result_from(heads)
        dev = (bytes(recs[0].cpu().numpy())[:head.n_written * 16], xys[0].cpu().numpy().tobytes(), bytes(head))
        t0 = time.perf_counter()
        hg = gray.cpu().numpy()
        hres, hrec, hxy = hs.corners_host(hg, capacity=CAPACITY, records=True, xy=True, params=prm)
        up = torch.from_numpy(hxy).cuda()
        torch.cuda.synchronize()
        res["host " + name] = (time.perf_counter() - t0) * 1e3
        assert (bytes(hrec)[:hres.n_written * 16], hxy.tobytes(), bytes(hres)) == dev, name
        res["survivors " + name] = int(head.n_survivors)
        res["candidates " + name] = int(head.n_candidates)
        del up

    def floor(name, W, H):
        a8, b8, a64 = new((H, W), torch.uint8), new((H, W), torch.uint8), new((H, W), torch.int64)

        def traffic():
            b8.copy_(a8)
            a64.fill_(1)          # one write of the score plane
            torch.max(a64)        # one read of it
        with torch.cuda.stream(s):
            res["floor " + name] = events(traffic)

    for name, W, H in (("1080p", 1920, 1080), ("600x480", 600, 480)):
        A, B = synth.translating_pair(W, H, seed=1)
        n = PAIRS if name == "1080p" else 1
        prm = hs.make_corners_params()
        with hs.HSFlow(W, H, n, stream=s.cuda_stream) as ctx:
            for k in range(n):
                ctx.set_frames(np.ascontiguousarray(A, np.uint8), np.ascontiguousarray(B, np.uint8), pair=k)
            ctx.synchronize()
            gray = torch.from_numpy(ctx.frames(0)[0]).cuda()
            torch.cuda.synchronize()

            def one_pair():
                assert L.hsflow_corners_device(ctx._h, 0, 0, None, 0, ctypes.byref(prm), P(recs[0]), CAPACITY, P(xys[0]), P(heads)) == 0
            res[name] = events(one_pair)
            against_host(name, gray, prm, ctx)
            if n > 1:
                rl = (ctypes.c_void_p * n)(*[recs[k].data_ptr() for k in range(n)])
                xl = (ctypes.c_void_p * n)(*[xys[k].data_ptr() for k in range(n)])

                def batch():
                    assert L.hsflow_corners_batch_device(ctx._h, 0, n, 0, None, 0, ctypes.byref(prm), rl, CAPACITY, xl, P(heads)) == 0
                res[name + " x8"] = events(batch)
                ctx.synchronize()
                raw = bytes(heads.cpu().numpy())
                assert raw == raw[:64] * n
                # the worst case of the ranking: noise, every local maximum a candidate
                W2, H2 = W, H
                noise = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (H2, W2), dtype=np.uint8)).cuda()
                torch.cuda.synchronize()
                worst = hs.make_corners_params(nms_r=1, quality_q16=0)

                def cap():
                    assert L.hsflow_corners_planes_device(ctx._h, P(noise), W2, None, 0, ctypes.byref(worst), P(recs[0]), CAPACITY, P(xys[0]), P(heads)) == 0
                res["noise cap"] = events(cap)
                against_host("noise cap", noise, worst, ctx)
        floor(name, W, H)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corners_time.txt"))
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
    text = ["the points to follow (hsflow_corners_device, _batch_device, _planes_device), records + xy + header at capacity %d: ms per CALL; medians of %d"
            % (CAPACITY, args.sessions),
            "sessions, each %d calls back to back between device events after 10 warm-up calls (host: a host clock around ONE round of read-back,"
            % args.reps,
            "hsflow_corners_host and upload per session, taken once; its outputs equal the device's byte for byte).  survivors / candidates: "
            + ", ".join("%s %d / %d" % (m, first["survivors " + m], first["candidates " + m]) for m in ("1080p", "600x480", "noise cap"))]
    med = {}
    for row in ROWS:
        vals = [s[row] for s in sessions]
        med[row] = median(vals)
        text.append("  %-16s %9.4f   (sessions: %s)" % (row, med[row], ", ".join("%.4f" % t for t in vals)))
    text.append("  1080p / floor %.1f; 600x480 / floor %.1f; 1080p x8 per pair / 1080p %.2f; noise cap / 1080p %.1f; host 1080p / 1080p %.0f; host noise cap / noise cap %.0f"
                % (med["1080p"] / med["floor 1080p"], med["600x480"] / med["floor 600x480"], med["1080p x8"] / PAIRS / med["1080p"], med["noise cap"] / med["1080p"],
                   med["host 1080p"] / med["1080p"], med["host noise cap"] / med["noise cap"]))
    text = "\n".join(text) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
