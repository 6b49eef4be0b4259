#!/usr/bin/env python3
"""What "are these two flow fields the same" costs, on the device against through a download.  Per size:
  A  the old way: hsflow_get_flow of both planes into page-locked memory + np.array_equal on u and on v;
  B  hsflow_compare_flow_device against two planes in device memory (memset of the records, two launches of
     k_plane_compare, one copy of 80 bytes, a wait for the event behind it);
  C  the device's time for B's work, by events on the context's stream around the call -- two launches, the memset and
     the small copy, so an upper bound for the two kernels -- and from it the bytes per second over the 16 bytes per pixel
     the kernels read.
A and B alternate, medians of --reps repetitions after warm-up; both answer "equal" (checked).  Then a whole hsflow_verify
beside the solve it checks (host clock around the call; events around hsflow_solve_async).
Every case runs in a child process of its own under a time limit; after a case that failed nothing more is started.
   usage: tools/verify_time.py [--reps 30] [--out profiles/verify_time.txt] [--label TEXT]"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CASES = {"1080p": (1920, 1080), "4k": (3840, 2160)}


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n & 1 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def run_case(case, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opticalflowhs_amd as hs
    from opticalflowhs_amd import synth
    L = hs._lib.load()
    W, H = CASES[case]
    A, B = synth.translating_pair(W, H, seed=1)   # the benchmark's seed-1 texture
    s = torch.cuda.Stream()
    u, v = hs.pinned_empty((H, W), np.float32), hs.pinned_empty((H, W), np.float32)
    p = hs.make_params(lam=1.0, max_iter=100, term_type=hs.TERM_ITER)
    with hs.HSFlow(W, H, 1, stream=s.cuda_stream) as ctx:
        ctx.set_frames(A, B)
        ctx.solve(p)
        ub, vb = ctx.flow()                       # side b on the host ...
        du, dv = torch.from_numpy(ub).cuda(), torch.from_numpy(vb).cuda()   # ... and on the device (dense, 16-byte aligned)
        torch.cuda.synchronize()
        print("%dx%d, 100 sweeps  (flow %.1f MB)" % (W, H, 2 * W * H * 4 / 1e6), flush=True)
        ru, rv = hs._lib.HsflowPlaneDiff(), hs._lib.HsflowPlaneDiff()

        def way_a():
            assert L.hsflow_get_flow(ctx._h, 0, u.ctypes.data, W * 4, v.ctypes.data, W * 4) == 0
            t1 = time.perf_counter()
            return t1, np.array_equal(u, ub) and np.array_equal(v, vb)

        def way_b():
            assert L.hsflow_compare_flow_device(ctx._h, 0, du.data_ptr(), W * 4, dv.data_ptr(), W * 4, ctypes.byref(ru), ctypes.byref(rv)) == 0
            return ru.differing == 0 and rv.differing == 0

        for _ in range(5):
            way_a()
            way_b()
        ta, ta_copy, tb = [], [], []
        same = True
        for _ in range(reps):   # alternating, so that both see the same machine
            t0 = time.perf_counter()
            t1, ok_a = way_a()
            t2 = time.perf_counter()
            ok_b = way_b()
            t3 = time.perf_counter()
            same = same and ok_a and ok_b
            ta.append((t2 - t0) * 1e3)
            ta_copy.append((t1 - t0) * 1e3)
            tb.append((t3 - t2) * 1e3)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        tc = []
        for i in range(reps + 5):
            e0.record(s)
            way_b()
            e1.record(s)
            e1.synchronize()
            if i >= 5:
                tc.append(e0.elapsed_time(e1))
        c = median(tc)
        print("    A  get_flow + np.array_equal     %.4f ms  (copy %.4f + comparison %.4f)" % (median(ta), median(ta_copy), median(ta) - median(ta_copy)), flush=True)
        print("    B  hsflow_compare_flow_device    %.4f ms  (B / A = %.3f)" % (median(tb), median(tb) / median(ta)), flush=True)
        print("    C  device time of B              %.4f ms  = %.2f TB/s over %.1f MB read" % (c, 16.0 * W * H / (c * 1e-3) / 1e12, 16.0 * W * H / 1e6), flush=True)
        print("    A and B both say equal: %s" % same, flush=True)
        assert same
        if case == "1080p":   # a whole verify beside the solve it checks
            r = ctx.verify()
            assert r.ok == 1 and r.u.differing == 0 and r.v.differing == 0
            tv, ts = [], []
            for i in range(reps // 2 + 3):
                t0 = time.perf_counter()
                r = ctx.verify()
                t1 = time.perf_counter()
                if i >= 3:
                    tv.append((t1 - t0) * 1e3)
            for i in range(reps + 5):
                e0.record(s)
                ctx.solve_async(p)
                e1.record(s)
                e1.synchronize()
                ctx.synchronize()
                if i >= 5:
                    ts.append(e0.elapsed_time(e1))
            print("    hsflow_verify (100 one-sweep launches + 3 comparisons)  %.4f ms;  the solve it checks  %.4f ms  (verify / solve = %.1f)" % (
                median(tv), median(ts), median(tv) / median(ts)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_time.txt"))
    ap.add_argument("--label", default="")
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--limit", type=int, default=240, help="seconds per case")
    args = ap.parse_args()
    if args.reps < 30:
        ap.error("--reps must be at least 30")
    if args.case:
        run_case(args.case, args.reps)
        return 0
    lines = ["flow comparison: download + np.array_equal against hsflow_compare_flow_device; medians of %d repetitions  %s" % (args.reps, args.label)]
    rc = 0
    for case in ("1080p", "4k"):   # each case in a process of its own, under its own time limit; nothing is started after a failure
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(args.reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        lines += r.stdout.splitlines()
        if r.returncode != 0:
            lines += ["case %s ended with status %d; nothing further was run" % (case, r.returncode)] + r.stderr.splitlines()[-12:]
            rc = r.returncode
            break
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)
    return rc


if __name__ == "__main__":
    sys.exit(main())
