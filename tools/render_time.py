#!/usr/bin/env python3
"""What the flow picture costs, on the device against on the host (the render section).  Per case:
  A  the host picture the old way: hsflow_get_flow of both planes into page-locked memory + the host drawing
     (pnm.hpp's circle and line behind tools/bin/librender_host_draw.so);
  B  hsflow_render_flow into page-locked memory;
  C  the two render launches alone, bracketed by events on the context's stream, and the same pair's solve beside them.
Medians of --reps timed repetitions after warm-up; A and B are host clocks around calls that return when the bytes are
there, C is device events.  A, B and C draw the same picture (checked).
Every case runs in a child process of its own under a time limit; after a case that failed nothing more is started.
   usage: tools/render_time.py [--reps 30] [--out profiles/render_time.txt] [--label TEXT]"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CASES = ("1080p", "city")


def read_pgm(path):
    import numpy as np
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P5"
        w, h = [int(t) for t in f.readline().split()]
        assert int(f.readline()) == 255
        return np.frombuffer(f.read(w * h), dtype=np.uint8).reshape(h, w).copy()


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
    so = os.path.join(ROOT, "tools", "bin", "librender_host_draw.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "tools"), "-s", "bin/librender_host_draw.so"])
    draw = ctypes.CDLL(so).render_host_draw
    draw.restype = None
    draw.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L = hs._lib.load()
    if case == "1080p":   # the benchmark's seed-1 pair, 100 sweeps
        A, B = synth.translating_pair(1920, 1080, seed=1)
        blur, kw, what = False, dict(lam=1.0, max_iter=100, term_type=hs.TERM_ITER), "1920x1080 seed-1 pair, 100 sweeps"
    else:                 # the reference's city pair as its CPU route solves it (tests/refpics.py)
        g = os.path.join(ROOT, "tests", "golden")
        A, B = read_pgm(os.path.join(g, "city_1_gray.pgm")), read_pgm(os.path.join(g, "city_2_gray.pgm"))
        blur, kw = True, dict(lam=0.1, max_iter=10, term_type=hs.TERM_ITER | hs.TERM_EPS, epsilon=float(np.float32(1e-6)))
        what = "%dx%d city pair, blur, lambda 0.1, 10 sweeps" % (A.shape[1], A.shape[0])
    H, W = A.shape
    s = torch.cuda.Stream()
    u, v = hs.pinned_empty((H, W), np.float32), hs.pinned_empty((H, W), np.float32)
    pic_a, pic_b = hs.pinned_empty((H, W, 3), np.uint8), hs.pinned_empty((H, W, 3), np.uint8)
    dev = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    p = hs.make_params(**kw)
    with hs.HSFlow(W, H, 1, stream=s.cuda_stream) as ctx:
        if blur:
            ctx.set_frames_gray_blur(A, B)
        else:
            ctx.set_frames(A, B)
        ctx.solve(p)
        print("%s  (flow %.1f MB, picture %.1f MB)" % (what, 2 * W * H * 4 / 1e6, W * H * 3 / 1e6), flush=True)
        for route, preset in (("cv", 0), ("cl", 1)):
            rp = hs.make_render_params(route)

            def way_a():
                st = L.hsflow_get_flow(ctx._h, 0, u.ctypes.data, W * 4, v.ctypes.data, W * 4)
                assert st == 0
                t1 = time.perf_counter()
                draw(u.ctypes.data, v.ctypes.data, W, H, preset, pic_a.ctypes.data)
                return t1

            def way_b():
                assert L.hsflow_render_flow(ctx._h, 0, ctypes.byref(rp), pic_b.ctypes.data, W * 3) == 0

            for _ in range(5):
                way_a()
                way_b()
            ta, ta_copy, tb = [], [], []
            for _ in range(reps):   # alternating, so that both see the same machine
                t0 = time.perf_counter()
                t1 = way_a()
                t2 = time.perf_counter()
                way_b()
                t3 = time.perf_counter()
                ta.append((t2 - t0) * 1e3)
                ta_copy.append((t1 - t0) * 1e3)
                tb.append((t3 - t2) * 1e3)
            same = bool(np.array_equal(pic_a, pic_b))
            drawn = int((pic_b != 0).any(axis=2).sum())
            # C: the launches alone
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            tc = []
            for i in range(reps + 5):
                e0.record(s)
                assert L.hsflow_render_flow_device(ctx._h, 0, ctypes.byref(rp), dev.data_ptr(), W * 3) == 0
                e1.record(s)
                e1.synchronize()
                if i >= 5:
                    tc.append(e0.elapsed_time(e1))
            e0.record(s)
            for _ in range(20):
                L.hsflow_render_flow_device(ctx._h, 0, ctypes.byref(rp), dev.data_ptr(), W * 3)
            e1.record(s)
            e1.synchronize()
            tc20 = e0.elapsed_time(e1) / 20
            same = same and bool(np.array_equal(dev.cpu().numpy(), pic_b))
            print("  %s preset, %d pixels drawn, A = B = C pictures: %s" % (route, drawn, same), flush=True)
            print("    A  get_flow + host drawing      %.4f ms  (copy %.4f + drawing %.4f)" % (median(ta), median(ta_copy), median(ta) - median(ta_copy)), flush=True)
            print("    B  hsflow_render_flow           %.4f ms  (B / A = %.2f)" % (median(tb), median(tb) / median(ta)), flush=True)
            print("    C  two render launches          %.4f ms alone, %.4f ms each in 20 back to back" % (median(tc), tc20), flush=True)
            assert same
        ts = []
        for i in range(reps + 5):
            e0.record(s)
            ctx.solve_async(p)
            e1.record(s)
            e1.synchronize()
            ctx.synchronize()
            if i >= 5:
                ts.append(e0.elapsed_time(e1))
        print("    the solve beside it             %.4f ms (events around hsflow_solve_async)" % median(ts), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_time.txt"))
    ap.add_argument("--label", default="")
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--limit", type=int, default=240, help="seconds per case")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.case:
        run_case(args.case, args.reps)
        return 0
    lines = ["flow picture: host drawing against hsflow_render_flow; medians of %d repetitions  %s" % (args.reps, args.label)]
    rc = 0
    for case in CASES:   # each case in a process of its own, under its own time limit; nothing is started after a failure
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
