#!/usr/bin/env python3
"""What the flow picture's JPEG file costs, encoded on the device against on the host.  Per case and preset:
  A  the route without the device encoder: hsflow_render_flow into page-locked memory + the host rule's encode
     (hsflow_jpeg_encode_host), host clocks;
  B  hsflow_render_flow_jpeg into page-locked memory, a host clock around the synchronous call;
  C  the encode's launches alone (hsflow_jpeg_encode_device of the rendered picture) between device events, next to the
     render's two launches and the pair's solve;
  the file's size and the bytes that crossed PCIe in A and in B.
Medians of --reps timed repetitions after warm-up; A and B alternate within one process and must give identical bytes
(checked, and C's file too).  Every case runs in a child process of its own under a time limit; after a case that failed
nothing more is started.
   usage: tools/jpeg_time.py [--reps 30] [--out profiles/jpeg_time.txt] [--label TEXT]"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CASES = ("1080p", "city")
QUALITY = 95


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
    bound = hs.jpeg_bound(W, H)
    s = torch.cuda.Stream()
    pic = hs.pinned_empty((H, W, 3), np.uint8)
    file_a, file_b = hs.pinned_empty((bound,), np.uint8), hs.pinned_empty((bound,), np.uint8)
    dev_pic = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    dev_file = torch.zeros(bound, dtype=torch.uint8, device="cuda")
    dev_size = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    p = hs.make_params(**kw)
    na, nb = ctypes.c_size_t(), ctypes.c_size_t()
    with hs.HSFlow(W, H, 1, stream=s.cuda_stream) as ctx:
        if blur:
            ctx.set_frames_gray_blur(A, B)
        else:
            ctx.set_frames(A, B)
        ctx.solve(p)
        print("%s  (picture %.1f MB, quality %d)" % (what, W * H * 3 / 1e6, QUALITY), flush=True)
        for route in ("cv", "cl"):
            rp = hs.make_render_params(route)

            def way_a():
                assert L.hsflow_render_flow(ctx._h, 0, ctypes.byref(rp), pic.ctypes.data, W * 3) == 0
                t1 = time.perf_counter()
                assert L.hsflow_jpeg_encode_host(pic.ctypes.data, W * 3, W, H, QUALITY, file_a.ctypes.data, bound, ctypes.byref(na)) == 0
                return t1

            def way_b():
                assert L.hsflow_render_flow_jpeg(ctx._h, 0, ctypes.byref(rp), QUALITY, file_b.ctypes.data, bound, ctypes.byref(nb)) == 0

            for _ in range(3):
                way_a()
                way_b()
            ta, ta_render, tb = [], [], []
            for _ in range(reps):   # alternating, so that both see the same machine
                t0 = time.perf_counter()
                t1 = way_a()
                t2 = time.perf_counter()
                way_b()
                t3 = time.perf_counter()
                ta.append((t2 - t0) * 1e3)
                ta_render.append((t1 - t0) * 1e3)
                tb.append((t3 - t2) * 1e3)
            same = na.value == nb.value and bool(np.array_equal(file_a[:na.value], file_b[:nb.value]))
            # C: the launches alone
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            assert L.hsflow_render_flow_device(ctx._h, 0, ctypes.byref(rp), dev_pic.data_ptr(), W * 3) == 0
            tc, tr = [], []
            for i in range(reps + 5):
                e0.record(s)
                assert L.hsflow_jpeg_encode_device(ctx._h, dev_pic.data_ptr(), W * 3, QUALITY, dev_file.data_ptr(), bound, dev_size.data_ptr()) == 0
                e1.record(s)
                e1.synchronize()
                if i >= 5:
                    tc.append(e0.elapsed_time(e1))
            for i in range(reps + 5):
                e0.record(s)
                assert L.hsflow_render_flow_device(ctx._h, 0, ctypes.byref(rp), dev_pic.data_ptr(), W * 3) == 0
                e1.record(s)
                e1.synchronize()
                if i >= 5:
                    tr.append(e0.elapsed_time(e1))
            e0.record(s)
            for _ in range(20):
                L.hsflow_jpeg_encode_device(ctx._h, dev_pic.data_ptr(), W * 3, QUALITY, dev_file.data_ptr(), bound, dev_size.data_ptr())
            e1.record(s)
            e1.synchronize()
            tc20 = e0.elapsed_time(e1) / 20
            nc = int(dev_size.item())
            same = same and nc == nb.value and bool(np.array_equal(dev_file[:nc].cpu().numpy(), file_b[:nb.value]))
            print("  %s preset, file %d bytes, A = B = C files: %s" % (route, nb.value, same), flush=True)
            print("    A  render_flow + host encode    %.4f ms  (render and copy %.4f + encode %.4f); %d bytes over PCIe" %
                  (median(ta), median(ta_render), median(ta) - median(ta_render), W * H * 3), flush=True)
            print("    B  hsflow_render_flow_jpeg      %.4f ms  (B / A = %.4f); %d bytes over PCIe" % (median(tb), median(tb) / median(ta), 8 + nb.value), flush=True)
            print("    C  the encode's launches        %.4f ms alone, %.4f ms each in 20 back to back; the render's two launches %.4f ms" %
                  (median(tc), tc20, median(tr)), flush=True)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_time.txt"))
    ap.add_argument("--label", default="")
    ap.add_argument("--case", choices=CASES)
    ap.add_argument("--limit", type=int, default=240, help="seconds per case")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.case:
        run_case(args.case, args.reps)
        return 0
    lines = ["flow picture as a JPEG file: host encode against hsflow_render_flow_jpeg; medians of %d repetitions  %s" % (args.reps, args.label)]
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
