#!/usr/bin/env python3
"""What the dense colour picture (hsflow_color_flow*) costs on the device.  Two cases, those of
tools/jpeg_time.py: the 1920x1080 seed-1 pair after 100 sweeps and the reference's 600x480 city pair as its CPU route
solves it.  For the scale taken from the picture (AUTO) and a fixed one (FIXED, a third of AUTO's):
  device   hsflow_color_flow_device, device events around --reps calls back to back, per picture;
  batch8   hsflow_color_flow_batch_device of 8 pairs, the same way, per picture;
  jpeg     hsflow_color_flow_jpeg (synchronous, quality 95), a host clock around --reps calls, per file, and the file's size;
beside them, the same way as `device`:
  arrows   hsflow_render_flow_device of the same pair (cv preset);
  copy     a device-to-device copy of 19 bytes per pixel (8 read and 3 written per pixel, 8 more for the AUTO pass): the floor.
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported, and after
a session that failed nothing more is started.
   usage: tools/color_time.py [--reps 200] [--sessions 3] [--out profiles/color_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = ("1080p", "city")
ROWS = ("device AUTO", "device FIXED", "batch8 AUTO", "batch8 FIXED", "jpeg AUTO", "jpeg FIXED", "arrows", "copy")


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n & 1 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def read_pgm(path):
    import numpy as np
    with open(path, "rb") as f:
        assert f.readline().strip() == b"P5"
        w, h = [int(t) for t in f.readline().split()]
        assert int(f.readline()) == 255
        return np.frombuffer(f.read(w * h), dtype=np.uint8).reshape(h, w).copy()


def the_case(hs, case):
    import numpy as np
    from opticalflowhs_amd import synth
    if case == "1080p":
        A, B = synth.translating_pair(1920, 1080, seed=1)
        return A, B, False, dict(lam=1.0, max_iter=100, term_type=hs.TERM_ITER)
    g = os.path.join(ROOT, "tests", "golden")
    A, B = read_pgm(os.path.join(g, "city_1_gray.pgm")), read_pgm(os.path.join(g, "city_2_gray.pgm"))
    return A, B, True, dict(lam=0.1, max_iter=10, term_type=hs.TERM_ITER | hs.TERM_EPS, epsilon=float(np.float32(1e-6)))


def run_child(reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opticalflowhs_amd as hs
    L = hs._lib.load()
    N = 8
    out = {}
    for case in CASES:
        A, B, blur, kw = the_case(hs, case)
        H, W = A.shape
        s = torch.cuda.Stream()
        with hs.HSFlow(W, H, N, stream=s.cuda_stream) as ctx:
            for p in range(N):
                if blur:
                    ctx.set_frames_gray_blur(A, B, pair=p)
                else:
                    ctx.set_frames(A, B, pair=p)
            ctx.solve(**kw)
            u, v = ctx.flow()
            want, m = hs.color_flow_host(u, v, return_scale=True)
            pics = torch.zeros((N, H, W, 3), dtype=torch.uint8, device="cuda")
            ptrs = (ctypes.c_void_p * N)(*[pics[i].data_ptr() for i in range(N)])
            src, dst = (torch.zeros(19 * W * H, dtype=torch.uint8, device="cuda") for _ in range(2))
            rp = hs.make_render_params("cv")
            torch.cuda.synchronize()

            def events(fn):
                for _ in range(10):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(reps):
                    fn()
                e1.record(s)
                e1.synchronize()
                return e0.elapsed_time(e1) / reps

            res = {}
            for name, mf in (("AUTO", None), ("FIXED", m / 3)):
                cp = hs.make_color_params(mf)
                ref = ctypes.byref(cp)
                res["device " + name] = events(lambda: L.hsflow_color_flow_device(ctx._h, 0, ref, ptrs[0], 3 * W))
                res["batch8 " + name] = events(lambda: L.hsflow_color_flow_batch_device(ctx._h, 0, N, ref, ptrs, 3 * W)) / N
                ctx.synchronize()
                assert np.array_equal(pics[N - 1].cpu().numpy(), hs.color_flow_host(u, v, max_flow=mf)), (case, name)
                size = len(ctx.color_jpeg(max_flow=mf))
                t0 = time.perf_counter()
                for _ in range(reps):
                    ctx.color_jpeg(max_flow=mf)
                res["jpeg " + name] = (time.perf_counter() - t0) * 1e3 / reps
                res["bytes " + name] = size
            res["arrows"] = events(lambda: L.hsflow_render_flow_device(ctx._h, 0, ctypes.byref(rp), ptrs[0], 3 * W))
            with torch.cuda.stream(s):
                res["copy"] = events(lambda: dst.copy_(src))
            out[case] = dict(res, width=W, height=H)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "color_time.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return run_child(args.reps)
    sessions = []
    for k in range(args.sessions):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)], capture_output=True, text=True, timeout=240)
        lines = [t for t in r.stdout.splitlines() if t.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("session %d failed (status %d); nothing more is started" % (k + 1, r.returncode))
        sessions.append(json.loads(lines[-1][7:]))
    text = ["colour picture (hsflow_color_flow*): ms per picture or file; medians of %d sessions, each %d calls back to back between device events"
            % (args.sessions, args.reps), "(jpeg: a host clock around the synchronous call)"]
    for case in CASES:
        first = sessions[0][case]
        W, H = first["width"], first["height"]
        text.append("%s, %dx%d  (flow %.1f MB, picture %.1f MB; files: AUTO %d bytes, FIXED %d bytes)"
                    % (case, W, H, 8e-6 * W * H, 3e-6 * W * H, first["bytes AUTO"], first["bytes FIXED"]))
        for row in ROWS:
            vals = [s[case][row] for s in sessions]
            text.append("  %-14s %8.4f   (sessions: %s)" % (row, median(vals), ", ".join("%.4f" % t for t in vals)))
        copy = median([s[case]["copy"] for s in sessions])
        for name in ("AUTO", "FIXED"):
            t = median([s[case]["device " + name] for s in sessions])
            px = (19 if name == "AUTO" else 11) * W * H
            text.append("  device %-5s moves %2d B per pixel: %.0f GB/s; the copy moves 19 B per pixel each way: %.0f GB/s read + written"
                        % (name, 19 if name == "AUTO" else 11, px / t * 1e-6, 2 * 19 * W * H / copy * 1e-6))
    text = "\n".join(text) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
