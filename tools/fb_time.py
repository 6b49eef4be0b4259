#!/usr/bin/env python3
"""What the forward-backward check of two flows on the device (hsflow_fb*) costs.  Two sizes, 1920x1080
(the seed-1 translating pair, 100 sweeps) and 600x480 (the reference's city pair as its CPU route solves it), each a
context of two pairs, the second made by hsflow_set_frames_reversed.  Two flows each: the solver's own (a pixel or so) and
Gaussian flows of sigma 8 pixels written by the caller, whose taps scatter.  Per check of pair 0 against pair 1:
  mask         hsflow_fb_device with the mask alone, device events around --reps calls back to back;
  full         mask + err2 + statistics;
  stats        statistics alone;
  copy         a device-to-device copy of the bytes per pixel `full` moves: 8 of forward flow and 24 of backward taps read
               (three new taps per plane and pixel where neighbours share one), 1 of mask and 4 of err2 written, 37 in all; the
               copy reads 37 and writes 37, so it moves 74 bytes per pixel, twice what `full` moves;
  host         four flow planes read back + hsflow_fb_host of the same, a host clock around --host-reps calls.
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported, and after
a session that failed nothing more is started.
   usage: tools/fb_time.py [--reps 200] [--sessions 3] [--out profiles/fb_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = ("1080p", "600x480")
FLOWS = ("solver", "sigma8")
ROWS = ("mask", "full", "stats", "copy", "host")
MOVED = 37


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


def run_child(reps, host_reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opticalflowhs_amd as hs
    L = hs._lib.load()
    out = {}
    for case in CASES:
        A, B, blur, kw = the_case(hs, case)
        H, W = A.shape
        s = torch.cuda.Stream()
        with hs.HSFlow(W, H, 2, stream=s.cuda_stream) as ctx:
            if blur:
                ctx.set_frames_gray_blur(A, B)
            else:
                ctx.set_frames(A, B)
            ctx.set_frames_reversed(1, 0)
            ctx.solve(**kw)
            mask = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
            err2 = torch.zeros((H, W), dtype=torch.float32, device="cuda")
            stats = torch.zeros(64, dtype=torch.uint8, device="cuda")
            a, b = (torch.zeros(MOVED * W * H, dtype=torch.uint8, device="cuda") for _ in range(2))
            fp = hs.make_fb_params()
            r = ctypes.byref(fp)
            pm, pe, pst = (ctypes.c_void_p(t.data_ptr()) for t in (mask, err2, stats))
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

            rng = np.random.default_rng(8)
            for flow in FLOWS:
                if flow == "sigma8":
                    for pair in range(2):
                        ud, vd = (torch.from_numpy((rng.standard_normal((H, W)) * 8.0).astype(np.float32)).cuda() for _ in range(2))
                        torch.cuda.synchronize()
                        ctx.set_flow_rows_from(ud, vd, 0, H, pair=pair)
                    ctx.synchronize()
                (uf, vf), (ub, vb) = ctx.flow(0), ctx.flow(1)
                res = {}
                res["full"] = events(lambda: L.hsflow_fb_device(ctx._h, 0, 1, r, pm, W, pe, 4 * W, pst))
                ctx.synchronize()
                wm, we, ws = hs.fb_host(uf, vf, ub, vb, mask=True, err2=True, stats=True)
                got = hs.fb_stats_from(stats)
                assert np.array_equal(mask.cpu().numpy(), wm) and np.array_equal(err2.cpu().numpy().view(np.uint32), we.view(np.uint32)), (case, flow)
                assert bytes(got) == bytes(ws), (case, flow)
                res["mask"] = events(lambda: L.hsflow_fb_device(ctx._h, 0, 1, r, pm, W, None, 0, None))
                res["stats"] = events(lambda: L.hsflow_fb_device(ctx._h, 0, 1, r, None, 0, None, 0, pst))
                with torch.cuda.stream(s):
                    res["copy"] = events(lambda: b.copy_(a))
                t0 = time.perf_counter()
                for _ in range(host_reps):
                    (u0, v0), (u1, v1) = ctx.flow(0), ctx.flow(1)
                    hs.fb_host(u0, v0, u1, v1, mask=True, err2=True, stats=True)
                res["host"] = (time.perf_counter() - t0) * 1e3 / host_reps
                for k in ("consistent", "inconsistent", "outside", "unknown"):
                    res[k] = int(getattr(ws, k))
                out[case + " " + flow] = dict(res, width=W, height=H)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fb_time.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return run_child(args.reps, args.host_reps)
    sessions = []
    for k in range(args.sessions):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--host-reps", str(args.host_reps)],
                           capture_output=True, text=True, timeout=240)
        lines = [t for t in r.stdout.splitlines() if t.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("session %d failed (status %d); nothing more is started" % (k + 1, r.returncode))
        sessions.append(json.loads(lines[-1][7:]))
    text = ["forward-backward check (hsflow_fb*): ms per check; medians of %d sessions, each %d calls back to back between device events"
            % (args.sessions, args.reps),
            "(host: a host clock around %d calls of four-plane read-back + hsflow_fb_host)" % args.host_reps]
    for case in CASES:
        for flow in FLOWS:
            first = sessions[0][case + " " + flow]
            W, H = first["width"], first["height"]
            text.append("%s, %dx%d, %s flows  (four planes %.1f MB; consistent %d, inconsistent %d, outside %d, unknown %d)"
                        % (case, W, H, flow, 16e-6 * W * H, first["consistent"], first["inconsistent"], first["outside"], first["unknown"]))
            for row in ROWS:
                vals = [s[case + " " + flow][row] for s in sessions]
                text.append("  %-10s %9.4f   (sessions: %s)" % (row, median(vals), ", ".join("%.4f" % t for t in vals)))
            full = median([s[case + " " + flow]["full"] for s in sessions])
            copy = median([s[case + " " + flow]["copy"] for s in sessions])
            host = median([s[case + " " + flow]["host"] for s in sessions])
            text.append("  full moves %d B per pixel: %.0f GB/s; the copy moves %d B per pixel each way: %.0f GB/s read + written; full / copy %.2f, host / full %.0f"
                        % (MOVED, MOVED * W * H / full * 1e-6, MOVED, 2 * MOVED * W * H / copy * 1e-6, full / copy, host / full))
    text = "\n".join(text) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
