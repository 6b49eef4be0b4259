#!/usr/bin/env python3
"""What warping a picture by the flow on the device (hsflow_warp*) costs.  Two sizes, 1920x1080 (the
seed-1 translating pair, 100 sweeps) and 600x480 (the reference's city pair as its CPU route solves it); the picture is
the second frame as a BGR picture (the gray frame, tinted), the reference the first.  Two flows each: the solver's own
(a pixel or so) and one written by the caller, uniform in +-8 pixels, whose taps scatter.  Per picture:
  device       hsflow_warp_device with picture and statistics, device events around --reps calls back to back;
  picture      the same without statistics (no reference is read);
  stats        the same without a picture (d_dst == NULL);
  own          the context's own gray frames (d_src == NULL), picture and statistics;
  copy         a device-to-device copy of the bytes `device` moves at least: 8 of flow, 3 of source, 3 of reference read and
               3 written per pixel, 17 in all;
  host         both flow planes read back + hsflow_warp_host of the same picture, a host clock around --host-reps calls.
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported, and after
a session that failed nothing more is started.
   usage: tools/warp_time.py [--reps 200] [--sessions 3] [--out profiles/warp_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = ("1080p", "600x480")
FLOWS = ("solver", "pm8")
ROWS = ("device", "picture", "stats", "own", "copy", "host")


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
    tint = np.array([0.6, 0.8, 1.0])
    for case in CASES:
        A, B, blur, kw = the_case(hs, case)
        H, W = A.shape
        bgr = [np.clip(np.rint(g[..., None] * tint), 0, 255).astype(np.uint8) for g in (A, B)]
        s = torch.cuda.Stream()
        with hs.HSFlow(W, H, stream=s.cuda_stream) as ctx:
            if blur:
                ctx.set_frames_gray_blur(A, B)
            else:
                ctx.set_frames(A, B)
            ctx.solve(**kw)
            dref, dsrc = (torch.from_numpy(f).cuda() for f in bgr)
            dst = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            gray = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
            stats = torch.zeros(64, dtype=torch.uint8, device="cuda")
            a, b = (torch.zeros(17 * W * H, dtype=torch.uint8, device="cuda") for _ in range(2))
            wp3, wp1 = hs.make_warp_params(3), hs.make_warp_params(1)
            r3, r1 = ctypes.byref(wp3), ctypes.byref(wp1)
            ps, pr, pd, pg, pst = (ctypes.c_void_p(t.data_ptr()) for t in (dsrc, dref, dst, gray, stats))
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
                if flow == "pm8":
                    ud, vd = (torch.from_numpy(rng.uniform(-8.0, 8.0, (H, W)).astype(np.float32)).cuda() for _ in range(2))
                    torch.cuda.synchronize()
                    ctx.set_flow_rows_from(ud, vd, 0, H)
                    ctx.synchronize()
                u, v = ctx.flow()
                res = {}
                res["device"] = events(lambda: L.hsflow_warp_device(ctx._h, 0, r3, ps, 3 * W, pr, 3 * W, pd, 3 * W, pst))
                ctx.synchronize()
                want, ws = hs.warp_host(u, v, bgr[1], ref=bgr[0], return_stats=True)
                got = hs.warp_stats_from(stats)
                assert np.array_equal(dst.cpu().numpy(), want) and bytes(got) == bytes(ws), (case, flow)
                res["picture"] = events(lambda: L.hsflow_warp_device(ctx._h, 0, r3, ps, 3 * W, None, 0, pd, 3 * W, None))
                res["stats"] = events(lambda: L.hsflow_warp_device(ctx._h, 0, r3, ps, 3 * W, pr, 3 * W, None, 0, pst))
                res["own"] = events(lambda: L.hsflow_warp_device(ctx._h, 0, r1, None, 0, None, 0, pg, W, pst))
                with torch.cuda.stream(s):
                    res["copy"] = events(lambda: b.copy_(a))
                t0 = time.perf_counter()
                for _ in range(host_reps):
                    uu, vv = ctx.flow()
                    hs.warp_host(uu, vv, bgr[1], ref=bgr[0], return_stats=True)
                res["host"] = (time.perf_counter() - t0) * 1e3 / host_reps
                res["sad_warped"], res["sad_plain"], res["inside"] = int(ws.sad_warped), int(ws.sad_plain), int(ws.inside)
                out[case + " " + flow] = dict(res, width=W, height=H)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_time.txt"))
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
    text = ["warp by the flow (hsflow_warp*): ms per picture; medians of %d sessions, each %d calls back to back between device events"
            % (args.sessions, args.reps),
            "(host: a host clock around %d calls of flow read-back + hsflow_warp_host)" % args.host_reps]
    for case in CASES:
        for flow in FLOWS:
            first = sessions[0][case + " " + flow]
            W, H = first["width"], first["height"]
            text.append("%s, %dx%d BGR, %s flow  (flow %.1f MB, picture %.1f MB; inside %d, sad_warped %d, sad_plain %d)"
                        % (case, W, H, flow, 8e-6 * W * H, 3e-6 * W * H, first["inside"], first["sad_warped"], first["sad_plain"]))
            for row in ROWS:
                vals = [s[case + " " + flow][row] for s in sessions]
                text.append("  %-10s %9.4f   (sessions: %s)" % (row, median(vals), ", ".join("%.4f" % t for t in vals)))
            dev = median([s[case + " " + flow]["device"] for s in sessions])
            copy = median([s[case + " " + flow]["copy"] for s in sessions])
            text.append("  device moves at least 17 B per pixel: %.0f GB/s; the copy moves 17 B per pixel each way: %.0f GB/s read + written"
                        % (17 * W * H / dev * 1e-6, 2 * 17 * W * H / copy * 1e-6))
    text = "\n".join(text) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
