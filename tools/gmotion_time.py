#!/usr/bin/env python3
"""What the global motion of a flow (hsflow_gmotion_fit_device / _batch_device, hsflow_gmotion_warp_device)
costs beside today's routes.  Two sizes, 1920x1080 and 600x480, on a context of 8 pairs whose flows are a slow similarity
plus a smooth ripple of a third of a pixel, different for every pair, and a block of foreground that moves on its own.
Per CALL, device events around --reps calls back to back, the C entries called with arguments prepared once:
  fit 1         one pair, the record only; FIXED and AUTO, 1 and 3 passes;
  fit 1 +out    the same with the mask and the two residual planes;
  fit 8         the 8 pairs by one hsflow_gmotion_fit_batch_device, records only (ms per CALL, not per pair);
  fit 8 +out    the same with masks and residual planes;
  gwarp bgr     hsflow_gmotion_warp_device of a BGR picture by a fitted model;
  copy          (a) a device-to-device copy of both flow planes of a pair;
  warp bgr      (b) hsflow_warp_device of the same picture by the dense flow;
  host          (c) the flow read back (hsflow_get_flow) and hsflow_gmotion_fit_host, AFFINE, FIXED, 3 passes; a host clock around
                one round, and its record equals the device's bit for bit.
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported, and after
a session that failed nothing more is started.
   usage: tools/gmotion_time.py [--reps 100] [--sessions 3] [--out profiles/gmotion_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = (("1080p", 1920, 1080), ("600x480", 600, 480))
PAIRS = 8
FITS = (("fixed", 1), ("fixed", 3), ("auto", 1), ("auto", 3))
ROWS = ["%s %s %dp" % (what, mode, passes) for what in ("fit 1", "fit 1 +out", "fit 8", "fit 8 +out") for mode, passes in FITS] + ["gwarp bgr", "copy", "warp bgr", "host"]


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n & 1 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def flow_of(W, H, k):
    import numpy as np
    x, y = np.meshgrid(np.arange(W, dtype=np.float64) - (W - 1) / 2.0, np.arange(H, dtype=np.float64) - (H - 1) / 2.0)
    c, s = 1.002 * np.cos(0.003), 1.002 * np.sin(0.003)
    ripple = np.sin(x / 37.0 + k) * np.cos(y / 29.0 - k) / 3.0
    u, v = c * x - s * y - x + 1.5 + ripple, s * x + c * y - y - 0.75 + 0.5 * ripple
    u[H // 4:H // 2, W // 3:W // 2] += 5.0 + k
    v[H // 4:H // 2, W // 3:W // 2] -= 4.0
    return u.astype(np.float32), v.astype(np.float32)


def run_child(reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opticalflowhs_amd as hs
    L = hs._lib.load()
    out = {}
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

    for case, W, H in CASES:
        with hs.HSFlow(W, H, PAIRS, stream=s.cuda_stream) as ctx:
            for k in range(PAIRS):
                u, v = flow_of(W, H, k)
                ud, vd = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
                torch.cuda.synchronize()
                ctx.set_flow_rows_from(ud, vd, 0, H, pair=k)
                ctx.synchronize()
            new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
            masks, rus, rvs = new((PAIRS, H, W), torch.uint8), new((PAIRS, H, W), torch.float32), new((PAIRS, H, W), torch.float32)
            recs = new((64 * PAIRS,), torch.uint8)
            a, b = new((2, H, W), torch.float32), new((2, H, W), torch.float32)
            rng = np.random.default_rng(1)
            pic, dst = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda(), new((H, W, 3), torch.uint8)
            P = lambda t: ctypes.c_void_p(t.data_ptr())
            plist = lambda t: (ctypes.c_void_p * PAIRS)(*[t[k].data_ptr() for k in range(PAIRS)])
            ml, ul, vl = plist(masks), plist(rus), plist(rvs)
            torch.cuda.synchronize()
            res = {}
            for mode, passes in FITS:
                gp = hs.make_gmotion_params("affine", passes, mode)
                tag = "%s %dp" % (mode, passes)

                def one(outs):
                    assert L.hsflow_gmotion_fit_device(ctx._h, 0, None, 0, ctypes.byref(gp), P(masks[0]) if outs else None, W, P(rus[0]) if outs else None,
                                                       P(rvs[0]) if outs else None, 4 * W, P(recs)) == 0

                def batch(outs):
                    assert L.hsflow_gmotion_fit_batch_device(ctx._h, 0, PAIRS, None, 0, ctypes.byref(gp), ml if outs else None, W, ul if outs else None,
                                                             vl if outs else None, 4 * W, P(recs)) == 0
                res["fit 1 " + tag] = events(lambda: one(False))
                res["fit 1 +out " + tag] = events(lambda: one(True))
                res["fit 8 " + tag] = events(lambda: batch(False))
                res["fit 8 +out " + tag] = events(lambda: batch(True))
            gp = hs.make_gmotion_params("affine", 3, "fixed")
            batch(True)
            ctx.synchronize()
            dev = hs.gmotion_result_from(recs, PAIRS)
            masks_dev = masks.cpu().numpy()
            t0 = time.perf_counter()
            hu, hv = ctx.flow(0)
            hrec, hmask, _, _ = hs.global_motion_host(hu, hv, mask=True, params=gp)
            res["host"] = (time.perf_counter() - t0) * 1e3
            assert bytes(hrec) == bytes(dev[0]) and np.array_equal(hmask, masks_dev[0]), case
            res["inliers"] = int(dev[0].cls[0]) / float(W * H)
            res["model"] = [float(x) for x in dev[0].p]
            model = (ctypes.c_float * 6)(*dev[0].p)
            wp = hs.make_warp_params(3)
            res["gwarp bgr"] = events(lambda: L.hsflow_gmotion_warp_device(ctx._h, model, ctypes.byref(wp), P(pic), 3 * W, None, 0, P(dst), 3 * W, None))
            ctx.synchronize()
            assert np.array_equal(dst.cpu().numpy(), hs.gmotion_warp_host(dev[0], pic.cpu().numpy())), case
            res["warp bgr"] = events(lambda: L.hsflow_warp_device(ctx._h, 0, ctypes.byref(wp), P(pic), 3 * W, None, 0, P(dst), 3 * W, None))
            with torch.cuda.stream(s):
                res["copy"] = events(lambda: b.copy_(a))
            out[case] = dict(res, width=W, height=H)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmotion_time.txt"))
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
    text = ["the global motion of a flow (hsflow_gmotion_fit_device, _fit_batch_device, hsflow_gmotion_warp_device): ms per CALL; medians of %d sessions,"
            % args.sessions,
            "each %d calls back to back between device events (host: a host clock around one round; its record and mask equal the device's bit for bit)" % args.reps]
    for case, W, H in CASES:
        first = sessions[0][case]
        text.append("%s, %dx%d  (inliers of pair 0: %.1f %% of the pixels; model %s)" % (case, W, H, 100 * first["inliers"], " ".join("%.6g" % x for x in first["model"])))
        med = {}
        for row in ROWS:
            vals = [s[case][row] for s in sessions]
            med[row] = median(vals)
            text.append("  %-22s %9.4f   (sessions: %s)" % (row, med[row], ", ".join("%.4f" % t for t in vals)))
        text.append("  fit 1 fixed 3p / copy %.2f; fit 8 fixed 3p per pair / copy %.2f; gwarp / warp %.2f; host / fit 1 fixed 3p %.0f"
                    % (med["fit 1 fixed 3p"] / med["copy"], med["fit 8 fixed 3p"] / PAIRS / med["copy"], med["gwarp bgr"] / med["warp bgr"],
                       med["host"] / med["fit 1 fixed 3p"]))
    text = "\n".join(text) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
