#!/usr/bin/env python3
"""What following pixels and points through n flows (hsflow_chain_flow_device, hsflow_track_points_device)
costs beside today's routes.  Two sizes, 1920x1080 and 600x480, on a context of 32 pairs whose flows are a slow rotation
about the centre (0.002 rad per pair) plus a smooth ripple of a pixel, different for every pair; n = 2, 8, 32.  Per CALL,
device events around --reps calls back to back, the C entries called with arguments prepared once:
  flow          hsflow_chain_flow_device, U and V only;
  flow+st+stats the same with the status plane and the statistics;
  points 4096   hsflow_track_points_device with the full track, last positions, status and age; 4096 points on a grid;
  points 262144 the same with 262 144 points;
  copy          a device-to-device copy of two fp32 planes (what U and V alone would cost to move);
  fb x (n-1)    n - 1 mask-only hsflow_fb_planes_device launches on the same planes (pair k-1 forwards, pair k as the backward
                planes): the same gathers, today's nearest device route;
  host          the n pairs read back (hsflow_get_flow) and hsflow_chain_flow_host; a host clock around one round, and its
                U and V equal the device's bit for bit.
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported, and after
a session that failed nothing more is started.
The launches themselves are timed from kernel traces: the caller runs `--trace CASE N` (30 flow-only chains and 30 times the
n - 1 checks, nothing else) under the profiler's kernel trace with statistics into DIR/CASE_nN/, a process and a run of its
own per case; `--sessions 0 --trace-dir DIR` then appends the kernels' times per launch to the report as it is.
   usage: tools/chain_time.py [--reps 200] [--sessions 3] [--trace CASE N] [--trace-dir DIR] [--out profiles/chain_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = (("1080p", 1920, 1080), ("600x480", 600, 480))
NS = (2, 8, 32)
PAIRS = 32
ROWS = ("flow", "flow+st+stats", "points 4096", "points 262144", "copy", "fb x (n-1)", "host")


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n & 1 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def flow_of(W, H, k):
    import numpy as np
    x, y = np.meshgrid(np.arange(W, dtype=np.float64) - (W - 1) / 2.0, np.arange(H, dtype=np.float64) - (H - 1) / 2.0)
    c, s = np.cos(0.002), np.sin(0.002)
    ripple = np.sin(x / 37.0 + k) * np.cos(y / 29.0 - k)
    return (c * x - s * y - x + ripple).astype(np.float32), (s * x + c * y - y + 0.5 * ripple).astype(np.float32)


def run_child(reps, only=None):
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
        if only and only[0] != case:
            continue
        with hs.HSFlow(W, H, PAIRS, stream=s.cuda_stream) as ctx:
            for k in range(PAIRS):
                u, v = flow_of(W, H, k)
                ud, vd = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
                torch.cuda.synchronize()
                ctx.set_flow_rows_from(ud, vd, 0, H, pair=k)
                ctx.synchronize()
            new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
            U, V, st, mask = new((H, W), torch.float32), new((H, W), torch.float32), new((H, W), torch.uint8), new((H, W), torch.uint8)
            rec = new((64,), torch.uint8)
            a, b = new((2, H, W), torch.float32), new((2, H, W), torch.float32)
            cp, fp = hs.make_chain_params(), hs.make_fb_params()
            P = lambda t: ctypes.c_void_p(t.data_ptr())
            views = []
            for k in range(PAIRS):
                pu, pv, sb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
                assert L.hsflow_flow_view_device(ctx._h, k, ctypes.byref(pu), ctypes.byref(pv), ctypes.byref(sb)) == 0
                views.append((pu, pv, sb.value))
            points = {}
            for m in (4096, 262144):
                side = int(m ** 0.5)
                gx, gy = np.meshgrid(np.linspace(0, W - 1, side, dtype=np.float32), np.linspace(0, H - 1, m // side, dtype=np.float32))
                xy = torch.from_numpy(np.stack([gx.ravel(), gy.ravel()], -1).copy()).cuda()
                points[m] = (xy, new((PAIRS + 1, m, 2), torch.float32), new((m, 2), torch.float32), new((m,), torch.uint8), new((m,), torch.uint8))
            torch.cuda.synchronize()
            for n in NS:
                if only and only[1] != n:
                    continue
                ints = (ctypes.c_int * n)(*range(n))
                res = {}
                if only:
                    for _ in range(30):
                        assert L.hsflow_chain_flow_device(ctx._h, ints, n, None, 0, None, None, 0, ctypes.byref(cp), P(U), P(V), W * 4, None, 0, None, 0, None) == 0
                        for k in range(1, n):
                            assert L.hsflow_fb_planes_device(ctx._h, k - 1, views[k][0], views[k][1], views[k][2], ctypes.byref(fp), P(mask), W, None, 0, None) == 0
                    ctx.synchronize()
                    continue

                def chain(status, stats):
                    assert L.hsflow_chain_flow_device(ctx._h, ints, n, None, 0, None, None, 0, ctypes.byref(cp), P(U), P(V), W * 4, P(st) if status else None, W,
                                                      None, 0, P(rec) if stats else None) == 0
                res["flow"] = events(lambda: chain(False, False))
                res["flow+st+stats"] = events(lambda: chain(True, True))
                for m, (xy, track, last, pst, pag) in points.items():
                    def track_call():
                        assert L.hsflow_track_points_device(ctx._h, ints, n, None, 0, ctypes.byref(cp), P(xy), m, P(track), P(last), P(pst), P(pag), None) == 0
                    res["points %d" % m] = events(track_call)
                with torch.cuda.stream(s):
                    res["copy"] = events(lambda: b.copy_(a))

                def fb_chain():
                    for k in range(1, n):
                        assert L.hsflow_fb_planes_device(ctx._h, k - 1, views[k][0], views[k][1], views[k][2], ctypes.byref(fp), P(mask), W, None, 0, None) == 0
                res["fb x (n-1)"] = events(fb_chain)
                chain(False, False)
                ctx.synchronize()
                t0 = time.perf_counter()
                flows = [ctx.flow(k) for k in range(n)]
                hU, hV, _, _, _ = hs.chain_flow_host([f[0] for f in flows], [f[1] for f in flows])
                res["host"] = (time.perf_counter() - t0) * 1e3
                assert np.array_equal(U.cpu().numpy().view(np.uint32), hU.view(np.uint32)) and np.array_equal(V.cpu().numpy().view(np.uint32), hV.view(np.uint32)), (case, n)
                chain(True, True)
                ctx.synchronize()
                r = hs.chain_stats_from(rec)
                res["alive"] = int(r.cls[0]) / float(W * H)
                out["%s n=%d" % (case, n)] = dict(res, width=W, height=H)
    print("RESULT " + json.dumps(out))


def kernel_report(trace_dir):
    """The per-launch times of k_chain_dense and k_fb_batch from DIR/CASE_nN/**/*kernel_stats.csv, as lines of text."""
    import csv
    import glob
    import re
    text = ["", "kernel by kernel: ms per LAUNCH, average / shortest / longest in a kernel trace with statistics of `--trace CASE N`, a process and a",
            "profiler run of its own per case (30 flow-only chains, 30 times the n - 1 mask-only checks)"]
    for d in sorted(glob.glob(os.path.join(trace_dir, "*_n*"))):
        found = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if not found:
            continue
        text.append(os.path.basename(d))
        with open(found[-1], newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or r.get("Kernel_Name") or ""
                m = re.search(r"(k_chain_\w+<[^>]*>|k_fb_batch<[^>]*>)", name)
                if not m:
                    continue
                calls = int(r.get("Calls") or r.get("calls") or 0)
                avg, low, high = (float(r.get(k) or 0.0) * 1e-6 for k in ("AverageNs", "MinNs", "MaxNs"))
                text.append("  %-28s %9.4f / %.4f / %.4f   (%d launches)" % (m.group(1), avg, low, high, calls))
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_time.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", nargs=2, metavar=("CASE", "N"), help="what a kernel trace is taken of: one size, one n")
    ap.add_argument("--trace-dir", help="the kernel traces' directory: their per-kernel times go behind the report")
    args = ap.parse_args()
    if args.trace:
        return run_child(10, (args.trace[0], int(args.trace[1])))
    if args.child:
        return run_child(args.reps)
    kernels = kernel_report(args.trace_dir) if args.trace_dir else []
    if args.sessions == 0:
        kept = open(args.out).read().split("\nkernel by kernel:")[0].rstrip("\n").split("\n")
        text = "\n".join(kept + kernels) + "\n"
        sys.stdout.write(text)
        with open(args.out, "w") as f:
            f.write(text)
        return
    sessions = []
    for k in range(args.sessions):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)], capture_output=True, text=True, timeout=280)
        lines = [t for t in r.stdout.splitlines() if t.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("session %d failed (status %d); nothing more is started" % (k + 1, r.returncode))
        sessions.append(json.loads(lines[-1][7:]))
    text = ["pixels and points through n flows (hsflow_chain_flow_device, hsflow_track_points_device): ms per CALL; medians of %d sessions, each %d calls"
            % (args.sessions, args.reps),
            "back to back between device events (host: a host clock around one round; its U and V equal the device's bit for bit)"]
    for case, W, H in CASES:
        for n in NS:
            key = "%s n=%d" % (case, n)
            text.append("%s, %dx%d, n = %d  (ALIVE at the end: %.1f %% of the pixels)" % (case, W, H, n, 100 * sessions[0][key]["alive"]))
            med = {}
            for row in ROWS:
                vals = [s[key][row] for s in sessions]
                med[row] = median(vals)
                text.append("  %-14s %9.4f   (sessions: %s)" % (row, med[row], ", ".join("%.4f" % t for t in vals)))
            text.append("  flow / copy %.2f; flow / fb x (n-1) %.2f; host / flow %.0f" % (med["flow"] / med["copy"], med["flow"] / med["fb x (n-1)"], med["host"] / med["flow"]))
    text = "\n".join(text + kernels) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
