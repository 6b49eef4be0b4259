#!/usr/bin/env python3
"""What the frame between the two frames of a pair costs on the device (hsflow_interp*).  Two sizes,
1920x1080 (the seed-1 translating pair, 100 sweeps) and 600x480 (the reference's city pair as its CPU route solves it);
the pictures are the two frames as BGR pictures (the gray frames, tinted), the reference the first.  One time (t = 0.5)
and eight (t = 1/9 .. 8/9).  Per CALL of n times, device events around --reps calls back to back:
  whole        hsflow_interp_batch_device with pictures, reference and statistics;
  picture      the same without reference and statistics;
  own          the context's own gray frames (d_prev == NULL), pictures and statistics;
  memset       a fill of the key planes' bytes (8 per pixel of the pitched plane and time) -- what goes in front of the splat;
  project0     hsflow_project_flow_device with fill_passes 0 and statistics into caller planes (one time only);
  project4     the same with the default 4 passes (one time only);
  copy         a device-to-device copy of the bytes `picture` must move: 8 of flow and 6 of frames read once, 3 written per
               time and pixel;
  warp2        two hsflow_warp_device calls per time (both frames warped to t, no blend: the nearest thing there was);
  host         both flow planes read back + hsflow_interp_host per time, a host clock around one call.
The single launches -- splat, resolve, the fill's passes, blend -- are timed kernel by kernel from kernel traces: the caller
runs `--trace CASE N` (one size, one count: 30 calls each of whole, picture, own and warp2, nothing else) under the
profiler's kernel trace with statistics, one run per size and count into DIR/CASE_nN/, each a process and a run of its own;
`--trace-dir DIR` then appends the kernels' average and shortest times per launch to the report.  k_warp_batch<3, false>
stands beside the splat: the same four-tap gather of a BGR picture over the same pixels, without the atomics.
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported, and after
a session that failed nothing more is started.
   usage: tools/interp_time.py [--reps 200] [--sessions 3] [--trace-dir DIR] [--out profiles/interp_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = ("1080p", "600x480")
COUNTS = (1, 8)
ROWS = ("whole", "picture", "own", "memset", "project0", "project4", "copy", "warp2", "host")


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


def run_child(reps, host, cases, counts=None, trace=False):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opticalflowhs_amd as hs
    L = hs._lib.load()
    out = {}
    tint = np.array([0.6, 0.8, 1.0])
    for case in cases:
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
            u, v = ctx.flow()
            pitch = ctx.info()["pitch"]
            dprev, dcurr = (torch.from_numpy(f).cuda() for f in bgr)
            pp, pc = ctypes.c_void_p(dprev.data_ptr()), ctypes.c_void_p(dcurr.data_ptr())
            fu, fv = (torch.zeros((H, W), dtype=torch.float32, device="cuda") for _ in range(2))
            pfu, pfv = ctypes.c_void_p(fu.data_ptr()), ctypes.c_void_p(fv.data_ptr())
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

            for n in (counts or COUNTS):
                times = [0.5] if n == 1 else [(k + 1) / (n + 1.0) for k in range(n)]
                tt = (ctypes.c_float * n)(*times)
                dst = torch.zeros((n, H, W, 3), dtype=torch.uint8, device="cuda")
                gray = torch.zeros((n, H, W), dtype=torch.uint8, device="cuda")
                stats = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
                keys = torch.zeros(8 * pitch * H * n, dtype=torch.uint8, device="cuda")
                moved = (8 + 6 + 3 * n) * W * H
                a, b = (torch.zeros(moved, dtype=torch.uint8, device="cuda") for _ in range(2))
                lst = lambda t: (ctypes.c_void_p * n)(*[t[i].data_ptr() for i in range(n)])
                pd, pg, pr, pst = lst(dst), lst(gray), (ctypes.c_void_p * n)(*[dprev.data_ptr()] * n), ctypes.c_void_p(stats.data_ptr())
                ip3, ip1, ip0 = hs.make_interp_params(3), hs.make_interp_params(1), hs.make_interp_params(3, fill_passes=0)
                r3, r1, r0 = ctypes.byref(ip3), ctypes.byref(ip1), ctypes.byref(ip0)
                wp3 = [(hs.make_warp_params(3, -t), hs.make_warp_params(3, 1.0 - t)) for t in times]
                torch.cuda.synchronize()
                ok = lambda st: st == 0 or sys.exit("status %d: %s" % (st, L.hsflow_last_error(ctx._h)))
                if trace:
                    for k in range(3):  # (the kernels' names tell the rows apart)
                        events(lambda: ok(L.hsflow_interp_batch_device(ctx._h, 0, n, tt, r3, pp, 3 * W, pc, 3 * W, None, 0, None, 0, pr, 3 * W, pd, 3 * W, None, 0, pst)))
                        events(lambda: ok(L.hsflow_interp_batch_device(ctx._h, 0, n, tt, r3, pp, 3 * W, pc, 3 * W, None, 0, None, 0, None, 0, pd, 3 * W, None, 0, None)))
                        events(lambda: ok(L.hsflow_interp_batch_device(ctx._h, 0, n, tt, r1, None, 0, None, 0, None, 0, None, 0, None, 0, pg, W, None, 0, pst)))
                        for wa, wb in wp3:
                            events(lambda: ok(L.hsflow_warp_device(ctx._h, 0, ctypes.byref(wb), pc, 3 * W, None, 0, pd[0], 3 * W, None)))
                    ctx.synchronize()
                    continue
                res = {}
                res["whole"] = events(lambda: ok(L.hsflow_interp_batch_device(ctx._h, 0, n, tt, r3, pp, 3 * W, pc, 3 * W, None, 0, None, 0, pr, 3 * W, pd, 3 * W,
                                                                              None, 0, pst)))
                ctx.synchronize()
                got = hs.interp_stats_from(stats, n)
                got = got if n > 1 else [got]
                want, _, ws = hs.interp_host(u, v, bgr[0], bgr[1], t=times[-1], ref=bgr[0], stats=True)
                assert np.array_equal(dst[n - 1].cpu().numpy(), want) and bytes(got[-1]) == bytes(ws), (case, n)
                res["picture"] = events(lambda: ok(L.hsflow_interp_batch_device(ctx._h, 0, n, tt, r3, pp, 3 * W, pc, 3 * W, None, 0, None, 0, None, 0, pd, 3 * W,
                                                                                None, 0, None)))
                res["own"] = events(lambda: ok(L.hsflow_interp_batch_device(ctx._h, 0, n, tt, r1, None, 0, None, 0, None, 0, None, 0, None, 0, pg, W, None, 0, pst)))
                with torch.cuda.stream(s):
                    res["memset"] = events(lambda: keys.fill_(255))
                    res["copy"] = events(lambda: b.copy_(a))
                if n == 1:
                    res["project0"] = events(lambda: ok(L.hsflow_project_flow_device(ctx._h, 0, 0.5, r0, pp, 3 * W, pc, 3 * W, pfu, pfv, 4 * W, None, 0, pst)))
                    res["project4"] = events(lambda: ok(L.hsflow_project_flow_device(ctx._h, 0, 0.5, r3, pp, 3 * W, pc, 3 * W, pfu, pfv, 4 * W, None, 0, pst)))
                else:
                    res["project0"] = res["project4"] = 0.0

                def warp2():
                    for k, (wa, wb) in enumerate(wp3):
                        ok(L.hsflow_warp_device(ctx._h, 0, ctypes.byref(wa), pp, 3 * W, None, 0, pd[k], 3 * W, None))
                        ok(L.hsflow_warp_device(ctx._h, 0, ctypes.byref(wb), pc, 3 * W, None, 0, pd[k], 3 * W, None))
                res["warp2"] = events(warp2)
                ctx.synchronize()
                if host:
                    t0 = time.perf_counter()
                    uu, vv = ctx.flow()
                    for t in times:
                        hs.interp_host(uu, vv, bgr[0], bgr[1], t=t, ref=bgr[0], stats=True)
                    res["host"] = (time.perf_counter() - t0) * 1e3
                else:
                    res["host"] = 0.0
                rec = {k: int(getattr(ws, k)) for k in ("blended", "prev_only", "curr_only", "clamped", "holes", "unfilled", "collisions", "left")}
                out["%s n=%d" % (case, n)] = dict(res, width=W, height=H, pitch=pitch, moved=moved, **rec)
    print("RESULT " + json.dumps(out))


KERNELS = ("k_interp_splat", "k_interp_resolve", "k_median_batch", "k_interp_blend", "k_warp_batch")


def kernel_report(trace_dir):
    """The per-launch times of the kernels from DIR/CASE_nN/**/*kernel_stats.csv (a kernel trace with statistics of
    `--trace CASE N`), as lines of text."""
    import csv
    import glob
    import re
    text = ["", "kernel by kernel: ms per LAUNCH of n times (blockIdx.z = the time), average and shortest of all launches in a kernel trace with statistics of",
            "`--trace CASE N`, a process and a profiler run of its own per size and count (whole, picture, own and one warp per time, 60 calls each)"]
    for case in CASES:
        for n in COUNTS:
            found = sorted(glob.glob(os.path.join(trace_dir, "%s_n%d" % (case, n), "**", "*kernel_stats.csv"), recursive=True))
            if not found:
                raise SystemExit("no kernel statistics for %s n=%d under %s" % (case, n, trace_dir))
            text.append("%s, %d time%s" % (case, n, "" if n == 1 else "s"))
            rows = []
            with open(found[-1], newline="") as f:
                for r in csv.DictReader(f):
                    name = r.get("Name") or r.get("KernelName") or r.get("Kernel_Name") or ""
                    if not any(k in name for k in KERNELS):
                        continue
                    m = re.search(r"(k_\w+<[^>]*>)", name)
                    calls = int(r.get("Calls") or r.get("calls") or 0)
                    avg = float(r.get("AverageNs") or r.get("Average") or r.get("average_ns") or 0.0)
                    low = float(r.get("MinNs") or r.get("Min") or 0.0)
                    rows.append((m.group(1) if m else name[:60], calls, avg * 1e-6, low * 1e-6))
            for name, calls, avg, low in sorted(rows):
                text.append("  %-34s %9.4f   (shortest %.4f, %d launches)" % (name, avg, low, calls))
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sessions", type=int, default=3, help="0: the timed part of --out is kept as it is")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "interp_time.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", nargs=2, metavar=("CASE", "N"), help="what a kernel trace is taken of: one size, one count")
    ap.add_argument("--trace-dir", help="the kernel traces' directory: their per-kernel times go behind the report")
    args = ap.parse_args()
    if args.trace:
        return run_child(10, False, (args.trace[0],), (int(args.trace[1]),), True)
    if args.child:
        return run_child(args.reps, True, CASES)
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
    text = ["the frame between two frames (hsflow_interp*): ms per CALL of n times; medians of %d sessions, each %d calls back to back between device events"
            % (args.sessions, args.reps),
            "(host: a host clock around one flow read-back + n calls of hsflow_interp_host)"]
    for case in CASES:
        for n in COUNTS:
            key = "%s n=%d" % (case, n)
            first = sessions[0][key]
            W, H = first["width"], first["height"]
            text.append("%s, %dx%d BGR, solver flow, %d time%s  (last time: blended %d prev_only %d curr_only %d clamped %d holes %d unfilled %d collisions %d left %d)"
                        % (case, W, H, n, "" if n == 1 else "s", first["blended"], first["prev_only"], first["curr_only"], first["clamped"], first["holes"],
                           first["unfilled"], first["collisions"], first["left"]))
            med = {}
            for row in ROWS:
                vals = [s[key][row] for s in sessions]
                med[row] = median(vals)
                if n > 1 and row in ("project0", "project4"):
                    continue
                text.append("  %-10s %9.4f   (sessions: %s)" % (row, med[row], ", ".join("%.4f" % t for t in vals)))
            text.append("  picture moves at least %.1f MB: %.0f GB/s; the copy moves them each way: %.0f GB/s read + written; per time %.4f ms"
                        % (first["moved"] * 1e-6, first["moved"] / med["picture"] * 1e-6, 2 * first["moved"] / med["copy"] * 1e-6, med["picture"] / n))
    text = "\n".join(text + kernels) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
