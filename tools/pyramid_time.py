#!/usr/bin/env python3
"""What a coarse-to-fine solve (hsflow_solve_pyramid) costs beside the solves it is made of.  Two sizes,
1920x1080 (the seed-1 translating texture shifted by (9, 6) px) and 600x480 (the reference's city pair); auto levels, 100
sweeps per solve, ITER, lambda 0.003, warps 1 and 2.  Per CALL, device events around --reps calls back to back:
  plain        one hsflow_solve_async of the frame, one level: what the library did before;
  level sum    the sum over the plan's levels of `warps` plain solves at that level's size, each size timed on a context of
               its own: the floor the pyramid's own kernels add to;
  pyramid      hsflow_solve_pyramid;
  host         what a caller pays for the same flow without it: per level and step the flow read back, the host rules
               (hsflow_pyramid_down_host, _prolong_host, hsflow_warp_host), the frames uploaded to a context of the level's
               size and its solve; a host clock around one round;
  copy <k>     a device-to-device copy of as many bytes as kernel <k> moves at level 0 (level 1 for the first down), read
               plus written, halved: the copy reads and writes each of its bytes.
The single launches -- k_pyr_down, k_pyr_step, k_pyr_total -- are timed kernel by kernel from kernel traces: the caller runs
`--trace CASE WARPS` (30 calls of hsflow_solve_pyramid, nothing else) under the profiler's kernel trace with statistics, one
run per size and warp count into DIR/CASE_wWARPS/, each a process and a run of its own; `--trace-dir DIR` then appends the
kernels' average and shortest times per launch (all levels together) to the report.
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported, and after
a session that failed nothing more is started.
   usage: tools/pyramid_time.py [--reps 200] [--sessions 3] [--trace-dir DIR] [--out profiles/pyramid_time.txt]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = ("1080p", "600x480")
WARPS = (1, 2)
ROWS = ("plain", "level sum", "pyramid", "host", "copy down", "copy step", "copy total")
KERNELS = ("k_pyr_down", "k_pyr_step", "k_pyr_total")
LAM, SWEEPS = 0.003, 100


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


def the_case(case):
    from opticalflowhs_amd import synth
    if case == "1080p":
        return synth.translating_pair(1920, 1080, seed=1, dx=9.0, dy=6.0)
    g = os.path.join(ROOT, "tests", "golden")
    return read_pgm(os.path.join(g, "city_1_gray.pgm")), read_pgm(os.path.join(g, "city_2_gray.pgm"))


def host_route(hs, A, B, sizes, warps, params):
    """The flow of the pyramid by the caller's own hands; returns the level-0 total."""
    import numpy as np
    prevs, currs = [A], [B]
    for _ in sizes[1:]:
        prevs.append(hs.pyramid_down_host(prevs[-1]))
        currs.append(hs.pyramid_down_host(currs[-1]))
    u = v = None
    for l in range(len(sizes) - 1, -1, -1):
        W, H = sizes[l]
        with hs.HSFlow(W, H, 1, own_stream=True) as c:
            for k in range(warps):
                if u is None:
                    c.set_frames(prevs[l], currs[l])
                    c.solve(params)
                    u, v = c.flow()
                    continue
                if k == 0:
                    u, v = hs.pyramid_prolong_host(u, W, H), hs.pyramid_prolong_host(v, W, H)
                c.set_frames(prevs[l], hs.warp_host(u, v, currs[l], border="replicate"))
                c.solve(params)
                du, dv = c.flow()
                u, v = (u + du).astype(np.float32), (v + dv).astype(np.float32)
    return u, v


def run_child(reps, cases, warps_list, trace):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opticalflowhs_amd as hs
    out = {}
    for case in cases:
        A, B = the_case(case)
        H, W = A.shape
        sizes = hs.pyramid_plan(W, H)
        params = hs.make_params(lam=LAM, max_iter=SWEEPS, term_type=hs.TERM_ITER)
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

        if trace:
            with hs.HSFlow(W, H, 1, stream=s.cuda_stream) as ctx:
                ctx.set_frames(A, B)
                for w in warps_list:
                    pp = hs.make_pyramid_params(warps=w)
                    for _ in range(30):
                        ctx.solve_pyramid(params, pyramid=pp)
                    ctx.synchronize()
            continue
        per_level = []
        for (w, h) in sizes:
            with hs.HSFlow(w, h, 1, stream=s.cuda_stream) as c:
                c.set_frames(np.ascontiguousarray(A[:h, :w]), np.ascontiguousarray(B[:h, :w]))  # (an ITER solve's time does not depend on the content)
                per_level.append(events(lambda: c.solve_async(params)))
                c.synchronize()
        a, b = (torch.zeros(16 * W * H, dtype=torch.uint8, device="cuda") for _ in range(2))

        def copy_ms(nbytes):
            n = max(int(nbytes) // 2, 4)
            with torch.cuda.stream(s):
                return events(lambda: b[:n].copy_(a[:n]))

        with hs.HSFlow(W, H, 1, stream=s.cuda_stream) as ctx:
            ctx.set_frames(A, B)
            for w in warps_list:
                pp = hs.make_pyramid_params(warps=w)
                res = {"plain": per_level[0], "level sum": w * sum(per_level)}
                res["pyramid"] = events(lambda: ctx.solve_pyramid(params, pyramid=pp))
                ctx.synchronize()
                got = ctx.flow()
                info = ctx.pyramid_info()
                t0 = time.perf_counter()
                want = host_route(hs, A, B, sizes, w, params)
                res["host"] = (time.perf_counter() - t0) * 1e3
                for g, x in zip(got, want):
                    assert np.array_equal(g.view(np.uint32), x.view(np.uint32)), (case, w)
                px = W * H
                # down of both frames: 2 px read, px / 2 written; step at level 0: 2 px of coarse flow and px of frame read, 9 px
                # written; total: 16 px read, 8 px written
                moved = {"down": 2.5 * px, "step": 12 * px, "total": 24 * px}
                for k, nbytes in moved.items():
                    res["copy " + k] = copy_ms(nbytes)
                out["%s w=%d" % (case, w)] = dict(res, width=W, height=H, levels=len(sizes), per_level=per_level, moved=moved,
                                                  launches=[info["down_launches"], info["step_launches"], info["total_launches"]])
    print("RESULT " + json.dumps(out))


def kernel_report(trace_dir):
    """The per-launch times of the pyramid's kernels from DIR/CASE_wWARPS/**/*kernel_stats.csv, as lines of text."""
    import csv
    import glob
    import re
    text = ["", "kernel by kernel: ms per LAUNCH, average and shortest over the launches of ALL levels in a kernel trace with statistics of",
            "`--trace CASE WARPS`, a process and a profiler run of its own per size and warp count (30 calls)"]
    for case in CASES:
        for w in WARPS:
            found = sorted(glob.glob(os.path.join(trace_dir, "%s_w%d" % (case, w), "**", "*kernel_stats.csv"), recursive=True))
            if not found:
                raise SystemExit("no kernel statistics for %s warps=%d under %s" % (case, w, trace_dir))
            text.append("%s, warps %d" % (case, w))
            rows = []
            with open(found[-1], newline="") as f:
                for r in csv.DictReader(f):
                    name = r.get("Name") or r.get("KernelName") or r.get("Kernel_Name") or ""
                    if not any(k in name for k in KERNELS):
                        continue
                    m = re.search(r"(k_\w+<[^>]*>)", name)
                    calls = int(r.get("Calls") or r.get("calls") or 0)
                    total = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0.0)
                    avg = float(r.get("AverageNs") or r.get("Average") or r.get("average_ns") or 0.0)
                    low = float(r.get("MinNs") or r.get("Min") or 0.0)
                    high = float(r.get("MaxNs") or r.get("Max") or 0.0)
                    rows.append((m.group(1) if m else name[:60], calls, avg * 1e-6, low * 1e-6, high * 1e-6, total * 1e-6 / 30))
            for name, calls, avg, low, high, per_call in sorted(rows):
                text.append("  %-24s %9.4f   (shortest %.4f, longest %.4f, %d launches; %.4f ms per pyramid call)" % (name, avg, low, high, calls, per_call))
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--sessions", type=int, default=3, help="0: the timed part of --out is kept as it is")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_time.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", nargs=2, metavar=("CASE", "WARPS"), help="what a kernel trace is taken of: one size, one warp count")
    ap.add_argument("--trace-dir", help="the kernel traces' directory: their per-kernel times go behind the report")
    args = ap.parse_args()
    if args.trace:
        return run_child(10, (args.trace[0],), (int(args.trace[1]),), True)
    if args.child:
        return run_child(args.reps, CASES, WARPS, False)
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
    text = ["coarse-to-fine solves (hsflow_solve_pyramid): ms per CALL; auto levels, %d sweeps per solve, ITER, lambda %g; medians of %d sessions, each %d calls"
            % (SWEEPS, LAM, args.sessions, args.reps),
            "back to back between device events (host: a host clock around one round; its flow equals the pyramid's bit for bit)"]
    for case in CASES:
        for w in WARPS:
            key = "%s w=%d" % (case, w)
            first = sessions[0][key]
            text.append("%s, %dx%d, %d levels, warps %d  (launches per call: down %d, step %d, total %d; plain solves per level: %s ms)"
                        % ((case, first["width"], first["height"], first["levels"], w) + tuple(first["launches"])
                           + (", ".join("%.4f" % median([s[key]["per_level"][l] for s in sessions]) for l in range(first["levels"])),)))
            med = {}
            for row in ROWS:
                vals = [s[key][row] for s in sessions]
                med[row] = median(vals)
                text.append("  %-11s %9.4f   (sessions: %s)" % (row, med[row], ", ".join("%.4f" % t for t in vals)))
            text.append("  pyramid / plain %.2f; pyramid - level sum %.4f ms (%.1f %% of the pyramid: the three kernels, the frame's copy aside and back, launch gaps); host / pyramid %.0f"
                        % (med["pyramid"] / med["plain"], med["pyramid"] - med["level sum"], 100 * (med["pyramid"] - med["level sum"]) / med["pyramid"], med["host"] / med["pyramid"]))
    text = "\n".join(text + kernels) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
