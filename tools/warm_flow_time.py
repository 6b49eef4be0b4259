#!/usr/bin/env python3
"""What a warm start costs once the caller has written flow ("caller-written flow"): after
hsflow_set_flow_device a strip / fold solve measures the planes before it plans its launches (one small launch, one word
back, the host waits).  1920x1080, lambda 1, ITER, synchronous solves with reuse_derivatives, host clock per repetition,
medians of --reps after warm-up:
  halo     hsflow_set_flow_device of 16 rows (the context's own flow, copied out once) + a 16-sweep warm solve -- the
           pattern of a row slab's halo exchange;
  full     hsflow_set_flow_device of the whole plane + a 100-sweep warm solve;
  nowrite  a 16-sweep warm solve, nothing written since the cold solve before the loop (the planes stay tame: this row must
           not move);
  vouched  halo with HSFLOW_FLOW_SOLVER_MADE (hsflow_set_flow_device_ex), as the row-slab drivers write their halo rows:
           nothing is measured; this tree only, to be held against the parent's halo row;
  classic, classic_R3, classic_R4   a cold 100-sweep classic solve (alpha 15) on the classic strip kernel: its default shape
           and strip_rows 3 / threads 1024, strip_rows 4 / threads 768 -- the shapes that divide with the hoisted reciprocal,
           whose division now treats numerators far above the denominator separately.
This tree and, with --parent ROOT (a checkout of the parent commit, built), the parent's, each in a child process of its
own, alternating, --rounds times each; the spread of the parent's medians is what a difference has to exceed.  After a
child that failed nothing more is started.
   usage: tools/warm_flow_time.py [--reps 40] [--rounds 3] [--parent ROOT] [--out profiles/warm_flow_time.txt]"""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ROWS = ("halo", "full", "nowrite", "vouched", "classic", "classic_R3", "classic_R4")
W, H = 1920, 1080


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n & 1 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def run_child(reps, pkg):
    sys.path.insert(0, pkg)
    import torch
    import opticalflowhs_amd as hs
    from opticalflowhs_amd import synth
    A, B = synth.translating_pair(W, H, seed=1)
    with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
        ctx.set_frames(A, B)
        ctx.solve(lam=1.0, max_iter=100, term_type=hs.TERM_ITER)
        ud = torch.empty((H, W), dtype=torch.float32, device="cuda")
        vd = torch.empty((H, W), dtype=torch.float32, device="cuda")
        ctx.flow_rows_to(ud, vd, 0, H)
        ctx.synchronize()

        def halo():
            ctx.set_flow_rows_from(ud[H - 16:], vd[H - 16:], H - 16, 16)
            ctx.solve(lam=1.0, max_iter=16, term_type=hs.TERM_ITER, use_previous=True, reuse_derivatives=True)

        def full():
            ctx.set_flow_rows_from(ud, vd, 0, H)
            ctx.solve(lam=1.0, max_iter=100, term_type=hs.TERM_ITER, use_previous=True, reuse_derivatives=True)

        def nowrite():
            ctx.solve(lam=1.0, max_iter=16, term_type=hs.TERM_ITER, use_previous=True, reuse_derivatives=True)

        def vouched():
            ctx.set_flow_rows_from(ud[H - 16:], vd[H - 16:], H - 16, 16, solver_made=True)
            ctx.solve(lam=1.0, max_iter=16, term_type=hs.TERM_ITER, use_previous=True, reuse_derivatives=True)

        def classic(**kw):
            return lambda: ctx.solve(mode=hs.MODE_CLASSIC, alpha=15.0, max_iter=100, term_type=hs.TERM_ITER, kernel=hs.KERNEL_STRIP, **kw)

        cases = [("nowrite", nowrite), ("halo", halo), ("full", full)]
        if hasattr(hs._lib.load(), "hsflow_set_flow_device_ex"):
            cases.append(("vouched", vouched))
        cases += [("classic", classic()), ("classic_R3", classic(strip_rows=3, threads=1024)), ("classic_R4", classic(strip_rows=4, threads=768))]
        for name, fn in cases:
            if name in ("nowrite", "vouched"):   # the planes are the solver's own again
                ctx.solve(lam=1.0, max_iter=100, term_type=hs.TERM_ITER)
            ts = []
            for i in range(reps + 5):
                t0 = time.perf_counter()
                fn()
                t1 = time.perf_counter()
                if i >= 5:
                    ts.append((t1 - t0) * 1e3)
            print("%s ms=%.5f" % (name, median(ts)))


def child(pkg, reps, limit=200):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--pkg", os.path.abspath(pkg), "--reps", str(reps)], capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError("child (%s) failed (%d): %s" % (pkg, r.returncode, r.stderr[-2000:]))
    return {line.split()[0]: float(line.split("=")[1]) for line in r.stdout.splitlines() if " ms=" in line}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--pkg", default=ROOT)
    a = ap.parse_args()
    if a.child:
        run_child(a.reps, a.pkg)
        return 0
    lines = ["warm_flow_time: %dx%d, lambda 1, ITER, synchronous warm solves, host clock, ms; medians of %d, %d rounds per side, alternating" % (W, H, a.reps, a.rounds)]
    try:
        tree, parent = [], []
        for _ in range(a.rounds):          # alternating: parent, tree, parent, tree, ...
            if a.parent:
                parent.append(child(a.parent, a.reps))
            tree.append(child(ROOT, a.reps))
        what = {"halo": "set_flow_device of 16 rows + 16-sweep warm solve", "full": "set_flow_device of the plane + 100-sweep warm solve",
                "nowrite": "16-sweep warm solve, nothing written", "vouched": "halo with HSFLOW_FLOW_SOLVER_MADE; parent: its halo row",
                "classic": "cold classic strip solve, 100 sweeps, default shape", "classic_R3": "the same, strip_rows 3, threads 1024",
                "classic_R4": "the same, strip_rows 4, threads 768"}
        for row in ROWS:
            lines.append("%s (%s):" % (row, what[row]))
            for name, runs in (("parent", parent), ("this tree", tree)):
                if runs:
                    xs = [r[row if row in r else "halo"] for r in runs]
                    lines.append("  %-9s %s   median %.4f, min %.4f, max %.4f, spread %.4f" % (name, "  ".join("%.4f" % x for x in xs), median(xs), min(xs), max(xs), max(xs) - min(xs)))
            if parent:
                ps, ts = [r[row if row in r else "halo"] for r in parent], [r[row] for r in tree]
                sp = max(ps) - min(ps)
                d = median(ts) - median(ps)
                if row not in ("halo", "full"):
                    inside = min(ps) - sp <= median(ts) <= max(ps) + sp
                    lines.append("  difference %+.4f ms (%+.1f %%): this tree's median %s the parent's range widened by its spread (%.4f .. %.4f)" % (
                        d, 100.0 * d / median(ps), "lies inside" if inside else "lies OUTSIDE", min(ps) - sp, max(ps) + sp))
                else:
                    lines.append("  cost of measuring the planes: %+.4f ms (%+.1f %%); the parent's spread is %.4f" % (d, 100.0 * d / median(ps), sp))
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        lines.append("failed: %s" % e)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if "failed" in text else 0


if __name__ == "__main__":
    sys.exit(main())
