#!/usr/bin/env python3
"""What the median filter / hole filling of the flow on the device (hsflow_median*) costs.  Two sizes,
1920x1080 (the seed-1 translating pair, 100 sweeps) and 600x480 (the reference's city pair as its CPU route solves it),
each a context of two pairs, the second made by hsflow_set_frames_reversed.  Radius 1 and 2; FILTER on the solver's flow
without a state plane, FILL with the hsflow_fb mask of the solver's two flows as the state.  Per case:
  pass         one pass into caller planes (hsflow_median_device, flow out), device events around --reps calls back to back;
  pass+rec     the same with the record;
  apply4       hsflow_median_apply with four passes (the pair's flow replaced; the flow changes from call to call, the
               work does not: every lane runs the same exchanges whatever the values), per CALL of four passes;
  apply4+rec   the same with the record of the last pass;
  copy         a device-to-device copy of both fp32 planes: 8 bytes per pixel read and 8 written, the flow traffic of one
               pass (FILL reads one state byte per pixel more);
  host         hsflow_get_flow + hsflow_median_host (one pass) + upload and hsflow_set_flow_device, a host clock around
               --host-reps rounds.
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported, and after
a session that failed nothing more is started.
   usage: tools/median_time.py [--reps 200] [--sessions 3] [--out profiles/median_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
CASES = ("1080p", "600x480")
MODES = ("filter", "fill")
ROWS = ("pass", "pass+rec", "apply4", "apply4+rec", "copy", "host")


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
            u0, v0 = ctx.flow(0)
            du, dv = torch.from_numpy(u0).cuda(), torch.from_numpy(v0).cuda()
            mask = ctx.fb(0, 1, mask=True, device=True)[0]
            ctx.synchronize()
            mask_host = mask.cpu().numpy()
            uo, vo = (torch.zeros((H, W), dtype=torch.float32, device="cuda") for _ in range(2))
            stats = torch.zeros(64, dtype=torch.uint8, device="cuda")
            a, b = (torch.zeros(8 * W * H, dtype=torch.uint8, device="cuda") for _ in range(2))
            pu, pv, pst, pm = (ctypes.c_void_p(t.data_ptr()) for t in (uo, vo, stats, mask))
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

            def restore():
                ctx.set_flow_rows_from(du, dv, 0, H, pair=0)
                ctx.synchronize()

            for radius in (1, 2):
                for mode in MODES:
                    mp = hs.make_median_params(radius, mode, 1)
                    r = ctypes.byref(mp)
                    st, ss, st_host = (pm, W, mask_host) if mode == "fill" else (None, 0, None)
                    res = {}
                    res["pass+rec"] = events(lambda: L.hsflow_median_device(ctx._h, 0, r, st, ss, pu, pv, 4 * W, None, 0, pst))
                    ctx.synchronize()
                    wu, wv, _, wrec = hs.median_host(u0, v0, st_host, stats=True, params=mp)
                    assert np.array_equal(uo.cpu().numpy().view(np.uint32), wu.view(np.uint32)), (case, radius, mode)
                    assert np.array_equal(vo.cpu().numpy().view(np.uint32), wv.view(np.uint32)), (case, radius, mode)
                    assert bytes(hs.median_stats_from(stats)) == bytes(wrec), (case, radius, mode)
                    res["pass"] = events(lambda: L.hsflow_median_device(ctx._h, 0, r, st, ss, pu, pv, 4 * W, None, 0, None))
                    res["apply4"] = events(lambda: L.hsflow_median_apply(ctx._h, 0, r, 4, st, ss, None, 0, None))
                    restore()
                    res["apply4+rec"] = events(lambda: L.hsflow_median_apply(ctx._h, 0, r, 4, st, ss, None, 0, pst))
                    restore()
                    with torch.cuda.stream(s):
                        res["copy"] = events(lambda: b.copy_(a))
                    t0 = time.perf_counter()
                    for _ in range(host_reps):
                        hu, hv = ctx.flow(0)
                        fu, fv, _, _ = hs.median_host(hu, hv, st_host, params=mp)
                        tu, tv = torch.from_numpy(fu).cuda(), torch.from_numpy(fv).cuda()
                        torch.cuda.synchronize()
                        ctx.set_flow_rows_from(tu, tv, 0, H, pair=0)
                        ctx.synchronize()
                    res["host"] = (time.perf_counter() - t0) * 1e3 / host_reps
                    restore()
                    for k in ("kept", "filled", "unfilled", "changed"):
                        res[k] = int(getattr(wrec, k))
                    out["%s r%d %s" % (case, radius, mode)] = dict(res, width=W, height=H)
    print("RESULT " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "median_time.txt"))
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
    text = ["median filter / hole filling (hsflow_median*): ms per call; medians of %d sessions, each %d calls back to back between device events"
            % (args.sessions, args.reps),
            "(host: a host clock around %d rounds of flow read-back + hsflow_median_host + upload and hsflow_set_flow_device)" % args.host_reps]
    for key in sessions[0]:
        first = sessions[0][key]
        W, H = first["width"], first["height"]
        text.append("%s, %dx%d  (both planes %.1f MB; one pass: kept %d, filled %d, unfilled %d, changed %d)"
                    % (key, W, H, 8e-6 * W * H, first["kept"], first["filled"], first["unfilled"], first["changed"]))
        for row in ROWS:
            vals = [s[key][row] for s in sessions]
            text.append("  %-11s %9.4f   (sessions: %s)" % (row, median(vals), ", ".join("%.4f" % t for t in vals)))
        one, four, copy, host = (median([s[key][row] for s in sessions]) for row in ("pass", "apply4", "copy", "host"))
        text.append("  one pass moves 16 B of flow per pixel: %.0f GB/s; the copy moves the same: %.0f GB/s; pass / copy %.2f, apply4 / (4 copy) %.2f, host / pass %.0f"
                    % (16 * W * H / one * 1e-6, 16 * W * H / copy * 1e-6, one / copy, four / (4 * copy), host / one))
    text = "\n".join(text) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
