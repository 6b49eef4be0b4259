#!/usr/bin/env python3
"""What linking the regions of consecutive pairs (hsflow_link_regions_device / _batch_device) costs beside
the route it replaces.  One size, 1920x1080, on a context of 8 pairs that all hold the flow of the benchmark's pair (the
translating texture of seed 1, lambda 1, 100 iterations).  Per CALL, device events around --reps calls back to back after 10
warm-ups, the C entries called with arguments prepared once; links (256), both sides and the header are asked for, caps 64
unless said:
  fit           (a) one step on the label planes that hsflow_regions gives from the fit's foreground mask of that flow;
  fit x8        (b) 8 steps by one hsflow_link_regions_batch_device (ms per CALL, not per step);
  fit256        (a) at caps 256 x 256, the caps of the CLI's HSFLOW_CAMERA_OBJECTS: more regions below the cap, the LDS hash;
  one           (c) both planes ONE region: every vote in one cell;
  random4096    (d) random labels 0 .. 4096 at caps 4096 x 4096;
  copy          (e) a device-to-device copy of two label planes, the floor;
  host ...      (f) the route it replaces: two label planes and the flow read back, hsflow_link_regions_host, the records in
                hand; a host clock around each of 3 rounds, their median per session, and the outputs equal the device's
                byte for byte.  The sessions' range is reported, not a ratio: the host's time moves by a factor of 2.
With --trace NAME the child runs case NAME alone (fit or one), for a rocprofv3 --kernel-trace --stats run of its own:
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/link_time.py --child --trace fit
Every session is a child process of its own under a time limit; the medians of --sessions sessions are reported, and after
a session that failed nothing more is started.
   usage: tools/link_time.py [--reps 50] [--sessions 3] [--out profiles/link_time.txt]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
W, H, STEPS, CAP, LINKS = 1920, 1080, 8, 64, 256
CASES = ("fit", "fit256", "one", "random4096")
HOST_ROUNDS = 3
ROWS = ["fit", "fit x8", "fit256", "one", "random4096", "copy"] + ["host " + m for m in CASES]


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n & 1 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def run_child(reps, trace):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opticalflowhs_amd as hs
    from opticalflowhs_amd import synth
    L = hs._lib.load()
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

    A, B = synth.translating_pair(W, H, seed=1)
    with hs.HSFlow(W, H, 1) as one:
        one.set_frames(np.ascontiguousarray(A, np.uint8), np.ascontiguousarray(B, np.uint8))
        one.solve(lam=1.0, max_iter=100)
        u, v = one.flow(0)
    _, gmask, _, _ = hs.global_motion_host(u, v, mask=True, params=hs.make_gmotion_params(values=(0, 255, 0, 0)))
    _, fit_labels, _ = hs.regions_host(gmask, u, v, labels=True, records=False, capacity=0)
    rng = np.random.RandomState(4096)
    planes = {"fit": (fit_labels, fit_labels, CAP), "fit256": (fit_labels, fit_labels, 256), "one": (np.ones((H, W), np.int32), np.ones((H, W), np.int32), CAP),
              "random4096": (rng.randint(0, 4097, size=(H, W)).astype(np.int32), rng.randint(0, 4097, size=(H, W)).astype(np.int32), 4096)}
    res = {}
    with hs.HSFlow(W, H, STEPS, stream=s.cuda_stream) as ctx:
        ud, vd = torch.from_numpy(u).cuda(), torch.from_numpy(v).cuda()
        torch.cuda.synchronize()
        for k in range(STEPS):
            ctx.set_flow_rows_from(ud, vd, 0, H, pair=k)
        ctx.synchronize()
        new = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        for name in CASES if not trace else (trace,):
            la, lb, cap = planes[name]
            da, db = torch.from_numpy(la).cuda(), torch.from_numpy(lb).cuda()
            links, sa, sb, heads = new((STEPS, LINKS * 16), torch.uint8), new((STEPS, cap * 32), torch.uint8), new((STEPS, cap * 32), torch.uint8), new((STEPS * 64,), torch.uint8)
            lp = hs.make_link_params(cap, cap)
            torch.cuda.synchronize()

            def one_step():
                assert L.hsflow_link_regions_device(ctx._h, 0, P(da), P(db), 4 * W, ctypes.byref(lp), P(links[0]), LINKS, P(sa[0]), P(sb[0]), P(heads)) == 0
            res[name] = events(one_step)
            ctx.synchronize()
            if trace:
                continue
            head = hs.link_result_from(heads)
            dev = (bytes(links[0].cpu().numpy())[:head.n_written * 16], bytes(sa[0].cpu().numpy()), bytes(sb[0].cpu().numpy()), bytes(head))
            rounds = []
            for _ in range(HOST_ROUNDS):
                t0 = time.perf_counter()
                ha, hb = da.cpu().numpy(), db.cpu().numpy()
                hu, hv = ctx.flow(0)
                hres, hlinks, hsa, hsb = hs.link_regions_host(ha, hb, hu, hv, link_capacity=LINKS, params=lp)
                rounds.append((time.perf_counter() - t0) * 1e3)
            res["host " + name] = median(rounds)
            assert (bytes(hlinks)[:hres.n_written * 16], bytes(hsa), bytes(hsb), bytes(hres)) == dev, name
            res["links " + name] = int(head.n_links)
            if name == "fit":
                plist = lambda t: (ctypes.c_void_p * STEPS)(*[t[k].data_ptr() for k in range(STEPS)])
                ll, kl, al, bl = (ctypes.c_void_p * (STEPS + 1))(*[da.data_ptr()] * (STEPS + 1)), plist(links), plist(sa), plist(sb)

                def batch():
                    assert L.hsflow_link_regions_batch_device(ctx._h, 0, STEPS, ll, 4 * W, ctypes.byref(lp), kl, LINKS, al, bl, P(heads)) == 0
                res["fit x8"] = events(batch)
                ctx.synchronize()
                assert bytes(heads.cpu().numpy()) == dev[3] * STEPS
                a32, b32, c32, d32 = (new((H, W), torch.int32) for _ in range(4))

                def copy():
                    b32.copy_(a32)
                    d32.copy_(c32)
                with torch.cuda.stream(s):
                    res["copy"] = events(copy)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sessions", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "link_time.txt"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", default="", choices=("", "fit", "one"))
    args = ap.parse_args()
    if args.child:
        return run_child(args.reps, args.trace)
    sessions = []
    for k in range(args.sessions):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)], capture_output=True, text=True, timeout=280)
        lines = [t for t in r.stdout.splitlines() if t.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit("session %d failed (status %d); nothing more is started" % (k + 1, r.returncode))
        sessions.append(json.loads(lines[-1][7:]))
    first = sessions[0]
    text = ["regions linked across pairs (hsflow_link_regions_device, _batch_device), %dx%d, %d links + both sides + header, caps %d (random4096: 4096): ms per CALL;"
            % (W, H, LINKS, CAP),
            "medians of %d sessions, each %d calls back to back between device events after 10 warm-ups (host: a host clock around each of %d rounds of read-back and"
            % (args.sessions, args.reps, HOST_ROUNDS),
            "hsflow_link_regions_host, their median per session; its outputs equal the device's byte for byte).  links: " + ", ".join("%s %d" % (m, first["links " + m]) for m in CASES)]
    med = {}
    for row in ROWS:
        vals = [s[row] for s in sessions]
        med[row] = median(vals)
        text.append("  %-16s %9.4f   (sessions: %s)" % (row, med[row], ", ".join("%.4f" % t for t in vals)))
    host = lambda m: "%.1f .. %.1f" % (min(s["host " + m] for s in sessions), max(s["host " + m] for s in sessions))
    text.append("  fit / copy %.1f; one / fit %.2f; fit256 / fit %.2f; random4096 / fit %.2f; fit x8 per step / fit %.2f; host, the sessions' range in ms: fit %s, one %s"
                % (med["fit"] / med["copy"], med["one"] / med["fit"], med["fit256"] / med["fit"], med["random4096"] / med["fit"], med["fit x8"] / STEPS / med["fit"],
                   host("fit"), host("one")))
    text = "\n".join(text) + "\n"
    sys.stdout.write(text)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
