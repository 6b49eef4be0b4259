#!/usr/bin/env python3
"""What a flow picture's JPEG file costs when the pairs of a context are drawn and encoded as a batch
(hsflow_render_flow_jpeg_batch[_device]) against one by one (hsflow_render_flow_jpeg), DESIGN.md 4.9 "batched".  Two
cases, those of tools/jpeg_time.py: the 1920x1080 seed-1 pair after 100 sweeps and the reference's 600x480 city pair as
its CPU route solves it, `cv` preset, quality 95, in every pair of a 32-pair context.  Medians of --reps timed
repetitions after warm-up.
  batch    one call for n pairs, n in 1 .. 32, for every candidate HSFLOW_JPEG_BATCH_MAX (the environment variable of the
           same name), per file: a host clock around the synchronous form, device events around the device form;
  single   n hsflow_render_flow_jpeg calls back to back, a host clock, per file; the launches of the device form
           (hsflow_render_flow_jpeg_device) and of the encode alone (C of tools/jpeg_time.py) between device events -- by
           this tree's library and, with --parent ROOT (a checkout of the parent commit, built), by the parent's, in
           alternating child processes, --rounds times each: the spread of the parent's repeated medians is what a
           difference has to exceed;
  chain    9 files in -> 8 files out: hsflow_set_sequence_jpeg + one solve + hsflow_render_flow_jpeg_batch against
           hsflow_set_frames_jpeg + solve + hsflow_render_flow_jpeg pair by pair, host clocks, with the bytes that cross.
Every measurement runs in a child process of its own under a time limit; after one that failed nothing more is started.
   usage: tools/jpeg_batch_time.py [--reps 30] [--rounds 3] [--parent ROOT] [--out profiles/jpeg_batch_time.txt]"""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NS = (1, 2, 4, 8, 16, 32)
ALL_CANDIDATES = (4, 8, 16, 32)
CASES = ("1080p", "city")
ENV_MAX = "HSFLOW_JPEG_BATCH_MAX"
QUALITY = 95
with open(os.path.join(ROOT, "include", "hsflow.h")) as _f:
    HEADER_MAX = int(re.search(r"^#define HSFLOW_JPEG_BATCH_MAX\s+(\d+)", _f.read(), re.M).group(1))
# the environment variable reaches 1 .. the header's constant: a candidate above it needs a build with that constant
CANDIDATES = tuple(m for m in ALL_CANDIDATES if m <= HEADER_MAX)


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
    """(A, B, blur, solve parameters) of tools/jpeg_time.py's two cases."""
    import numpy as np
    from opticalflowhs_amd import synth
    if case == "1080p":
        A, B = synth.translating_pair(1920, 1080, seed=1)
        return A, B, False, dict(lam=1.0, max_iter=100, term_type=hs.TERM_ITER)
    g = os.path.join(ROOT, "tests", "golden")
    A, B = read_pgm(os.path.join(g, "city_1_gray.pgm")), read_pgm(os.path.join(g, "city_2_gray.pgm"))
    return A, B, True, dict(lam=0.1, max_iter=10, term_type=hs.TERM_ITER | hs.TERM_EPS, epsilon=float(np.float32(1e-6)))


def the_files(hs, case):
    """Two consecutive frames as JPEG files: the chain's input."""
    import numpy as np
    if case == "1080p":
        A, B, _, _ = the_case(hs, case)
        return [hs.encode_jpeg(np.ascontiguousarray(np.repeat(X[:, :, None], 3, axis=2)), QUALITY) for X in (A, B)]
    out = []
    for k in (1, 2):
        with open(os.path.join(ROOT, "tests", "golden", "ref_city_%d.jpg" % k), "rb") as f:
            out.append(f.read())
    return out


def set_pairs(ctx, A, B, blur, n):
    for p in range(n):
        if blur:
            ctx.set_frames_gray_blur(A, B, pair=p)
        else:
            ctx.set_frames(A, B, pair=p)


def host_timed(fn, reps):
    out = []
    for i in range(reps + 3):
        t0 = time.perf_counter()
        fn()
        if i >= 3:
            out.append((time.perf_counter() - t0) * 1e3)
    return median(out)


def event_timed(stream, fn, reps):
    import torch
    out = []
    for i in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        if i >= 3:
            out.append(e0.elapsed_time(e1))
    return median(out)


def run_child(mode, pkg_root, reps):
    import numpy as np
    import torch
    sys.path.insert(0, pkg_root)
    import opticalflowhs_amd as hs
    L = hs._lib.load()
    nmax = max(NS)
    for case in CASES:
        A, B, blur, kw = the_case(hs, case)
        H, W = A.shape
        p = hs.make_params(**kw)
        rp = hs.make_render_params("cv")
        s = torch.cuda.Stream()
        if mode in ("batch", "single"):
            with hs.HSFlow(W, H, 1, stream=s.cuda_stream) as one:   # the file, and the capacity the buffers get
                set_pairs(one, A, B, blur, 1)
                one.solve(p)
                want = one.render_jpeg("cv", quality=QUALITY)
            cap = (len(want) * 5 // 4 + 4095) // 4096 * 4096
            print("file %s bytes=%d" % (case, len(want)))
            host = hs.pinned_empty((nmax, cap), np.uint8)
            hp = (ctypes.c_void_p * nmax)(*[host[i].ctypes.data for i in range(nmax)])
            hn = (ctypes.c_size_t * nmax)()
            dev = torch.zeros((nmax, cap), dtype=torch.uint8, device="cuda")
            dp = (ctypes.c_void_p * nmax)(*[dev[i].data_ptr() for i in range(nmax)])
            dn = torch.zeros(nmax, dtype=torch.int64, device="cuda")
            pic = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
        if mode == "batch":
            with hs.HSFlow(W, H, nmax, stream=s.cuda_stream) as ctx:
                set_pairs(ctx, A, B, blur, nmax)
                ctx.solve(p)
                for m in CANDIDATES:
                    os.environ[ENV_MAX] = str(m)
                    for n in NS:
                        def sync_form():
                            assert L.hsflow_render_flow_jpeg_batch(ctx._h, 0, n, ctypes.byref(rp), QUALITY, hp, cap, hn) == 0

                        def device_form():
                            assert L.hsflow_render_flow_jpeg_batch_device(ctx._h, 0, n, ctypes.byref(rp), QUALITY, dp, cap, ctypes.c_void_p(dn.data_ptr())) == 0

                        print("batch_host %s max=%d n=%d per_file_ms=%.4f" % (case, m, n, host_timed(sync_form, reps) / n))
                        print("batch_dev %s max=%d n=%d per_file_ms=%.4f" % (case, m, n, event_timed(s, device_form, reps) / n))
                        ctx.synchronize()
                        for i in (0, n - 1):
                            assert host[i, :hn[i]].tobytes() == want and dev[i, :int(dn[i].item())].cpu().numpy().tobytes() == want, (m, n, i)
                os.environ.pop(ENV_MAX, None)
        elif mode == "single":
            with hs.HSFlow(W, H, nmax, stream=s.cuda_stream) as ctx:
                set_pairs(ctx, A, B, blur, nmax)
                ctx.solve(p)
                n1 = ctypes.c_size_t()
                for n in NS:
                    def singles():
                        for i in range(n):
                            assert L.hsflow_render_flow_jpeg(ctx._h, i, ctypes.byref(rp), QUALITY, hp[i], cap, ctypes.byref(n1)) == 0

                    print("single_host %s n=%d per_file_ms=%.4f" % (case, n, host_timed(singles, reps) / n))
                assert host[nmax - 1, :n1.value].tobytes() == want

                def device_form():
                    assert L.hsflow_render_flow_jpeg_device(ctx._h, 0, ctypes.byref(rp), QUALITY, dp[0], cap, ctypes.c_void_p(dn.data_ptr())) == 0

                def encode_alone():
                    assert L.hsflow_jpeg_encode_device(ctx._h, ctypes.c_void_p(pic.data_ptr()), 3 * W, QUALITY, dp[0], cap, ctypes.c_void_p(dn.data_ptr())) == 0

                print("single_dev %s per_file_ms=%.4f" % (case, event_timed(s, device_form, reps)))
                assert L.hsflow_render_flow_device(ctx._h, 0, ctypes.byref(rp), ctypes.c_void_p(pic.data_ptr()), 3 * W) == 0
                print("single_C %s per_file_ms=%.4f" % (case, event_timed(s, encode_alone, reps)))
                assert dev[0, :int(dn[0].item())].cpu().numpy().tobytes() == want
        else:   # the chain: 9 files in, 8 files out
            f = the_files(hs, case)
            files = [f[k & 1] for k in range(9)]
            bound = hs.jpeg_bound(W, H)
            if mode == "chain_batch":
                with hs.HSFlow(W, H, 8, own_stream=True) as ctx:
                    ctx.set_pair_termination(True)   # every pair stops as it does alone
                    out = []

                    def chain():
                        ctx.set_sequence_jpeg(files, blur=blur)
                        ctx.solve(p)
                        out[:] = ctx.render_jpeg_batch("cv", quality=QUALITY)

                    t = host_timed(chain, max(reps // 3, 5))
            else:
                with hs.HSFlow(W, H, 1, own_stream=True) as ctx:
                    out = [None] * 8

                    def chain():
                        for k in range(8):
                            ctx.set_frames_jpeg(files[k], files[k + 1], blur=blur)
                            ctx.solve(p)
                            out[k] = ctx.render_jpeg("cv", quality=QUALITY)

                    t = host_timed(chain, max(reps // 3, 5))
            print("%s %s ms=%.4f" % (mode, case, t))
            print("%s_in %s bytes=%d" % (mode, case, sum(len(x) for x in files) if mode == "chain_batch" else sum(len(files[k]) + len(files[k + 1]) for k in range(8))))
            print("%s_out %s bytes=%d" % (mode, case, sum(len(x) for x in out) + 8 * len(out)))
            print("%s_check %s crc=%d" % (mode, case, sum(sum(x[::97]) for x in out) % 1000003))


def child(mode, pkg_root, reps, limit=280):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", mode, "--pkg", pkg_root, "--reps", str(reps)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s of %s failed (%d): %s" % (mode, pkg_root, r.returncode, r.stderr[-2000:]))
    sys.stderr.write("%s of %s done\n" % (mode, pkg_root))
    sys.stderr.flush()
    out = {}
    for line in r.stdout.splitlines():
        parts = line.split()
        if len(parts) >= 2 and "=" in parts[-1]:
            out[" ".join(parts[:-1])] = float(parts[-1].split("=")[1])
    return out


def spread(xs):
    return max(xs) - min(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--pkg", default=ROOT)
    a = ap.parse_args()
    if a.child:
        run_child(a.child, a.pkg, a.reps)
        return 0
    lines = ["jpeg_batch_time (medians of %d; ms per file unless said otherwise; cv preset, quality %d; HSFLOW_JPEG_BATCH_MAX of include/hsflow.h: %d)" % (a.reps, QUALITY, HEADER_MAX)]
    if len(CANDIDATES) < len(ALL_CANDIDATES):
        lines.append("candidates above the header's constant are not measured: the environment variable reaches 1 .. %d (build with a larger constant to measure them)" % HEADER_MAX)
    try:
        b = child("batch", ROOT, a.reps)
        tree, parent, ctree, cparent = [], [], [], []
        for _ in range(a.rounds):          # alternating: tree, parent, tree, parent, ...
            tree.append(child("single", ROOT, a.reps))
            if a.parent:
                parent.append(child("single", os.path.abspath(a.parent), a.reps))
        cb = child("chain_batch", ROOT, a.reps)
        for _ in range(a.rounds):
            ctree.append(child("chain_pairwise", ROOT, a.reps))
            if a.parent:
                cparent.append(child("chain_pairwise", os.path.abspath(a.parent), a.reps))
        for case in CASES:
            lines.append("%s (file %d bytes):" % (case, b["file %s" % case]))
            for form, title in (("batch_host", "hsflow_render_flow_jpeg_batch, one call of n pairs, host clock"), ("batch_dev", "hsflow_render_flow_jpeg_batch_device, its launches, device events")):
                lines.append("  %-70s" % title + "".join("  n=%-7d" % n for n in NS))
                for m in CANDIDATES:
                    lines.append("    %-68s" % ("HSFLOW_JPEG_BATCH_MAX = %d" % m) + "".join("  %-9.4f" % b["%s %s max=%d n=%d" % (form, case, m, n)] for n in NS))
            for name, runs in (("this tree", tree), ("parent", parent)):
                for k, r in enumerate(runs):
                    lines.append("  %-70s" % ("n hsflow_render_flow_jpeg back to back, %s %d" % (name, k + 1)) + "".join("  %-9.4f" % r["single_host %s n=%d" % (case, n)] for n in NS))
            key = "batch_host %s max=%%d n=32" % case
            best = min(b[key % m] for m in CANDIDATES)
            pick = min(m for m in CANDIDATES if b[key % m] <= 1.05 * best)
            if case == "1080p":   # the one line that decides the constant (the rule is stated at 1080p)
                lines.append("  %s: per file of one synchronous call at n = 32 (32 / maximum chunks behind each other), best %.4f; the smallest maximum within 5 %% of it: %d" % (
                    "DECIDES HSFLOW_JPEG_BATCH_MAX" if len(CANDIDATES) == len(ALL_CANDIDATES) else "of the candidates measured (the constant was decided with all four)", best, pick))
            else:
                lines.append("  (for information only, the constant is chosen at 1080p) per file at n = 32: best %.4f; the smallest maximum within 5 %% of it: %d" % (best, pick))
            dkey = "batch_dev %s max=%%d n=32" % case
            dbest = min(b[dkey % m] for m in CANDIDATES)
            lines.append("  (for information) the device form's launches per file at n = 32: best %.4f; the smallest maximum within 5 %% of it: %d" % (
                dbest, min(m for m in CANDIDATES if b[dkey % m] <= 1.05 * dbest)))
            if parent:
                for form, skey, what in (("batch_host", "single_host %s n=1" % case, "one synchronous call, against the parent's hsflow_render_flow_jpeg"),
                                         ("batch_dev", "single_dev %s" % case, "the device form's launches, against the parent's hsflow_render_flow_jpeg_device")):
                    chosen = b["%s %s max=%d n=%d" % (form, case, HEADER_MAX, HEADER_MAX)]
                    ps = [r[skey] for r in parent]
                    lines.append("  claim, %s: batch per file at the header's maximum %d, n = %d: %.4f against %.4f .. %.4f (spread %.4f): %s" % (
                        what, HEADER_MAX, HEADER_MAX, chosen, min(ps), max(ps), spread(ps), "below by more than the spread" if min(ps) - chosen > spread(ps) else "NOT below by more than the spread"))
            for skey, what in (("single_C %s" % case, "the single encode's launches alone (C of tools/jpeg_time.py)"), ("single_dev %s" % case, "hsflow_render_flow_jpeg_device, its launches")):
                ts = [r[skey] for r in tree]
                text = "  %s: this tree %s" % (what, ", ".join("%.4f" % x for x in ts))
                if parent:
                    ps = [r[skey] for r in parent]
                    inside = min(ps) - spread(ps) <= median(ts) <= max(ps) + spread(ps)
                    text += "; parent %s (spread %.4f): this tree's median %.4f %s" % (", ".join("%.4f" % x for x in ps), spread(ps), median(ts), "inside the parent's range widened by its spread" if inside else (
                        "BELOW the parent's range" if median(ts) < min(ps) else "ABOVE the parent's range widened by its spread"))
                lines.append(text)
            lines.append("  9 files in -> 8 files out: hsflow_set_sequence_jpeg + one solve + hsflow_render_flow_jpeg_batch %.3f ms (%d bytes in, %d bytes out over PCIe); "
                         "8 x (hsflow_set_frames_jpeg + solve + hsflow_render_flow_jpeg): this tree %s ms%s (%d bytes in, %d bytes out); the same files: %s" % (
                             cb["chain_batch %s" % case], cb["chain_batch_in %s" % case], cb["chain_batch_out %s" % case],
                             ", ".join("%.3f" % r["chain_pairwise %s" % case] for r in ctree),
                             "; parent %s ms" % ", ".join("%.3f" % r["chain_pairwise %s" % case] for r in cparent) if cparent else "",
                             ctree[0]["chain_pairwise_in %s" % case], ctree[0]["chain_pairwise_out %s" % case],
                             all(r["chain_pairwise_check %s" % case] == cb["chain_batch_check %s" % case] for r in ctree + cparent)))
    except (RuntimeError, KeyError) as e:
        lines.append("failed: %s" % e)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if "failed" in text else 0


if __name__ == "__main__":
    sys.exit(main())
