#!/usr/bin/env python3
"""What a JPEG file costs when files are decoded as a batch (hsflow_jpeg_decode_batch_device) against one by one
(hsflow_jpeg_decode_device), DESIGN.md 4.10 "batched".  Two pictures: the 1080p file of tools/jpegd_time.py
(self-encoded at quality 95) and ref_city_1.jpg.  Medians of --reps timed repetitions after warm-up.
  batch   device events around ONE batch call of n copies of the file (staging copy, memsets and launches included),
          n in 1 .. 32, for every candidate HSFLOW_JPEGD_BATCH_MAX (the environment variable of the same name), per file;
  single  device events around n single decodes enqueued back to back, per file -- by this tree's library and, with
          --parent ROOT (a checkout of the parent commit, built), by the parent's, in alternating child processes,
          --rounds times each: the spread of the parent's repeated medians is what a difference has to exceed;
  seq     hsflow_set_sequence_jpeg of 9 frames against 8 hsflow_set_frames_jpeg, host clocks (both synchronous);
  pipe    PairPipeline.submit_jpeg at depth 6 / lanes 2 against push_frame_jpeg + solve in a loop, host clocks per pair.
Every measurement runs in a child process of its own under a time limit; after one that failed nothing more is started.
   usage: tools/jpegd_batch_time.py [--reps 30] [--rounds 3] [--parent ROOT] [--out profiles/jpegd_batch_time.txt]"""
import argparse
import ctypes
import os
import re
import subprocess
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
NS = (1, 2, 4, 8, 16, 32)
CANDIDATES = (4, 8, 16, 32)
PICS = ("1080p", "city")
ENV_MAX = "HSFLOW_JPEGD_BATCH_MAX"
with open(os.path.join(ROOT, "include", "hsflow.h")) as _f:
    HEADER_MAX = int(re.search(r"^#define HSFLOW_JPEGD_BATCH_MAX\s+(\d+)", _f.read(), re.M).group(1))


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n & 1 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def the_file(hs, pic):
    import numpy as np
    from opticalflowhs_amd import synth
    if pic == "1080p":
        A, _ = synth.translating_pair(1920, 1080, seed=1)
        return hs.encode_jpeg(np.ascontiguousarray(np.repeat(A[:, :, None], 3, axis=2)), 95)
    with open(os.path.join(ROOT, "tests", "golden", "ref_city_1.jpg"), "rb") as f:
        return f.read()


def timed(stream, fn, reps):
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


def host_timed(fn, reps):
    out = []
    for i in range(reps + 3):
        t0 = time.perf_counter()
        fn()
        if i >= 3:
            out.append((time.perf_counter() - t0) * 1e3)
    return median(out)


def run_child(mode, pkg_root, reps):
    import numpy as np
    import torch
    sys.path.insert(0, pkg_root)
    import opticalflowhs_amd as hs
    L = hs._lib.load()
    for pic in PICS:
        data = the_file(hs, pic)
        info = hs.jpeg_read_header(data)
        W, H = info["width"], info["height"]
        buf = np.frombuffer(data, np.uint8)
        want = hs.jpeg_decode_host(data, "bgr")
        nmax = max(NS)
        dst = torch.zeros((nmax, H, W, 3), dtype=torch.uint8, device="cuda")
        words = torch.zeros(nmax, dtype=torch.int32, device="cuda")
        s = torch.cuda.Stream()
        if mode == "single":
            with hs.HSFlow(W, H, stream=s.cuda_stream) as ctx:
                def singles(n):
                    for i in range(n):
                        assert L.hsflow_jpeg_decode_device(ctx._h, ctypes.c_void_p(buf.ctypes.data), buf.size, 0, ctypes.c_void_p(dst[i].data_ptr()), 3 * W,
                                                           ctypes.c_void_p(words.data_ptr() + 4 * i)) == 0
                for n in NS:
                    t = timed(s, lambda: singles(n), reps)
                    print("single %s n=%d per_file_ms=%.4f" % (pic, n, t / n))
                assert np.array_equal(dst[nmax - 1].cpu().numpy(), want) and not words.any().item()
            with hs.HSFlow(W, H, 8, own_stream=True) as ctx:
                def eight():
                    for k in range(8):
                        ctx.set_frames_jpeg(data, data, blur=True, pair=k)
                print("seq8 %s set_frames_jpeg_x8_ms=%.4f" % (pic, host_timed(eight, max(reps // 3, 5))))
            with hs.HSFlow(W, H, own_stream=True) as ctx:
                p = hs.make_params(lam=1.0, max_iter=100, term_type=hs.TERM_ITER)
                ctx.set_frames_jpeg(data, data, blur=True)

                def push():
                    ctx.push_frame_jpeg(data, blur=True)
                    ctx.solve(p)
                print("loop %s push_frame_jpeg_solve_ms=%.4f" % (pic, host_timed(push, reps)))
        else:
            files = (ctypes.c_void_p * nmax)(*[buf.ctypes.data] * nmax)
            sizes = (ctypes.c_size_t * nmax)(*[buf.size] * nmax)
            pix = (ctypes.c_void_p * nmax)(*[dst[i].data_ptr() for i in range(nmax)])
            with hs.HSFlow(W, H, stream=s.cuda_stream) as ctx:
                for m in CANDIDATES:
                    os.environ[ENV_MAX] = str(m)
                    for n in NS:
                        t = timed(s, lambda: L.hsflow_jpeg_decode_batch_device(ctx._h, files, sizes, n, 0, pix, 3 * W, ctypes.c_void_p(words.data_ptr())), reps)
                        print("batch %s max=%d n=%d per_file_ms=%.4f" % (pic, m, n, t / n))
                    assert not words.any().item() and all(np.array_equal(dst[i].cpu().numpy(), want) for i in (0, nmax - 1)), m
                os.environ.pop(ENV_MAX, None)
            with hs.HSFlow(W, H, 8, own_stream=True) as ctx:
                print("seq9 %s set_sequence_jpeg_9_ms=%.4f" % (pic, host_timed(lambda: ctx.set_sequence_jpeg([data] * 9, blur=True), max(reps // 3, 5))))
            with hs.PairPipeline(W, H, depth=6, lanes=2) as pl:
                p = hs.make_params(lam=1.0, max_iter=100, term_type=hs.TERM_ITER)

                def stream(npairs=24):
                    for _ in range(npairs):
                        pl.submit_jpeg(data, data, blur=True, params=p)
                    pl.drain()
                print("pipe %s submit_jpeg_per_pair_ms=%.4f" % (pic, host_timed(stream, max(reps // 3, 5)) / 24))


def child(mode, pkg_root, reps, limit=280):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode, "--pkg", pkg_root, "--reps", str(reps)], capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        raise RuntimeError("%s of %s failed (%d): %s" % (mode, pkg_root, r.returncode, r.stderr[-2000:]))
    sys.stderr.write("%s of %s done\n" % (mode, pkg_root))
    sys.stderr.flush()
    out = {}
    for line in r.stdout.splitlines():
        parts = line.split()
        out[" ".join(parts[:-1])] = float(parts[-1].split("=")[1])
    return out


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
    lines = ["jpegd_batch_time (medians of %d; ms per file unless said otherwise)" % a.reps]
    try:
        b = child("batch", ROOT, a.reps)
        tree, parent = [], []
        for _ in range(a.rounds):          # alternating: tree, parent, tree, parent, ...
            tree.append(child("single", ROOT, a.reps))
            if a.parent:
                parent.append(child("single", os.path.abspath(a.parent), a.reps))
        for pic in PICS:
            lines.append("%s:" % pic)
            lines.append("  batch, one call of n files        " + "".join("  n=%-7d" % n for n in NS))
            for m in CANDIDATES:
                lines.append("    HSFLOW_JPEGD_BATCH_MAX = %-2d      " % m + "".join("  %-9.4f" % b["batch %s max=%d n=%d" % (pic, m, n)] for n in NS))
            for name, runs in (("this tree", tree), ("parent", parent)):
                for k, r in enumerate(runs):
                    lines.append("  n singles back to back, %-9s %d" % (name, k + 1) + "".join("  %-9.4f" % r["single %s n=%d" % (pic, n)] for n in NS))
            best = min(b["batch %s max=%d n=%d" % (pic, m, 32)] for m in CANDIDATES)
            pick = min(m for m in CANDIDATES if b["batch %s max=%d n=%d" % (pic, m, 32)] <= 1.05 * best)
            if pic == "1080p":  # the one line that decides the constant (the rule is stated at 1080p)
                lines.append("  DECIDES HSFLOW_JPEGD_BATCH_MAX: per file at n = 32 (32 / maximum chunks behind each other), best %.4f; the smallest maximum within 5 %% of it: %d" % (best, pick))
            else:
                lines.append("  (for information only, the constant is chosen at 1080p) per file at n = 32: best %.4f; the smallest maximum within 5 %% of it: %d" % (best, pick))
            if parent:
                chosen = b["batch %s max=%d n=%d" % (pic, HEADER_MAX, 32)]
                ps1 = [r["single %s n=1" % (pic,)] for r in parent]
                lines.append("  claim: batch per file at the header's maximum %d, n = 32: %.4f against the parent's one file alone %.4f .. %.4f (spread %.4f): %s" % (
                    HEADER_MAX, chosen, min(ps1), max(ps1), max(ps1) - min(ps1), "below by more than the spread" if min(ps1) - chosen > max(ps1) - min(ps1) else "NOT below by more than the spread"))
            if parent:
                ps = [r["single %s n=1" % (pic,)] for r in parent]
                lines.append("  parent, one file alone: medians %s, spread %.4f" % (", ".join("%.4f" % x for x in ps), max(ps) - min(ps)))
            lines.append("  hsflow_set_sequence_jpeg, 9 frames: %.3f ms; 8 x hsflow_set_frames_jpeg: %s ms (this tree)%s" % (
                b["seq9 %s" % pic], ", ".join("%.3f" % r["seq8 %s" % pic] for r in tree),
                "; %s ms (parent)" % ", ".join("%.3f" % r["seq8 %s" % pic] for r in parent) if parent else ""))
            lines.append("  PairPipeline.submit_jpeg depth 6 / lanes 2, 100 sweeps: %.3f ms per pair; push_frame_jpeg + solve in a loop: %s ms (this tree)%s" % (
                b["pipe %s" % pic], ", ".join("%.3f" % r["loop %s" % pic] for r in tree),
                "; %s ms (parent)" % ", ".join("%.3f" % r["loop %s" % pic] for r in parent) if parent else ""))
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
