#!/usr/bin/env python3
"""What a pair of input frames costs as JPEG files, decoded on the device against on the host.  Per case:
  A  the route without the device decoder: hsflow_jpeg_decode_host of both files into page-locked memory +
     hsflow_set_frames_bgr8(blur 1) from there, host clocks;
  B  hsflow_set_frames_jpeg(blur 1), a host clock around the synchronous call;
  C  the launches of ONE decode alone (hsflow_jpeg_decode_device) between device events, for every subsequence length
     in --subseq (the environment variable HSFLOW_JPEGD_SUBSEQ_BITS per call);
  the files' sizes and the bytes that cross PCIe in A and in B.
Medians of --reps timed repetitions after warm-up; A and B alternate within one process and must leave identical planes
(checked, and C's pictures against the host rule).  Every case runs in a child process of its own under a time limit;
after a case that failed nothing more is started.
   usage: tools/jpegd_time.py [--reps 30] [--out profiles/jpegd_time.txt] [--label TEXT]"""
import argparse
import ctypes
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
CASES = ("1080p", "city")
SUBSEQ = (128, 256, 512, 1024, 2048, 4096)


def median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n & 1 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def run_case(case, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import opticalflowhs_amd as hs
    from opticalflowhs_amd import synth
    L = hs._lib.load()
    if case == "1080p":   # the benchmark's seed-1 pair as gray-valued colour pictures, written by the host encoder at 95
        A, B = synth.translating_pair(1920, 1080, seed=1)
        files = [hs.encode_jpeg(np.ascontiguousarray(np.repeat(f[:, :, None], 3, axis=2)), 95) for f in (A, B)]
        what = "1920x1080 seed-1 pair, self-encoded at quality 95 (4:2:0)"
    else:                 # the reference's own inputs
        g = os.path.join(ROOT, "tests", "golden")
        files = [open(os.path.join(g, "ref_city_%d.jpg" % k), "rb").read() for k in (1, 2)]
        what = "the reference's city pair (ref_city_1.jpg, ref_city_2.jpg)"
    info = hs.jpeg_read_header(files[0])
    W, H = info["width"], info["height"]
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    pics = [hs.pinned_empty((H, W, 3), np.uint8) for _ in range(2)]
    s = torch.cuda.Stream()
    with hs.HSFlow(W, H, stream=s.cuda_stream) as ctx:
        h = ctx._h

        def route_a():
            for b, p in zip(bufs, pics):
                assert L.hsflow_jpeg_decode_host(ctypes.c_void_p(b.ctypes.data), b.size, 0, ctypes.c_void_p(p.ctypes.data), 3 * W, None) == 0
            assert L.hsflow_set_frames_bgr8(h, 0, ctypes.c_void_p(pics[0].ctypes.data), 3 * W, ctypes.c_void_p(pics[1].ctypes.data), 3 * W, 1) == 0

        def route_b():
            assert L.hsflow_set_frames_jpeg(h, 0, ctypes.c_void_p(bufs[0].ctypes.data), bufs[0].size, ctypes.c_void_p(bufs[1].ctypes.data), bufs[1].size, 1) == 0

        ta, tb, tdec = [], [], []
        for i in range(reps + 3):
            t0 = time.perf_counter(); route_a(); t1 = time.perf_counter()
            fa = [x.copy() for x in ctx.frames()]
            t2 = time.perf_counter(); route_b(); t3 = time.perf_counter()
            fb = ctx.frames()
            assert all(np.array_equal(x, y) for x, y in zip(fa, fb)), "routes A and B leave different planes"
            t4 = time.perf_counter()
            assert L.hsflow_jpeg_decode_host(ctypes.c_void_p(bufs[0].ctypes.data), bufs[0].size, 0, ctypes.c_void_p(pics[0].ctypes.data), 3 * W, None) == 0
            t5 = time.perf_counter()
            if i >= 3:
                ta.append((t1 - t0) * 1e3); tb.append((t3 - t2) * 1e3); tdec.append((t5 - t4) * 1e3)
        print("%s: %s" % (case, what))
        print("  files %d + %d bytes (scan %d + %d), %s, picture %d bytes" % (len(files[0]), len(files[1]), info["scan_bytes"], hs.jpeg_read_header(files[1])["scan_bytes"],
                                                                           "%dx%d luma sampling" % (info["h_samp"], info["v_samp"]), 3 * W * H))
        print("  A host decode x2 + set_frames_bgr8(blur)   %9.3f ms   (one host decode %.3f ms)   PCIe in: %d bytes" % (median(ta), median(tdec), 2 * 3 * W * H))
        print("  B hsflow_set_frames_jpeg(blur)              %9.3f ms   PCIe in: about %d bytes (segments + tables)" % (median(tb), info["scan_bytes"] + hs.jpeg_read_header(files[1])["scan_bytes"] + 2 * 6144))
        want = hs.jpeg_decode_host(files[0], "bgr")
        dst = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        word = torch.zeros(1, dtype=torch.int32, device="cuda")
        for S in SUBSEQ:
            os.environ["HSFLOW_JPEGD_SUBSEQ_BITS"] = str(S)
            tc = []
            for i in range(reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                assert L.hsflow_jpeg_decode_device(h, ctypes.c_void_p(bufs[0].ctypes.data), bufs[0].size, 0, ctypes.c_void_p(dst.data_ptr()), 3 * W, ctypes.c_void_p(word.data_ptr())) == 0
                e1.record(s)
                e1.synchronize()
                if i >= 3:
                    tc.append(e0.elapsed_time(e1))
            assert int(word.item()) == 0 and np.array_equal(dst.cpu().numpy(), want), S
            print("  C one decode on the device, S = %4d         %9.3f ms   (copy, memsets and launches between device events)" % (S, median(tc)))
        os.environ.pop("HSFLOW_JPEGD_SUBSEQ_BITS", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--label", default="")
    ap.add_argument("--case", default=None)
    a = ap.parse_args()
    if a.case:
        run_case(a.case, a.reps)
        return 0
    lines = ["jpegd_time %s (medians of %d)" % (a.label, a.reps)]
    for case in CASES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case, "--reps", str(a.reps)], capture_output=True, text=True, timeout=280)
        lines.append(r.stdout.rstrip())
        if r.returncode != 0:
            lines.append("case %s failed (%d): %s" % (case, r.returncode, r.stderr[-2000:]))
            break
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if "failed" not in text else 1


if __name__ == "__main__":
    sys.exit(main())
