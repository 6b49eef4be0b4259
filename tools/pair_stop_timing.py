#!/usr/bin/env python3
"""What the per-pair stop (hsflow_set_pair_termination) costs a batched context.

16 pairs of 600x480 in one context, lambda 0.1, ITER|EPS with epsilon 1e-6, 100 sweeps, asynchronous graph solves:
  (a) 16 translating pairs -- nothing stops: a parent build of the library (--parent, optional), this build with the
      switch off, this build with the switch on;
  (b) 12 pairs of identical frames (they stop after sweep 1) + 4 translating pairs: switch off and on, and the parent
      build with the switch on where it has one.
Two figures per case, in ms per solve of the whole batch, five blocks each, the cases taking turns inside every block:
  stream   300 solves enqueued back to back (each takes the owed check of the one before over), one synchronize;
  settled  100 solves, each followed by synchronize -- the early-stop check settled every time: the re-runs of (b).
The libraries are driven through ctypes directly, so that a parent build without the new entry points can stand beside
this one in the same process.

usage: python tools/pair_stop_timing.py [--parent path/to/parent/libhsflow.so] [--blocks 5]
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import opticalflowhs_amd as hs  # noqa: E402  (torch's HIP runtime first, the structs, the shipped library's path)
from opticalflowhs_amd import synth  # noqa: E402

W, H, N, SWEEPS, LAM, EPSILON = 600, 480, 16, 100, 0.1, float(np.float32(1e-6))
_vp, _i, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t


def open_lib(path):
    lib = ctypes.CDLL(path)
    lib.hsflow_create.argtypes = [ctypes.POINTER(_vp), _i, _i, _i, _i, _vp, _i]
    lib.hsflow_set_frames_u8.argtypes = [_vp, _i, _vp, _sz, _vp, _sz]
    lib.hsflow_solve_async.argtypes = [_vp, ctypes.POINTER(hs._lib.HsflowParams)]
    lib.hsflow_synchronize.argtypes = [_vp]
    lib.hsflow_destroy.argtypes = [_vp]
    lib.hsflow_get_info.argtypes = [_vp, ctypes.POINTER(hs._lib.HsflowInfo)]
    lib.hsflow_last_error.argtypes = [_vp]
    lib.hsflow_last_error.restype = ctypes.c_char_p
    if hasattr(lib, "hsflow_set_pair_termination"):
        lib.hsflow_set_pair_termination.argtypes = [_vp, _i]
    return lib


class Case(object):
    def __init__(self, name, lib, pairs, per_pair):
        self.name, self.lib, self.h = name, lib, _vp()
        self.check(lib.hsflow_create(ctypes.byref(self.h), 0, W, H, len(pairs), None, 1))
        for i, (A, B) in enumerate(pairs):
            A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
            self.check(lib.hsflow_set_frames_u8(self.h, i, A.ctypes.data, W, B.ctypes.data, W))
        if per_pair:
            self.check(lib.hsflow_set_pair_termination(self.h, 1))
        self.p = hs.make_params(lam=LAM, max_iter=SWEEPS, epsilon=EPSILON, term_type=hs.TERM_ITER | hs.TERM_EPS, use_graph=True)
        self.stream, self.settled = [], []

    def check(self, st):
        if st:
            raise RuntimeError("%s: status %d: %s" % (self.name, st, (self.lib.hsflow_last_error(self.h) or b"").decode()))

    def run_stream(self, n):
        for _ in range(n):
            self.check(self.lib.hsflow_solve_async(self.h, ctypes.byref(self.p)))
        self.check(self.lib.hsflow_synchronize(self.h))

    def run_settled(self, n):
        for _ in range(n):
            self.check(self.lib.hsflow_solve_async(self.h, ctypes.byref(self.p)))
            self.check(self.lib.hsflow_synchronize(self.h))

    def info(self):
        i = hs._lib.HsflowInfo()
        i.struct_size = ctypes.sizeof(i)
        self.check(self.lib.hsflow_get_info(self.h, ctypes.byref(i)))
        return i

    def close(self):
        self.lib.hsflow_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="libhsflow.so of the parent commit: case (a), and (b) with the switch on if it has the switch")
    ap.add_argument("--blocks", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing to measure")
    moving = [synth.translating_pair(W, H, seed=20 + s) for s in range(N)]
    still = [(A, A.copy()) for A, _ in moving[:12]]
    mixed = still + moving[12:]
    this = open_lib(hs._lib.LIB_PATH)
    cases = []
    parent = open_lib(args.parent) if args.parent else None
    if parent:
        cases.append(Case("(a) parent", parent, moving, False))
    cases += [Case("(a) switch off", this, moving, False), Case("(a) switch on", this, moving, True),
              Case("(b) switch off", this, mixed, False), Case("(b) switch on", this, mixed, True)]
    if parent and hasattr(parent, "hsflow_set_pair_termination"):
        cases.insert(-1, Case("(b) parent on", parent, mixed, True))
    for c in cases:   # warm-up: every shape, the graph capture, the clocks
        c.run_stream(100)
        c.run_settled(20)
    for _ in range(args.blocks):
        for c in cases:
            t0 = time.perf_counter()
            c.run_stream(300)
            c.stream.append((time.perf_counter() - t0) / 300 * 1e3)
        for c in cases:
            t0 = time.perf_counter()
            c.run_settled(100)
            c.settled.append((time.perf_counter() - t0) / 100 * 1e3)
    print("# %d pairs of %dx%d, lambda %g, ITER|EPS eps %g, %d sweeps, async graph solves; ms per solve of the batch" % (N, W, H, LAM, EPSILON, SWEEPS))
    for c in cases:
        i = c.info()
        for what, t in (("stream ", c.stream), ("settled", c.settled)):
            print("%-15s %s  min %.4f  median %.4f  max %.4f  spread %.4f   blocks %s   iterations_done %d eps_rerun %d launches %d"
                  % (c.name, what, min(t), sorted(t)[len(t) // 2], max(t), max(t) - min(t), " ".join("%.4f" % x for x in t),
                     i.iterations_done, i.eps_rerun, i.jacobi_launches))
        c.close()


if __name__ == "__main__":
    main()
