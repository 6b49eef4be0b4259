#!/usr/bin/env python3
"""What the pre-processing of a SEQUENCE costs: 9 resident BGR frames into a context of 8 pairs, format BGR8_BLUR, by
hsflow_set_sequence_device_ex (one launch, every frame read once) against the calls that existed before, the latter
measured on a built tree of the parent commit (--parent-root) as well as on this tree.

  seq0   this tree only: set_sequence_device, flags 0                                    -- (a)
  pairs  8 x hsflow_set_frames_device_ex(f_k, f_k+1), what hsflow_set_sequence_jpeg ran    -- (a)'s comparison leg
  seq1   this tree only: set_sequence_device, HSFLOW_SEQ_REBLUR                          -- (b)
  loop   pair 0: set_frames_device_ex(f_0, f_1); pair k >= 1: set_frames_device_ex(f_k, f_k) +
         push_frame_device_ex(f_k+1, reblur_prev = 1), the same planes by the existing calls -- (b)'s comparison leg

HIP events on the context's stream around blocks of --reps repetitions (5 blocks after a warm-up; the figure includes
what the host needs to enqueue the launches), in ms per PAIR.  Every leg runs in a fresh child process under a time limit
of its own; the legs of one size alternate, and the first child that fails ends the run.
usage: tools/pre_sequence_time.py [--out profiles/pre_sequence_time.txt] [--reps 200] [--rounds 2] [--parent-root DIR]"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
SIZES = [(1920, 1080), (600, 480)]
BLOCKS = 5
PAIRS = 8


def child(args):
    sys.path.insert(0, os.path.abspath(args.root or ROOT))
    import numpy as np
    import torch
    import opticalflowhs_amd as hs
    from opticalflowhs_amd import synth
    W, H = args.width, args.height
    gray = [synth.translating_pair(W, H, seed=3, dx=0.75 * i, dy=-0.5 * i)[1] for i in range(PAIRS + 1)]
    bgr = [torch.from_numpy(np.ascontiguousarray(np.repeat(g[:, :, None], 3, axis=2))).cuda() for g in gray]
    s = torch.cuda.Stream()
    with hs.HSFlow(W, H, PAIRS, stream=s.cuda_stream) as ctx:
        if args.child == "seq0":
            def once():
                ctx.set_sequence_device(bgr, "bgr_blur")
        elif args.child == "seq1":
            def once():
                ctx.set_sequence_device(bgr, "bgr_blur", reblur=True)
        elif args.child == "pairs":
            def once():
                for k in range(PAIRS):
                    ctx.set_frames_device(bgr[k], bgr[k + 1], "bgr_blur", pair=k)
        else:
            def once():
                ctx.set_frames_device(bgr[0], bgr[1], "bgr_blur", pair=0)
                for k in range(1, PAIRS):
                    ctx.set_frames_device(bgr[k], bgr[k], "bgr_blur", pair=k)
                    ctx.push_frame_ex(bgr[k + 1], "bgr_blur", reblur_prev=True, pair=k)
        for _ in range(30):
            once()
        ctx.synchronize()
        blocks = []
        for _ in range(BLOCKS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(args.reps):
                once()
            e1.record(s)
            e1.synchronize()
            blocks.append(e0.elapsed_time(e1) / args.reps / PAIRS)
        ctx.synchronize()
        planes = [ctx.frames(k) for k in range(PAIRS)]
    import zlib
    crc = 0
    for a, b in planes:
        crc = zlib.crc32(b.tobytes(), zlib.crc32(a.tobytes(), crc))
    print("RESULT " + json.dumps({"what": args.child, "width": W, "height": H, "version": hs._lib.load().hsflow_version(), "blocks": blocks, "planes_crc": crc}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pre_sequence_time.txt"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--root", default=None)
    ap.add_argument("--parent-root", default=None, help="a tree of the parent commit, built: the comparison legs are measured on it too")
    ap.add_argument("--limit", type=int, default=180, help="seconds a child may take")
    ap.add_argument("--child", choices=["seq0", "seq1", "pairs", "loop"])
    ap.add_argument("--width", type=int)
    ap.add_argument("--height", type=int)
    args = ap.parse_args()
    if args.child:
        return child(args)
    legs = [("seq0", None), ("pairs", None), ("seq1", None), ("loop", None)]
    if args.parent_root:
        legs += [("pairs", args.parent_root), ("loop", args.parent_root)]
    runs = {}
    for W, H in SIZES:
        for _ in range(args.rounds):
            for what, root in legs:
                cmd = [sys.executable, os.path.abspath(__file__), "--child", what, "--width", str(W), "--height", str(H), "--reps", str(args.reps)] + (["--root", root] if root else [])
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)   # a child killed at its limit raises: the run ends
                line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
                if r.returncode != 0 or not line:
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    sys.exit("step %r failed (%d): nothing further is started" % (cmd[3:], r.returncode))
                res = json.loads(line[0][7:])
                key = (W, H, what, "parent" if root else "this tree")
                runs.setdefault(key, {"blocks": [], "crc": set(), "version": res["version"]})
                runs[key]["blocks"] += res["blocks"]
                runs[key]["crc"].add(res["planes_crc"])
                print("%-6s %4dx%-4d %-9s %s" % (what, W, H, key[3], " ".join("%.5f" % x for x in res["blocks"])), flush=True)
    text = ["pre_sequence_time: %d resident BGR frames into a context of %d pairs, BGR8_BLUR; HIP events on the context's stream around %d repetitions, "
            "%d blocks x %d rounds per leg, the legs alternating; ms per PAIR, median (min .. max)" % (PAIRS + 1, PAIRS, args.reps, BLOCKS, args.rounds)]

    def stat(key):
        b = sorted(runs[key]["blocks"])
        return b[len(b) // 2], b[0], b[-1]

    def row(label, key):
        if key not in runs:
            return None
        m, lo, hi = stat(key)
        text.append("    %-78s %.5f (%.5f .. %.5f)   ABI 0.%d" % (label, m, lo, hi, runs[key]["version"] % 1000))
        return m, lo, hi

    for W, H in SIZES:
        text.append("%dx%d:" % (W, H))
        for new, old, title, new_label, old_label in (
                ("seq0", "pairs", "(a) flags 0", "hsflow_set_sequence_device_ex, flags 0, one launch", "8 x hsflow_set_frames_device_ex(f_k, f_k+1)"),
                ("seq1", "loop", "(b) HSFLOW_SEQ_REBLUR", "hsflow_set_sequence_device_ex, HSFLOW_SEQ_REBLUR, one launch",
                 "set_frames_device_ex(f_0, f_1); 7 x (set_frames_device_ex(f_k, f_k) + push_frame_device_ex(f_k+1, 1))")):
            text.append("  %s" % title)
            a = row(new_label + ", this tree", (W, H, new, "this tree"))
            row(old_label + ", this tree", (W, H, old, "this tree"))
            b = row(old_label + ", parent", (W, H, old, "parent")) or stat((W, H, old, "this tree"))
            spread = max(a[2] - a[1], b[2] - b[1])
            verdict = "below by more than the spread" if a[0] + spread < b[0] else "ABOVE by more than the spread" if a[0] > b[0] + spread else "within the spread"
            text.append("    the new entry against the existing calls%s: %.5f against %.5f (spread %.5f): %s; ratio %.2f" %
                        (" on the parent" if (W, H, old, "parent") in runs else " (no parent tree given: this tree's)", a[0], b[0], spread, verdict, b[0] / a[0]))
            crcs = set()
            for who in ("this tree", "parent"):
                for what in (new, old):
                    crcs |= runs.get((W, H, what, who), {"crc": set()})["crc"]
            text.append("    the planes of all legs are the same bytes: %s" % (len(crcs) == 1))
    out = "\n".join(text) + "\n"
    print(out)
    with open(args.out, "w") as f:
        f.write(out)


if __name__ == "__main__":
    main()
