#!/usr/bin/env python3
"""Times the mask head's 3^3 conv at dilation 2 (padding 2) in training - forward, backward-data, backward-weights - on the library
against the two paths it can be compared with, at the shipped shapes R x 256 -> 256 channels: 7^3 at R = 16 (the nuclei step), 64 (the
soma step: 2 images x 32 fg RoIs) and 300 (DETECTIONS_PER_IM), and 14^3 at R = 16.  In one process, alternating:

  forward  m3d     PackedConv3d(W, W_PLAIN)(x, shift=b, dilation=2)                 (m3d_conv3d_forward_dilated)
           torch   F.conv3d(x, W, b, padding=2, dilation=2)                         (what compat.set_conv_dilated("torch") runs)
           dil1    PackedConv3d(W, W_PLAIN)(x, shift=b): the library's dilation-1 conv of the same shape - the same 27-tap work, so
                   the ratio to m3d is what the wider halo costs
  dgrad    m3d     PackedConv3d(W, W_DGRAD)(gy, dilation=2)
           torch   autograd's gx of the retained F.conv3d graph
           dil1    PackedConv3d(W, W_DGRAD)(gy)
  wgrad    m3d     ops.conv3d_wgrad(x, gy, 3, dilation=2): the tile the library chooses (m3d_conv3d_wgrad_dilated)
           t16/t8  the same on the 2 x 4 x 16 / 2 x 8 x 8 voxel tile asked for by name - the A/B behind the library's choice
           torch   autograd's gW of the retained graph
           dil1    ops.conv3d_wgrad(x, gy, 3)

Protocol of tools/bench_upconv.py: warm-up, then `--reps` repetitions with the variants alternating inside every repetition; each
measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median and spread (min ..
max) in ms.  Beside every time: the algorithmic FLOP (2 * R * V * 27 * Cin * Cout per direction), the achieved rate and its fraction of
the 157.3 TFLOP/s of v_mfma_f32_32x32x2_f32.  No threshold is set on any of it.  The record in the repository:
`--out profiles/conv_dilated_train.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
MFMA_PEAK = 157.3e12

SHAPES = [("nuclei step", 16, 256, 7), ("soma step", 64, 256, 7), ("detection", 300, 256, 7), ("14^3 grid", 16, 256, 14)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--shapes", type=int, nargs="*", default=None, help="indices into the shape list (default: all)")
    ap.add_argument("--out", default=None, help="also write the table to this file (rewritten after every shape)")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from m3d import ops
    assert torch.cuda.is_available(), "bench_conv_dilated needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    def measure(variants):
        times = {v: [] for v, _ in variants}
        for i in range(a.warmup + a.reps):
            order = variants[i % len(variants):] + variants[:i % len(variants)]
            for v, fn in order:
                t = timed(fn)
                if i >= a.warmup:
                    times[v].append(t)
        return {v: (statistics.median(t), min(t), max(t)) for v, t in times.items()}

    def report(name, R, r, direction, res, flop):
        for v, (med, lo, hi) in res.items():
            say("%-11s %4d %2d^3 %-7s %-5s | %-28s | %7.2f | %7.2f %5.1f%%"
                % (name, R, r, direction, v, "%.3f (%.3f .. %.3f)" % (med, lo, hi), flop / 1e9, flop / med / 1e9, 100.0 * flop / (med * 1e-3) / MFMA_PEAK))

    def compare(name, what, res, new, old):
        (ma, la, ha), (mb, lb, hb) = res[new], res[old]
        sa, sb = ha - la, hb - lb
        verdict = ("%s is faster beyond the spreads" % new if ma < mb - (sa + sb) else
                   "%s is SLOWER beyond the spreads" % new if ma > mb + (sa + sb) else "the two do NOT separate beyond the spreads")
        say("# %s, %s: %s %.3f ms against %s %.3f ms = x%.2f, spreads %.3f + %.3f ms: %s" % (name, what, new, ma, old, mb, mb / ma, sa, sb, verdict))

    say("# 3^3 conv, dilation 2, padding 2, fp32, in training: x [R,256,r,r,r], W [256,256,3,3,3], gy [R,256,r,r,r]")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# GFLOP: 2 R r^3 27 Cin Cout, per direction; TFLOP/s at the median and its share of the 157.3 TFLOP/s fp32 MFMA bound")
    say("%-11s %4s %4s %-7s %-5s | %-28s | %7s | %7s %6s" % ("shape", "R", "grid", "pass", "path", "ms per call", "GFLOP", "TFLOP/s", "of peak"))
    torch.manual_seed(0)
    for i, (name, R, Cc, r) in enumerate(SHAPES):
        if a.shapes is not None and i not in a.shapes:
            continue
        x = torch.randn(R, Cc, r, r, r, device="cuda")
        w = torch.randn(Cc, Cc, 3, 3, 3, device="cuda") * (2.0 / (27 * Cc)) ** 0.5
        b = torch.randn(Cc, device="cuda") * 0.1
        gy = torch.randn(R, Cc, r, r, r, device="cuda")
        flop = 2.0 * R * r ** 3 * 27 * Cc * Cc
        plain, dg = ops.PackedConv3d(w, ops.W_PLAIN), ops.PackedConv3d(w, ops.W_DGRAD)
        plan = ops.conv3d_wgrad_dilated_plan(R, Cc, Cc, r, r, r)
        say("# %s: the library's wgrad tile is 2 x %d x %d, %d split-K slots" % (name, plan["tile_y"], plan["tile_x"], plan["slots"]))
        res = measure((("m3d", lambda: plain(x, shift=b, dilation=2)), ("torch", lambda: F.conv3d(x, w, b, 1, 2, 2)),
                       ("dil1", lambda: plain(x, shift=b))))
        report(name, R, r, "forward", res, flop)
        compare(name, "forward", res, "m3d", "torch")
        compare(name, "forward", res, "m3d", "dil1")
        xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        yt = F.conv3d(xg, wg, b, 1, 2, 2)
        res = measure((("m3d", lambda: dg(gy, dilation=2)), ("torch", lambda: torch.autograd.grad(yt, xg, gy, retain_graph=True)),
                       ("dil1", lambda: dg(gy))))
        report(name, R, r, "dgrad", res, flop)
        compare(name, "dgrad", res, "m3d", "torch")
        compare(name, "dgrad", res, "m3d", "dil1")
        res = measure((("m3d", lambda: ops.conv3d_wgrad(x, gy, 3, dilation=2)), ("t16", lambda: ops.conv3d_wgrad(x, gy, 3, dilation=2, tile_x=16)),
                       ("t8", lambda: ops.conv3d_wgrad(x, gy, 3, dilation=2, tile_x=8)),
                       ("torch", lambda: torch.autograd.grad(yt, wg, gy, retain_graph=True)), ("dil1", lambda: ops.conv3d_wgrad(x, gy, 3))))
        report(name, R, r, "wgrad", res, flop)
        compare(name, "wgrad", res, "m3d", "torch")
        compare(name, "wgrad", res, "m3d", "dil1")
        compare(name, "wgrad", res, "t8", "t16")
        del x, w, b, gy, plain, dg, xg, wg, yt
        torch.cuda.empty_cache()
        flush()


if __name__ == "__main__":
    main()
