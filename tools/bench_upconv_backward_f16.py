#!/usr/bin/env python3
"""Times the backward of the mask head's ConvTranspose3d(2, 2) + ReLU on the f16 matrix cores (csrc/upconv3d_bwd_f16.hip, the "f16x2"
cut) against the fp32-input MFMA kernels of csrc/upconv3d.hip, at the shipped shape R x 256 -> 256 channels, 7^3 -> 14^3 with the ReLU
mask: R = 4, 16 (the nuclei step), 64 (the soma step: 2 images x 32 fg RoIs) and 300.  In one process, alternating:

  dgrad     fp32    ops.upconv3d_2x_dgrad(gy, W, y=y)
            f16x2   ZwConv3d.bound_of(gy) + ops.upconv3d_2x_dgrad_f16x2(gy, W, y=y, gy_max, w_max)       (max|W| cached: swept outside)
  wgrad     fp32    ops.upconv3d_2x_wgrad(gy, x, y=y)                                                     (gb out of the same launch)
            f16x2   ZwConv3d.bound_of(gy) + ops.upconv3d_2x_wgrad_f16x2(gy, x, y=y, gy_max, x_max=None)   (x swept by the call)
  backward  fp32    the two fp32 calls
            f16x2   ONE bound_of(gy) + the two f16x2 calls            (what train._UpConv3d2x.backward runs under set_upconv_backward)

Protocol of tools/bench_upconv.py: warm-up, then `--reps` repetitions with the variants alternating inside every repetition; each
measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median and spread (min ..
max) in ms.  Beside every time: the achieved rate of the gy + y read (every pass reads both once: 2 x 4 R Cout 8 V bytes) in TB/s, and
the fraction of the f16 matrix peak (2.5 PFLOP/s) the three MFMA products per fp32 product reach.  A row counts as a win only where it
separates from the fp32 row by more than the sum of the two spreads; conv_plan.UPCONV_BWD_F16_MIN_* are set from those verdicts.  The
record in the repository: `--out profiles/upconv_backward_f16.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
F16_PEAK = 2.5e15

ROIS = (4, 16, 64, 300)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--rois", type=int, nargs="*", default=list(ROIS))
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    from m3d import ops
    assert torch.cuda.is_available(), "bench_upconv_backward_f16 needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

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

    def report(R, what, res, passes, flop, gbytes):
        for v, (med, lo, hi) in res.items():
            frac = "%6.1f%%" % (100.0 * 3 * flop / (med * 1e-3) / F16_PEAK) if v == "f16x2" else "      -"
            say("%4d %-8s %-6s | %-26s | %7.2f %7.1f | %6.2f %s"
                % (R, what, v, "%.3f (%.3f .. %.3f)" % (med, lo, hi), flop / 1e9, passes * gbytes / 1e6, passes * gbytes / med / 1e9, frac))
        (ma, la, ha), (mb, lb, hb) = res["f16x2"], res["fp32"]
        sa, sb = ha - la, hb - lb
        verdict = ("f16x2 WINS beyond the spreads" if ma < mb - (sa + sb) else
                   "f16x2 LOSES beyond the spreads" if ma > mb + (sa + sb) else "the two do NOT separate beyond the spreads")
        say("# R = %d, %s: f16x2 %.3f ms against fp32 %.3f ms = x%.2f, spreads %.3f + %.3f ms: %s" % (R, what, ma, mb, mb / ma, sa, sb, verdict))

    Cc, r = 256, 7
    V = r ** 3
    say("# Backward of ConvTranspose3d(2, 2) + ReLU of the mask head: gy, y [R,256,14,14,14], x [R,256,7,7,7], W [256,256,2,2,2], fp32 tensors")
    say("# fp32 = m3d_upconv3d_2x_dgrad / _wgrad (csrc/upconv3d.hip); f16x2 = m3d_upconv3d_2x_dgrad_f16x2 / _wgrad_f16x2 with the gy sweep")
    say("# inside the window (one sweep for the pair), max|W| cached, x swept by the wgrad call")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# GFLOP: 2 R V Cin 8 Cout per pass; MB: the gy + y read of the passes; TB/s: that read at the median; f16 peak: 3 x FLOP / 2.5 PFLOP/s")
    say("%4s %-8s %-6s | %-26s | %7s %7s | %6s %s" % ("R", "pass", "kernel", "ms per call", "GFLOP", "gy+y MB", "TB/s", "f16 peak"))
    torch.manual_seed(0)
    for R in a.rois:
        x = torch.relu(torch.randn(R, Cc, r, r, r, device="cuda"))
        w = torch.randn(Cc, Cc, 2, 2, 2, device="cuda") * (2.0 / Cc) ** 0.5
        b = torch.randn(Cc, device="cuda") * 0.1
        y = ops.upconv3d_2x_forward(x, w, b, relu=True)
        gy = torch.randn_like(y)
        w_max = ops.ZwConv3d.bound_of(w)
        flop = 2.0 * R * V * Cc * 8 * Cc
        gbytes = 2 * 4.0 * R * Cc * 8 * V

        def pair():
            gm = ops.ZwConv3d.bound_of(gy)
            return (ops.upconv3d_2x_dgrad_f16x2(gy, w, y=y, gy_max=gm, w_max=w_max), ops.upconv3d_2x_wgrad_f16x2(gy, x, y=y, gy_max=gm))
        rows = (
            ("dgrad", 1, (("fp32", lambda: ops.upconv3d_2x_dgrad(gy, w, y=y)),
                          ("f16x2", lambda: ops.upconv3d_2x_dgrad_f16x2(gy, w, y=y, gy_max=ops.ZwConv3d.bound_of(gy), w_max=w_max)))),
            ("wgrad", 1, (("fp32", lambda: ops.upconv3d_2x_wgrad(gy, x, y=y)),
                          ("f16x2", lambda: ops.upconv3d_2x_wgrad_f16x2(gy, x, y=y, gy_max=ops.ZwConv3d.bound_of(gy))))),
            ("backward", 2, (("fp32", lambda: (ops.upconv3d_2x_dgrad(gy, w, y=y), ops.upconv3d_2x_wgrad(gy, x, y=y))), ("f16x2", pair))),
        )
        for what, passes, variants in rows:
            report(R, what, measure(variants), passes, passes * flop, gbytes)
        del x, w, b, y, gy
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
