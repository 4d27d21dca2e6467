#!/usr/bin/env python3
"""Times the mask head's ConvTranspose3d(2, 2) + ReLU (csrc/upconv3d.hip) against the paths the project takes without it, at the shipped
shapes R x 256 -> 256 channels, 7^3 -> 14^3: R = 64 (the soma training step: 2 images x 32 fg RoIs), 16 (the nuclei step), 300
(detection with MASK_ON, DETECTIONS_PER_IM).  In one process, alternating:

  forward   m3d      ops.upconv3d_2x_forward(x, W, b, relu=True): one launch, bias + ReLU in the epilogue
            torch    F.conv_transpose3d(x, W, b, stride=2) + torch.relu             (train.MaskHead under set_upconv("torch"))
            shuffle  the 1x1x1 conv to 8 Cout channels (PackedConv3d, bias + ReLU fused) + view / permute / reshape to the 2x grid
                     (mask_head.MaskHeadM3D.up under set_upconv("torch"))
  backward  m3d      ops.upconv3d_2x_dgrad + ops.upconv3d_2x_wgrad (gb out of the wgrad launch), the ReLU mask taken from y while staging
            torch    autograd's backward of F.conv_transpose3d + relu on a retained graph: gx, gW, gb

Protocol of tools/bench_sgd.py: warm-up, then `--reps` repetitions with the variants alternating inside every repetition; each
measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median and spread (min ..
max) in ms.  Beside every time, from the shape alone: the algorithmic FLOP and bytes (every operand moved once), the achieved rates, and
which of the two bounds - FLOP at the 157.3 TFLOP/s of v_mfma_f32_32x32x2_f32, bytes at 6.3 TB/s - is the larger.  No threshold is set
on any of it.  The record in the repository: `--out profiles/upconv.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
HBM_PEAK, MFMA_PEAK = 6.3e12, 157.3e12

SHAPES = [("soma step", 64, 256, 7), ("nuclei step", 16, 256, 7), ("detection", 300, 256, 7)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from m3d import ops
    assert torch.cuda.is_available(), "bench_upconv needs a GPU"
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

    def report(name, R, direction, res, flop, nbytes):
        t_mfma, t_hbm = flop / MFMA_PEAK * 1e3, nbytes / HBM_PEAK * 1e3
        for v, (med, lo, hi) in res.items():
            say("%-11s %4d %-8s %-7s | %-26s | %7.2f %7.1f | %7.1f %6.2f | %7.3f %7.3f %s"
                % (name, R, direction, v, "%.3f (%.3f .. %.3f)" % (med, lo, hi), flop / 1e9, nbytes / 1e6, flop / med / 1e9, nbytes / med / 1e9,
                   t_mfma, t_hbm, "mfma" if t_mfma >= t_hbm else "hbm"))

    def compare(name, what, res, new, old):
        (ma, la, ha), (mb, lb, hb) = res[new], res[old]
        sa, sb = ha - la, hb - lb
        verdict = ("%s is faster beyond the spreads" % new if ma < mb - (sa + sb) else
                   "%s is SLOWER beyond the spreads" % new if ma > mb + (sa + sb) else "the two do NOT separate beyond the spreads")
        say("# %s, %s: %s %.3f ms against %s %.3f ms = x%.2f, spreads %.3f + %.3f ms: %s" % (name, what, new, ma, old, mb, mb / ma, sa, sb, verdict))

    say("# ConvTranspose3d(2, 2) + ReLU of the mask head, fp32: x [R,256,7,7,7], W [256,256,2,2,2] -> y [R,256,14,14,14]")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# GFLOP, MB: algorithmic, from the shape (every operand once; the backward = dgrad + wgrad, both read gy and y)")
    say("# TFLOP/s, TB/s: achieved at the median; mfma ms = FLOP at 157.3 TFLOP/s, hbm ms = bytes at 6.3 TB/s; bound = the larger")
    say("%-11s %4s %-8s %-7s | %-26s | %7s %7s | %7s %6s | %7s %7s %s"
        % ("shape", "R", "pass", "variant", "ms per call", "GFLOP", "MB", "TFLOP/s", "TB/s", "mfma ms", "hbm ms", "bound"))
    torch.manual_seed(0)
    for name, R, Cc, r in SHAPES:
        V = r ** 3
        x = torch.randn(R, Cc, r, r, r, device="cuda")
        w = torch.randn(Cc, Cc, 2, 2, 2, device="cuda") * (2.0 / Cc) ** 0.5
        b = torch.randn(Cc, device="cuda") * 0.1
        pack = ops.PackedConv3d(w.permute(1, 2, 3, 4, 0).reshape(Cc * 8, Cc, 1, 1, 1).contiguous())
        b8, ones = b.repeat_interleave(8).contiguous(), torch.ones(Cc * 8, device="cuda")

        def shuffle():
            y = pack(x, scale=ones, shift=b8, relu=True)
            y = y.view(R, Cc, 2, 2, 2, r, r, r).permute(0, 1, 5, 2, 6, 3, 7, 4)
            return y.reshape(R, Cc, 2 * r, 2 * r, 2 * r)
        fwd = (("m3d", lambda: ops.upconv3d_2x_forward(x, w, b, relu=True)),
               ("torch", lambda: torch.relu(F.conv_transpose3d(x, w, b, stride=2))), ("shuffle", shuffle))
        flop = 2.0 * R * V * Cc * 8 * Cc
        n_x, n_w, n_y = R * Cc * V, Cc * Cc * 8, R * Cc * 8 * V
        res = measure(fwd)
        report(name, R, "forward", res, flop, 4.0 * (n_x + n_w + Cc + n_y))
        compare(name, "forward", res, "m3d", "torch")
        compare(name, "forward", res, "m3d", "shuffle")
        # backward: the graph of torch's forward is built once and retained
        xg, wg, bg = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        yt = torch.relu(F.conv_transpose3d(xg, wg, bg, stride=2))
        y = ops.upconv3d_2x_forward(x, w, b, relu=True)
        gy = torch.randn_like(y)

        def new():
            return ops.upconv3d_2x_dgrad(gy, w, y=y), ops.upconv3d_2x_wgrad(gy, x, y=y)
        bwd = (("m3d", new), ("torch", lambda: torch.autograd.grad(yt, (xg, wg, bg), gy, retain_graph=True)))
        res = measure(bwd)
        report(name, R, "backward", res, 2 * flop, 4.0 * (2 * 2 * n_y + n_w + n_x + n_x + n_w + Cc))
        compare(name, "backward", res, "m3d", "torch")
        del x, w, b, pack, b8, ones, xg, wg, bg, yt, y, gy, fwd, bwd
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
