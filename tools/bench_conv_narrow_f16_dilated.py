#!/usr/bin/env python3
"""Times the forward and the backward-data conv of the mask head's dilation-2 3^3 layers (7^3 RoI grids) on the dilation-2
instantiation of the narrow-map f16x2 kernel (ops.ZnConv3d(..., dilation=2), csrc/conv3d_zn.hip) against m3d_conv3d_forward_dilated,
the direct fp32 MFMA kernel they run on otherwise, and MaskHeadM3D.trunk with conv_f16 off and on at dilation 1 and 2.  The table
behind ZN_DILATED_MIN_UNITS of m3d.conv_plan.  The protocol is tools/bench_conv_narrow_f16.py's: in one process, alternating, what
m3d.compat runs for the call with set_conv_dilated_f16 on and off under set_conv_dilated("m3d") (the weight pack INSIDE the timed
window, as a training step makes it after every weight update):

  forward  f16x2   ZnConv3d.bound_of(x) (one sweep) + ZnConv3d(w)(x, x_max, shift=bias, dilation=2)
           fp32    PackedConv3d(w, W_PLAIN)(x, shift=bias, dilation=2)
  dgrad    f16x2   conv3d_gy_reduce(gy) (bias gradient + bound, one pass) + ZnConv3d.dgrad_of(w)(gy, gy_max, dilation=2)
           fp32    PackedConv3d(w, W_DGRAD)(gy, dilation=2) + conv3d_bias_grad(gy)

Shapes: 256 -> 256 at R = 16 / 64 / 300 and 128 -> 128 at R = 128 / 300.  Warm-up, then `--reps` repetitions with the variants
alternating inside every repetition; a measurement is the time between two device events around `--inner` consecutive calls, divided
by `--inner`; median and spread (max - min) in ms.  A row counts as faster only when the medians differ by more than the sum of the two
spreads.  "of f16 peak": three f16 products x 2 27 cin cout FLOP per voxel over the f16x2 median, against 2.5 PFLOP/s.  The trunk: four
conv_fcn layers of 256 channels on a [1, 256, 16, 16, 16] feature map whose bound is given (feat_max), packs built once as detection
builds them, conv_f16_min_units = 0 so that "on" is on whatever the threshold says.  The record in the repository:
`--out profiles/conv_narrow_f16_dilated.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
F16_PEAK = 2.5e15

SHAPES = [("mask head", 256, 256, (16, 64, 300)), ("mask head", 128, 128, (128, 300))]
TRUNK_ROIS = (64, 300)
TRUNK_DIM, TRUNK_CONVS = 256, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--parts", nargs="*", default=("conv", "trunk"), choices=("conv", "trunk"))
    ap.add_argument("--out", default=None, help="also write the table to this file (rewritten after every part)")
    a = ap.parse_args()
    import torch
    from m3d import conv_plan, ops
    from m3d.config import Cfg
    from m3d.mask_head import MaskHeadM3D
    assert torch.cuda.is_available(), "bench_conv_narrow_f16_dilated needs a GPU"
    Z = ops.ZnConv3d
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

    def verdict(new, old):
        (ma, la, ha), (mb, lb, hb) = new, old
        return "faster" if ma < mb - ((ha - la) + (hb - lb)) else "SLOWER" if ma > mb + ((ha - la) + (hb - lb)) else "no separation"

    def cell(r):
        return "%.3f (%.3f .. %.3f)" % r

    say("# forward and backward-data of the dilation-2 per-RoI 3^3 convs on 7^3 grids: the dilation-2 narrow-map f16x2 kernel against")
    say("# m3d_conv3d_forward_dilated (direct fp32 MFMA)")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    torch.manual_seed(0)
    if "conv" in a.parts:
        say("# f16x2 = bound sweep (forward) / gy_reduce (dgrad) + pack + the zn conv at dilation 2; fp32 = pack + the dilated direct kernel (+ m3d_conv3d_bias_grad for dgrad)")
        say("# ratio = fp32 median / f16x2 median; verdict: medians apart by more than the sum of the spreads; of f16 peak: 3 x 2 x 27 cin cout x voxels FLOP")
        say("%-10s %-7s %9s %5s %6s | %-26s | %-26s | %5s %-13s %8s %s"
            % ("layer", "dir", "channels", "R", "units", "f16x2 ms", "fp32 ms", "ratio", "verdict", "f16 peak", "routed at the default threshold"))
        setting = conv_plan.TrainSetting(dilated=conv_plan.DILATED_M3D)
        for name, cin, cout, rois in SHAPES:
            for R in rois:
                x = torch.relu(torch.randn(R, cin, 7, 7, 7, device="cuda"))
                gy = torch.randn(R, cout, 7, 7, 7, device="cuda")
                w = torch.randn(cout, cin, 3, 3, 3, device="cuda") * (2.0 / (27 * cin)) ** 0.5
                b = torch.randn(cout, device="cuda")
                plan = conv_plan.plan_train_conv(setting._replace(dilated_f16=conv_plan.ZN_DILATED_MIN_UNITS), tuple(x.shape), tuple(w.shape), 2,
                                                 (True, True, True))
                for direction in ("forward", "dgrad"):
                    ci, co = (cin, cout) if direction == "forward" else (cout, cin)
                    units = int(ops.lib().m3d_conv3d_zn_dilated_launch_units(R, ci, co, 7, 7, 7, 2))
                    if direction == "forward":
                        variants = (("f16x2", lambda: Z(w)(x, Z.bound_of(x), shift=b, out_max=False, dilation=2)),
                                    ("fp32", lambda: ops.PackedConv3d(w, ops.W_PLAIN)(x, shift=b, dilation=2)))
                    else:
                        variants = (("f16x2", lambda: Z.dgrad_of(w)(gy, ops.conv3d_gy_reduce(gy)[1], out_max=False, dilation=2)),
                                    ("fp32", lambda: (ops.PackedConv3d(w, ops.W_DGRAD)(gy, dilation=2), ops.conv3d_bias_grad(gy))))
                    r = measure(variants)
                    flop = 3 * 2.0 * 27 * cin * cout * 343 * R
                    say("%-10s %-7s %4d->%-3d %5d %6d | %-26s | %-26s | %5.2f %-13s %7.1f%% %s"
                        % (name, direction, cin, cout, R, units, cell(r["f16x2"]), cell(r["fp32"]), r["fp32"][0] / r["f16x2"][0],
                           verdict(r["f16x2"], r["fp32"]), 100.0 * flop / (r["f16x2"][0] * 1e-3) / F16_PEAK,
                           plan.forward if direction == "forward" else plan.dgrad))
                del x, gy, w, b
                torch.cuda.empty_cache()
        flush()
    if "trunk" in a.parts:
        say("# trunk: MaskHeadM3D.trunk (RoIAlign3D + %d conv_fcn layers %d -> %d + ReLU) on a [1,%d,16,16,16] feature map (a 128^3 tile at"
            % (TRUNK_CONVS, TRUNK_DIM, TRUNK_DIM, TRUNK_DIM))
        say("# stride 8) whose bound is given, random RoIs; conv_f16 off / on (conv_f16_min_units = 0), dilation 1 and 2")
        say("%-3s %-4s %5s | %-28s" % ("dil", "f16", "R", "ms per call"))
        g = torch.Generator().manual_seed(1)
        P = {}
        for i in range(TRUNK_CONVS):
            P["Mask_Head.conv_fcn.%d.weight" % (2 * i)] = (torch.randn((TRUNK_DIM, TRUNK_DIM, 3, 3, 3), generator=g) * (2.0 / (27 * TRUNK_DIM)) ** 0.5).cuda()
            P["Mask_Head.conv_fcn.%d.bias" % (2 * i)] = (torch.randn((TRUNK_DIM,), generator=g) * 0.1).cuda()
        P["Mask_Head.upconv.weight"] = (torch.randn((TRUNK_DIM, TRUNK_DIM, 2, 2, 2), generator=g) * (2.0 / TRUNK_DIM) ** 0.5).cuda()
        P["Mask_Head.upconv.bias"] = torch.zeros((TRUNK_DIM,)).cuda()
        cfg = Cfg.nuclei()
        P["Mask_Outs.classify.weight"] = (torch.randn((cfg.num_classes, TRUNK_DIM, 1, 1, 1), generator=g) * 0.05).cuda()
        P["Mask_Outs.classify.bias"] = torch.zeros((cfg.num_classes,)).cuda()
        feat = torch.relu(torch.randn(1, TRUNK_DIM, 16, 16, 16, device="cuda"))
        fmax = ops.ZwConv3d.bound_of(feat)
        for dil in (1, 2):
            kw = dict(resolution=14, roi_res=7, sampling_ratio=2, dilation=dil)
            off = MaskHeadM3D(P, cfg, conv_f16=False, **kw)
            on = MaskHeadM3D(P, cfg, conv_f16=True, conv_f16_min_units=0, **kw)
            default = conv_plan.ZN_DILATED_MIN_UNITS if dil == 2 else conv_plan.ZN_MIN_UNITS
            for R in TRUNK_ROIS:
                lo = torch.rand(R, 3, device="cuda") * 90
                rois = torch.cat([torch.zeros(R, 1, device="cuda"), lo, lo + 8 + torch.rand(R, 3, device="cuda") * 30], 1).contiguous()
                r = measure((("on", lambda: on.trunk(feat, rois, feat_max=fmax)), ("off", lambda: off.trunk(feat, rois))))
                for v in ("off", "on"):
                    say("%-3d %-4s %5d | %-28s" % (dil, v, R, cell(r[v])))
                units = on.zn[0].units((R, TRUNK_DIM, 7, 7, 7), dilation=dil)
                say("# trunk dilation %d R %d: on %.3f ms against off %.3f ms = x%.2f: %s; %d units per conv, default threshold %d: %s"
                    % (dil, R, r["on"][0], r["off"][0], r["off"][0] / r["on"][0], verdict(r["on"], r["off"]), units, default,
                       "routed" if units >= default else "not routed"))
        flush()


if __name__ == "__main__":
    main()
