#!/usr/bin/env python3
"""Times the forward and the backward-data conv of the per-RoI 3^3 layers (7^3 RoI grids) on the narrow-map f16x2 kernel
(ops.ZnConv3d, csrc/conv3d_zn.hip) against the direct fp32 MFMA kernel they run on otherwise, and the conv box head's
DetectorM3D.box_head_outputs with M3D_HEAD_CONV_F16 off and on.  The table behind ZN_MIN_UNITS of m3d.conv_plan.  In one process,
alternating, what m3d.compat runs for the call with set_conv_train_narrow on and off (the weight pack INSIDE the timed window, as a
training step makes it after every weight update):

  forward  f16x2   ZnConv3d.bound_of(x) (one sweep) + ZnConv3d(w)(x, x_max, shift=bias)
           fp32    PackedConv3d(w, W_PLAIN)(x, shift=bias)
  dgrad    f16x2   conv3d_gy_reduce(gy) (bias gradient + bound, one pass) + ZnConv3d.dgrad_of(w)(gy, gy_max)
           fp32    PackedConv3d(w, W_DGRAD)(gy) + conv3d_bias_grad(gy)

Shapes (those of profiles/conv_box_head.txt): head conv1 256 -> 128 and head conv2 128 -> 128 at R = 128 / 300 / 1000, the mask head's
256 -> 256 at R = 16 / 64 / 300.  Protocol of tools/bench_conv_box_head.py: warm-up, then `--reps` repetitions with the variants
alternating inside every repetition; a measurement is the time between two device events around `--inner` consecutive calls, divided by
`--inner`; median and spread (max - min) in ms.  A row counts as faster only when the medians differ by more than the sum of the two
spreads.  "of f16 peak": three f16 products x 2 27 cin cout FLOP per voxel over the f16x2 median, against 2.5 PFLOP/s.  The record in the
repository: `--out profiles/conv_narrow_f16.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
F16_PEAK = 2.5e15

SHAPES = [("head conv1", 256, 128, (128, 300, 1000)), ("head conv2", 128, 128, (128, 300, 1000)), ("mask head", 256, 256, (16, 64, 300))]
HEAD_ROIS = (300, 1000, 4000)
HEAD = "roi_Xconv1fc_head"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--parts", nargs="*", default=("conv", "head"), choices=("conv", "head"))
    ap.add_argument("--out", default=None, help="also write the table to this file (rewritten after every part)")
    a = ap.parse_args()
    import torch
    from m3d import conv_plan, ops
    from m3d.config import Cfg
    from m3d.model import DetectorM3D
    from m3d.synth import make_params
    assert torch.cuda.is_available(), "bench_conv_narrow_f16 needs a GPU"
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

    say("# forward and backward-data of the per-RoI 3^3 convs on 7^3 grids: the narrow-map f16x2 kernel against the direct fp32 MFMA kernel")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    torch.manual_seed(0)
    if "conv" in a.parts:
        say("# f16x2 = bound sweep (forward) / gy_reduce (dgrad) + pack + the zn conv; fp32 = pack + the direct kernel (+ m3d_conv3d_bias_grad for dgrad)")
        say("# ratio = fp32 median / f16x2 median; verdict: medians apart by more than the sum of the spreads; of f16 peak: 3 x 2 x 27 cin cout x voxels FLOP")
        say("%-10s %-7s %9s %5s %6s | %-26s | %-26s | %5s %-13s %8s %s"
            % ("layer", "dir", "channels", "R", "units", "f16x2 ms", "fp32 ms", "ratio", "verdict", "f16 peak", "routed (narrow=True)"))
        for name, cin, cout, rois in SHAPES:
            for R in rois:
                x = torch.relu(torch.randn(R, cin, 7, 7, 7, device="cuda"))
                gy = torch.randn(R, cout, 7, 7, 7, device="cuda")
                w = torch.randn(cout, cin, 3, 3, 3, device="cuda") * (2.0 / (27 * cin)) ** 0.5
                b = torch.randn(cout, device="cuda")
                for direction in ("forward", "dgrad"):
                    ci, co = (cin, cout) if direction == "forward" else (cout, cin)
                    units = int(ops.lib().m3d_conv3d_zn_launch_units(R, ci, co, 7, 7, 7))
                    if direction == "forward":
                        variants = (("f16x2", lambda: Z(w)(x, Z.bound_of(x), shift=b, out_max=False)),
                                    ("fp32", lambda: ops.PackedConv3d(w, ops.W_PLAIN)(x, shift=b)))
                    else:
                        variants = (("f16x2", lambda: Z.dgrad_of(w)(gy, ops.conv3d_gy_reduce(gy)[1], out_max=False)),
                                    ("fp32", lambda: (ops.PackedConv3d(w, ops.W_DGRAD)(gy), ops.conv3d_bias_grad(gy))))
                    r = measure(variants)
                    flop = 3 * 2.0 * 27 * cin * cout * 343 * R
                    say("%-10s %-7s %4d->%-3d %5d %6d | %-26s | %-26s | %5.2f %-13s %7.1f%% %s"
                        % (name, direction, cin, cout, R, units, cell(r["f16x2"]), cell(r["fp32"]), r["fp32"][0] / r["f16x2"][0],
                           verdict(r["f16x2"], r["fp32"]), 100.0 * flop / (r["f16x2"][0] * 1e-3) / F16_PEAK,
                           conv_plan.train_conv_kernel(direction, R, cin, cout, 7, 7, 7, "fp32", narrow=True)))
                del x, gy, w, b
                torch.cuda.empty_cache()
        flush()
    if "head" in a.parts:
        say("# head: DetectorM3D.box_head_outputs of the conv head (256 -> 128 -> 128 -> fc) on a [1,256,16,16,16] feature map (a 128^3 tile at")
        say("# stride 8) that carries its bound, random RoIs; M3D_HEAD_CONV_F16 off / on")
        say("%-4s %5s | %-28s" % ("f16", "R", "ms per call"))
        cuda = lambda P: {k: v.cuda() for k, v in P.items()}
        P = cuda(make_params(stride=8, num_anchors=35, seed=1, box_head=HEAD, conv_head_dim=128, num_stacked_convs=2))
        cfg = Cfg.nuclei(box_head=HEAD, conv_head_dim=128, num_stacked_convs=2)
        prev = os.environ.pop("M3D_HEAD_CONV_F16", None)
        off = DetectorM3D(P, cfg)
        os.environ["M3D_HEAD_CONV_F16"] = "1"
        on = DetectorM3D(P, cfg)
        if prev is None:
            del os.environ["M3D_HEAD_CONV_F16"]
        else:
            os.environ["M3D_HEAD_CONV_F16"] = prev
        feat = torch.randn(1, 256, 16, 16, 16, device="cuda")
        bound = ops.ZwConv3d.bound_of(feat)
        feat._m3d_bound = (bound, feat._version)
        for R in HEAD_ROIS:
            lo = torch.rand(R, 3, device="cuda") * 90
            rois = torch.cat([torch.zeros(R, 1, device="cuda"), lo, lo + 8 + torch.rand(R, 3, device="cuda") * 30], 1).contiguous()
            r = measure((("on", lambda: on.box_head_outputs(feat, rois)), ("off", lambda: off.box_head_outputs(feat, rois))))
            for v in ("off", "on"):
                say("%-4s %5d | %-28s" % (v, R, cell(r[v])))
            say("# box_head_outputs R %d: on %.3f ms against off %.3f ms = x%.2f: %s; plans %s"
                % (R, r["on"][0], r["off"][0], r["off"][0] / r["on"][0], verdict(r["on"], r["off"]),
                   [c.plan((R, 7, 7, 7)).kind for c in on.head_convs]))
        flush()


if __name__ == "__main__":
    main()
