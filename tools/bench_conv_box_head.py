#!/usr/bin/env python3
"""Times the conv box head (roi_Xconv1fc_head, lib/modeling/fast_rcnn_heads.py:120-179) and the dilation-1 weight gradient of its
per-RoI convs.  In one process, alternating:

  wgrad    narrow  ops.conv3d_wgrad_narrow(x, gy): the 2 x 8 x 8 voxel tile (m3d_conv3d_wgrad_narrow)
           wide    ops.conv3d_wgrad(x, gy, 3): the 2 x 4 x 16 voxel tile (m3d_conv3d_wgrad)
           at 256 -> 128 and 128 -> 128 channels on 7^3 with R = 128, 256, 512 (the head's two convs at the nuclei YAML's numbers), and at
           256 -> 256 with R = 16, 64, 300 (the mask head at MRCNN.DILATION = 1)
  head     conv    DetectorM3D.box_head_outputs of the conv head (nuclei: 256 -> 128 -> 128 -> 1024) at R = 300, 1000, 4000
           mlp     the same call on the two-FC head (256 * 343 -> 1024 -> 1024) at the same R
  step     off/on  one forward + backward of m3d.ConvBoxHead (256 -> 128 -> 128 -> 1024) at R = 128 under compat.install() with
                   compat.set_conv_wgrad_narrow(False / True)

Protocol of tools/bench_conv_dilated.py: warm-up, then `--reps` repetitions with the variants alternating inside every repetition; each
measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median and spread (min ..
max) in ms.  Beside every wgrad time: the algorithmic FLOP (2 * R * 343 * 27 * Cin * Cout), the achieved rate and its fraction of the
157.3 TFLOP/s of v_mfma_f32_32x32x2_f32, and whether the two kernels separate by more than the sum of their spreads (max - min).  No
threshold is set on any of it.  The record in the repository: `--out profiles/conv_box_head.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
MFMA_PEAK = 157.3e12

WGRAD_SHAPES = [("head conv1", 256, 128, (128, 256, 512)), ("head conv2", 128, 128, (128, 256, 512)), ("mask head", 256, 256, (16, 64, 300))]
HEAD_ROIS = (300, 1000, 4000)
STEP_ROIS = 128
HEAD = "roi_Xconv1fc_head"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--parts", nargs="*", default=("wgrad", "head", "step"), choices=("wgrad", "head", "step"))
    ap.add_argument("--out", default=None, help="also write the table to this file (rewritten after every part)")
    a = ap.parse_args()
    import torch
    import m3d
    import m3d.compat as compat
    from m3d import ops
    from m3d.config import Cfg
    from m3d.model import DetectorM3D
    from m3d.synth import make_params
    assert torch.cuda.is_available(), "bench_conv_box_head needs a GPU"
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

    def compare(what, res, new, old):
        (ma, la, ha), (mb, lb, hb) = res[new], res[old]
        sa, sb = ha - la, hb - lb
        verdict = ("%s is faster beyond the spreads" % new if ma < mb - (sa + sb) else
                   "%s is SLOWER beyond the spreads" % new if ma > mb + (sa + sb) else "the two do NOT separate beyond the spreads")
        say("# %s: %s %.3f ms against %s %.3f ms = x%.2f, spreads %.3f + %.3f ms: %s" % (what, new, ma, old, mb, mb / ma, sa, sb, verdict))

    say("# conv box head (roi_Xconv1fc_head) and the dilation-1 conv weight gradient on 7^3 RoI grids, fp32")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    torch.manual_seed(0)
    if "wgrad" in a.parts:
        say("# wgrad: x [R,Cin,7,7,7], gy [R,Cout,7,7,7]; GFLOP: 2 R 343 27 Cin Cout; TFLOP/s at the median and its share of the 157.3 "
            "TFLOP/s fp32 MFMA bound")
        say("%-11s %9s %4s %-6s | %-28s | %7s | %7s %6s" % ("layer", "channels", "R", "kernel", "ms per call", "GFLOP", "TFLOP/s", "of peak"))
        for name, cin, cout, rois in WGRAD_SHAPES:
            for R in rois:
                x = torch.randn(R, cin, 7, 7, 7, device="cuda")
                gy = torch.randn(R, cout, 7, 7, 7, device="cuda")
                flop = 2.0 * R * 343 * 27 * cin * cout
                res = measure((("narrow", lambda: ops.conv3d_wgrad_narrow(x, gy)), ("wide", lambda: ops.conv3d_wgrad(x, gy, 3))))
                for v, (med, lo, hi) in res.items():
                    say("%-11s %4d->%-3d %4d %-6s | %-28s | %7.2f | %7.2f %5.1f%%"
                        % (name, cin, cout, R, v, "%.3f (%.3f .. %.3f)" % (med, lo, hi), flop / 1e9, flop / med / 1e9,
                           100.0 * flop / (med * 1e-3) / MFMA_PEAK))
                compare("%s %d->%d R %d (%d split-K slots)" % (name, cin, cout, R, ops.conv3d_wgrad_narrow_plan(R, cin, cout, 7, 7, 7)["slots"]),
                        res, "narrow", "wide")
                del x, gy
                torch.cuda.empty_cache()
        flush()
    if "head" in a.parts:
        say("# head: DetectorM3D.box_head_outputs on a [1,256,16,16,16] feature map (a 128^3 tile at stride 8), random RoIs")
        say("%-5s %5s | %-28s" % ("head", "R", "ms per call"))
        cuda = lambda P: {k: v.cuda() for k, v in P.items()}
        conv = DetectorM3D(cuda(make_params(stride=8, num_anchors=35, seed=1, box_head=HEAD, conv_head_dim=128, num_stacked_convs=2)),
                           Cfg.nuclei(box_head=HEAD, conv_head_dim=128, num_stacked_convs=2))
        mlp = DetectorM3D(cuda(make_params(stride=8, num_anchors=35, seed=1)), Cfg.nuclei())
        feat = torch.randn(1, 256, 16, 16, 16, device="cuda")
        for R in HEAD_ROIS:
            lo = torch.rand(R, 3, device="cuda") * 90
            rois = torch.cat([torch.zeros(R, 1, device="cuda"), lo, lo + 8 + torch.rand(R, 3, device="cuda") * 30], 1).contiguous()
            res = measure((("conv", lambda: conv.box_head_outputs(feat, rois)), ("mlp", lambda: mlp.box_head_outputs(feat, rois))))
            for v, (med, l, h) in res.items():
                say("%-5s %5d | %-28s" % (v, R, "%.3f (%.3f .. %.3f)" % (med, l, h)))
            compare("box_head_outputs R %d" % R, res, "conv", "mlp")
        del conv, mlp, feat
        torch.cuda.empty_cache()
        flush()
    if "step" in a.parts:
        say("# step: forward + backward of m3d.ConvBoxHead(256, 8) (256 -> 128 -> 128 -> 1024) at R = %d under compat.install()" % STEP_ROIS)
        say("%-7s | %-28s" % ("narrow", "ms per call"))
        head = m3d.ConvBoxHead(256, 8).cuda()
        feat = torch.randn(1, 256, 16, 16, 16, device="cuda", requires_grad=True)
        lo = torch.rand(STEP_ROIS, 3, device="cuda") * 90
        rois = torch.cat([torch.zeros(STEP_ROIS, 1, device="cuda"), lo, lo + 8 + torch.rand(STEP_ROIS, 3, device="cuda") * 30], 1).contiguous()
        compat.install()

        def step(narrow):
            compat.set_conv_wgrad_narrow(narrow)
            cls, bbox = head(feat, rois)
            (cls.sum() + bbox.sum()).backward()
            compat.set_conv_wgrad_narrow(False)
        res = measure((("on", lambda: step(True)), ("off", lambda: step(False))))
        for v, (med, l, h) in res.items():
            say("%-7s | %-28s" % (v, "%.3f (%.3f .. %.3f)" % (med, l, h)))
        compare("ConvBoxHead forward + backward R %d" % STEP_ROIS, res, "on", "off")
        flush()


if __name__ == "__main__":
    main()
