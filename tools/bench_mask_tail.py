#!/usr/bin/env python3
"""Times the mask head's tail - ConvTranspose3d(2, 2) + ReLU, the 1x1x1 classifier, the sigmoid - as ONE f16x2 launch
(ops.UpConvF16.tail, csrc/upconv3d_f16.hip) against the three launches it replaces, at the shipped shape R x 256 -> 256 channels,
7^3 -> 14^3, K = 2 classes, R = 16, 64, 300.  In one process, alternating:

  tail       bound    UpConvF16.tail with the operand bound given (what the last trunk conv hands on under conv_f16)
             sweep    ... with its own ZwConv3d.bound_of sweep of x inside the window
  parent     3 calls  ops.upconv3d_2x_forward (fp32 MFMA, compat.set_upconv("m3d")) + the classify conv (PackedConv3d) + torch.sigmoid;
             up / classify / sigmoid: its three parts alone, each on the input the part before it left
  plain      f16      UpConvF16.__call__ (the plain epilogue, bound given; `f16+sw`: with its own sweep) against `up` above
  mask_net   off/on   MaskHeadM3D(conv_f16=True, dilation 2).mask_net end to end (RoIAlign + 4 convs + tail), tail_f16 off -> on,
                      R = 64 and 300 (--no-head skips it)

The weight pack is made once, outside every window (the head packs at construction); the sweep is inside the window where the row says
so.  Protocol of tools/bench_upconv.py: warm-up, then `--reps` repetitions with the variants alternating inside every repetition; each
measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median and spread (min ..
max) in ms.  Beside the f16 rows: the achieved fraction of the 2.5 PFLOP/s f16 MFMA bound, three f16 products per fp32 product.  The
record in the repository: `--out profiles/mask_tail_f16.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
F16_PEAK = 2.5e15
RS = (16, 64, 300)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--no-head", action="store_true", help="skip the MaskHeadM3D.mask_net end-to-end rows")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    from m3d import compat, ops
    from m3d.config import Cfg
    from m3d.mask_head import MaskHeadM3D
    assert torch.cuda.is_available(), "bench_mask_tail needs a GPU"
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

    def report(R, res, flop3=None):
        for v, (med, lo, hi) in res.items():
            frac = "  %4.1f %% of the f16 bound" % (100.0 * flop3 / (med * 1e-3) / F16_PEAK) if flop3 and ("tail" in v or "f16" in v) else ""
            say("%4d %-16s | %-26s%s" % (R, v, "%.4f (%.4f .. %.4f)" % (med, lo, hi), frac))

    def compare(R, res, new, old):
        (ma, la, ha), (mb, lb, hb) = res[new], res[old]
        sa, sb = ha - la, hb - lb
        verdict = ("%s is faster beyond the spreads" % new if ma < mb - (sa + sb) else
                   "%s is SLOWER beyond the spreads" % new if ma > mb + (sa + sb) else "the two do NOT separate beyond the spreads")
        say("# R = %d: %s %.4f ms against %s %.4f ms = x%.2f, spreads %.4f + %.4f ms: %s" % (R, new, ma, old, mb, mb / ma, sa, sb, verdict))
        return ma < mb - (sa + sb)

    say("# Mask head tail: x [R,256,7,7,7] -> up-conv 256 -> 256 (2, 2) + ReLU -> classify 1^3 to K = 2 -> sigmoid -> [R,2,14,14,14]")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# the weight pack is outside every window; the bound sweep is inside where the row says sweep / +sw")
    say("# f16 bound: 3 x 2 R 343 256 2048 FLOP at 2.5 PFLOP/s")
    say("%4s %-16s | %-26s" % ("R", "variant", "ms per call"))
    torch.manual_seed(0)
    Cc, K, r = 256, 2, 7
    wins = []
    prev = compat.set_upconv("m3d")
    try:
        for R in RS:
            x = torch.relu(torch.randn(R, Cc, r, r, r, device="cuda"))
            w = torch.randn(Cc, Cc, 2, 2, 2, device="cuda") * (2.0 / Cc) ** 0.5
            b = torch.randn(Cc, device="cuda") * 0.1
            wc = torch.randn(K, Cc, device="cuda") * (1.0 / Cc) ** 0.5
            bc = torch.randn(K, device="cuda") * 0.1
            up = ops.UpConvF16(w)
            cls = ops.PackedConv3d(wc.view(K, Cc, 1, 1, 1).contiguous())
            one = torch.ones(K, device="cuda")
            bound = ops.ZwConv3d.bound_of(x)
            y = ops.upconv3d_2x_forward(x, w, b, relu=True)
            logits = cls(y, scale=one, shift=bc)

            def parent():
                return torch.sigmoid(cls(ops.upconv3d_2x_forward(x, w, b, relu=True), scale=one, shift=bc))
            variants = (("tail bound", lambda: up.tail(x, bound, b, wc, bc)), ("tail sweep", lambda: up.tail(x, None, b, wc, bc)),
                        ("parent 3 calls", parent), ("parent up", lambda: ops.upconv3d_2x_forward(x, w, b, relu=True)),
                        ("parent classify", lambda: cls(y, scale=one, shift=bc)), ("parent sigmoid", lambda: torch.sigmoid(logits)),
                        ("plain f16", lambda: up(x, bound, bias=b, relu=True)), ("plain f16+sw", lambda: up(x, None, bias=b, relu=True)))
            res = measure(variants)
            report(R, res, 3 * 2.0 * R * r ** 3 * Cc * 8 * Cc)
            a_ = compare(R, res, "tail bound", "parent 3 calls")
            b_ = compare(R, res, "tail sweep", "parent 3 calls")
            compare(R, res, "plain f16", "parent up")
            compare(R, res, "plain f16+sw", "parent up")
            if a_ and b_:
                wins.append(R)
            del x, w, b, wc, bc, up, cls, y, logits, variants
            torch.cuda.empty_cache()
        say("# the fused call, with or without its sweep, beats the three launches beyond the spreads at R = %s" % (wins,))
        if not a.no_head:
            say("# MaskHeadM3D.mask_net end to end: RoIAlign (feature map [1,256,16,32,32]) + 4 dilation-2 convs on the narrow f16x2 kernel + tail")
            g = torch.Generator().manual_seed(1)
            P, c = {}, Cc
            for i in range(4):
                P["Mask_Head.conv_fcn.%d.weight" % (2 * i)] = torch.randn((Cc, c, 3, 3, 3), generator=g) * (2.0 / (27 * c)) ** 0.5
                P["Mask_Head.conv_fcn.%d.bias" % (2 * i)] = torch.randn((Cc,), generator=g) * 0.1
            P["Mask_Head.upconv.weight"] = torch.randn((Cc, Cc, 2, 2, 2), generator=g) * (2.0 / Cc) ** 0.5
            P["Mask_Head.upconv.bias"] = torch.randn((Cc,), generator=g) * 0.1
            P["Mask_Outs.classify.weight"] = torch.randn((K, Cc, 1, 1, 1), generator=g) * (1.0 / Cc) ** 0.5
            P["Mask_Outs.classify.bias"] = torch.randn((K,), generator=g) * 0.1
            G = {k: v.cuda() for k, v in P.items()}
            cfg = Cfg.nuclei(mlp_dim=64)
            kw = dict(resolution=14, roi_res=7, sampling_ratio=2, dilation=2, conv_f16=True)
            off, on = MaskHeadM3D(G, cfg, tail_f16=False, **kw), MaskHeadM3D(G, cfg, tail_f16=True, tail_f16_min_rois=0, **kw)
            feat = torch.relu(torch.randn((1, Cc, 16, 32, 32), generator=g)).cuda()
            for R in (64, 300):
                st = float(cfg.stride)                              # boxes (x, y, z) inside the 32 x 32 x 16 map at the head's stride
                lo = torch.rand((R, 3), generator=g) * torch.tensor([20.0, 20.0, 8.0]) * st
                sz = (torch.rand((R, 3), generator=g) * 6 + 2) * st
                rois = torch.cat([torch.zeros(R, 1), lo, lo + sz], 1).cuda()
                res = measure((("mask_net off", lambda: off.mask_net(feat, rois)), ("mask_net on", lambda: on.mask_net(feat, rois))))
                report(R, res)
                compare(R, res, "mask_net on", "mask_net off")
    finally:
        compat.set_upconv(prev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
