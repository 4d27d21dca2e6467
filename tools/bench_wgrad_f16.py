#!/usr/bin/env python3
"""Times the f16x2 conv weight gradient (csrc/conv3d_wgrad_f16.hip) against the fp32 kernel it is an option for, and samples its error
at full size.  The table behind the rule of m3d.conv_plan.wgrad_kernel.

Layers: the six 3^3 layers of the stride-8 body (m3d.train.DsnBody, width 32) on one 128^3 volume (the shapes of
profiles/r01_conv_backward.txt) and on four, and the four 3^3 layers of the stride-4 soma body on its 64 x 256 x 256 tile; then, to
find where the routing rule has to stop, the stride-8 body on a 32 x 64 x 64 tile and the mask head's 7^3 RoI maps.  Two ways to get dW
from x and gy:

  (a) f16x2   ops.conv3d_wgrad_f16x2(x, gy): the two bound sweeps (ZwConv3d.bound_of), the kernel and its reduce - the whole path
  (b) fp32    ops.conv3d_wgrad(x, gy, 3): m3d_conv3d_wgrad, the yardstick, in the same run

Protocol of tools/bench_linear_backward.py: warm-up, then `--reps` repetitions with the variants alternating inside every repetition;
each measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median and spread
(max - min) in ms.  "wins" = the median of (a) lies below that of (b) by more than the sum of the two spreads.  TFLOP/s counts the
2 x 27 cin cout voxels FLOP of the gradient once for both (the f16x2 kernel issues three times as many fp16 products).

Accuracy (--accuracy, on by default): conv2b and conv4b on four 128^3 volumes with N(0,1) gy and ReLU'd N(0,1) x; 256 seeded (co, ci, tap)
elements recomputed in fp64 on the device; the largest |error| / max |dW| of both kernels.  The project's envelope for its f16x2 convs
is 3e-6 of the largest output; a figure outside it ends the tool with a non-zero status.  The record in the repository: `--out profiles/conv_wgrad_f16.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
F16_PEAK = 2.5e15
ENVELOPE = 3e-6

BODY8 = [("conv2a", 32, 64, 2), ("conv2b", 64, 64, 2), ("conv3a", 64, 128, 4), ("conv3b", 128, 128, 4), ("conv4a", 128, 256, 8),
         ("conv4b", 256, 256, 8)]
BODY4 = BODY8[:4]


def layers():
    out = []
    for batch in (1, 4):
        out += [("s8 %s" % n, batch, ci, co, 128 // d, 128 // d, 128 // d) for n, ci, co, d in BODY8]
    out += [("s4 %s" % n, 1, ci, co, 64 // d, 256 // d, 256 // d) for n, ci, co, d in BODY4]
    # below the asked-for shapes, to find where the rule has to stop: the stride-8 body on a 32 x 64 x 64 tile (the default tile of
    # tools/train_detector.py) and the mask head's 7^3 RoI maps (a quarter of a 2 x 4 x 16 tile is voxels) on 8 and 64 RoIs
    out += [("t8 %s" % n, 1, ci, co, 32 // d, 64 // d, 64 // d) for n, ci, co, d in BODY8]
    out += [("m7 mask", r, 256, 256, 7, 7, 7) for r in (8, 64)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window")
    ap.add_argument("--no-accuracy", dest="accuracy", action="store_false")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    from m3d import conv_plan, ops
    assert torch.cuda.is_available(), "bench_wgrad_f16 needs a GPU"
    lines = []
    inside = True

    def say(s):
        print(s, flush=True)
        lines.append(s)

    variants = (("f16x2", lambda x, gy: ops.conv3d_wgrad_f16x2(x, gy)), ("fp32", lambda x, gy: ops.conv3d_wgrad(x, gy, 3)))

    def timed(fn, args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.inner):
            fn(*args)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    say("# dW of a 3^3 conv from x [B,cin,D,H,W] and gy [B,cout,D,H,W], fp32 in and out; f16x2 = two bound sweeps + kernel + reduce")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# TFLOP/s = 54 cin cout B D H W / median; wins = f16x2 median below fp32 median by more than the sum of the spreads (max - min)")
    say("%-10s %2s %4s %4s %-12s %5s %4s | %-26s %7s | %-26s %7s | %6s %5s %s"
        % ("layer", "B", "cin", "cout", "map", "slots", "t/s", "f16x2 ms", "TFLOP/s", "fp32 ms", "TFLOP/s", "ratio", "wins", "routed"))
    torch.manual_seed(0)
    totals = {}
    for name, B, cin, cout, D, H, W in layers():
        x = torch.relu(torch.randn(B, cin, D, H, W, device="cuda"))
        gy = torch.randn(B, cout, D, H, W, device="cuda")
        args = (x, gy)
        p = ops.conv3d_wgrad_f16x2_plan(B, cin, cout, D, H, W)
        times = {v: [] for v, _ in variants}
        for i in range(a.warmup + a.reps):
            order = variants[i % 2:] + variants[:i % 2]
            for v, fn in order:
                t = timed(fn, args)
                if i >= a.warmup:
                    times[v].append(t)
        flop = 54.0 * cin * cout * B * D * H * W
        res = {v: (statistics.median(times[v]), min(times[v]), max(times[v])) for v, _ in variants}
        (mf, lf, hf), (m3, l3, h3) = res["f16x2"], res["fp32"]
        wins = mf < m3 - ((hf - lf) + (h3 - l3))
        routed = conv_plan.wgrad_kernel(B, cin, cout, D, H, W, "f16x2")
        say("%-10s %2d %4d %4d %-12s %5d %4d | %-26s %7.1f | %-26s %7.1f | %6.2f %5s %s"
            % (name, B, cin, cout, "%dx%dx%d" % (D, H, W), p["slots"], p["tiles_per_slot"], "%.3f (%.3f .. %.3f)" % (mf, lf, hf),
               flop / mf / 1e9, "%.3f (%.3f .. %.3f)" % (m3, l3, h3), flop / m3 / 1e9, m3 / mf, "yes" if wins else "no", routed))
        key = "%s B=%d" % (name[:2], B) if name[0] == "s" else name[:2]
        tf, t3, tr = totals.get(key, (0.0, 0.0, 0.0))
        totals[key] = (tf + mf, t3 + m3, tr + (mf if routed == conv_plan.WGRAD_F16X2 else m3))
        del x, gy, args
        torch.cuda.empty_cache()
    for key, (tf, t3, tr) in totals.items():
        say("# %s: sum of the medians, all layers on f16x2 %.3f ms, all on fp32 %.3f ms, as routed by conv_plan.wgrad_kernel %.3f ms" % (key, tf, t3, tr))

    if a.accuracy:
        say("# sampled error at full size: B = 4, gy ~ N(0,1), x = relu(N(0,1)); %d seeded (co, ci, tap) elements against fp64 on the device;"
            % a.samples)
        say("# largest |error| / max |dW|; the envelope of the project's f16x2 convs is %.0e" % ENVELOPE)
        g = torch.Generator().manual_seed(1)
        for name, cin, cout, d in (BODY8[1], BODY8[5]):
            n = 128 // d
            x = torch.relu(torch.randn(4, cin, n, n, n, device="cuda"))
            gy = torch.randn(4, cout, n, n, n, device="cuda")
            got = {"f16x2": ops.conv3d_wgrad_f16x2(x, gy), "fp32": ops.conv3d_wgrad(x, gy, 3)}
            xp = torch.nn.functional.pad(x, (1, 1, 1, 1, 1, 1))                   # fp32 zeros around, once
            picks = torch.stack([torch.randint(0, m, (a.samples,), generator=g) for m in (cout, cin, 27)], 1).tolist()
            ref = torch.zeros(a.samples, dtype=torch.float64, device="cuda")
            for i, (co, ci, tap) in enumerate(picks):                             # no host synchronisation inside the loop
                dz, dy, dx = tap // 9, tap // 3 % 3, tap % 3
                ref[i] = (gy[:, co].double() * xp[:, ci, dz:dz + n, dy:dy + n, dx:dx + n].double()).sum()
            idx = torch.tensor(picks, device="cuda")
            top = float(got["fp32"].abs().max())
            worst = {v: float((t.reshape(cout, cin, 27)[idx[:, 0], idx[:, 1], idx[:, 2]].double() - ref).abs().max()) / top
                     for v, t in got.items()}
            inside = inside and worst["f16x2"] <= ENVELOPE
            say("%s 4x%d^3 cin %d cout %d: max |dW| %.4g; f16x2 %.3g (%s the envelope), fp32 %.3g"
                % (name, n, cin, cout, top, worst["f16x2"], "within" if worst["f16x2"] <= ENVELOPE else "OUTSIDE", worst["fp32"]))
            del x, gy, xp, got
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not inside:
        sys.exit("the f16x2 weight gradient left the %.0e envelope: the chain and fold design does not hold" % ENVELOPE)


if __name__ == "__main__":
    main()
