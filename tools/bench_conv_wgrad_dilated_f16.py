#!/usr/bin/env python3
"""Times the weight gradient of the mask head's dilation-2 3^3 convs (7^3 RoI grids) on the dilation-2 instantiation of the narrow-map
f16x2 kernel (m3d_conv3d_wgrad_narrow_dilated_f16x2, csrc/conv3d_wgrad_narrow_f16.hip) against the kernel that takes these layers
today, each as m3d.compat would run it.  The table behind WGRAD_DILATED_F16X2_MIN_WORK of m3d.conv_plan.  In one process, alternating:

  (a)   fp32 dilated   ops.conv3d_wgrad(x, gy, 3, dilation=2)                              set_conv_dilated("m3d")
  (c)   f16x2 dilated  ops.conv3d_wgrad_narrow_f16x2(x, gy, dilation=2): two sweeps inside  set_conv_wgrad_dilated_f16(True)
  (c')  f16x2 dilated  ... with both bounds handed over, as the step runs it under set_conv_dilated_f16(True) as well

Shapes: the mask head's 256 -> 256 at R = 4 / 8 / 16 / 64 / 300 and 128 -> 128 at R = 128 / 300.  One more row, 256 -> 256 at R = 300,
puts the dilation-1 instantiation (ops.conv3d_wgrad_narrow_f16x2(x, gy), the same GEMM on the 4 x 10-row halo, two workgroups per CU)
beside the dilation-2 one: what the wider halo costs.  Protocol of tools/bench_conv_wgrad_narrow_f16.py: warm-up, then `--reps`
repetitions with the variants alternating inside every repetition; a measurement is the time between two device events around `--inner`
consecutive calls, divided by `--inner`; median and spread (max - min) in ms.  (c) wins a row only when its median is below (a)'s by more
than the sum of the two spreads.  "of f16 peak": three f16 products x 2 27 cin cout FLOP per voxel over the (c) median, against
2.5 PFLOP/s.  ws: the split-K workspace of (c) and of (a), MiB.

Accuracy: at R = 300, 256 seeded (co, ci, tap) elements per shape recomputed in fp64 on the device; the largest |error| / max |dW|.  The
project's envelope for its f16x2 convs is 3e-6 of the largest gradient; a figure outside it ends the tool with a non-zero status.  The
record in the repository: `--out profiles/conv_wgrad_dilated_f16.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
F16_PEAK = 2.5e15
ENVELOPE = 3e-6

SHAPES = [("mask head", 256, 256, (4, 8, 16, 64, 300)), ("mask head", 128, 128, (128, 300))]
ACCURACY_R = 300
HALO_ROW = (256, 256, 300)              # cin, cout, R of the row against the dilation-1 instantiation


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--samples", type=int, default=256, help="elements checked against fp64 per shape")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    from m3d import conv_plan, ops
    assert torch.cuda.is_available(), "bench_conv_wgrad_dilated_f16 needs a GPU"
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

    def verdict(new, old):
        (ma, la, ha), (mb, lb, hb) = new, old
        return "wins" if ma < mb - ((ha - la) + (hb - lb)) else "LOSES" if ma > mb + ((ha - la) + (hb - lb)) else "no separation"

    def cell(r):
        return "%.3f (%.3f .. %.3f)" % r

    say("# weight gradient of the dilation-2 3^3 convs on 7^3 grids: (a) fp32 dilated, (c) f16x2 dilated + 2 sweeps, (c') f16x2 dilated with")
    say("# both bounds handed over")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# work = R 343 cin cout products per tap; ratio = (a) over (c); verdict of (c) against (a): medians apart by more than the sum of")
    say("# the spreads; of f16 peak: 3 x 2 x 27 cin cout x voxels FLOP over the (c) / (c') median; ws MiB: (c) / (a)")
    say("%-10s %9s %5s %11s | %-23s | %-23s | %-23s | %5s %-13s %6s %6s %11s"
        % ("layer", "channels", "R", "work", "(a) fp32 dilated", "(c) f16x2 dilated", "(c') bounds given", "ratio", "verdict", "peak c", "c'", "ws MiB"))
    torch.manual_seed(0)
    inside = True
    rows = []
    for name, cin, cout, rois in SHAPES:
        for R in rois:
            x = torch.relu(torch.randn(R, cin, 7, 7, 7, device="cuda"))
            gy = torch.randn(R, cout, 7, 7, 7, device="cuda")
            xm, gm = ops.ZwConv3d.bound_of(x), ops.ZwConv3d.bound_of(gy)
            variants = (("a", lambda: ops.conv3d_wgrad(x, gy, 3, dilation=2)),
                        ("c", lambda: ops.conv3d_wgrad_narrow_f16x2(x, gy, dilation=2)),
                        ("c'", lambda: ops.conv3d_wgrad_narrow_f16x2(x, gy, xm, gm, dilation=2)))
            r = measure(variants)
            work = R * 343 * cin * cout
            flop = 3 * 2.0 * 27 * cin * cout * 343 * R
            ws_c = ops.lib().m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(R, cin, cout, 7, 7, 7, 2) / 2.0 ** 20
            ws_a = ops.lib().m3d_conv3d_wgrad_dilated_workspace_bytes(R, cin, cout, 7, 7, 7, 3, 2) / 2.0 ** 20
            v = verdict(r["c"], r["a"])
            rows.append((work, v))
            say("%-10s %4d->%-3d %5d %11d | %-23s | %-23s | %-23s | %5.2f %-13s %5.1f%% %5.1f%% %5.1f/%-5.1f"
                % (name, cin, cout, R, work, cell(r["a"]), cell(r["c"]), cell(r["c'"]), r["a"][0] / r["c"][0], v,
                   100.0 * flop / (r["c"][0] * 1e-3) / F16_PEAK, 100.0 * flop / (r["c'"][0] * 1e-3) / F16_PEAK, ws_c, ws_a))
            if R == ACCURACY_R:
                rnd = random.Random(R * cin + cout)
                picks = [(rnd.randrange(cout), rnd.randrange(cin), rnd.randrange(27)) for _ in range(a.samples)]
                xp = torch.nn.functional.pad(x, (2, 2, 2, 2, 2, 2))
                ref = torch.zeros(a.samples, dtype=torch.float64, device="cuda")
                for i, (co, ci, tap) in enumerate(picks):                         # no host synchronisation inside the loop
                    dz, dy, dx = 2 * (tap // 9), 2 * (tap // 3 % 3), 2 * (tap % 3)
                    ref[i] = (gy[:, co].double() * xp[:, ci, dz:dz + 7, dy:dy + 7, dx:dx + 7].double()).sum()
                idx = torch.tensor(picks, device="cuda")
                got = {"a": ops.conv3d_wgrad(x, gy, 3, dilation=2), "c": ops.conv3d_wgrad_narrow_f16x2(x, gy, dilation=2)}
                top = float(got["a"].abs().max())
                worst = {k: float((t.reshape(cout, cin, 27)[idx[:, 0], idx[:, 1], idx[:, 2]].double() - ref).abs().max()) / top
                         for k, t in got.items()}
                inside = inside and worst["c"] <= ENVELOPE
                say("#   error at R = %d, %d elements against fp64, |error| / max |dW|: (c) %.3g (%s the %.0e envelope), (a) %.3g"
                    % (R, a.samples, worst["c"], "within" if worst["c"] <= ENVELOPE else "OUTSIDE", ENVELOPE, worst["a"]))
                del xp, ref, got
            if (cin, cout, R) == HALO_ROW:
                h = measure((("d1", lambda: ops.conv3d_wgrad_narrow_f16x2(x, gy)), ("d2", lambda: ops.conv3d_wgrad_narrow_f16x2(x, gy, dilation=2)),
                             ("d1'", lambda: ops.conv3d_wgrad_narrow_f16x2(x, gy, xm, gm)),
                             ("d2'", lambda: ops.conv3d_wgrad_narrow_f16x2(x, gy, xm, gm, dilation=2))))
                say("#   the wider halo at %d->%d, R = %d: dilation 1 %s, dilation 2 %s, %.2f x (%s); bounds given: %s, %s, %.2f x"
                    % (cin, cout, R, cell(h["d1"]), cell(h["d2"]), h["d2"][0] / h["d1"][0],
                       {"wins": "dilation 2 faster", "LOSES": "dilation 2 slower", "no separation": "no separation"}[verdict(h["d2"], h["d1"])],
                       cell(h["d1'"]), cell(h["d2'"]), h["d2'"][0] / h["d1'"][0]))
            del x, gy
            torch.cuda.empty_cache()
    # the routing threshold the table gives: the work of the smallest measured shape at which (c) wins, provided every larger one wins too
    rows.sort()
    thr = None
    for i, (work, v) in enumerate(rows):
        if all(w == "wins" for _, w in rows[i:]):
            thr = work
            break
    say("# threshold from this table: %s (conv_plan.WGRAD_DILATED_F16X2_MIN_WORK is %d)"
        % ("no measured shape from which every row wins" if thr is None else "%d products per tap" % thr, conv_plan.WGRAD_DILATED_F16X2_MIN_WORK))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not inside:
        sys.exit("the dilated f16x2 weight gradient left the %.0e envelope: the chain and fold design does not hold" % ENVELOPE)


if __name__ == "__main__":
    main()
