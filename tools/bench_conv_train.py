#!/usr/bin/env python3
"""Times the forward and the backward-data conv of a training layer on the f16x2 kernel (m3d.compat.set_conv_train("f16x2"):
m3d_conv3d_zw_forward, csrc/conv3d_zw.hip) against the direct fp32 MFMA kernel they are an option for, times the two small kernels of
that mode alone, and samples the error at full size.  The table behind the rule of m3d.conv_plan.train_conv_kernel.

Layers (those of tools/bench_wgrad_f16.py): the six 3^3 layers of the stride-8 body (m3d.train.DsnBody, width 32) on one 128^3 volume
and on four, the four 3^3 layers of the stride-4 soma body on its 64 x 256 x 256 tile, and, to find where the rule has to stop, the
stride-8 body on a 32 x 64 x 64 tile.  Per layer and direction, what m3d.compat runs in each mode:

  forward  f16x2   ZwConv3d.bound_of(x) (one sweep) + ZwConv3d(w)(x, x_max, shift=bias)
           fp32    PackedConv3d(w, W_PLAIN)(x, shift=bias)
  dgrad    f16x2   conv3d_gy_reduce(gy) (bias gradient + bound, one pass) + ZwConv3d.dgrad_of(w)(gy, gy_max)
           fp32    PackedConv3d(w, W_DGRAD)(gy) + conv3d_bias_grad(gy)

each with the weight pack made once outside the timed window, and again ("+pack") with the pack made inside it, as a training step does
after every weight update.  Protocol of tools/bench_wgrad_f16.py: warm-up, then `--reps` repetitions with the variants alternating inside
every repetition; a measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median
and spread (max - min) in ms.  "wins" = the f16x2 +pack median lies below the fp32 +pack median by more than the sum of the two spreads.

Accuracy (on by default): conv2b and conv4b on four 128^3 volumes, x = relu(N(0,1)), gy ~ N(0,1); 256 seeded output elements of each
direction recomputed in fp64 on the device; the largest |error| / max |output| of both kernels.  The project's envelope for its f16x2
convs is 3e-6; a figure outside it ends the tool with a non-zero status.  The record in the repository: `--out
profiles/conv_train_f16.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
ENVELOPE = 3e-6

BODY8 = [("conv2a", 32, 64, 2), ("conv2b", 64, 64, 2), ("conv3a", 64, 128, 4), ("conv3b", 128, 128, 4), ("conv4a", 128, 256, 8),
         ("conv4b", 256, 256, 8)]
BODY4 = BODY8[:4]


def layers():
    out = []
    for batch in (1, 4):
        out += [("s8 %s" % n, batch, ci, co, 128 // d, 128 // d, 128 // d) for n, ci, co, d in BODY8]
    out += [("s4 %s" % n, 1, ci, co, 64 // d, 256 // d, 256 // d) for n, ci, co, d in BODY4]
    out += [("t8 %s" % n, 1, ci, co, 32 // d, 64 // d, 64 // d) for n, ci, co, d in BODY8]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window")
    ap.add_argument("--no-accuracy", dest="accuracy", action="store_false")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    from m3d import conv_plan, ops
    assert torch.cuda.is_available(), "bench_conv_train needs a GPU"
    Z = ops.ZwConv3d
    lines = []
    inside = True

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

    def race(variants):
        """{name: (median, min, max)} of the variants, alternating"""
        times = {v: [] for v, _ in variants}
        for i in range(a.warmup + a.reps):
            k = i % len(variants)
            for v, fn in variants[k:] + variants[:k]:
                t = timed(fn)
                if i >= a.warmup:
                    times[v].append(t)
        return {v: (statistics.median(t), min(t), max(t)) for v, t in times.items()}

    def cell(r):
        return "%.3f (%.3f .. %.3f)" % r

    def wins(f, p):
        return f[0] < p[0] - ((f[2] - f[1]) + (p[2] - p[1]))

    say("# forward and backward-data of a 3^3 training conv, fp32 in and out.  f16x2 = bound sweep (forward) / gy_reduce (dgrad) + the zw conv;")
    say("# fp32 = the direct MFMA kernel (+ m3d_conv3d_bias_grad for dgrad).  +pack: the weight pack inside the timed window (every training step)")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# ratio = fp32 +pack median / f16x2 +pack median; wins = the f16x2 +pack median below the fp32 +pack median by more than the sum of the spreads")
    say("%-10s %-7s %2s %4s %4s %-12s %5s | %-24s %-24s | %-24s %-24s | %6s %5s %s"
        % ("layer", "dir", "B", "cin", "cout", "map", "units", "f16x2 ms", "f16x2 +pack ms", "fp32 ms", "fp32 +pack ms", "ratio", "wins", "routed"))
    torch.manual_seed(0)
    totals = {}
    for name, B, cin, cout, D, H, W in layers():
        x = torch.relu(torch.randn(B, cin, D, H, W, device="cuda"))
        gy = torch.randn(B, cout, D, H, W, device="cuda")
        w = torch.randn(cout, cin, 3, 3, 3, device="cuda") * (2.0 / (27 * cin)) ** 0.5
        b = torch.randn(cout, device="cuda")
        for direction in ("forward", "dgrad"):
            ci, co = (cin, cout) if direction == "forward" else (cout, cin)
            if not (Z.supported(w if direction == "forward" else w.transpose(0, 1), (D, H, W))):
                continue
            units = int(ops.lib().m3d_conv3d_zw_launch_units(B, ci, co, D, H, W))
            if direction == "forward":
                zp, pp = Z(w), ops.PackedConv3d(w, ops.W_PLAIN)
                variants = [("f16x2", lambda: zp(x, Z.bound_of(x), shift=b, out_max=False)),
                            ("f16x2+pack", lambda: Z(w)(x, Z.bound_of(x), shift=b, out_max=False)),
                            ("fp32", lambda: pp(x, shift=b)),
                            ("fp32+pack", lambda: ops.PackedConv3d(w, ops.W_PLAIN)(x, shift=b))]
            else:
                zp, pp = Z.dgrad_of(w), ops.PackedConv3d(w, ops.W_DGRAD)
                variants = [("f16x2", lambda: zp(gy, ops.conv3d_gy_reduce(gy)[1], out_max=False)),
                            ("f16x2+pack", lambda: Z.dgrad_of(w)(gy, ops.conv3d_gy_reduce(gy)[1], out_max=False)),
                            ("fp32", lambda: (pp(gy), ops.conv3d_bias_grad(gy))),
                            ("fp32+pack", lambda: (ops.PackedConv3d(w, ops.W_DGRAD)(gy), ops.conv3d_bias_grad(gy)))]
            r = race(variants)
            routed = conv_plan.train_conv_kernel(direction, B, cin, cout, D, H, W, "f16x2")
            won = wins(r["f16x2+pack"], r["fp32+pack"])
            say("%-10s %-7s %2d %4d %4d %-12s %5d | %-24s %-24s | %-24s %-24s | %6.2f %5s %s"
                % (name, direction, B, cin, cout, "%dx%dx%d" % (D, H, W), units, cell(r["f16x2"]), cell(r["f16x2+pack"]), cell(r["fp32"]),
                   cell(r["fp32+pack"]), r["fp32+pack"][0] / r["f16x2+pack"][0], "yes" if won else "no", routed))
            key = "%s B=%d %s" % (name[:2], B, direction)
            tf, t3, tr = totals.get(key, (0.0, 0.0, 0.0))
            mf, m3 = r["f16x2+pack"][0], r["fp32+pack"][0]
            totals[key] = (tf + mf, t3 + m3, tr + (mf if routed == conv_plan.TRAIN_F16X2 else m3))
            del zp, pp, variants
        del x, gy, w, b
        torch.cuda.empty_cache()
    for key, (tf, t3, tr) in totals.items():
        say("# %s: sum of the +pack medians, all layers on f16x2 %.3f ms, all on fp32 %.3f ms, as routed by conv_plan.train_conv_kernel %.3f ms"
            % (key, tf, t3, tr))

    say("# the two new kernels alone, ms: median (min .. max)")
    for cin, cout in ((64, 64), (128, 256), (256, 256)):
        w = torch.randn(cout, cin, 3, 3, 3, device="cuda")
        r = race([("new", lambda: Z.dgrad_of(w)), ("old", lambda: Z(w.flip(2, 3, 4).transpose(0, 1).contiguous()))])
        say("pack_dgrad cin %d cout %d: m3d_conv3d_zw_pack_dgrad %s | torch flip + transpose + m3d_conv3d_zw_pack %s | %.2f x, wins %s"
            % (cin, cout, cell(r["new"]), cell(r["old"]), r["old"][0] / r["new"][0], "yes" if wins(r["new"], r["old"]) else "no"))
    for B, cout, n in ((1, 64, 64), (4, 64, 64), (4, 128, 32), (4, 256, 16), (1, 256, 16)):
        gy = torch.randn(B, cout, n, n, n, device="cuda")
        r = race([("new", lambda: ops.conv3d_gy_reduce(gy)), ("old", lambda: (Z.bound_of(gy), ops.conv3d_bias_grad(gy)))])
        gbytes = gy.numel() * 4 / 1e9
        say("gy_reduce %dx%dx%d^3 (%.0f MB): m3d_conv3d_gy_reduce %s, %.0f GB/s | bound_of + m3d_conv3d_bias_grad %s | %.2f x, wins %s"
            % (B, cout, n, gbytes * 1e3, cell(r["new"]), gbytes / (r["new"][0] * 1e-3), cell(r["old"]), r["old"][0] / r["new"][0],
               "yes" if wins(r["new"], r["old"]) else "no"))
        del gy
        torch.cuda.empty_cache()

    if a.accuracy:
        say("# sampled error at full size: B = 4, x = relu(N(0,1)), gy ~ N(0,1), w ~ N(0, 2 / (27 cin)); %d seeded output elements per direction"
            % a.samples)
        say("# against fp64 on the device; largest |error| / max |output|; the envelope of the project's f16x2 convs is %.0e" % ENVELOPE)
        g = torch.Generator().manual_seed(1)
        for name, cin, cout, d in (BODY8[1], BODY8[5]):
            n = 128 // d
            w = torch.randn(cout, cin, 3, 3, 3, device="cuda") * (2.0 / (27 * cin)) ** 0.5
            b = torch.randn(cout, device="cuda")
            x = torch.relu(torch.randn(4, cin, n, n, n, device="cuda"))
            gy = torch.randn(4, cout, n, n, n, device="cuda")
            wd = w.flip(2, 3, 4).transpose(0, 1).contiguous()
            for direction, src, wt, bias, nout in (("forward", x, w, b, cout), ("dgrad", gy, wd, None, cin)):
                if direction == "forward":
                    got = {"f16x2": Z(w)(x, Z.bound_of(x), shift=b, out_max=False)[0], "fp32": ops.PackedConv3d(w, ops.W_PLAIN)(x, shift=b)}
                else:
                    got = {"f16x2": Z.dgrad_of(w)(gy, ops.conv3d_gy_reduce(gy, bias=False)[1], out_max=False)[0],
                           "fp32": ops.PackedConv3d(w, ops.W_DGRAD)(gy)}
                sp = torch.nn.functional.pad(src, (1, 1, 1, 1, 1, 1))             # fp32 zeros around, once
                picks = torch.stack([torch.randint(0, m, (a.samples,), generator=g) for m in (4, nout, n, n, n)], 1).tolist()
                ref = torch.zeros(a.samples, dtype=torch.float64, device="cuda")
                for i, (bi, co, z, y, xx) in enumerate(picks):                    # no host synchronisation inside the loop
                    ref[i] = (sp[bi, :, z:z + 3, y:y + 3, xx:xx + 3].double() * wt[co].double()).sum()
                    if bias is not None:
                        ref[i] += bias[co].double()
                idx = torch.tensor(picks, device="cuda")
                top = float(got["fp32"].abs().max())
                worst = {v: float((t[idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3], idx[:, 4]].double() - ref).abs().max()) / top
                         for v, t in got.items()}
                inside = inside and worst["f16x2"] <= ENVELOPE
                say("%s %s 4x%d^3 cin %d cout %d: max |output| %.4g; f16x2 %.3g (%s the envelope), fp32 %.3g"
                    % (name, direction, n, cin, cout, top, worst["f16x2"], "within" if worst["f16x2"] <= ENVELOPE else "OUTSIDE", worst["fp32"]))
                del got, sp
            del x, gy, w, wd
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not inside:
        sys.exit("an f16x2 training conv left the %.0e envelope" % ENVELOPE)


if __name__ == "__main__":
    main()
