#!/usr/bin/env python3
"""Times the backward of the box head's FC layers on the f16 matrix cores (csrc/fc_backward_f16.hip, the "f16x2" cut) against the fp32
MFMA kernels it can replace (csrc/fc_backward.hip) and against torch, in one process, with the protocol of
tools/bench_linear_backward.py: warm-up, then `--reps` repetitions with the variants alternating inside every repetition; each
measurement is the time between two device events around `--inner` consecutive backwards, divided by `--inner`; median (min .. max), ms.

Rows: fc1 of the nuclei detector (128 x 1024 x 87 808) and of the soma detector (256 x 1024 x 43 904), fc2 (128 x 1024 x 1024), and
M = 64 and 512 at the nuclei K.  Variants, each giving gx, gw and gb from gy [M,N], W [N,K] and x [M,K]:

  f16x2        what m3d.compat runs with the switch on and max|W| cached: one sweep of gy shared by both GEMMs, x swept by the wgrad
               call - both INSIDE the window -, the weight's bound given
  f16x2+wsweep the same with the weight's sweep inside the window too (the first backward after a weight update that nobody cached)
  fp32         ops.linear_dgrad + ops.linear_wgrad
  torch        gy @ W, gy.t() @ x, gy.sum(0)
  dgrad / wgrad alone: "f16x2 dgrad" (gy swept inside, max|W| given), "fp32 dgrad", "f16x2 wgrad" (gy and x swept inside), "fp32 wgrad"

Beside them, from the sizes alone: "bytes" = every operand of both GEMMs moved once ((N K + M K + M N) x 4 each) at 6.3 TB/s, "f16 mfma"
= 3 x 4 M N K FLOP at the 2.5 PFLOP/s of the dense f16 MFMA.  A row counts as a win only where the medians separate by more than the sum
of the two spreads (max - min); conv_plan.LINEAR_BACKWARD_F16X2_MIN_WORK is the M N K of the smallest row where "f16x2" wins against
"fp32".  The error sample: `--samples` outputs of gx and of gw at the full fc1 size against fp64, as the largest |error| / sum |a b| in
units of 2^-24, for both kernels.  The record in the repository: `--out profiles/linear_backward_f16.txt`.  Needs a GPU."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
HBM_PEAK, F16_PEAK = 6.3e12, 2.5e15

SHAPES = [("fc2", 128, 1024, 1024), ("fc1 M=64", 64, 1024, 87808), ("nuclei fc1", 128, 1024, 87808), ("soma fc1", 256, 1024, 43904),
          ("fc1 M=512", 512, 1024, 87808)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="backwards per timed window")
    ap.add_argument("--samples", type=int, default=256, help="outputs of each GEMM compared with fp64")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    from m3d import ops
    assert torch.cuda.is_available(), "bench_linear_backward_f16 needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def f16_cached(gy, w, x, wmax):
        gm = ops.absmax(gy)
        gx = ops.linear_dgrad_f16x2(gy, w, gm, wmax)
        gw, gb = ops.linear_wgrad_f16x2(gy, x, gm, None)
        return gx, gw, gb

    def f16_wsweep(gy, w, x, wmax):
        gm = ops.absmax(gy)
        gx = ops.linear_dgrad_f16x2(gy, w, gm, None)
        gw, gb = ops.linear_wgrad_f16x2(gy, x, gm, None)
        return gx, gw, gb

    def fp32(gy, w, x, wmax):
        gx = ops.linear_dgrad(gy, w)
        gw, gb = ops.linear_wgrad(gy, x)
        return gx, gw, gb

    def plain(gy, w, x, wmax):
        return gy @ w, gy.t() @ x, gy.sum(0)
    variants = (("f16x2", f16_cached), ("f16x2+wsweep", f16_wsweep), ("fp32", fp32), ("torch", plain),
                ("f16x2 dgrad", lambda gy, w, x, wmax: ops.linear_dgrad_f16x2(gy, w, None, wmax)),
                ("fp32 dgrad", lambda gy, w, x, wmax: ops.linear_dgrad(gy, w)),
                ("f16x2 wgrad", lambda gy, w, x, wmax: ops.linear_wgrad_f16x2(gy, x, None, None)),
                ("fp32 wgrad", lambda gy, w, x, wmax: ops.linear_wgrad(gy, x)))

    def timed(fn, args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.inner):
            fn(*args)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    def sample_error(gy, w, x, got_gx, got_gw):
        """largest |error| / sum |a b| over a.samples outputs of each GEMM, in units of 2^-24 (fp64 reference on the device)"""
        M, N = gy.shape
        K = w.shape[1]
        gen = torch.Generator().manual_seed(1)                             # the same outputs for both kernels
        k = torch.randint(0, K, (a.samples,), generator=gen).cuda()
        m = torch.randint(0, M, (a.samples,), generator=gen).cuda()
        n = torch.randint(0, N, (a.samples,), generator=gen).cuda()
        g64, out = gy.double(), []
        wc = w[:, k].double()                                              # [N, S]
        ref, mag = (g64[m] * wc.t()).sum(1), (g64[m].abs() * wc.t().abs()).sum(1)
        out.append(float(((got_gx[m, k].double() - ref).abs() / mag).max()) * 2.0 ** 24)
        xc = x[:, k].double()                                              # [M, S]
        ref, mag = (g64[:, n] * xc).sum(0), (g64[:, n].abs() * xc.abs()).sum(0)
        out.append(float(((got_gw[n, k].double() - ref).abs() / mag).max()) * 2.0 ** 24)
        return out

    say("# backward of nn.Linear on the f16 matrix cores (f16x2 cut) against the fp32 MFMA kernels and torch; gy [M,N], W [N,K], x [M,K], fp32")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# f16x2: gy and x sweeps inside the window, max|W| given; f16x2+wsweep: the weight's sweep inside too")
    say("# bytes = every operand of both GEMMs once at 6.3 TB/s; f16 mfma = 3 x 4 M N K FLOP at 2.5 PFLOP/s")
    say("%-11s %4s %5s %6s %-13s | %-28s | %8s %8s" % ("layer", "M", "N", "K", "variant", "ms per call", "bytes ms", "f16 mfma"))
    torch.manual_seed(0)
    wins = []
    for name, M, N, K in SHAPES:
        gy = torch.randn(M, N, device="cuda") * 2.0 ** -10
        w = torch.randn(N, K, device="cuda") * 0.01
        x = torch.randn(M, K, device="cuda")
        args = (gy, w, x, ops.absmax(w))
        times = {v: [] for v, _ in variants}
        for i in range(a.warmup + a.reps):
            order = variants[i % len(variants):] + variants[:i % len(variants)]
            for v, fn in order:
                t = timed(fn, args)
                if i >= a.warmup:
                    times[v].append(t)
        t_bytes = 2 * 4.0 * (N * K + M * K + M * N) / HBM_PEAK * 1e3
        t_mfma = 3 * 4.0 * M * N * K / F16_PEAK * 1e3
        res = {}
        for v, _ in variants:
            med, lo, hi = statistics.median(times[v]), min(times[v]), max(times[v])
            res[v] = (med, hi - lo)
            half = 0.5 if ("dgrad" in v or "wgrad" in v) else 1.0
            say("%-11s %4d %5d %6d %-13s | %-28s | %8.3f %8.3f"
                % (name, M, N, K, v, "%.3f (%.3f .. %.3f)" % (med, lo, hi), half * t_bytes, half * t_mfma))
        for mine, other in (("f16x2", "fp32"), ("f16x2", "torch"), ("f16x2+wsweep", "fp32"), ("f16x2 dgrad", "fp32 dgrad"),
                            ("f16x2 wgrad", "fp32 wgrad")):
            (ma, sa), (mb, sb) = res[mine], res[other]
            verdict = "WINS" if ma < mb - (sa + sb) else ("LOSES" if mb < ma - (sa + sb) else "no separation")
            say("# %s: %s %.3f ms against %s %.3f ms (%.2f x), spreads %.3f + %.3f ms: %s" % (name, mine, ma, other, mb, mb / ma, sa, sb, verdict))
            if (mine, other) == ("f16x2", "fp32") and verdict == "WINS":
                wins.append((M * N * K, name, M, N, K))
        if "fc1" in name and M in (128, 256):
            e16 = sample_error(gy, w, x, *f16_cached(*args)[:2])
            e32 = sample_error(gy, w, x, *fp32(*args)[:2])
            say("# %s: largest |error| / sum|a b| over %d sampled outputs, x 2^-24: f16x2 gx %.3f gw %.3f; fp32 kernels gx %.3f gw %.3f"
                % (name, a.samples, e16[0], e16[1], e32[0], e32[1]))
        del gy, w, x, args
        torch.cuda.empty_cache()
    if wins:
        work, name, M, N, K = min(wins)
        say("# smallest row where f16x2 wins against fp32: %s (%d x %d x %d), M N K = %d" % (name, M, N, K, work))
    else:
        say("# f16x2 wins against fp32 on no row")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
