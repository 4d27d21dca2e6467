#!/usr/bin/env python3
"""Times the backward of the box head's nn.Linear layers at the shipped training shapes (IMS_PER_BATCH = 2 x BATCH_SIZE_PER_IM rows):
fc1 of the nuclei detector (128 x 1024 x 87 808) and of the soma detector (256 x 1024 x 43 904), fc2 (128 x 1024 x 1024) and the two
heads (cls_score N = 2, bbox_pred N = 12; K = 1024).  Three ways to get gx, gw and gb from gy [M,N], W [N,K] and x [M,K]:

  (a) m3d      ops.linear_dgrad + ops.linear_wgrad (csrc/fc_backward.hip): two launches (plus a reduce each where the reduction is split)
  (b) parent   what _LinearFn.backward did before these kernels, restated here: ops.linear on W.t().contiguous() and on
               gy.t().contiguous(), x.t().contiguous() where the forward kernel's K % 4 rule allows, else gy @ W / gy.t() @ x; gy.sum(0)
  (c) torch    gy @ W, gy.t() @ x, gy.sum(0)

Protocol of tools/bench_sgd.py: warm-up, then `--reps` repetitions with the variants alternating inside every repetition; each
measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median and spread (min ..
max) in ms.  Beside them, from the sizes alone and without a threshold on either: "bytes" = every operand moved once ((N K + M K + M N)
x 4 per GEMM) at 6.3 TB/s, "mfma" = 2 x 2 M N K FLOP at the 157 TFLOP/s of v_mfma_f32_32x32x2_f32.
The requirement is taken against (b), never against the code under test: at both fc1 shapes the median of (a) lies below that of (b) by
more than the sum of the two spreads (max - min).  "peak MB" is torch.cuda.max_memory_allocated over one backward minus what was
allocated before it.  The record in the repository: `--out profiles/linear_backward.txt`.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
HBM_PEAK, MFMA_PEAK = 6.3e12, 157e12

SHAPES = [("nuclei fc1", 128, 1024, 87808), ("soma fc1", 256, 1024, 43904), ("fc2", 128, 1024, 1024),
          ("cls_score", 128, 2, 1024), ("bbox_pred", 128, 12, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    from m3d import ops
    assert torch.cuda.is_available(), "bench_linear_backward needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def new(gy, w, x):
        gx = ops.linear_dgrad(gy, w)
        gw, gb = ops.linear_wgrad(gy, x)
        return gx, gw, gb

    def parent(gy, w, x):
        gx = ops.linear(gy, w.t().contiguous()) if gy.shape[1] % 4 == 0 else gy @ w
        gw = ops.linear(gy.t().contiguous(), x.t().contiguous()) if gy.shape[0] % 4 == 0 else gy.t() @ x
        return gx, gw, gy.sum(0)

    def plain(gy, w, x):
        return gy @ w, gy.t() @ x, gy.sum(0)
    variants = (("m3d", new), ("parent", parent), ("torch", plain))

    def timed(fn, args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.inner):
            fn(*args)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    def peak(fn, args):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        out = fn(*args)
        torch.cuda.synchronize()
        del out
        return (torch.cuda.max_memory_allocated() - before) / 1e6

    say("# backward of nn.Linear: gx = gy W, gw = gy^T x, gb = sum gy; gy [M,N], W [N,K], x [M,K], fp32")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per backward between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# bytes = every operand once at 6.3 TB/s; mfma = 4 M N K FLOP at 157 TFLOP/s; peak MB = max_memory_allocated over one backward")
    say("%-11s %5s %5s %6s %-7s | %-28s %9s | %8s %8s" % ("layer", "M", "N", "K", "variant", "ms per backward", "peak MB", "bytes ms", "mfma ms"))
    torch.manual_seed(0)
    for name, M, N, K in SHAPES:
        gy = torch.randn(M, N, device="cuda") * 2.0 ** -10
        w = torch.randn(N, K, device="cuda") * 0.01
        x = torch.randn(M, K, device="cuda")
        args = (gy, w, x)
        times = {v: [] for v, _ in variants}
        for i in range(a.warmup + a.reps):
            order = variants[i % len(variants):] + variants[:i % len(variants)]
            for v, fn in order:
                t = timed(fn, args)
                if i >= a.warmup:
                    times[v].append(t)
        t_bytes = 2 * 4.0 * (N * K + M * K + M * N) / HBM_PEAK * 1e3
        t_mfma = 4.0 * M * N * K / MFMA_PEAK * 1e3
        res = {}
        for v, fn in variants:
            med, lo, hi = statistics.median(times[v]), min(times[v]), max(times[v])
            res[v] = (med, hi - lo)
            say("%-11s %5d %5d %6d %-7s | %-28s %9.1f | %8.3f %8.3f"
                % (name, M, N, K, v, "%.3f (%.3f .. %.3f)" % (med, lo, hi), peak(fn, args) if v != "torch" else float("nan"), t_bytes, t_mfma))
        if "fc1" in name:
            (ma, sa), (mb, sb) = res["m3d"], res["parent"]
            ok = ma < mb - (sa + sb)
            say("# %s: m3d %.3f ms against parent %.3f ms, spreads %.3f + %.3f ms: the requirement (median below by more than the sum of "
                "the spreads) %s" % (name, ma, mb, sa, sb, "holds" if ok else "DOES NOT HOLD"))
        del gy, w, x, args
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
