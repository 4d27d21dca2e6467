#!/usr/bin/env python3
"""Times peak stimulation (lib/prm/peak_stimulation_3d.py:6-52) on the two shipped class response maps - nuclei [1,A,16,16,16] (a 128^3
tile at stride 8) and the soma tile's [1,A,16,40,40] (TEST.IN_SIZE at stride 4), A and the strides from m3d/config.py - with the
reference's defaults (win 3, median filter):

  m3d                 m3d.peak_stimulation_3d: five launches of csrc/peak_stim.hip and one host read (the count, pinned mirror + event)
  m3d, no host read   m3d.peak_stimulation_3d_dev with a fixed cap: the same launches, nothing waited for
  torch composition   the reference's own statements on the device: ConstantPad3d(-inf), max_pool3d(stride 1, return_indices),
                      indices == arange volume, torch.median threshold, torch.nonzero (a host read), masked mean

Protocol of tools/bench_sgd.py: warm-up, then `--reps` repetitions with the variants alternating inside every repetition; each
measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median and spread
(min .. max) in ms - the time of a call as a user sees it on an idle stream, host issue time included where the kernels are shorter.
"MB" is what the variant must move, counted from the sizes (n = elements): m3d reads x for the thresholds (4 radix passes), for the map
and for the sums (6 x 4n), writes and twice reads the byte map (3n); the composition writes the padded copy, reads it, writes int64
indices, reads them and the int64 arange volume, writes and reads a bool map, sorts for the median (counted as one read), reads x and
the map for the mean.  An accounting figure, not a counter reading.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--win", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    import m3d
    from m3d.config import Cfg
    assert torch.cuda.is_available(), "bench_peak_stimulation needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def composition(x, win):
        o = win // 2
        p = F.pad(x, (o,) * 6, value=float("-inf"))
        b, c, s, h, w = p.shape
        el = torch.arange(0, s * h * w, device=x.device).view(1, 1, s, h, w)[:, :, o:s - o, o:h - o, o:w - o]
        _, ind = F.max_pool3d(p, kernel_size=win, stride=1, return_indices=True)
        pm = ind == el
        thr = x.view(b, c, -1).median(2)[0].view(b, c, 1, 1, 1)
        pm = pm & (x >= thr)
        peaks = torch.nonzero(pm)
        pf = pm.float()
        return peaks, (x * pf).view(b, c, -1).sum(2) / pf.view(b, c, -1).sum(2)

    nuc, soma = Cfg.nuclei(), Cfg.soma()
    shapes = [("nuclei", (1, nuc.num_anchors) + tuple(v // nuc.stride for v in (128, 128, 128))),
              ("soma tile", (1, soma.num_anchors) + tuple(v // soma.stride for v in soma.in_size))]
    say("# peak stimulation, win %d, median filter; %d warm-up + %d alternating repetitions of %d calls; ms per call between device events: "
        "median (min .. max)" % (a.win, a.warmup, a.reps, a.inner))
    say("%-10s %-18s %-18s | %-28s %8s %7s" % ("map", "shape", "variant", "ms per call", "MB", "peaks"))
    torch.manual_seed(0)
    for tag, shp in shapes:
        x = torch.sigmoid(torch.randn(shp, device="cuda") * 4)
        n = x.numel()
        o = a.win // 2
        npad = shp[0] * shp[1] * (shp[2] + 2 * o) * (shp[3] + 2 * o) * (shp[4] + 2 * o)
        pk, agg = m3d.peak_stimulation_3d(x, True, a.win, "median")
        rp, ragg = composition(x, a.win)
        same = torch.equal(pk, rp) and torch.allclose(agg, ragg, rtol=1e-5, atol=0, equal_nan=True)
        cap = int(pk.shape[0]) + 64
        variants = {
            "m3d": (lambda: m3d.peak_stimulation_3d(x, True, a.win, "median"), 27.0 * n),
            "m3d, no host read": (lambda: m3d.peak_stimulation_3d_dev(x, a.win, "median", cap=cap), 27.0 * n),
            "torch composition": (lambda: composition(x, a.win), 4.0 * n + 8.0 * npad + 24.0 * n + 2.0 * n + 4.0 * n + 9.0 * n),
        }

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / a.inner
        names = list(variants)
        times = {k: [] for k in names}
        for i in range(a.warmup + a.reps):
            for name in names[i % len(names):] + names[:i % len(names)]:
                t = timed(variants[name][0])
                if i >= a.warmup:
                    times[name].append(t)
        res = {}
        for name in names:
            t = times[name]
            res[name] = (statistics.median(t), min(t), max(t))
            say("%-10s %-18s %-18s | %-28s %8.2f %7d" % (tag, "x".join(str(v) for v in shp), name, "%.4f (%.4f .. %.4f)" % res[name],
                                                           variants[name][1] / 1e6, pk.shape[0]))
        mine, other = res["m3d"], res["torch composition"]
        apart = mine[2] < other[1] or other[2] < mine[1]
        say("# %s: same peak list and aggregation as the composition: %s; torch composition / m3d = %.2f; the spreads (%.4f .. %.4f "
            "against %.4f .. %.4f ms) %s" % (tag, same, other[0] / mine[0], mine[1], mine[2], other[1], other[2],
                                             "do not overlap: the ratio exceeds the spread" if apart else
                                             "overlap: the ratio does not exceed the spread"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
