#!/usr/bin/env python3
"""Times the RoIAlign3D backward at the training shapes: the atomic path as a user gets it (m3d.roi_align3d_backward: torch.zeros + the
scatter kernel of csrc/roi_align3d.hip) beside the ordered path (m3d.roi_align3d_backward_ordered: torch.empty, the prologue launch and
the gather kernel of csrc/roi_align3d_bwd.hip).  DESIGN.md, "RoIAlign3D backward, ordered".

Shapes: the nuclei box head (256 channels, 16^3 map at stride 8, 64 sampled RoIs per image, 7^3 bins, sampling grid 2) with 2 and 4
images; the soma tile's map (128 channels, 16 x 64 x 64 at stride 4) with the box head's 64 RoIs per image and with the mask branch's
RoIAlign (MRCNN.ROI_XFORM_RESOLUTION 7, the foreground RoIs only: 16 per image); and 14^3 bins on the nuclei map (more than 1024 bins:
the ordered kernel reads `top` from global memory instead of staging it).
RoIs are seeded and drawn like the proposals tools/train_detector.py trains on: an anchor size of the config's RPN.SIZES per box,
every edge scaled by exp(0.2 randn), the centre uniform in the image, clipped to the image; no edge shorter than 4 voxels.

Protocol of tools/bench_sgd.py: warm-up, then `--reps` repetitions with the two paths alternating inside every repetition; each
measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median and spread
(min .. max) in ms.  Also printed: the largest |ordered - atomic| relative to the largest |gradient|, and whether two ordered calls are
bit-equal.  Needs a GPU; there is no CPU path."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))

NUCLEI_SIZES = (10, 27, 33, 38, 42, 46, 50)
SOMA_SIZES = (10, 12, 14, 16, 18, 20, 22, 24, 28, 30, 34, 36, 38, 40)

# name, images, channels, map (S, H, W), stride, RoIs per image, bins, anchor sizes
SHAPES = (
    ("nuclei box head, B = 2", 2, 256, (16, 16, 16), 8, 64, 7, NUCLEI_SIZES),
    ("nuclei box head, B = 4", 4, 256, (16, 16, 16), 8, 64, 7, NUCLEI_SIZES),
    ("soma tile, box head", 2, 128, (16, 64, 64), 4, 64, 7, SOMA_SIZES),
    ("soma tile, mask branch", 2, 128, (16, 64, 64), 4, 16, 7, SOMA_SIZES),
    ("nuclei map, 14^3 bins", 2, 256, (16, 16, 16), 8, 16, 14, NUCLEI_SIZES),
)


def draw_rois(rs, images, per_image, dims, stride, sizes):
    """fp32 [images * per_image, 7]: (batch, x1, y1, z1, x2, y2, z2) in image voxels, grouped by image like BoxHeadTargets.rois7"""
    S, H, W = dims
    ext = np.array([W, H, S], np.float64) * stride
    rows = []
    for b in range(images):
        for _ in range(per_image):
            while True:
                edge = rs.choice(sizes) * np.exp(0.2 * rs.randn(3))
                ctr = rs.uniform(0, 1, 3) * ext
                lo, hi = np.clip(ctr - edge / 2, 0, ext - 1), np.clip(ctr + edge / 2, 0, ext - 1)
                if (hi - lo).min() >= 4:
                    break
            rows.append([b, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]])
    return np.array(rows, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    import m3d
    assert torch.cuda.is_available(), "bench_roi_align_backward needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("# RoIAlign3D backward: atomic (torch.zeros + m3d_roi_align3d_backward) beside ordered (torch.empty + m3d_roi_align3d_backward_ordered)")
    say("# %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# diff = max |ordered - atomic| / max |atomic|; repro = two ordered calls bit-equal")
    say("%-26s %-8s | %-28s | %9s %5s" % ("shape", "path", "ms per call", "diff", "repro"))

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    for name, B, Cc, dims, stride, per_image, res, sizes in SHAPES:
        rs = np.random.RandomState(a.seed)
        rois = torch.from_numpy(draw_rois(rs, B, per_image, dims, stride, sizes)).cuda()
        top = torch.from_numpy(rs.randn(rois.shape[0], Cc, res, res, res).astype(np.float32)).cuda()
        shape = (B, Cc) + dims
        paths = {
            "atomic": lambda: m3d.roi_align3d_backward(top, rois, shape, res, res, res, 1.0 / stride, 2),
            "ordered": lambda: m3d.roi_align3d_backward_ordered(top, rois, shape, res, res, res, 1.0 / stride, 2),
        }
        ga, go, go2 = paths["atomic"](), paths["ordered"](), paths["ordered"]()
        diff = float((go - ga).abs().max() / ga.abs().max())
        repro = bool(torch.equal(go, go2))
        del ga, go, go2
        times = {n: [] for n in paths}
        names = list(paths)
        for i in range(a.warmup + a.reps):
            for n in names[i % 2:] + names[:i % 2]:
                t = timed(paths[n])
                if i >= a.warmup:
                    times[n].append(t)
        for n in names:
            say("%-26s %-8s | %-28s | %9.2e %5s" % (name, n, "%.3f (%.3f .. %.3f)" % (statistics.median(times[n]), min(times[n]), max(times[n])),
                                                  diff, "yes" if repro else "NO"))
        ma, mo = statistics.median(times["atomic"]), statistics.median(times["ordered"])
        say("# %s: R = %d, atomic / ordered = %.1f; spreads %.3f .. %.3f against %.3f .. %.3f ms"
            % (name, rois.shape[0], ma / mo, min(times["atomic"]), max(times["atomic"]), min(times["ordered"]), max(times["ordered"])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
