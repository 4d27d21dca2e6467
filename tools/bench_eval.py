#!/usr/bin/env python3
"""Times the label-volume evaluation path (csrc/eval3d.hip) on synthetic pairs (m3d.synth.synth_label_pair) and prints one JSON line:
  soma size   96 x 256 x 256, 2 500 GT instances;   nuclei size   59 x 350 x 350, 150 GT instances.
Per size, HIP-event times after a warm-up (median of --iters): label_overlap (one call = the voxel pass, the table passes, and the
host read of the pair count it synchronises on), label_iou_best, the whole in-memory soma AP of one volume (m3d.evaluate.soma_prec_rec,
host parts included), and box_union_overlap_counts with the TP boxes of the nuclei segmentation F1.  CPU baseline: a NumPy contingency
table (np.unique on combined keys) of the same pair, single-threaded NumPy.  HBM floor = the bytes of the two label volumes at 8 TB/s.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_eval.py --iters 5` run."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))

HBM_BYTES_PER_S = 8.0e12


def time_gpu(fn, iters):
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        out.append(s.elapsed_time(e) * 1e3)
    return float(np.median(out))


def time_cpu(fn, iters):
    out = []
    for _ in range(iters):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e6)
    return float(np.median(out))


def contingency_np(a, b):
    key = a.astype(np.int64) * (1 << 24) + b
    return np.unique(key, return_counts=True)


def tp_ranges(pred, gt, E):
    """the TP boxes' slices of the nuclei segmentation F1 (box per instance on both sides)"""
    def boxes(v):
        out = []
        for i in np.unique(v)[1:]:
            z, y, x = np.nonzero(v == i)
            out.append((x.min(), y.min(), z.min(), x.max(), y.max(), z.max()))
        return np.array(out, np.float64).reshape(-1, 6)
    gb, pb = boxes(gt), boxes(pred)
    seen = np.zeros(len(gb), bool)
    ranges = []
    for bb in pb:
        ov = E._box_overlaps(bb, gb)
        j = int(np.argmax(ov))
        if ov[j] > 0.4 and not seen[j]:
            seen[j] = True
            ranges.append(E.box_slices(bb, pred.shape))
    return np.array(ranges, np.int64).reshape(-1, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    import torch
    import m3d
    from m3d import evaluate as E
    from m3d.synth import synth_label_pair
    assert torch.cuda.is_available(), "bench_eval needs a GPU"
    rec = {"tool": "bench_eval", "iters": a.iters, "numpy_threads": 1}
    for name, shape, n in (("soma", (96, 256, 256), 2500), ("nuclei", (59, 350, 350), 150)):
        gt, pred, table = synth_label_pair(shape, n, 0)
        gd, pd = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
        ov = m3d.label_overlap(pd, gd)
        rows = table[E.score_order(table[:, 1]), 0].astype(np.int64)
        r = {"shape": list(shape), "gt_instances": int(len(np.unique(gt)) - 1), "pred_instances": int(len(table)),
             "pairs": int(ov.pairs.shape[0])}
        r["hbm_floor_us"] = 2 * gt.nbytes / HBM_BYTES_PER_S * 1e6
        r["label_overlap_us"] = time_gpu(lambda: m3d.label_overlap(pd, gd), a.iters)
        r["label_iou_best_us"] = time_gpu(lambda: m3d.label_iou_best(ov, rows), a.iters)
        r["soma_ap_us"] = time_gpu(lambda: E.soma_prec_rec([pd], [gd], [table], 0.5), a.iters)
        ranges = tp_ranges(pred, gt, E)
        r["tp_boxes"] = int(len(ranges))
        r["box_union_counts_us"] = time_gpu(lambda: m3d.box_union_overlap_counts(pd, gd, ranges), a.iters)
        r["cpu_numpy_contingency_us"] = time_cpu(lambda: contingency_np(pred, gt), max(3, a.iters // 5))
        rec[name] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
