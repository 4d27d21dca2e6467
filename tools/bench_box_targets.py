#!/usr/bin/env python3
"""Times the box-head training step (csrc/box_head_train.hip).  profiles/box_head_targets.txt is this tool's output plus notes.

For both shipped shapes (nuclei: 40 boxes, batch 64; soma: 60 boxes, batch 128; 2000 proposals per image, B = 2 images), HIP-event
times after a warm-up (median of --iters), milliseconds per call:
  targets_ms   m3d.box_head_targets on device-resident proposals and boxes: two launches (label, select) and five output allocations;
  loss_ms      m3d.box_head_losses forward: two memsets and one launch (three results and both gradients);
  blobs_ms     BoxHeadTargets.blobs(): the dense export, one launch;
and next to them what the reference's host detour costs on this host's CPU, wall time, median of --iters:
  numpy_ms     the proposals' device -> host copy, the NumPy restatement of labelling and sampling for the B images
               (tests/box_head_train_reference.py: an IoU matrix per image, as add_proposals builds one), the dense blobs, and the
               host -> device copy of the five blobs.
Nothing is asserted about either number."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

TILE = (64, 256, 256)
SHAPES = [("nuclei", 40), ("soma", 60)]


def make_inputs(seed, K, n):
    """K boxes; n proposals: jittered copies of the boxes plus random boxes"""
    from bench_rpn_targets import boxes
    rng = np.random.RandomState(seed)
    gt = boxes(seed, K, TILE)
    copies = n // (5 * K)
    jit = np.repeat(gt, copies, 0) + rng.uniform(-4, 4, (K * copies, 6))
    rest = boxes(seed + 1, n - len(jit), TILE) + rng.uniform(-0.5, 0.5, (n - len(jit), 6))
    return gt, np.concatenate([jit, rest], 0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--proposals", type=int, default=2000)
    ap.add_argument("--no-cpu", action="store_true", help="skip the NumPy restatement")
    a = ap.parse_args()
    import torch
    import m3d
    import box_head_train_reference as BR
    from bench_rpn_targets import time_gpu
    assert torch.cuda.is_available(), "bench_box_targets needs a GPU"
    B, n = a.images, a.proposals
    print("# box-head training step, %d images, %d proposals each, iters %d, device %s" % (B, n, a.iters, torch.cuda.get_device_name(0)))
    print("# config  K  batch  rows  fg  bg  fg_cand  bg_cand | targets_ms  loss_ms  blobs_ms | numpy_ms")
    for name, K in SHAPES:
        cfg = getattr(m3d.BoxHeadTrainCfg, name)()
        rc = BR.make_cfg(cfg.batch_per_im, cfg.fg_fraction, cfg.fg_thresh, cfg.bg_thresh_hi, cfg.bg_thresh_lo, cfg.num_classes, cfg.bbox_reg_weights)
        ins = [make_inputs(10 * K + b, K, n) for b in range(B)]
        rois = np.zeros((B, n, 7), np.float32)
        for b, (_, pr) in enumerate(ins):
            rois[b, :, 0], rois[b, :, 1:] = b, pr
        d_rois, d_num = torch.from_numpy(rois).cuda(), torch.full((B,), n, dtype=torch.int32, device="cuda")
        d_gt = [torch.from_numpy(gt).cuda() for gt, _ in ins]
        T = m3d.box_head_targets(d_rois, d_num, d_gt, cfg, 1)
        N, C = B * cfg.batch_per_im, cfg.num_classes
        score, pred = torch.randn(N, C, device="cuda"), torch.randn(N, 6 * C, device="cuda")
        c = T.counts.cpu().numpy()[0]
        t_targets = time_gpu(lambda: m3d.box_head_targets(d_rois, d_num, d_gt, cfg, 1), a.iters)
        t_loss = time_gpu(lambda: m3d.box_head_losses(score, pred, T), a.iters)
        t_blobs = time_gpu(lambda: T.blobs(), a.iters)
        t_np = float("nan")
        if not a.no_cpu:
            def host_detour():
                host = d_rois.cpu().numpy()                                   # the proposals go .numpy()
                blobs = []
                for b, (gt, _) in enumerate(ins):
                    S = BR.box_head_targets(gt, host[b, :, 1:], rc, 1 + b)
                    blobs.append((S["labels"], np.concatenate([np.full((len(S["rois"]), 1), b, np.float32), S["rois"]], 1)) + BR.blobs(S, rc))
                out = [torch.from_numpy(np.concatenate([bl[i] for bl in blobs], 0)).cuda() for i in range(5)]   # five blobs go back
                torch.cuda.synchronize()
                return out
            host_detour()
            ts = []
            for _ in range(a.iters):
                t0 = time.perf_counter()
                host_detour()
                ts.append((time.perf_counter() - t0) * 1e3)
            t_np = float(np.median(ts))
        print("%-7s %3d %5d %5d %4d %4d %6d %6d | %8.3f %8.3f %8.3f | %8.2f" % (
            name, K, cfg.batch_per_im, c[0], c[1], c[2], c[3], c[4], t_targets, t_loss, t_blobs, t_np))


if __name__ == "__main__":
    main()
