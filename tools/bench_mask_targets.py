#!/usr/bin/env python3
"""Times the mask-branch training step (csrc/mask_train.hip).  profiles/mask_targets.txt is this tool's output once someone has run it
on an MI355X.

The two shipped shapes: soma (anno_type 'spot', B = 2 images, 32 fg rows each) and nuclei (anno_type 'mask', B = 1, 16 fg rows, a
uint16 label volume), tile 64 x 256 x 256, M = 14.  The fg rows are jittered copies of the objects' boxes, placed as the sampler's
output (no sampler runs).  Protocol of tools/bench_sgd.py: warm-up, then --reps repetitions; each measurement is the time between two
device events around --inner consecutive calls, divided by --inner; median and spread (min .. max), milliseconds per call:
  targets   m3d.mask_targets: one memset and one launch for all images, four output allocations;
  loss      m3d.mask_losses forward on logits [B fg_per_im, 1, 14, 14, 14]: three launches (partials, finish, gradient);
and beside them the wall-clock time, on this host's CPU, of the reference's host path in the restatement's direct form
(tests/mask_train_reference.py: per fg row the fill, oracle.skimage_resize_nd, the threshold) plus the upload of the int32 blob.  The
reference itself is slower than that figure: its fill is a triple Python loop (lib/utils/segms.py:141-146), here it is one NumPy
expression.  The host blob is compared with the device's first: the device must hold every voxel of it, and the count of voxels it holds
beyond (where the host path's fp32 resize underflows; DESIGN, "Mask-branch training targets") is printed.  Nothing is asserted about
the times."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("instanceseg-without-voxelwise-labeling_amd", "tests", "oracle"):
    sys.path.insert(0, os.path.join(ROOT, p))
TILE = (64, 256, 256)
SHAPES = [("soma", 2, 128, 40), ("nuclei", 1, 64, 24)]          # name, images, BATCH_SIZE_PER_IM, objects per image


def make_image(seed, K, rows):
    """K spheres inside the tile, their roidb boxes, a label volume painted from them, and `rows` fg RoIs: jittered copies of the boxes"""
    rng = np.random.RandomState(seed)
    S, H, W = TILE
    r = rng.uniform(5, 18, K)
    c = np.stack([rng.uniform(20, W - 20, K), rng.uniform(20, H - 20, K), rng.uniform(20, S - 20, K)], 1)
    spots = np.concatenate([c, r[:, None]], 1).astype(np.float32)
    top = np.array([W - 1, H - 1, S - 1] * 2, np.float64)
    gt = np.clip(np.floor(np.concatenate([c - r[:, None], c + r[:, None]], 1)), 0, top).astype(np.float32)
    vol = np.zeros(TILE, np.uint16)
    z, y, x = np.ogrid[:S, :H, :W]
    for k in range(K):
        ball = (x - c[k, 0]) ** 2 + (y - c[k, 1]) ** 2 + (z - c[k, 2]) ** 2 < r[k] ** 2
        vol[ball & (vol == 0)] = k + 1
    pick = rng.randint(0, K, rows)
    rois = np.clip(gt[pick] + rng.uniform(-2, 2, (rows, 6)), 0, top).astype(np.float32)
    return spots, gt, np.arange(1, K + 1, dtype=np.int32), vol, rois


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true", help="skip the NumPy host path")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    import m3d
    import mask_train_reference as MR
    assert torch.cuda.is_available(), "bench_mask_targets needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        out = []
        for i in range(a.warmup + a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                out.append(e0.elapsed_time(e1) / a.inner)
        return "%.3f (%.3f .. %.3f)" % (statistics.median(out), min(out), max(out))

    say("# mask-branch training step, tile %s, M 14, device %s" % (TILE, torch.cuda.get_device_name(0)))
    say("# %d warm-up + %d repetitions of %d calls; ms per call between device events: median (min .. max); host: wall ms, median of %d"
        % (a.warmup, a.reps, a.inner, a.host_reps))
    say("%-7s %2s %4s %9s | %-26s %-26s | %s" % ("config", "B", "fg", "positive", "targets", "loss", "numpy host path"))
    for name, B, batch, K in SHAPES:
        bcfg = m3d.BoxHeadTrainCfg(batch_per_im=batch)
        mcfg = getattr(m3d.MaskTrainCfg, name)()
        F = bcfg.fg_per_im
        ims = [make_image(100 * K + b, K, F) for b in range(B)]
        labels = np.full((B, batch), 0, np.int32)
        labels[:, :F] = 1
        rois = np.zeros((B, batch, 6), np.float32)
        for b, im in enumerate(ims):
            rois[b, :F] = im[4]
        counts = np.tile(np.array([batch, F, batch - F, F, batch - F, 0, K, 0], np.int64), (B, 1))
        T = m3d.BoxHeadTargets(torch.full((B, batch), -1, dtype=torch.int64, device="cuda"), torch.from_numpy(labels).cuda(),
                               torch.from_numpy(rois).cuda(), torch.zeros((B, batch, 6), device="cuda"), torch.from_numpy(counts).cuda(), bcfg)
        if mcfg.anno_type == "spot":
            kw = dict(spots=[torch.from_numpy(im[0]).cuda() for im in ims])
        else:
            kw = dict(gt_boxes=[torch.from_numpy(im[1]).cuda() for im in ims], markers=[torch.from_numpy(im[2]).cuda() for im in ims],
                      labels=[torch.from_numpy(im[3]).cuda() for im in ims])
        MT = m3d.mask_targets(T, mcfg, **kw)
        pred = torch.randn((B * F, 1, 14, 14, 14), device="cuda")
        t_targets = timed(lambda: m3d.mask_targets(T, mcfg, **kw))
        t_loss = timed(lambda: m3d.mask_losses(pred, MT))
        host = "skipped"
        if not a.no_cpu:
            def host_path():
                blobs = []
                for b, im in enumerate(ims):
                    hk = dict(spots=im[0], in_size=TILE) if mcfg.anno_type == "spot" else dict(gt_boxes=im[1], markers=im[2], label_volume=im[3])
                    blobs.append(MR.mask_targets(labels[b], rois[b], 14, form="direct", **hk)["masks"])
                out = torch.from_numpy(np.concatenate(blobs, 0)).cuda()
                torch.cuda.synchronize()
                return out
            ref = host_path()
            ref = ref.reshape(B, F, -1)
            assert not bool(((ref == 1) & (MT.masks != 1)).any()), "the device misses a voxel of the host path"
            extra = int((ref != MT.masks).sum())                  # voxels the host path's fp32 resize underflows (DESIGN)
            ts = []
            for _ in range(a.host_reps):
                t0 = time.perf_counter()
                host_path()
                ts.append((time.perf_counter() - t0) * 1e3)
            host = "%.1f (%.1f .. %.1f), %d voxels differ" % (statistics.median(ts), min(ts), max(ts), extra)
        say("%-7s %2d %4d %9d | %-26s %-26s | %s" % (name, B, F, int(MT.counts[:, 1].sum()), t_targets, t_loss, host))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
