#!/usr/bin/env python3
"""Times one training minibatch at the soma shape - B = 2 volumes of 128 x 256 x 256 uint16, tiles of 64 x 256 x 256 fp32 - three ways:

  m3d.train_sample   the device path (csrc/train_sample.hip): crop search, box filter and normalised crop from volumes resident on the
                     device with their statistics, two launches
  ops.norm1_batched  on a [2, 64, 256, 256] uint16 input: the same output bytes (and three reads of the input for its own statistics);
                     the yardstick for the apply kernel
  NumPy host path    what the reference does per sample and step (lib/utils/blob.py:97-202): astype(float32) of the whole volume,
                     mean / std over the mask, the candidate search, the crop, and the upload of the fp32 tile

The device variants follow tools/bench_sgd.py: warm-up, then `--reps` repetitions with the variants alternating inside every
repetition; each measurement is the time between two device events around `--inner` consecutive calls, divided by `--inner`; median and
spread (min .. max) in ms.  The host path is wall-clock time per minibatch including the upload and its synchronisation, `--host-reps`
repetitions.  "MB" is what the device variants must move, counted from the sizes; HBM = those bytes over the median over 6.3 TB/s: an
accounting figure, not a counter reading.  Needs a GPU; there is no CPU path."""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
HBM_PEAK = 6.3e12


def host_sample(vol, boxes, in_size, rng):
    """prep_im_for_blob(..., 'train') + crop_data_3d in NumPy, vectorised over the boxes as the reference is"""
    im = vol.astype(np.float32, copy=False)
    mask = im > 0
    im = (im - np.mean(im[mask])) / np.std(im[mask])
    D, H, W = im.shape
    ss = in_size
    lo = [math.floor(boxes[:, a].min()) for a in range(3)]
    smax = [min(lo[0], W - ss[2]), min(lo[1], H - ss[1]), min(lo[2], D - ss[0])]
    st = [0 if m == 0 else int(rng.randint(0, m + 1)) for m in smax]
    xs = list(range(st[0], W - ss[2], ss[2] // 2)) + [W - ss[2]]
    ys = list(range(st[1], H - ss[1], ss[1] // 2)) + [H - ss[1]]
    zs = list(range(st[2], D - ss[0], ss[0] // 2)) + [D - ss[0]]
    hi = np.array([ss[2] - 1, ss[1] - 1, ss[0] - 1] * 2, np.float32)

    def clipped(o):
        b = np.clip(boxes - np.array(o * 2, np.float32), 0, hi)
        return b, ~((b[:, 0] == b[:, 3]) | (b[:, 1] == b[:, 4]) | (b[:, 2] == b[:, 5]))
    best, pos = 0, [xs[0], ys[0], zs[0]]
    for z in zs:
        for y in ys:
            for x in xs:
                b, ok = clipped([x, y, z])
                b = b[ok]
                v = np.sum((b[:, 3] - b[:, 0] + 1) * (b[:, 4] - b[:, 1] + 1) * (b[:, 5] - b[:, 2] + 1))
                if v > best:
                    best, pos = v, [x, y, z]
    x, y, z = pos
    b, ok = clipped(pos)
    return np.ascontiguousarray(im[z:z + ss[0], y:y + ss[1], x:x + ss[2]]), b[ok]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--boxes", type=int, default=60, help="ground-truth boxes per volume")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    import m3d
    assert torch.cuda.is_available(), "bench_train_sample needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    B, dims, in_size = 2, (128, 256, 256), (64, 256, 256)
    rng = np.random.RandomState(0)
    vols, anns = [], []
    for i in range(B):
        v = rng.randint(0, 4000, dims).astype(np.uint16)
        v[rng.uniform(size=dims) < 0.3] = 0
        c = np.stack([rng.uniform(16, dims[2] - 16, a.boxes), rng.uniform(16, dims[1] - 16, a.boxes), rng.uniform(16, dims[0] - 16, a.boxes)], 1)
        r = rng.uniform(4, 12, (a.boxes, 1))
        b = np.round(np.concatenate([c - r, c + r], 1)).astype(np.float32)
        vols.append(v)
        anns.append((b, np.ones(a.boxes, np.int32), np.zeros(a.boxes, bool)))
    ts = m3d.TrainSet(vols, anns, m3d.SampleCfg.soma())
    images = [(ts.volumes[i], ts.stats[i], ts.boxes[i], ts.start_max[i]) for i in range(B)]
    n_out = B * in_size[0] * in_size[1] * in_size[2]
    data = torch.empty((n_out,), dtype=torch.float32, device="cuda")
    meta = torch.empty((B * (8 + ts.max_boxes),), dtype=torch.int32, device="cuda")
    tiles = torch.stack([ts.volumes[i][:in_size[0]] for i in range(B)]).contiguous()
    tiles_out = torch.empty(tiles.shape, dtype=torch.float32, device="cuda")
    step = [0]

    def sample():
        step[0] += 1
        m3d.train_sample(images, in_size, True, [2 * step[0], 2 * step[0] + 1], ts.max_boxes, data=data, meta=meta)

    def norm1_batched():
        m3d.norm1_batched(tiles, out=tiles_out)
    variants = {"m3d.train_sample": (sample, 2.0 * n_out + 4.0 * n_out), "ops.norm1_batched": (norm1_batched, 3 * 2.0 * n_out + 4.0 * n_out)}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.inner):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner
    say("# one training minibatch at the soma shape: B = %d, %d x %d x %d uint16 -> %d x %d x %d fp32 tiles, %d boxes per volume"
        % ((B,) + dims + in_size + (a.boxes,)))
    say("# device variants: %d warm-up + %d alternating repetitions of %d calls; time per call between device events, ms: median (min .. max)"
        % (a.warmup, a.reps, a.inner))
    say("# MB = bytes the variant must move (from the sizes); HBM = MB / median / 6.3 TB/s")
    say("%-20s | %-28s %8s %6s" % ("variant", "ms per minibatch", "MB", "HBM"))
    names = list(variants)
    times = {n: [] for n in names}
    for i in range(a.warmup + a.reps):
        for n in names[i % len(names):] + names[:i % len(names)]:
            t = timed(variants[n][0])
            if i >= a.warmup:
                times[n].append(t)
    med = {}
    for n in names:
        med[n], mb = statistics.median(times[n]), variants[n][1] / 1e6
        say("%-20s | %-28s %8.1f %5.1f%%" % (n, "%.3f (%.3f .. %.3f)" % (med[n], min(times[n]), max(times[n])), mb,
                                             100.0 * mb * 1e6 / (med[n] * 1e-3) / HBM_PEAK))
    host = []
    hrng = np.random.RandomState(1)
    for i in range(1 + a.host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = [host_sample(vols[b], anns[b][0], in_size, hrng) for b in range(B)]
        dev = torch.from_numpy(np.stack([o[0] for o in out])[:, None]).cuda()
        torch.cuda.synchronize()
        if i:
            host.append((time.perf_counter() - t0) * 1e3)
        del dev
    hm = statistics.median(host)
    say("%-20s | %-28s %8s %6s" % ("NumPy host path", "%.1f (%.1f .. %.1f)" % (hm, min(host), max(host)), "-", "-"))
    say("# m3d.train_sample / ops.norm1_batched = %.2f; NumPy host path / m3d.train_sample = %.0f (wall clock, %d repetitions, against device time)"
        % (med["m3d.train_sample"] / med["ops.norm1_batched"], hm / med["m3d.train_sample"], a.host_reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
