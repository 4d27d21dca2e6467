#!/usr/bin/env python3
"""Times the RPN training step (csrc/rpn_train.hip).  profiles/rpn_targets.txt is this tool's output, both modes, plus notes.

Default mode (needs a GPU): for both shipped configurations (tile 64 x 256 x 256) and K = 8, 64, 256 ground-truth boxes, HIP-event
times after a warm-up (median of --iters), milliseconds per call:
  targets_ms   m3d.rpn_targets: one memset and five launches (per-box maxima, labels, scan, draws, finalize), five output allocations;
  loss_ms      m3d.rpn_losses forward: two memsets and one launch (both losses and both gradients), the stacking of the target set;
  wide_ms      RpnTargets.wide(): the dense export, four memsets over 19 x anchors x 4 bytes and one scatter launch;
  numpy_ms     wall time of the NumPy restatement of the targets (tests/rpn_train_reference.py) on this host's CPU, one run;
and what the work is by count: inside anchors x K IoUs per labelling pass (two passes), the dense export's bytes and their floor at
8 TB/s.  (The label pass itself writes one candidate bit per anchor and 4 bytes per fg anchor; the anchors are computed, not read.)

--kernel-table DB (no GPU): the median time per kernel and configuration from the SQLite file of a separate
`rocprofv3 --kernel-trace -- python tools/bench_rpn_targets.py --iters N --no-cpu` run (its `kernels` view, in dispatch order)."""
import argparse
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "instanceseg-without-voxelwise-labeling_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_BYTES_PER_S = 8.0e12
KERNELS = ("gt_max_kernel", "label_kernel", "scan_kernel", "draw_kernel", "finalize_kernel", "loss_kernel", "wide_kernel")
CONFIGS = [(name, K) for name in ("nuclei", "soma") for K in (8, 64, 256)]


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
        out.append(s.elapsed_time(e))
    return float(np.median(out))


def boxes(seed, K, im):
    rng = np.random.RandomState(seed)
    S, H, W = im
    c = np.stack([rng.uniform(8, W - 8, K), rng.uniform(8, H - 8, K), rng.uniform(6, S - 6, K)], 1)
    r = rng.uniform(4, 12, (K, 3))
    return np.round(np.concatenate([c - r, c + r], 1)).astype(np.float32)


def kernel_table(db):
    """The tool calls every kernel the same number of times per configuration, configurations in CONFIGS order: split each kernel's
    dispatches into six equal runs."""
    import sqlite3
    rows = list(sqlite3.connect(db).execute("select name, duration from kernels order by start"))
    print("# kernel times, microseconds, median per configuration (calls per configuration in brackets), from %s" % os.path.basename(db))
    print("# %-18s" % "kernel" + "".join("%14s" % ("%s K=%d" % c) for c in CONFIGS))
    for k in KERNELS:
        v = [d / 1e3 for n, d in rows if re.search(r"\b%s\b" % k, n)]
        per = len(v) // len(CONFIGS)
        if per == 0 or len(v) % len(CONFIGS):
            print("%-20s not split: %d dispatches" % (k, len(v)))
            continue
        print("%-20s" % ("%s [%d]" % (k, per)) + "".join("%14.1f" % float(np.median(v[i * per:(i + 1) * per])) for i in range(len(CONFIGS))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the NumPy restatement")
    ap.add_argument("--kernel-table", metavar="DB", help="print the kernel table from a rocprofv3 SQLite file and exit")
    a = ap.parse_args()
    if a.kernel_table:
        return kernel_table(a.kernel_table)
    import torch
    import m3d
    import rpn_train_reference as R
    assert torch.cuda.is_available(), "bench_rpn_targets needs a GPU"
    im = (64, 256, 256)
    cfgs = {"nuclei": m3d.RpnTrainCfg.nuclei(), "soma": m3d.RpnTrainCfg.soma()}
    print("# RPN training step, tile %s, iters %d, device %s" % (im, a.iters, torch.cuda.get_device_name(0)))
    print("# config  K  anchors  inside  fg_before  candidates | targets_ms  loss_ms  wide_ms  numpy_ms | IoUs/pass  wide_bytes  wide_hbm_floor_ms")
    for name, K in CONFIGS:
        cfg = cfgs[name]
        rc = R.make_cfg(cfg.stride, cfg.sizes, cfg.aspect_ratios, cfg.max_size, cfg.batch_per_im, cfg.positive_overlap, cfg.negative_overlap,
                        cfg.straddle_thresh, cfg.fg_fraction, cfg.coarsest_stride)
        A, F = cfg.num_anchors, cfg.field_size
        s, h, w = (v // cfg.stride for v in im)
        logits = torch.randn(1, A, s, h, w, device="cuda")
        pred = torch.randn(1, 6 * A, s, h, w, device="cuda")
        gt = boxes(K, K, im)
        dgt = torch.from_numpy(gt).cuda()
        T = m3d.rpn_targets(dgt, im, cfg, 1)
        c = T.counts.cpu().numpy()
        t_targets = time_gpu(lambda: m3d.rpn_targets(dgt, im, cfg, 1), a.iters)
        t_loss = time_gpu(lambda: m3d.rpn_losses(logits, pred, T), a.iters)
        t_wide = time_gpu(lambda: T.wide(), a.iters)
        t_np = float("nan")
        if not a.no_cpu:
            t0 = time.perf_counter()
            R.rpn_targets(gt, im, rc, 1)
            t_np = (time.perf_counter() - t0) * 1e3
        wide_bytes = 19 * A * F ** 3 * 4
        print("%-7s %4d %8d %7d %6d %7d | %8.3f %8.3f %8.3f %9.1f | %.3g  %d  %.4f" % (
            name, K, A * F ** 3, c[4], c[5], c[6], t_targets, t_loss, t_wide, t_np, float(c[4]) * K, wide_bytes,
            wide_bytes / HBM_BYTES_PER_S * 1e3))


if __name__ == "__main__":
    main()
