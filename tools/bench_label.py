#!/usr/bin/env python3
"""Times whole-volume labelling (csrc/label3d.hip) and prints one JSON line.  Two sizes, 96 x 256 x 256 (soma) and 59 x 350 x 350
(nuclei), three uint8 inputs each:
  blobs    the foreground of m3d.synth.synth_label_pair's prediction: a few dozen fat components;
  specks   the same plus 0.2 % single-voxel specks: thousands of components;
  random   a random mask at density 0.12: the tangled case.
Per input, HIP-event times after a warm-up (median of --iters):
  label_us / label_counts_us   m3d.label_components at connectivity 26 without / with counts (one call = five launches and the host
                               read of K it synchronises on; with counts a memset and a sixth launch);
  cc_largest_us                m3d.cc_largest_batch given the whole volume as ONE crop: the same union-find on the same voxels with
                               no label output - the nearest existing operation, the yardstick for the union phase;
  scipy_us                     scipy.ndimage.label (full structure) on this host: the path a user had before;
  hbm_floor_us                 the compulsory bytes V x (in_bytes + 4) at 8 TB/s.
Also soma_dsn: labelling + label_overlap + label_iou_best (m3d.evaluate_baselines.baseline_prec_rec) of one 96 x 256 x 256 pair.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/bench_label.py --iters 5 --no-cpu` run."""
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


def inputs(shape, n_gt):
    from m3d.synth import synth_label_pair
    gt, pred, _ = synth_label_pair(shape, n_gt, 0)
    blobs = ((pred > 0) * 255).astype(np.uint8)
    rng = np.random.RandomState(1)
    specks = blobs.copy()
    specks[rng.uniform(size=shape) < 0.002] = 255
    rnd = ((np.random.RandomState(2).uniform(size=shape) < 0.12) * 255).astype(np.uint8)
    return gt, {"blobs": blobs, "specks": specks, "random": rnd}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-cpu", action="store_true", help="skip the scipy.ndimage.label baseline")
    a = ap.parse_args()
    import torch
    from scipy import ndimage
    import m3d
    from m3d import evaluate_baselines as EB
    assert torch.cuda.is_available(), "bench_label needs a GPU"
    rec = {"tool": "bench_label", "iters": a.iters, "connectivity": 26}
    full = np.ones((3, 3, 3), bool)
    for name, shape, n in (("soma", (96, 256, 256), 40), ("nuclei", (59, 350, 350), 40)):
        gt, vols = inputs(shape, n)
        V = int(np.prod(shape))
        rec[name] = {"shape": list(shape), "hbm_floor_us": round(V * 5 / HBM_BYTES_PER_S * 1e6, 2)}
        offsets = torch.tensor([0, V], dtype=torch.int64, device="cuda")
        dims = torch.tensor([list(shape)], dtype=torch.int32, device="cuda")
        for key, vol in vols.items():
            d = torch.from_numpy(vol).cuda()
            labels, K = m3d.label_components(d)
            r = {"components": K, "foreground": round(float((vol > 0).mean()), 4)}
            r["label_us"] = time_gpu(lambda: m3d.label_components(d), a.iters)
            r["label_counts_us"] = time_gpu(lambda: m3d.label_components(d, return_counts=True), a.iters)
            flat = d.reshape(-1)
            r["cc_largest_us"] = time_gpu(lambda: m3d.cc_largest_batch(flat, offsets, dims), a.iters)
            r["ratio_to_cc_largest"] = r["label_us"] / r["cc_largest_us"]
            if not a.no_cpu:
                r["scipy_us"] = time_cpu(lambda: ndimage.label(vol, structure=full), 3)
                r["scipy_over_label"] = r["scipy_us"] / r["label_us"]
            rec[name][key] = {k: (round(v, 2) if isinstance(v, float) else v) for k, v in r.items()}
        if name == "soma":
            d, g = torch.from_numpy(vols["specks"]).cuda(), torch.from_numpy(gt).cuda()

            def dsn():
                return EB.baseline_prec_rec([m3d.label_components(d)[0]], [g], 0.5)
            rec["soma_dsn"] = {"input": "specks", "rows": int(len(dsn()[3][0])), "end_to_end_us": round(time_gpu(dsn, a.iters), 2)}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
