"""Synthetic inputs for benchmarks and smoke tests: seeded weights with the reference's state-dict key
layout and nuclei-style volumes.  No dataset or checkpoint ships with the reference (README.md:31)."""
import math

import numpy as np
import torch

from .model import dsn_layers


def make_params(stride=8, num_anchors=35, mlp_dim=1024, roi_res=7, num_classes=2, seed=0, head=True, box_head="roi_2mlp_head",
                conv_head_dim=128, num_stacked_convs=2):
    """kaiming-normal conv/linear, biases N(0,0.1), BN gamma U[0.5,1.5], beta N(0,0.1), mean N(0,0.1), var U[0.5,1.5].
    box_head = "roi_Xconv1fc_head": Box_Head.convs.{0,2,..} + Box_Head.fc (fast_rcnn_heads.py:120-179) instead of fc1 / fc2; the
    default output does not depend on the two conv-head arguments."""
    if box_head not in ("roi_2mlp_head", "roi_Xconv1fc_head"):
        raise ValueError("make_params(box_head=%r): 'roi_2mlp_head' or 'roi_Xconv1fc_head'" % (box_head,))
    g = torch.Generator().manual_seed(seed)
    P = {}
    chans = {"conv1a": (1, 32, 5), "conv2a": (32, 64, 3), "conv2b": (64, 64, 3), "conv3a": (64, 128, 3),
             "conv3b": (128, 128, 3), "conv4a": (128, 256, 3), "conv4b": (256, 256, 3)}

    def conv(name, cin, cout, k, scale=1.0):
        P[name + ".weight"] = torch.randn(cout, cin, k, k, k, generator=g) * math.sqrt(2.0 / (cin * k ** 3)) * scale
        P[name + ".bias"] = torch.randn(cout, generator=g) * 0.1

    def lin(name, cin, cout, scale=1.0):
        P[name + ".weight"] = torch.randn(cout, cin, generator=g) * math.sqrt(2.0 / cin) * scale
        P[name + ".bias"] = torch.randn(cout, generator=g) * 0.1

    for cname, bname, _ in dsn_layers(stride):
        cin, cout, k = chans[cname]
        conv("Conv_Body." + cname, cin, cout, k)
        P["Conv_Body.%s.weight" % bname] = torch.rand(cout, generator=g) + 0.5
        P["Conv_Body.%s.bias" % bname] = torch.randn(cout, generator=g) * 0.1
        P["Conv_Body.%s.running_mean" % bname] = torch.randn(cout, generator=g) * 0.1
        P["Conv_Body.%s.running_var" % bname] = torch.rand(cout, generator=g) + 0.5
    dim = 256 if stride == 8 else 128
    conv("RPN.RPN_conv", dim, dim, 3)
    conv("RPN.RPN_cls_score", dim, num_anchors, 1, scale=2.0)
    conv("RPN.RPN_bbox_pred", dim, num_anchors * 6, 1, scale=0.2)
    if head and box_head == "roi_Xconv1fc_head":
        cin = dim
        for i in range(num_stacked_convs):
            conv("Box_Head.convs.%d" % (2 * i), cin, conv_head_dim, 3)
            cin = conv_head_dim
        lin("Box_Head.fc", cin * roi_res ** 3, mlp_dim)
    elif head:
        lin("Box_Head.fc1", dim * roi_res ** 3, mlp_dim)
        lin("Box_Head.fc2", mlp_dim, mlp_dim)
    if head:
        lin("Box_Outs.cls_score", mlp_dim, num_classes)
        lin("Box_Outs.bbox_pred", mlp_dim, 6 * num_classes, scale=0.3)
    return P


def unsaturated_rpn(P, scale=0.25):
    """A copy of `P` with RPN_cls_score's weight and bias scaled.  The random init of the stride-8 net gives RPN class logits of +-40: the
    sigmoid of every top-ranked position is exactly 1.0f, its derivative (1 - y) y exactly 0, and the reference's peak back-propagation then
    returns 0 / 0 maps for every kept peak (lib/prm/peak_response_mapping_3d.py:164-171).  Logits of +-10, as a trained net has, keep the
    proposals' ranking (a monotone function of the same logits, up to the former ties) and give the PRM workloads maps that are not empty."""
    P = dict(P)
    for k in ("RPN.RPN_cls_score.weight", "RPN.RPN_cls_score.bias"):
        P[k] = P[k] * scale
    return P


def synth_volume(i, shape=(128, 128, 128)):
    """N(100,10) background + 40 isotropic Gaussian blobs, clipped to uint16; returns the raw uint16 volume."""
    rng = np.random.RandomState(1234 + i)
    S, H, W = shape
    v = rng.normal(100, 10, shape).astype(np.float32)
    zz, yy, xx = np.mgrid[0:S, 0:H, 0:W].astype(np.float32)
    for _ in range(40):
        c = rng.uniform(0, 1, 3) * np.array(shape)
        s = rng.uniform(4, 8)
        a = rng.uniform(300, 900)
        r = int(4 * s)
        z0, z1 = max(0, int(c[0]) - r), min(S, int(c[0]) + r + 1)
        y0, y1 = max(0, int(c[1]) - r), min(H, int(c[1]) + r + 1)
        x0, x1 = max(0, int(c[2]) - r), min(W, int(c[2]) + r + 1)
        d2 = (zz[z0:z1, y0:y1, x0:x1] - c[0]) ** 2 + (yy[z0:z1, y0:y1, x0:x1] - c[1]) ** 2 + (xx[z0:z1, y0:y1, x0:x1] - c[2]) ** 2
        v[z0:z1, y0:y1, x0:x1] += a * np.exp(-d2 / (2 * s * s))
    return np.clip(v, 0, 65535).astype(np.uint16)


def synth_volume_boxes(i, shape=(128, 128, 128), k=2.0):
    """Ground-truth boxes fp32 [40, 6] (x1, y1, z1, x2, y2, z2) of synth_volume(i, shape)'s blobs: centre -+ k sigma, rounded and clipped to
    the volume (the same random sequence, replayed without painting)."""
    rng = np.random.RandomState(1234 + i)
    S, H, W = shape
    rng.normal(100, 10, shape)
    out = np.zeros((40, 6), np.float32)
    for n in range(40):
        c = rng.uniform(0, 1, 3) * np.array(shape)
        s = rng.uniform(4, 8)
        rng.uniform(300, 900)
        lo, hi = np.round(c - k * s), np.round(c + k * s)
        out[n] = [max(lo[2], 0), max(lo[1], 0), max(lo[0], 0), min(hi[2], W - 1), min(hi[1], H - 1), min(hi[0], S - 1)]
    return out


def _shifted(m, axis, d):
    """m moved by d voxels along axis, zero-filled (no wrap)."""
    out = np.zeros_like(m)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    src[axis] = slice(0, m.shape[axis] - d) if d > 0 else slice(-d, None)
    dst[axis] = slice(d, None) if d > 0 else slice(0, m.shape[axis] + d)
    out[tuple(dst)] = m[tuple(src)]
    return out


def synth_label_pair(shape, n_gt, seed):
    """A GT / prediction pair of uint16 label volumes for the evaluation tests and tools/bench_eval.py, and the prediction's score
    table float64 [P, 2] = [mask_id, score] (what m3d.io.save_segmentation writes for soma).
    GT: n_gt seeded random spheres filling ~15 % of the volume, ids 1..n_gt, the first sphere winning where spheres overlap.
    Prediction: per GT instance - dropped (10 %), split in two along z (10 %), shifted by one voxel (40 %), dilated by one voxel
    (20 %) or copied; plus n_gt // 10 false-positive spheres; ids randomly permuted; distinct scores."""
    rng = np.random.RandomState(seed)
    S, H, W = (int(v) for v in shape)
    r_mean = (0.15 * S * H * W / (max(n_gt, 1) * 4.19)) ** (1.0 / 3.0)

    def spheres(n):
        c = rng.uniform(0, 1, (n, 3)) * np.array([S, H, W])
        r = rng.uniform(0.7, 1.3, n) * r_mean
        return c, r

    def crop(c, r, margin):
        lo = np.maximum(np.floor(c - r).astype(int) - margin, 0)
        hi = np.minimum(np.ceil(c + r).astype(int) + margin + 1, (S, H, W))
        return tuple(slice(a, b) for a, b in zip(lo, hi))

    def ball(c, r, sl):
        zz, yy, xx = np.ogrid[sl[0], sl[1], sl[2]]
        return (zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 <= r * r

    gt = np.zeros((S, H, W), np.uint16)
    cg, rg = spheres(n_gt)
    for i in range(n_gt):
        sl = crop(cg[i], rg[i], 0)
        g = gt[sl]
        g[ball(cg[i], rg[i], sl) & (g == 0)] = i + 1
    pred = np.zeros_like(gt)
    nxt = 1
    for i in range(n_gt):
        sl = crop(cg[i], rg[i], 2)
        m = gt[sl] == i + 1
        u = rng.uniform()
        if u < 0.1 or not m.any():
            continue
        parts = [m]
        if u < 0.2:
            zc = int(np.round(np.nonzero(m)[0].mean()))
            top = m.copy()
            top[zc:] = False
            parts = [top, m & ~top]
        elif u < 0.6:
            parts = [_shifted(m, int(rng.randint(3)), int(rng.choice((-1, 1))))]
        elif u < 0.8:
            d = m.copy()
            for ax in range(3):
                d |= _shifted(m, ax, 1) | _shifted(m, ax, -1)
            parts = [d]
        p = pred[sl]
        for q in parts:
            q = q & (p == 0)
            if q.any():
                p[q] = nxt
                nxt += 1
    cf, rf = spheres(n_gt // 10)
    for i in range(len(rf)):
        sl = crop(cf[i], rf[i], 0)
        p = pred[sl]
        q = ball(cf[i], rf[i], sl) & (p == 0)
        if q.any():
            p[q] = nxt
            nxt += 1
    n_pred = nxt - 1
    perm = np.concatenate(([0], rng.permutation(n_pred) + 1)).astype(np.uint16)
    pred = perm[pred]
    ids = np.arange(1, n_pred + 1)
    scores = (rng.permutation(n_pred) + rng.uniform(0.05, 0.95)) / n_pred
    return gt, pred, np.stack([ids.astype(np.float64), scores], 1)
