"""GPU: the box-head training step (csrc/box_head_train.hip, m3d.train) against the reference's results
(tests/golden/box_head_train.npz), the NumPy restatement (tests/box_head_train_reference.py) and fp64 evaluations of the loss formulas.
Reads only tests/golden/ and the restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import box_head_train_reference as BR
from test_box_head_train_host import (CASES, LOSS_CASES, bits, case_inputs, check_blobs, check_losses_against_reference, check_sampled,
                                      loss_case, ulp_distance)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "box_head_train.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def dev_cfg(cfg):
    import m3d
    return m3d.BoxHeadTrainCfg(batch_per_im=cfg["batch"], fg_fraction=cfg["fg_fraction"], fg_thresh=cfg["fg_thresh"], bg_thresh_hi=cfg["bg_hi"],
                               bg_thresh_lo=cfg["bg_lo"], num_classes=cfg["num_classes"], bbox_reg_weights=cfg["weights"])


def proposal_blob(props, slack=3):
    """rois [B,rows,7] and num [B] as the proposal stage leaves them: column 0 and the rows beyond num[b] hold values nobody may read"""
    rows = max(len(p) for p in props) + slack
    rois = np.full((len(props), rows, 7), 1e6, np.float32)
    for b, p in enumerate(props):
        rois[b, :len(p), 1:] = p
        rois[b, :, 0] = 7 + b
    return torch.from_numpy(rois).cuda(), torch.tensor([len(p) for p in props], dtype=torch.int32).cuda()


def device_targets(images, cfg, seeds):
    """images: list of (gt, classes or None, crowd or None, proposals)"""
    import m3d
    rois, num = proposal_blob([im[3] for im in images])
    classes = [im[1] for im in images] if any(im[1] is not None for im in images) else None
    crowd = [im[2] for im in images] if any(im[2] is not None for im in images) else None
    return m3d.box_head_targets(rois, num, [im[0] for im in images], dev_cfg(cfg), seeds, gt_classes=classes, gt_crowd=crowd)


def check_padding(T, b, n):
    assert (T.rows[b, n:] == -1).all() and (T.labels[b, n:] == -1).all() and (T.rois[b, n:] == 0).all() and (T.targets[b, n:] == 0).all()
    assert (T.rows[b, :n] >= 0).all() and (T.labels[b, :n] >= 0).all()


def same_as_restatement(d, want):
    """device (trimmed) against the restatement: everything bit for bit but dw,dh,ds - two fp64 logs a few fp64 ulp apart, times the
    weight, round to the same fp32 value or to neighbours: 1 ulp"""
    for k in ("rows", "labels", "counts"):
        assert np.array_equal(d[k], want[k]), (k, d[k], want[k])
    assert np.array_equal(bits(d["rois"]), bits(want["rois"]))
    assert np.array_equal(bits(d["targets"][:, :3]), bits(want["targets"][:, :3]))
    assert (ulp_distance(d["targets"][:, 3:], want["targets"][:, 3:]) <= 1).all()


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(g, name):
    cfg, gt, cls, crowd, pr, seed = case_inputs(g, name)
    T = device_targets([(gt, cls, crowd, pr)], cfg, [seed])
    d = T.numpy()[0]
    check_sampled(d, cfg, g, name, "device")
    n = int(d["counts"][0])
    check_padding(T, 0, n)
    blobs = T.blobs()
    lab, r7 = blobs["labels_int32"].cpu().numpy(), blobs["rois"].cpu().numpy()
    bt, iw, ow = (blobs[k].cpu().numpy() for k in ("bbox_targets", "bbox_inside_weights", "bbox_outside_weights"))
    assert bt.shape == (cfg["batch"], 6 * cfg["num_classes"]) and r7.shape == (cfg["batch"], 7)
    check_blobs(bt[:n], iw[:n], ow[:n], g, name)
    assert np.array_equal(lab[:n], g[name + "_labels"]) and (lab[n:] == -1).all()
    assert np.array_equal(bits(r7[:n]), bits(g[name + "_rois"])) and (r7[n:] == 0).all()
    assert (bt[n:] == 0).all() and (iw[n:] == 0).all() and (ow[n:] == 0).all()


def boxes(seed, K, tile=(32, 64, 48)):
    rng = np.random.RandomState(seed)
    S, H, W = tile
    c = np.stack([rng.uniform(8, W - 8, K), rng.uniform(8, H - 8, K), rng.uniform(6, S - 6, K)], 1)
    r = rng.uniform(4, 12, (K, 3))
    return np.round(np.concatenate([c - r, c + r], 1)).astype(np.float32).reshape(K, 6)


def proposals(seed, gt, copies, extra, tile=(32, 64, 48)):
    rng = np.random.RandomState(seed)
    jit = np.repeat(gt, copies, 0) + rng.uniform(-4, 4, (len(gt) * copies, 6))
    return np.concatenate([jit.reshape(-1, 6), boxes(seed + 1, extra, tile) + rng.uniform(-0.5, 0.5, (extra, 6))], 0).astype(np.float32)


def test_cases_beyond_the_fixture():
    """No box, only crowd boxes, no proposals, more boxes than one LDS chunk of 256, and two images with different box and proposal
    counts in one call: device against the restatement."""
    cfg = BR.make_cfg()
    none = np.zeros((0, 6), np.float32)
    g6, g300 = boxes(51, 6), boxes(52, 300, (64, 128, 128))
    cls300 = (np.arange(300) % 2 + 1).astype(np.int32)
    runs = [
        ("no boxes", cfg, [(none, None, None, proposals(61, g6, 10, 40))]),
        ("all crowd", cfg, [(g6, None, np.ones(6, np.uint8), proposals(62, g6, 10, 40))]),
        ("no proposals", cfg, [(g6, None, None, none)]),
        ("300 boxes", BR.make_cfg(num_classes=3), [(g300, cls300, None, proposals(63, g300, 2, 100, (64, 128, 128)))]),
        ("two images", cfg, [(g6, None, np.array([0, 0, 1, 0, 0, 0], np.uint8), proposals(64, g6, 20, 100)),
                             (boxes(53, 2), None, None, proposals(65, boxes(53, 2), 4, 9))]),
        ("empty next to full", cfg, [(none, None, None, none), (g6, None, None, proposals(66, g6, 20, 100))]),
    ]
    for what, c, images in runs:
        seeds = [100 + i for i in range(len(images))]
        T = device_targets(images, c, seeds)
        got = T.numpy()
        for b, (gt, cls, crowd, pr) in enumerate(images):
            want = BR.box_head_targets(gt, pr, c, seeds[b], cls, crowd)
            same_as_restatement(got[b], want)
            check_padding(T, b, int(want["counts"][0]))
        c0 = got[0]["counts"]
        if what in ("no boxes", "all crowd"):
            assert c0[1] == 0 and c0[3] == 0 and c0[0] == c0[2] == 64 and c0[6] == 0      # no fg, the batch fills with bg rows
        if what == "no proposals":
            assert c0[7] == 0 and c0[0] == c0[1] == 6 and c0[2] == 0                        # the boxes themselves are the only rows
        if what == "300 boxes":
            assert (BR.label(gt, pr, cls, crowd)["assign"][300:] >= 256).any() and set(got[0]["labels"][:c0[1]].tolist()) == {1, 2}
        if what == "empty next to full":
            assert c0[0] == 0 and got[1]["counts"][0] == 64
    # a base seed means seed + b for image b
    images = runs[4][2]
    assert torch.equal(device_targets(images, cfg, 100).rows, device_targets(images, cfg, [100, 101]).rows)


def test_largest_batch_with_5000_candidates():
    """BATCH_SIZE_PER_IM 4096 (the limit) out of more than 5000 candidates: both selections sub-sample, every radix pass narrows a
    histogram of thousands of keys, and the prefix sum hands 4096 output slots to 85 candidate words."""
    gt = boxes(71, 40, (64, 256, 256))
    pr = proposals(72, gt, 60, 3000, (64, 256, 256))
    cfg = BR.make_cfg(batch=4096)
    want = BR.box_head_targets(gt, pr, cfg, 9)
    assert want["counts"][3] > want["counts"][1] == 1024 and want["counts"][4] > want["counts"][2] == 3072 and want["counts"][3] + want["counts"][4] > 5000
    T = device_targets([(gt, None, None, pr)], cfg, [9])
    same_as_restatement(T.numpy()[0], want)


def test_same_seed_same_bits_and_consecutive_seeds_differ(g):
    cfg, gt, cls, crowd, pr, seed = case_inputs(g, "nuclei")
    a, b, c = (device_targets([(gt, cls, crowd, pr)], cfg, [s]) for s in (seed, seed, seed + 1))
    for k in ("rows", "labels", "rois", "targets", "counts"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert torch.equal(a.counts, c.counts) and not torch.equal(a.rows, c.rows)
    same = np.intersect1d(a.rows.cpu().numpy(), c.rows.cpu().numpy()).size
    assert same < 32                                  # 64 of 2040 rows twice: unrelated draws share a handful, shifted draws nearly all


def loss_targets(g, lname):
    """BoxHeadTargets on the device holding the reference's own labels and compact targets of a loss case, and the fp32 inputs"""
    import m3d
    sc, pr, labels, targets, batch = loss_case(g, lname)
    B = len(labels) // batch
    counts = np.zeros((B, 8), np.int64)
    counts[:, 0] = (labels.reshape(B, batch) >= 0).sum(1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    T = m3d.BoxHeadTargets(dev(np.zeros((B, batch), np.int64)), dev(labels.reshape(B, batch)), dev(np.zeros((B, batch, 6), np.float32)),
                           dev(targets.reshape(B, batch, 6)), dev(counts), m3d.BoxHeadTrainCfg(batch_per_im=batch))
    return T, sc, pr, labels, targets


@pytest.mark.parametrize("lname", sorted(LOSS_CASES))
def test_losses_and_gradients(g, lname):
    """Against the fp64 restatement within one fp32 rounding (2^-23 relative on each loss, 2^-23 max(|g|, 1/R) on each gradient element,
    exactly 0 off the pattern and on padding rows), and against the reference's fp32 values within the host test's bounds."""
    import m3d
    T, sc, pr, labels, targets = loss_targets(g, lname)
    ts, tp = torch.from_numpy(sc).cuda().requires_grad_(), torch.from_numpy(pr).cuda().requires_grad_()
    lc, lb, acc = m3d.box_head_losses(ts, tp, T)
    assert not acc.requires_grad
    (lc + lb).backward()
    got = np.array([lc.item(), lb.item(), acc.item()], np.float64)
    gs, gp = ts.grad.cpu().numpy(), tp.grad.cpu().numpy()
    w = check_losses_against_reference(got, gs, gp, g, lname, "device")          # the same bounds the reference's values meet
    l64, gs64, gp64, R = w[:3], w[3], w[4], w[5]
    u = 2.0 ** -23
    print(lname, "device vs fp64:", [abs(got[i] - l64[i]) / max(l64[i], 1e-30) for i in range(3)], "of", u)
    assert all(abs(got[i] - l64[i]) <= u * l64[i] for i in range(3))
    assert (np.abs(gs - gs64) <= u * np.maximum(np.abs(gs64), 1.0 / R)).all() and (np.abs(gp - gp64) <= u * np.maximum(np.abs(gp64), 1.0 / R)).all()
    assert (gs[labels < 0] == 0).all() and (gp[labels < 0] == 0).all() and (gp[labels == 0] == 0).all()
    assert np.array_equal(gs != 0, gs64 != 0) and np.array_equal(gp != 0, gp64 != 0)
    ref = g[lname + "_losses"].astype(np.float64)                                 # device against the reference's own numbers
    n_fg = int((labels > 0).sum())
    assert abs(got[0] - ref[0]) <= (R + 9) * 2.0 ** -24 * l64[0] and abs(got[1] - ref[1]) <= (6 * n_fg + 9) * 2.0 ** -24 * l64[1]
    assert abs(got[2] - ref[2]) <= 2 * 2.0 ** -24
    # run to run: the same bits
    l2, g2s, g2p = m3d.box_head_loss_grad(ts.detach(), tp.detach(), T.labels, T.targets, T.counts)
    assert l2[0].item() == lc.item() and l2[1].item() == lb.item() and torch.equal(g2s, ts.grad) and torch.equal(g2p, tp.grad)


def test_no_sampled_rows_gives_zeros():
    import m3d
    none = np.zeros((0, 6), np.float32)
    T = device_targets([(none, None, None, none)], BR.make_cfg(), [1])
    assert T.counts[0, 0].item() == 0 and (T.rois7 == 0).all()
    ts, tp = torch.randn(64, 2, device="cuda", requires_grad=True), torch.randn(64, 12, device="cuda", requires_grad=True)
    lc, lb, acc = m3d.box_head_losses(ts, tp, T)
    (lc + lb).backward()
    assert lc.item() == 0 and lb.item() == 0 and acc.item() == 0 and (ts.grad == 0).all() and (tp.grad == 0).all()


def test_backward_reaches_every_head_parameter(g):
    """box_head_losses(...).backward() through m3d.compat's RoIAlign and linear layers: finite, non-zero gradients on the feature map
    and on every head parameter."""
    import m3d
    import m3d.compat as compat
    cfg, gt, cls, crowd, pr, seed = case_inputs(g, "small_crowd")
    T = device_targets([(gt, cls, crowd, pr)], cfg, [seed])
    torch.manual_seed(3)
    feat = torch.randn(1, 8, 4, 8, 6, device="cuda", requires_grad=True)           # tile 32 x 64 x 48 at stride 8
    mk = lambda *s: (torch.randn(*s, device="cuda") * 0.05).requires_grad_()  # noqa: E731
    params = dict(fc1_w=mk(64, 8 * 343), fc1_b=mk(64), fc2_w=mk(64, 64), fc2_b=mk(64), cls_w=mk(2, 64), cls_b=mk(2), box_w=mk(12, 64), box_b=mk(12))
    x = compat.RoIAlign_3d(7, 7, 7, 1.0 / 8, 2)(feat, T.rois7)
    assert x.shape == (64, 8, 7, 7, 7)
    x = torch.relu(compat.linear(x.reshape(64, -1), params["fc1_w"], params["fc1_b"]))
    x = torch.relu(compat.linear(x, params["fc2_w"], params["fc2_b"]))
    lc, lb, acc = m3d.box_head_losses(compat.linear(x, params["cls_w"], params["cls_b"]), compat.linear(x, params["box_w"], params["box_b"]), T)
    (lc + lb).backward()
    assert np.isfinite(lc.item()) and np.isfinite(lb.item()) and lc.item() > 0 and lb.item() > 0 and 0 <= acc.item() <= 1
    for name, p in list(params.items()) + [("features", feat)]:
        assert p.grad is not None and torch.isfinite(p.grad).all() and (p.grad != 0).any(), name


def test_train_detector_tool():
    """tools/train_detector.py in a fresh process: exit status 0 and four finite losses per step."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_detector.py"), "--steps", "3", "--width", "8"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("step ")]
    assert len(lines) == 3
    for ln in lines:
        vals = dict(zip(ln[2::2], ln[3::2]))
        four = [float(vals[k]) for k in ("loss_rpn_cls", "loss_rpn_bbox", "loss_cls", "loss_bbox")]
        assert all(np.isfinite(v) for v in four) and four[0] > 0 and four[2] > 0, ln
