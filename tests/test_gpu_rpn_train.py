"""GPU: the RPN training step (csrc/rpn_train.hip, m3d.train) against the reference's results (tests/golden/rpn_train.npz), the NumPy
restatement (tests/rpn_train_reference.py) and fp64 evaluations of the loss formulas.  Reads only tests/golden/ and the restatement."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rpn_train_reference as R
from test_rpn_train_host import (CASES, LOSS_CASES, case_inputs, check_targets, check_wide, loss_bounds, loss_inputs, ulp_distance)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "rpn_train.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def dev_cfg(cfg):
    import m3d
    return m3d.RpnTrainCfg(stride=cfg["stride"], sizes=cfg["sizes"], aspect_ratios=cfg["aspect_ratios"], max_size=cfg["max_size"],
                           coarsest_stride=cfg["coarsest_stride"], batch_per_im=cfg["batch"], fg_fraction=cfg["fg_fraction"],
                           positive_overlap=cfg["positive"], negative_overlap=cfg["negative"], straddle_thresh=cfg["straddle"])


def device_targets(g, name, seed=None, as_cuda=False):
    import m3d
    cfg, gt, dc, im, s = case_inputs(g, name)
    if as_cuda:
        gt, dc = torch.from_numpy(gt).cuda(), torch.from_numpy(dc).cuda()
    return m3d.rpn_targets(gt, im, dev_cfg(cfg), s if seed is None else seed, dc if len(dc) else None)


def as_dict(T):
    d = T.numpy()
    d.update(A=T.num_anchors, F=T.field_size, num_examples=int(d["counts"][3]))
    return d


def same_sets(a, b, logs_exact=False):
    for k in ("fg_index", "bg_index", "target_index", "counts"):
        assert np.array_equal(a[k], b[k]), k
    ta, tb = np.asarray(a["targets"], np.float32), np.asarray(b["targets"], np.float32)
    assert ta.shape == tb.shape and np.array_equal(ta[:, :3].view(np.uint32), tb[:, :3].view(np.uint32))
    assert (ulp_distance(ta[:, 3:], tb[:, 3:]) <= (0 if logs_exact else 2)).all()


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(g, name):
    T = device_targets(g, name)
    d = as_dict(T)
    check_targets(d, g, name)
    n_fg, n_bg, n_t = d["counts"][:3]
    assert (T.fg_index.cpu().numpy()[n_fg:] == -1).all() and (T.bg_index.cpu().numpy()[n_bg:] == -1).all()
    assert (T.target_index.cpu().numpy()[n_t:] == -1).all() and (T.targets.cpu().numpy()[n_t:] == 0).all()
    check_wide(tuple(t.cpu().numpy() for t in T.wide()), g, name)


def small_cfg(**kw):
    d = dict(stride=8, sizes=(10, 27, 33, 38, 42, 46, 50), aspect_ratios=[[1.0, 0.5], [0.5, 0.5], [2., 0.5], [0.2, 0.5], [3., 2.]],
             max_size=64, batch=64, positive=0.5, negative=0.3, straddle=0)
    d.update(kw)
    return R.make_cfg(**d)


def boxes(seed, K, im=(32, 64, 48)):
    rng = np.random.RandomState(seed)
    S, H, W = im
    c = np.stack([rng.uniform(8, W - 8, K), rng.uniform(8, H - 8, K), rng.uniform(6, S - 6, K)], 1)
    r = rng.uniform(4, 12, (K, 3))
    return np.round(np.concatenate([c - r, c + r], 1)).astype(np.float32).reshape(K, 6)


@pytest.mark.parametrize("K", [0, 1, 300])
def test_box_counts_beyond_the_fixture(K):
    """No box (defined as 'maximum overlap 0 everywhere'), one box, and more boxes than one LDS chunk of 256."""
    import m3d
    im = (32, 64, 48)
    for cfg in (small_cfg(), small_cfg(straddle=-1, batch=512)):
        gt = boxes(20 + K, K, im)
        want = R.rpn_targets(gt, im, cfg, 7)
        got = as_dict(m3d.rpn_targets(gt, im, dev_cfg(cfg), 7))
        same_sets(got, want)
        if K == 0:
            assert got["counts"][0] == 0 and got["counts"][5] == 0 and got["counts"][6] == got["counts"][4]


def test_more_dont_care_boxes_than_one_chunk():
    """300 don't-care boxes: the second chunk loop of the label pass re-synchronises between its chunks of 256."""
    import m3d
    im = (32, 64, 48)
    for cfg in (small_cfg(), small_cfg(straddle=-1, batch=512)):
        gt, dc = boxes(41, 6, im), boxes(42, 300, im)
        want = R.rpn_targets(gt, im, cfg, 9, dc)
        assert want["counts"][6] < R.rpn_targets(gt, im, cfg, 9)["counts"][6]          # the boxes do exclude candidates
        same_sets(as_dict(m3d.rpn_targets(gt, im, dev_cfg(cfg), 9, dc)), want)


def test_device_draws_are_the_documented_hash():
    """No boxes, every anchor kept: candidate r is field index r, so the bg set is the keys themselves.  The expected indices are
    computed here in plain integer arithmetic from the contract: stream = fin(seed), r_j = (hi32(fin(stream + 2^40 + j)) * n) >> 32."""
    import m3d
    M = (1 << 64) - 1

    def fin(x):
        z = (x * 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    assert fin(1) == 0xE220A8397B1DCDAF                     # splitmix64's first output for state 0
    cfg = small_cfg(straddle=-1)
    A, F3 = 35, 8 ** 3
    n = A * F3
    for seed in (1, 2, (1 << 63) + 5):
        st = fin(seed)
        field = sorted({((fin((st + (1 << 40) + j) & M) >> 32) * n) >> 32 for j in range(64)})
        wide = np.sort(np.array([(i % A) * F3 + i // A for i in field], np.int64))
        got = as_dict(m3d.rpn_targets(np.zeros((0, 6), np.float32), (32, 64, 48), dev_cfg(cfg), seed))
        assert got["counts"][6] == n and got["counts"][7] == 64 and np.array_equal(got["bg_index"], wide)


def test_labels_agree_with_bbox_overlaps3d():
    """The label pass evaluates IoUs with its own copy of m3d_bbox_overlaps3d's arithmetic: the fg set and the candidate count it
    finds must be the ones the tie / threshold rules give on that operator's matrix, bit for bit (fp32 equality decides the ties)."""
    import m3d
    im = (32, 64, 48)
    for cfg in (small_cfg(batch=4096), small_cfg(straddle=-1, batch=4096)):
        gt = boxes(77, 40, im)
        L = R.label(gt, None, im, cfg)
        ov = m3d.bbox_overlaps3d(torch.from_numpy(L["anchors"]).cuda(), torch.from_numpy(gt).cuda()).cpu().numpy()
        fg = (ov == ov.max(0)[None, :]).any(1) | (ov.max(1) >= np.float32(cfg["positive"]))
        cand = ov.max(1) < np.float32(cfg["negative"])
        assert 0 < fg.sum() <= 2048
        got = as_dict(m3d.rpn_targets(gt, im, dev_cfg(cfg), 3))
        assert got["counts"][5] == fg.sum() and got["counts"][6] == cand.sum()
        assert np.array_equal(got["target_index"], np.sort(R.wide_index(L, L["inside"][fg])))


def test_seeds_and_replay(g):
    a, b, c = (as_dict(device_targets(g, "nuclei", seed=s)) for s in (1, 1, 2))
    same_sets(a, b, logs_exact=True)
    assert not np.array_equal(a["fg_index"], c["fg_index"]) and not np.array_equal(a["bg_index"], c["bg_index"])
    same_sets(as_dict(device_targets(g, "small_dc", as_cuda=True)), as_dict(device_targets(g, "small_dc")), logs_exact=True)
    big = as_dict(device_targets(g, "soma", seed=(1 << 63) + 12345))          # the whole 64-bit seed is used
    cfg, gt, dc, im, _ = case_inputs(g, "soma")
    same_sets(big, R.rpn_targets(gt, im, cfg, (1 << 63) + 12345))


def run_loss(Ts, lg, pr):
    import m3d
    x, p = torch.from_numpy(lg).cuda().requires_grad_(), torch.from_numpy(pr).cuda().requires_grad_()
    lc, lb = m3d.rpn_losses(x, p, Ts)
    gl, = torch.autograd.grad(lc, x, retain_graph=True)
    gp, = torch.autograd.grad(lb, p)
    return lc.item(), lb.item(), gl.cpu().numpy(), gp.cpu().numpy()


def check_loss(Ts, lg, pr, batch, tag):
    lc, lb, gl, gp = run_loss(Ts, lg, pr)
    dicts = [as_dict(T) for T in Ts]                     # the same fp32 inputs: the device's own target rows
    lc64, lb64, gl64, gp64, W = R.losses(lg, pr, dicts, np.float64)
    bc, bb, bgl, bgp = loss_bounds((lc64, lb64), gl64, gp64, W, len(Ts), batch)
    egl, egp = np.abs(gl - gl64), np.abs(gp - gp64)
    print(tag, "W", W, "loss_cls err %.3g of %.3g, loss_bbox err %.3g of %.3g, grad err / bound: cls %.3g box %.3g" % (
        abs(lc - lc64), bc, abs(lb - lb64), bb, (egl / np.where(bgl > 0, bgl, 1)).max(), (egp / np.where(bgp > 0, bgp, 1)).max()))
    assert np.isfinite(lc) and np.isfinite(lb) and np.isfinite(gl).all() and np.isfinite(gp).all()
    assert abs(lc - lc64) <= bc and abs(lb - lb64) <= bb
    assert np.array_equal(gl != 0, gl64 != 0) or (gl[gl64 == 0] == 0).all()      # exactly zero off the sampled, in-crop anchors
    assert (gp[gp64 == 0] == 0).all() and (gl[gl64 == 0] == 0).all()
    assert (egl <= bgl).all() and (egp <= bgp).all()
    return lc, lb, gl, gp


@pytest.mark.parametrize("lname", sorted(LOSS_CASES))
def test_loss_golden_inputs(g, lname):
    names = LOSS_CASES[lname]
    Ts = [device_targets(g, n) for n in names]
    cfg, _, _, im, _ = case_inputs(g, names[0])
    st = cfg["stride"]
    lg, pr = loss_inputs(int(g[lname + "_seed"]), len(names), Ts[0].num_anchors, im[0] // st, im[1] // st, im[2] // st)
    lc, lb, gl, gp = check_loss(Ts, lg, pr, cfg["batch"], lname)
    # and the reference's own fp32 values, each side within its bound of the fp64 evaluation
    ref = g[lname + "_losses"]
    assert abs(lc - ref[0]) <= 2 * (len(names) * cfg["batch"] + 4) * 2.0 ** -24 * ref[0]
    assert np.array_equal(gl != 0, g[lname + "_grad_logits"] != 0)


def test_loss_extreme_logits_and_batch_of_four(g):
    """B = 4 images with their own seeds; logits include +-30 and +-90 at sampled anchors (no inf / NaN)."""
    cfg, gt, dc, im, _ = case_inputs(g, "small_outside")
    Ts = [device_targets(g, "small_outside", seed=s) for s in (4, 5, 6, 7)]
    lg, pr = loss_inputs(99, 4, Ts[0].num_anchors, im[0] // 8, im[1] // 8, im[2] // 8)
    extremes = np.array([30, -30, 90, -90], np.float32)
    F3 = Ts[0].field_size ** 3
    hit = 0
    for b, T in enumerate(Ts):
        d = as_dict(T)
        for k, wi in enumerate(np.concatenate([d["fg_index"], d["bg_index"]])):
            a, pos = wi // F3, wi % F3
            z, y, x = pos // 64, (pos // 8) % 8, pos % 8
            if z < lg.shape[2] and y < lg.shape[3] and x < lg.shape[4] and k % 3 == 0:
                lg[b, a, z, y, x] = extremes[(k // 3) % 4]
                hit += 1
    assert hit >= 16
    check_loss(Ts, lg, pr, cfg["batch"], "B4 extremes")


def test_end_to_end_gradients_match_fp64(g):
    """A 2-conv body + RPN head through compat.install(), rpn_targets, rpn_losses, .backward(): every parameter gradient against the
    same model in torch-CPU fp64 with the restatement's targets, max|d| <= 1e-4 max|grad| per tensor (the conv parity contract)."""
    import torch.nn as nn
    import torch.nn.functional as F
    import m3d
    import m3d.compat as compat
    compat.install()
    try:
        torch.manual_seed(0)
        cfg, gt, dc, im, seed = case_inputs(g, "small_dc")
        A = 35

        class Net(nn.Module):
            def __init__(self):
                super().__init__()
                self.c1, self.c2 = nn.Conv3d(1, 8, 3, 1, 1), nn.Conv3d(8, 16, 3, 1, 1)
                self.rpn, self.cls, self.box = nn.Conv3d(16, 16, 3, 1, 1), nn.Conv3d(16, A, 1, 1, 0), nn.Conv3d(16, 6 * A, 1, 1, 0)

            def forward(self, x):
                h = F.max_pool3d(F.relu(self.c1(x)), 2)
                h = F.max_pool3d(F.relu(self.c2(h)), 4)
                h = F.relu(self.rpn(h))
                return self.cls(h), self.box(h)
        net = Net()
        ref = Net().double()
        ref.load_state_dict({k: v.double() for k, v in net.state_dict().items()})
        net = net.cuda()
        x = torch.randn(1, 1, *im)
        T = m3d.rpn_targets(gt, im, dev_cfg(cfg), seed, dc)
        lc, lb = m3d.rpn_losses(*net(x.cuda()), T)
        (lc + lb).backward()
        compat.uninstall_conv3d()
        want = R.rpn_targets(gt, im, cfg, seed, dc)
        same_sets(as_dict(T), want)
        lw, tw, iw, ow = (torch.from_numpy(b) for b in R.wide(want))
        logits, pred = ref(x.double())
        s, h, w = logits.shape[2:]
        lab = lw[:, :, :s, :h, :w]
        wgt = (lab >= 0).double()
        rc = F.binary_cross_entropy_with_logits(logits, lab.clamp(min=0).double(), wgt, reduction="sum") / wgt.sum()
        d = iw[:, :, :s, :h, :w].double() * (pred - tw[:, :, :s, :h, :w].double())
        beta = 1.0 / 9
        sl1 = torch.where(d.abs() < beta, 0.5 * d * d / beta, d.abs() - 0.5 * beta)
        rb = (ow[:, :, :s, :h, :w].double() * sl1).sum() / logits.shape[0]
        (rc + rb).backward()
        assert abs(lc.item() - rc.item()) < 1e-5 * rc.item() and abs(lb.item() - rb.item()) < 1e-5 * max(rb.item(), 1e-3)
        for (n, p), (_, q) in zip(net.named_parameters(), ref.named_parameters()):
            err, ref_max = (p.grad.double().cpu() - q.grad).abs().max().item(), q.grad.abs().max().item()
            print(n, "max|d| %.3g of max|grad| %.3g" % (err, ref_max))
            assert ref_max > 0 and err <= 1e-4 * ref_max, n
    finally:
        compat.uninstall_conv3d()
        compat.uninstall_linear()


def test_train_rpn_tool_overfits_one_sample():
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tools", "train_rpn.py"), "--steps", "30"],
                       capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0
    tot = [float(ln.split()[-1]) for ln in r.stdout.splitlines() if ln.startswith("step ")]
    assert len(tot) == 30 and np.isfinite(tot).all()
    assert np.mean(tot[-5:]) < np.mean(tot[:5])
