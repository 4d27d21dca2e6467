"""GPU: the mask-branch training step (csrc/mask_train.hip, m3d.train) against the reference's results (tests/golden/mask_train.npz),
the NumPy restatement (tests/mask_train_reference.py) and fp64 evaluations of the loss and of the head.  Reads only tests/golden/ and the
restatement."""
import ctypes as C

import numpy as np
import pytest
import torch

import mask_train_reference as MR
from test_mask_train_host import CASES, GOLD, LOSS_CASES, case_inputs, check_targets, loss_case, restated

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLD))


def box_cfg(cfg):
    import m3d
    return m3d.BoxHeadTrainCfg(batch_per_im=cfg["batch"], fg_fraction=cfg["fg_fraction"], fg_thresh=cfg["fg_thresh"], bg_thresh_hi=cfg["bg_hi"],
                               bg_thresh_lo=cfg["bg_lo"], num_classes=cfg["num_classes"], bbox_reg_weights=cfg["weights"])


def mask_cfg(d, **kw):
    import m3d
    return m3d.MaskTrainCfg(resolution=d["M"], anno_type=d["mode"], cls_specific=d["cls_specific"], num_classes=d["num_classes"],
                            in_size=d["tile"], **kw)


def box_targets(ds):
    """m3d.box_head_targets on the cases' proposals (column 0 and the rows beyond num[b] hold values nobody may read)"""
    import m3d
    rows = max(len(d["proposals"]) for d in ds) + 3
    rois = np.full((len(ds), rows, 7), 1e6, f32)
    for b, d in enumerate(ds):
        rois[b, :len(d["proposals"]), 1:] = d["proposals"]
    num = torch.tensor([len(d["proposals"]) for d in ds], dtype=torch.int32).cuda()
    return m3d.box_head_targets(torch.from_numpy(rois).cuda(), num, [d["gt"] for d in ds], box_cfg(ds[0]["box_cfg"]), [d["seed"] for d in ds],
                                gt_classes=[d["classes"] for d in ds], gt_crowd=[d["crowd"] for d in ds])


def device_targets(ds, dtype=torch.uint16):
    import m3d
    T = box_targets(ds)
    kw = dict(gt_classes=[d["classes"] for d in ds], gt_crowd=[d["crowd"] for d in ds])
    if ds[0]["mode"] == "spot":
        kw["spots"] = [d["spots"] for d in ds]
    else:
        vols = [torch.from_numpy(d["volume"].astype(np.int32 if dtype == torch.int32 else np.uint16)).cuda() for d in ds]
        kw.update(gt_boxes=[d["gt"] for d in ds], markers=[d["markers"] for d in ds], labels=vols)
    return T, m3d.mask_targets(T, mask_cfg(ds[0]), **kw)


def check_padding(MT, b, n):
    assert (MT.masks[b, n:] == -1).all() and (MT.rois[b, n:] == 0).all() and (MT.assign[b, n:] == -1).all()
    assert (MT.masks[b, :n] >= -1).all() and (MT.assign[b, :n] >= 0).all()


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(g, name):
    d = case_inputs(g, name)
    dtypes = (torch.uint16, torch.int32) if d["mode"] == "mask" else (None,)
    for dt in dtypes:
        T, MT = device_targets([d], dt)
        got = MT.numpy()[0]
        check_targets(got, g, name, "device")
        want = restated(g, name, "closed")
        for k in ("masks", "assign", "counts"):
            assert np.array_equal(got[k], want[k]), k
        n = int(got["counts"][0])
        check_padding(MT, 0, n)
        F, Cm = T.cfg.fg_per_im, d["num_classes"] if d["cls_specific"] else 1
        assert tuple(MT.masks.shape) == (1, F, Cm * d["M"] ** 3) and MT.masks.dtype == torch.int32 and MT.counts.dtype == torch.int64
        blobs = MT.blobs()
        r7 = blobs["mask_rois"].cpu().numpy()
        assert r7.shape == (F, 7) and (r7[:, 0] == 0).all() and np.array_equal(r7[:n, 1:], g[name + "_rois"]) and (r7[n:] == 0).all()
        assert np.array_equal(blobs["roi_has_mask_int32"].cpu().numpy(), (T.labels.cpu().numpy().reshape(-1) > 0).astype(np.int32))
        assert torch.equal(blobs["masks_int32"], MT.masks[0])


@pytest.mark.parametrize("names", [("spot_small", "spot_nofg"), ("mask_nofg", "mask_small")])
def test_two_images_equal_two_calls(g, names):
    """an image without an fg row beside one with some: every output of the pair is the two single calls stacked"""
    ds = [case_inputs(g, n) for n in names]
    _, both = device_targets(ds)
    for b, d in enumerate(ds):
        _, one = device_targets([d])
        for k in ("masks", "rois", "assign", "counts"):
            assert torch.equal(getattr(both, k)[b], getattr(one, k)[0]), (names[b], k)
        check_targets(both.numpy()[b], g, names[b], "pair")
    r7 = both.rois7.cpu().numpy()
    F = both.assign.shape[1]
    fg = [int(c) for c in both.counts[:, 0].cpu()]
    assert (r7[F:F + fg[1], 0] == 1).all() and (r7[F + fg[1]:] == 0).all() and (r7[:F, 0] == 0).all()


def guarded(shape, dtype, pad=64):
    """(whole buffer, the view a kernel may write): NaN bit patterns before and after the view"""
    n = int(np.prod(shape))
    if dtype == torch.float32:
        whole = torch.full((n + 2 * pad,), float("nan"), dtype=dtype, device="cuda")
    else:
        whole = torch.full((n + 2 * pad,), 0x7FC00000, dtype=dtype, device="cuda")
    return whole, whole[pad:pad + n].view(shape), pad


def guards_intact(whole, pad, dtype):
    edge = torch.cat([whole[:pad], whole[-pad:]])
    return bool(torch.isnan(edge).all()) if dtype == torch.float32 else bool((edge == 0x7FC00000).all())


def test_guards_and_determinism(g):
    """the C entry points on caller-owned outputs between guard words: nothing outside an output is written, every element inside
    is, and two runs give the same bits (spot and mask mode, then the loss)"""
    from m3d import ops
    from m3d._lib import MaskImage, check, lib
    for name in ("spot_3cls", "mask_small"):
        d = case_inputs(g, name)
        T = box_targets([d])
        B, batch = T.labels.shape
        F, M = T.cfg.fg_per_im, d["M"]
        Cm = d["num_classes"] if d["cls_specific"] else 1
        off = np.array([0, len(d["gt"])], np.int32)
        cls, crowd = torch.from_numpy(d["classes"].astype(np.int32)).cuda(), torch.from_numpy(d["crowd"].astype(np.uint8)).cuda()
        spots = gt = markers = images = size = vol = None
        if d["mode"] == "spot":
            spots, size = torch.from_numpy(d["spots"]).cuda(), (C.c_int32 * 3)(*d["tile"])
        else:
            gt, markers = torch.from_numpy(d["gt"]).cuda(), torch.from_numpy(d["markers"]).cuda()
            vol = torch.from_numpy(d["volume"].astype(np.uint16)).cuda()
            images = (MaskImage * 1)()
            images[0].labels, images[0].dtype = vol.data_ptr(), 0
            images[0].depth, images[0].height, images[0].width = d["tile"]
        runs = []
        for _ in range(2):
            outs = [guarded((B, F, Cm * M ** 3), torch.int32), guarded((B, F, 6), torch.float32), guarded((B, F), torch.int32),
                    guarded((B, 4), torch.int64)]
            p = [C.c_void_p(o[1].data_ptr()) for o in outs]
            check(lib().m3d_mask_targets(ops._ptr(T.labels), ops._ptr(T.rois), ops._ptr(T.counts), B, batch, F, M, d["num_classes"],
                                         int(d["cls_specific"]), 0 if d["mode"] == "spot" else 1, off.ctypes.data_as(C.c_void_p),
                                         ops._ptr(cls), ops._ptr(crowd), ops._ptr(spots), size, ops._ptr(gt), ops._ptr(markers), images,
                                         p[0], p[1], p[2], p[3], ops._stream()), "mask_targets")
            torch.cuda.synchronize()
            for (whole, view, pad), dt in zip(outs, (torch.int32, torch.float32, torch.int32, torch.int64)):
                assert guards_intact(whole, pad, dt)
                assert not bool(torch.isnan(view).any()) if dt == torch.float32 else bool((view != 0x7FC00000).all())
            runs.append([o[1].clone() for o in outs])
        assert all(torch.equal(a, b) for a, b in zip(*runs))
        want = restated(g, name, "closed")
        n = len(want["assign"])
        assert np.array_equal(runs[0][0][0, :n].cpu().numpy(), want["masks"]) and np.array_equal(runs[0][3][0].cpu().numpy(), want["counts"])
    x, t, weight = loss_case(g, "loss_3cls")
    xd, td = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    N, Cm, M = x.shape[:3]
    nbytes = int(lib().m3d_mask_loss_workspace_bytes(C.c_int64(N), Cm, M))
    runs = []
    for _ in range(2):
        lo, gr, nu = guarded((1,), torch.float32), guarded(x.shape, torch.float32), guarded((1,), torch.int64)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
        check(lib().m3d_mask_loss(ops._ptr(xd), ops._ptr(td), C.c_int64(N), Cm, M, C.c_double(weight), C.c_void_p(lo[1].data_ptr()),
                                  C.c_void_p(nu[1].data_ptr()), C.c_void_p(gr[1].data_ptr()), ops._ptr(ws), C.c_size_t(nbytes), ops._stream()),
              "mask_loss")
        torch.cuda.synchronize()
        assert guards_intact(lo[0], lo[2], torch.float32) and guards_intact(gr[0], gr[2], torch.float32) and guards_intact(nu[0], nu[2], torch.int64)
        assert not bool(torch.isnan(gr[1]).any()) and not bool(torch.isnan(lo[1]).any()) and int(nu[1][0]) == int((t > -1).sum())
        runs.append((lo[1].clone(), gr[1].clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def manual_box_targets(rois, batch=16, fg_fraction=0.5, labels=None):
    """BoxHeadTargets of one image whose fg rows are the given RoIs (what the sampler would leave), without running the sampler"""
    import m3d
    cfg = m3d.BoxHeadTrainCfg(batch_per_im=batch, fg_fraction=fg_fraction)
    n = len(rois)
    lab = np.full((1, batch), -1, np.int32)
    lab[0, :n] = 1 if labels is None else labels
    r = np.zeros((1, batch, 6), f32)
    r[0, :n] = rois
    counts = np.array([[n, n, 0, n, 0, 0, 1, 0]], np.int64)
    return m3d.BoxHeadTargets(torch.full((1, batch), -1, dtype=torch.int64).cuda(), torch.from_numpy(lab).cuda(), torch.from_numpy(r).cuda(),
                              torch.zeros((1, batch, 6)).cuda(), torch.from_numpy(counts).cuda(), cfg)


@pytest.mark.parametrize("dtype", [np.uint16, np.int32])
def test_wide_rois_in_mask_mode(dtype):
    """A 255-wide RoI (footprints of 70 per axis), one longer than the volume, one reaching outside it on every side and one whose
    extent exceeds the device's clamp of 1024: device == restatement."""
    import m3d
    S, H, W = 24, 40, 300
    rng = np.random.RandomState(7)
    vol = np.zeros((S, H, W), dtype)
    z, y, x = np.meshgrid(np.arange(S), np.arange(H), np.arange(W), indexing="ij")
    marker = 40000 if dtype == np.uint16 else 70000
    vol[(((x - 150) / 140.0) ** 2 + ((y - 20) / 15.0) ** 2 + ((z - 12) / 9.0) ** 2 <= 1) & (rng.rand(S, H, W) < 0.01)] = marker
    vol[(vol == 0) & (rng.rand(S, H, W) < 0.01)] = 5
    gt = np.array([[8, 4, 2, 292, 36, 22], [0, 0, 0, 20, 20, 10]], f32)
    markers = np.array([marker, 5], np.int32)
    rois = np.array([[20, 5, 3, 275, 35, 21],                  # 255 wide
                     [10.5, 3.2, 1.7, 290.9, 37.5, 22.4],
                     [-50, -3, -2, 400, 100, 60],              # reaches outside the volume on every side
                     [0, 0, 0, 2000, 39, 23],                  # extent beyond the clamp
                     [100, 10, 5, 140, 30, 15]], f32)
    T = manual_box_targets(rois)
    cfg = m3d.MaskTrainCfg.nuclei(in_size=(S, H, W))
    lab = torch.from_numpy(vol).cuda()
    MT = m3d.mask_targets(T, cfg, gt_boxes=[gt], markers=[markers], labels=[lab])
    got = MT.numpy()[0]
    want = MR.mask_targets(T.labels.cpu().numpy()[0], T.rois.cpu().numpy()[0], 14, gt_boxes=gt, markers=markers, label_volume=vol)
    assert np.array_equal(got["assign"], want["assign"]) and (want["assign"] == 0).all()
    per = want["masks"].sum(1)
    assert ((per > 0) & (per < 14 ** 3)).all()                 # sparse voxels: neither empty nor full, so the interval ends matter
    assert np.array_equal(got["masks"], want["masks"]) and np.array_equal(got["counts"], want["counts"])
    check_padding(MT, 0, len(rois))


@pytest.mark.parametrize("lname", sorted(LOSS_CASES))
def test_loss_and_gradient(g, lname):
    from m3d import ops
    x, t, weight = loss_case(g, lname)
    l64, g64, W, abs_sum = MR.loss(x, t, weight)
    dev_loss, ref_loss, dev_grad, _ = MR.loss_bounds(l64, g64, W, abs_sum, weight, x.size)
    loss, num, grad = ops.mask_loss_grad(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda(), weight)
    loss, grad = float(loss.cpu()[0]), grad.cpu().numpy().astype(np.float64)
    print(lname, "loss err", abs(loss - l64), "of", dev_loss, "| grad err", np.abs(grad - g64).max(), "| vs reference",
          abs(loss - float(g[lname + "_loss"])), "of", ref_loss)
    assert int(num.cpu()[0]) == W
    assert abs(loss - l64) <= dev_loss and (np.abs(grad - g64) <= dev_grad).all()
    assert f32(loss) == f32(l64)                                                      # one rounding of the fp64 value
    assert abs(loss - float(g[lname + "_loss"])) <= ref_loss + dev_loss
    assert not grad.reshape(t.shape)[t == -1].any() and grad.reshape(t.shape)[t > -1].any()      # exactly 0 at ignored elements
    assert grad.shape == x.shape


def test_loss_without_labelled_voxels_and_backward_scale(g):
    """W = 0 is defined (loss 0, gradient 0); through autograd the stored gradient is scaled by the incoming scalar"""
    import m3d
    x, t, weight = loss_case(g, "loss_spot")
    cfg = m3d.MaskTrainCfg.soma(weight_loss_mask=2.5)
    rows = x.shape[0]

    def targets(masks):
        return m3d.MaskTargets(torch.from_numpy(masks).cuda().reshape(1, rows, -1), torch.zeros((1, rows, 6)).cuda(),
                               torch.zeros((1, rows), dtype=torch.int32).cuda(), torch.zeros((1, 4), dtype=torch.int64).cuda(), None, cfg)
    xd = torch.from_numpy(x).cuda().requires_grad_(True)
    none = m3d.mask_losses(xd, targets(np.full_like(t, -1)))
    none.backward()
    assert float(none.detach()) == 0.0 and not bool(xd.grad.any()) and not bool(torch.isnan(xd.grad).any())
    xd.grad = None
    loss = m3d.mask_losses(xd, targets(t))
    (3.0 * loss).backward()
    l64, g64, W, abs_sum = MR.loss(x, t, 2.5)
    dev_loss, _, dev_grad, _ = MR.loss_bounds(l64, g64, W, abs_sum, 2.5, x.size)
    assert abs(float(loss.detach()) - l64) <= dev_loss
    # the stored fp32 gradient times 3 in fp32: one more rounding
    assert (np.abs(xd.grad.cpu().numpy().astype(np.float64) - 3 * g64) <= 3 * dev_grad + 2.0 ** -24 * np.abs(3 * g64)).all()


def head_fp64(P, pooled, masks, weight):
    """the head after RoIAlign and the loss, in fp64 on the CPU with torch's own operators; parameter gradients by autograd.
    -> loss, gradients, logits, and per parameter element the sum of the absolute values of the terms its gradient adds up
    (sum over positions of |input| |upstream gradient|; every layer is linear in its parameters, so that is the gradient of the layer
    applied to |input| against |upstream gradient|)"""
    import torch.nn.functional as F
    P = {k: v.detach().double().cpu().requires_grad_(True) for k, v in P.items()}
    x = pooled.double().cpu()
    layers = []

    def layer(prefix, fn, x):
        out = fn(x, P[prefix + ".weight"], P[prefix + ".bias"])
        out.retain_grad()
        layers.append((prefix, fn, x.detach(), out))
        return out
    i = 0
    while "conv_fcn.%d.weight" % (2 * i) in P:
        x = F.relu(layer("conv_fcn.%d" % (2 * i), lambda a, w, b: F.conv3d(a, w, b, padding=1), x))
        i += 1
    x = F.relu(layer("upconv", lambda a, w, b: F.conv_transpose3d(a, w, b, stride=2), x))
    y = layer("classify", lambda a, w, b: F.conv3d(a, w, b), x)
    t = masks.double().cpu().reshape(y.shape)
    on = t > -1
    loss = weight * F.binary_cross_entropy_with_logits(y[on], t[on], reduction="sum") / on.sum()
    loss.backward()
    terms = {}
    for prefix, fn, xin, out in layers:
        w = torch.zeros_like(P[prefix + ".weight"]).requires_grad_(True)
        b = torch.zeros_like(P[prefix + ".bias"]).requires_grad_(True)
        (fn(xin.abs(), w, b) * out.grad.abs()).sum().backward()
        terms[prefix + ".weight"], terms[prefix + ".bias"] = w.grad, b.grad
    return float(loss.detach()), {k: v.grad for k, v in P.items()}, y.detach(), terms


def test_mask_head_gradients_and_training(g):
    """MaskHead at dim_in 16, dim_reduced 16 on an 8 x 16 x 12 feature map (stride 4 of the 32 x 64 x 48 tile) with 6 fg rows: the
    parameter gradients of mask_losses(...).backward() against a torch fp64 CPU run of the same head on the same targets (from the
    device's RoIAlign output, which has no parameters and is tested bit for bit elsewhere), element by element: rtol 1e-4 as the issue
    sets it, plus an atol for the elements whose terms cancel.  A gradient element is a sum of terms |input| |upstream gradient|; on the
    device every term carries the fp32 roundings of the up to five layers before and after it (a few 2^-24 each, relative) and the sum
    is accumulated in fp32 in blocks: 16 * 2^-24 of the element's sum of absolute terms, taken from the fp64 run.  Its state loads into
    MaskHeadM3D and back; 20 SGD steps on the fixed batch lower loss_mask."""
    import m3d
    from m3d.config import Cfg
    from m3d.mask_head import MaskHeadM3D
    d = case_inputs(g, "spot_small")
    T = manual_box_targets(d["gt"][:6], batch=16, fg_fraction=0.5)
    cfg = m3d.MaskTrainCfg.soma(in_size=d["tile"], dim_reduced=16, num_convs=2)
    MT = m3d.mask_targets(T, cfg, spots=[d["spots"]], gt_crowd=[d["crowd"]])
    assert int(MT.counts[0, 0]) == 6 and 0 < int(MT.counts[0, 1]) < int(MT.counts[0, 2]) == 6 * 14 ** 3
    torch.manual_seed(5)
    head = m3d.MaskHead(16, cfg, stride=4).cuda()
    with torch.no_grad():
        head.classify.weight.normal_(0, 0.05)                 # the reference's 0.001 leaves every logit at 0: nothing to compare
    feat = torch.randn((1, 16, 8, 16, 12), generator=torch.Generator().manual_seed(6)).cuda()
    rois7 = MT.rois7
    logits = head(feat, rois7)
    assert tuple(logits.shape) == (8, 1, 14, 14, 14)
    loss = m3d.mask_losses(logits, MT)
    loss.backward()
    pooled = m3d.roi_align3d_forward(feat, rois7, 7, 7, 7, 0.25, 2)
    l64, g64, y64, terms = head_fp64(dict(head.named_parameters()), pooled, MT.masks, cfg.weight_loss_mask)
    assert abs(float(loss) - l64) <= 1e-4 * abs(l64)
    for k, p in head.named_parameters():
        got, want = p.grad.double().cpu(), g64[k]
        err, allowed = (got - want).abs(), 1e-4 * want.abs() + 16 * 2.0 ** -24 * terms[k]
        print(k, "max |grad|", float(want.abs().max()), "max err", float(err.max()), "largest err / allowed", float((err / allowed).max()))
        assert float(want.abs().max()) > 0 and bool((terms[k] >= want.abs() * (1 - 1e-12)).all()) and bool((err <= allowed).all()), k
    # the state under the detector's keys drives the inference head, and comes back
    state = {k: v.detach().clone() for k, v in head.detector_state().items()}
    inf = MaskHeadM3D(state, Cfg.soma(), resolution=14, roi_res=7, sampling_ratio=2, dilation=1, cls_specific=False)
    prob = inf.mask_net(feat, rois7)
    assert float((prob.double().cpu() - torch.sigmoid(y64)).abs().max()) <= 1e-4
    other = m3d.MaskHead(16, cfg, stride=4).cuda()
    other.load_detector_state(state)
    assert all(torch.equal(a, b) for a, b in zip(head.state_dict().values(), other.state_dict().values()))
    # 20 SGD steps on the fixed batch
    opt = torch.optim.SGD(head.parameters(), lr=0.05, momentum=0.9)
    first = last = None
    for step in range(20):
        opt.zero_grad()
        last = m3d.mask_losses(head(feat, rois7), MT)
        last.backward()
        opt.step()
        first = float(last) if first is None else first
    print("loss_mask", first, "->", float(last))
    assert float(last) < first
