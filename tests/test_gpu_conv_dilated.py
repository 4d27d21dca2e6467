"""GPU: the backward of the k = 3, dilation 2, padding 2 conv on the library (csrc/conv3d_wgrad_dilated.hip for the weight gradient, the
W_DGRAD pack through m3d_conv3d_forward_dilated for the data gradient) against the fp64 reference of tests/conv_dilated_cases.py:
 (a) exact on integer operands, element by element, on the library's tile and on each tile asked for by name; twice the same bits;
 (b) within the summation bound on random operands (nothing measured sets it); `pytest -s` prints the worst ratio per case;
 (c) through m3d.compat under set_conv_dilated("m3d"): y, gx, gw, gb exact, nothing falls through to torch, the default mode does;
 (d) train.MaskHead at dilation 2 against the same module in fp64 on the CPU, and its state in MaskHeadM3D(dilation=2).
On one MI355X: the worst ratio of (b) is 0.073 (the D = 1 case); (d) measured e_m3d = 7.5e-7 and e_torch = 8.0e-7."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_dilated_cases as T

pytestmark = pytest.mark.gpu


def same(got, ref, what):
    """bit-equal to the fp64 reference cast to fp32; on a mismatch: how many, the first and the last wrong index, and the taps (for a weight
    gradient) or channels (for a map) that hold one"""
    got, ref = got.cpu(), ref.to(torch.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        if tuple(ref.shape[2:]) == (3, 3, 3):
            where = "taps (dz, dy, dx) %s" % sorted(set(map(tuple, bad[:, 2:].tolist())))
        else:
            where = "channels %s" % sorted(set(bad[:, 1].tolist()))[:40]
        raise AssertionError("%s: %d of %d elements differ; first %s got %r want %r; last %s; %s"
                             % (what, bad.shape[0], ref.numel(), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]),
                                bad[-1].tolist(), where))


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_exact_on_integers(case):
    from m3d import ops
    r = T.reference(case, "int")
    x, gy, w = r["x"].cuda(), r["gy"].cuda(), r["w"].cuda()
    for tile in T.TILES:
        got = ops.conv3d_wgrad(x, gy, 3, dilation=2, tile_x=tile)
        same(got, r["gw"], "wgrad, tile_x %d" % tile)
        assert torch.equal(ops.conv3d_wgrad(x, gy, 3, dilation=2, tile_x=tile), got)
    pack = ops.PackedConv3d(w, ops.W_DGRAD)
    assert (pack.cin, pack.cout) == (case[2], case[1])
    gx = pack(gy, dilation=2)
    same(gx, r["gx"], "dgrad pack, dilation 2")
    assert torch.equal(pack(gy, dilation=2), gx)
    # the keyword's default and dilation=1 are today's call
    assert torch.equal(ops.conv3d_wgrad(x, gy, 3, dilation=1), ops.conv3d_wgrad(x, gy, 3))
    same(ops.conv3d_wgrad(x, gy, 3), T.wgrad64(r["x"], r["gy"], 1), "wgrad, dilation 1")


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_bounded_on_random_data(case):
    from m3d import ops
    r = T.reference(case, "randn")
    x, gy = r["x"].cuda(), r["gy"].cuda()
    for tile in T.TILES:
        slots = ops.conv3d_wgrad_dilated_plan(*case, tile_x=tile)["slots"]
        n = T.terms(case) + slots + 1
        got = ops.conv3d_wgrad(x, gy, 3, dilation=2, tile_x=tile)
        ratio = T.worst_ratio(got.cpu(), r["gw"], r["A"], n)
        print("%s tile_x %2d slots %3d: worst |err| / bound %.4f" % (T.case_id(case), tile, slots, ratio))
        assert ratio < 1.0, (tile, ratio)
        assert torch.equal(ops.conv3d_wgrad(x, gy, 3, dilation=2, tile_x=tile), got)
    if case == T.D1_CASE:
        assert (got[:, :, 0] == 0).all() and (got[:, :, 2] == 0).all()


def test_refusals_reach_python():
    from m3d import ops
    from m3d._lib import M3DError
    x, gy = torch.zeros((1, 4, 3, 3, 3)).cuda(), torch.zeros((1, 5, 3, 3, 3)).cuda()
    for kw in (dict(k=3, dilation=3), dict(k=3, dilation=0), dict(k=1, dilation=2), dict(k=3, dilation=2, tile_x=4)):
        with pytest.raises(M3DError):
            ops.conv3d_wgrad(x, gy, **kw)
    assert (ops.conv3d_wgrad(x, gy, 3, dilation=2) == 0).all()                              # every element is written


@pytest.fixture
def conv_installed():
    import m3d.compat as compat
    compat.install_conv3d()
    prev = compat.get_conv_dilated()
    yield compat
    compat.set_conv_dilated(prev)
    compat.uninstall_conv3d()


def _run_layer(conv, x, gy):
    for p in conv.parameters():
        p.grad = None
    xin = x.clone().requires_grad_(True)
    y = conv(xin)
    y.backward(gy)
    return y.detach(), xin.grad, conv.weight.grad.clone(), conv.bias.grad.clone()


@pytest.mark.parametrize("case", T.COMPAT_CASES, ids=T.case_id)
def test_through_compat(case, conv_installed, monkeypatch):
    compat = conv_installed
    r = T.reference(case, "int")
    B, cin, cout, D, H, W = case
    conv = torch.nn.Conv3d(cin, cout, 3, padding=2, dilation=2).cuda()
    conv1 = torch.nn.Conv3d(cin, cout, 3, padding=1).cuda()
    with torch.no_grad():
        for c in (conv, conv1):
            c.weight.copy_(r["w"]), c.bias.copy_(r["bias"])
    x, gy = r["x"].cuda(), r["gy"].cuda()
    assert compat.get_conv_dilated() == "torch"
    before1 = _run_layer(conv1, x, gy)
    # the default mode: the call reaches the original
    calls, orig = [], compat._orig_conv3d
    monkeypatch.setattr(compat, "_orig_conv3d", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    _run_layer(conv, x, gy)
    assert len(calls) == 1
    # "m3d": nothing falls through, and every result is exact

    def refuse(*a, **k):
        raise AssertionError("torch's conv3d called under set_conv_dilated('m3d')")
    monkeypatch.setattr(compat, "_orig_conv3d", refuse)
    assert compat.set_conv_dilated("m3d") == "torch"
    y, gx, gw, gb = _run_layer(conv, x, gy)
    same(y, r["y"], "y"), same(gx, r["gx"], "gx"), same(gw, r["gw"], "gw")
    assert torch.equal(gb.cpu(), r["gb"].float())
    # without a bias, and with only the weight gradient asked for
    y0 = F.conv3d(x, conv.weight, None, 1, 2, 2)
    same(y0, r["y"] - r["bias"].double().view(1, -1, 1, 1, 1), "y without bias")
    gw_only, = torch.autograd.grad(F.conv3d(x, conv.weight, conv.bias, 1, (2, 2, 2), (2, 2, 2)), (conv.weight,), gy)
    assert torch.equal(gw_only, gw)
    # the backward follows the mode its forward ran under
    xin = x.clone().requires_grad_(True)
    ym = conv(xin)
    compat.set_conv_dilated("torch")
    gx2, gw2 = torch.autograd.grad(ym, (xin, conv.weight), gy)
    assert torch.equal(gx2, gx) and torch.equal(gw2, gw)
    compat.set_conv_dilated("m3d")
    # what the route does not take still reaches the original: another dilation, a non-contiguous input
    monkeypatch.setattr(compat, "_orig_conv3d", lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    n0 = len(calls)
    F.conv3d(x, conv.weight, conv.bias, 1, 3, 3)
    F.conv3d(x.transpose(3, 4), conv.weight, conv.bias, 1, 2, 2)
    F.conv3d(x, conv.weight, conv.bias, 1, 1, 2)
    assert len(calls) == n0 + 3
    # dilation-1 calls are bit-equal before and after switching the mode
    monkeypatch.setattr(compat, "_orig_conv3d", refuse)
    after1 = _run_layer(conv1, x, gy)
    assert all(torch.equal(a, b) for a, b in zip(before1, after1))
    # f16x2 training modes do not reach the dilated layers
    prev_t, prev_w = compat.set_conv_train("f16x2", min_units=0), compat.set_conv_wgrad("f16x2")
    try:
        assert all(torch.equal(a, b) for a, b in zip(_run_layer(conv, x, gy), (y, gx, gw, gb)))
    finally:
        compat.set_conv_train(prev_t), compat.set_conv_wgrad(prev_w)


def _head_fp64(head, feat, rois7, r, scale, ratio):
    """the module in fp64 on the CPU.  RoIAlign3D forward: the fp64 linear map of tests/f16x2_contract.py; its backward: the fp64 reference
    of tests/roi_align_backward_cases.py - the reference's backward kernel is NOT the transpose of its forward (it reads the pooled
    gradient in another bin order and has another z limit), and the library reproduces both, so autograd through the forward map would
    not be this module's feature-map gradient."""
    import roi_align_backward_cases as RB
    from f16x2_contract import roi_align_ref
    h = copy.deepcopy(head).cpu().double()
    x = roi_align_ref(feat.detach().cpu().double(), rois7.cpu(), scale, ratio).requires_grad_(True)
    logits = h.classify(torch.relu(h.upconv(h.conv_fcn(x))))
    (logits * r.cpu().double()).sum().backward()
    g = {k: p.grad for k, p in h.named_parameters()}
    g["feat"] = torch.from_numpy(RB.reference(x.grad.numpy(), rois7.cpu().numpy(), tuple(feat.shape), (7, 7, 7), scale, ratio).grad)
    return logits.detach(), g


def test_mask_head_at_dilation_2(conv_installed):
    import m3d
    import oracle as O
    from m3d.mask_head import MaskHeadM3D
    compat = conv_installed
    ocfg = O.Cfg(mlp_dim=64)
    stride = int(ocfg.stride)
    cfg = m3d.MaskTrainCfg(dim_reduced=32, num_convs=2, dilation=2)
    torch.manual_seed(7)
    head = m3d.MaskHead(16, cfg, stride=stride).cuda()
    with torch.no_grad():
        head.classify.weight.normal_(0, 0.05)
        for p in head.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    gen = torch.Generator().manual_seed(8)
    feat = torch.randn((1, 16, 8, 16, 16), generator=gen).cuda()
    ext = torch.tensor([16.0, 16.0, 8.0]) * stride
    lo = torch.rand((5, 3), generator=gen) * ext * 0.5
    hi = lo + (0.1 + 0.4 * torch.rand((5, 3), generator=gen)) * ext
    rois7 = torch.cat([torch.zeros(5, 1), lo, hi], 1).cuda()
    r = torch.randn((5, 1, 14, 14, 14), generator=gen).cuda()
    logits64, g64 = _head_fp64(head, feat, rois7, r, 1.0 / stride, int(cfg.sampling_ratio))
    e, logits = {}, {}
    for mode in ("torch", "m3d"):
        compat.set_conv_dilated(mode)
        for p in head.parameters():
            p.grad = None
        f = feat.clone().requires_grad_(True)
        logits[mode] = head(f, rois7)
        (logits[mode] * r).sum().backward()
        got = {k: p.grad for k, p in head.named_parameters()}
        got["feat"] = f.grad
        assert set(got) == set(g64)
        e[mode] = max(float((got[k].double().cpu() - g64[k]).abs().max() / g64[k].abs().max()) for k in g64)
        for k in g64:
            print("%-5s %-22s max |fp64 grad| %.4g max err %.3g" % (mode, k, float(g64[k].abs().max()),
                                                                      float((got[k].double().cpu() - g64[k]).abs().max())))
    print("MaskHead at dilation 2: e_m3d %.3g e_torch %.3g" % (e["m3d"], e["torch"]))
    assert all(float(g64[k].abs().max()) > 0 for k in g64)
    assert e["m3d"] <= 4 * e["torch"], e
    # the state dict trained here runs in the inference head at the same dilation
    compat.set_conv_dilated("m3d")
    infer = MaskHeadM3D({k: v.detach() for k, v in head.detector_state().items()}, ocfg, resolution=14, roi_res=7,
                        sampling_ratio=int(cfg.sampling_ratio), dilation=2, cls_specific=False)
    prob = infer.mask_net(feat, {"mask_rois": rois7})
    want = torch.sigmoid(logits["m3d"]).detach()
    assert prob.shape == want.shape
    assert np.allclose(prob.cpu().numpy(), want.cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert np.allclose(prob.cpu().numpy(), torch.sigmoid(logits64).numpy(), rtol=1e-4, atol=1e-5)
