"""GPU: the per-RoI convs on the narrow-map f16x2 kernel through the host layers: m3d.compat.set_conv_train_narrow (forward and
backward-data of an intercepted F.conv3d on a 7^3 grid, against fp64 autograd and the contract's bound; the default bit for bit),
m3d.train.ConvBoxHead's gradients against the fp64 module (margin and method of tests/test_gpu_conv_box_head.py), and DetectorM3D with
M3D_HEAD_CONV_F16 (both head convs planned `f16x2 narrow`, outputs against the fp64 chain; unset: today's plans and bits)."""
import pytest
import torch

import conv_f16_narrow_cases as T
import conv_train_cases as TC
import test_gpu_conv_box_head as BH

pytestmark = pytest.mark.gpu


@pytest.fixture
def compat():
    import m3d.compat as c
    was = (c._orig_conv3d is not None, c._orig_linear is not None)
    c.install()
    yield c
    c.set_conv_train_narrow(False)
    c.uninstall_conv3d(), c.uninstall_linear()
    if was[0]:
        c.install_conv3d()
    if was[1]:
        c.install_linear()


def _step(conv, x, r):
    conv.zero_grad()
    xr = x.clone().requires_grad_(True)
    y = conv(xr)
    (y * r).sum().backward()
    return y.detach(), xr.grad, conv.weight.grad.clone(), conv.bias.grad.clone()


def test_conv3d_forward_and_dgrad_on_the_narrow_kernel(compat):
    from m3d import ops, conv_plan as cp
    torch.manual_seed(4)
    conv = torch.nn.Conv3d(32, 64, 3, 1, 1).cuda()
    x = torch.relu(torch.randn(4, 32, 7, 7, 7, device="cuda")) * 3
    r = torch.randn(4, 64, 7, 7, 7, device="cuda")
    w, b = conv.weight.detach(), conv.bias.detach()
    assert compat.get_conv_train_narrow() is False
    base = _step(conv, x, r)                                               # before the switch was ever set in this test
    fp32 = (ops.PackedConv3d(w, ops.W_PLAIN)(x, shift=b), ops.PackedConv3d(w, ops.W_DGRAD)(r), ops.conv3d_wgrad(x, r, 3),
            ops.conv3d_bias_grad(r))
    assert all(torch.equal(p, q) for p, q in zip(base, fp32))
    # 8 launch units: below conv_plan.ZN_MIN_UNITS, so the default threshold keeps the layer on fp32 ...
    assert cp.train_conv_kernel("forward", 4, 32, 64, 7, 7, 7, "fp32", narrow=True) == cp.TRAIN_FP32
    assert compat.set_conv_train_narrow(True) is False
    assert all(torch.equal(p, q) for p, q in zip(_step(conv, x, r), base))
    # ... and min_units = 0 routes it
    assert compat.set_conv_train_narrow(True, min_units=0) is True
    y, gx, gw, gb = _step(conv, x, r)
    Z = ops.ZnConv3d
    assert torch.equal(y, Z(w)(x, Z.bound_of(x), shift=b, out_max=False)[0]) and not torch.equal(y, base[0])
    gb_want, gy_max = ops.conv3d_gy_reduce(r)
    assert torch.equal(gx, Z.dgrad_of(w)(r, gy_max, out_max=False)[0]) and not torch.equal(gx, base[1])
    assert torch.equal(gb, gb_want)                                        # one pass over gy: the bound and the bias gradient
    assert torch.equal(gw, base[2])                                        # the wgrad routing is untouched
    # against fp64 autograd, element by element
    c64 = torch.nn.Conv3d(32, 64, 3, 1, 1).double()
    c64.load_state_dict({k: v.detach().cpu().double() for k, v in conv.state_dict().items()})
    y64, gx64, gw64, gb64 = _step(c64, x.cpu().double(), r.cpu().double())
    yr, Ey, _ = T.contract("forward", x.cpu(), w.cpu(), None, b.cpu())
    assert torch.equal(yr, y64) or bool(((yr - y64).abs() <= 1e-12 * y64.abs().max()).all())
    assert bool(((y.cpu().double() - y64).abs() <= Ey).all())
    gxr, Eg, _ = T.contract("dgrad", r.cpu(), T.dgrad_weight(w.cpu()))
    assert bool(((gxr - gx64).abs() <= 1e-12 * gx64.abs().max()).all())
    assert bool(((gx.cpu().double() - gx64).abs() <= Eg).all())
    S, Eb = TC.gb_bound(r.cpu())                                           # the bound of tests/test_gpu_conv_train.py::test_gy_reduce
    assert bool(((S - gb64).abs() <= 1e-12 * gb64.abs().max()).all()) and bool(((gb.cpu().double() - S).abs() <= Eb).all())
    assert float((gw.cpu().double() - gw64).abs().max()) <= 1e-5 * float(gw64.abs().max())      # (fp32 kernel, unchanged: its own tests' envelope)
    # with the narrow fp32 wgrad as well: the two switches compose
    compat.set_conv_wgrad_narrow(True)
    try:
        y2, gx2, gw2, gb2 = _step(conv, x, r)
        assert torch.equal(y2, y) and torch.equal(gx2, gx) and torch.equal(gb2, gb) and torch.equal(gw2, ops.conv3d_wgrad_narrow(x, r))
    finally:
        compat.set_conv_wgrad_narrow(False)
    # a weight update drops the packs (the _packed cache keys on the parameter's version)
    with torch.no_grad():
        conv.weight.mul_(0.5)
    y3 = _step(conv, x, r)[0]
    assert torch.equal(y3, Z(conv.weight.detach())(x, Z.bound_of(x), shift=b, out_max=False)[0])
    with torch.no_grad():
        conv.weight.mul_(2.0)
    # the switch off again: the bits from before it was set
    assert compat.set_conv_train_narrow(False) is True
    assert all(torch.equal(p, q) for p, q in zip(_step(conv, x, r), base))


def test_conv_box_head_gradients(compat, monkeypatch):
    import m3d
    from m3d import ops
    stride = 4
    torch.manual_seed(11)
    head = m3d.ConvBoxHead(32, stride, conv_head_dim=32, num_stacked_convs=2, mlp_head_dim=64).cuda()
    with torch.no_grad():
        head.cls_score.weight.normal_(0, 0.05), head.bbox_pred.weight.normal_(0, 0.05)
        for p in head.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    gen = torch.Generator().manual_seed(12)
    feat = torch.randn((1, 32, 8, 8, 8), generator=gen).cuda()
    rois7 = torch.tensor([[0, 10.0, 12.0, 9.0, 16.5, 17.0, 13.0],
                          [0, 18.0, 10.0, 12.0, 31.0, 31.0, 31.0],
                          [0, 3.5, 8.0, 2.0, 30.0, 21.0, 20.0],
                          [0, 10.0, 5.0, 14.0, 25.0, 30.0, 29.0],
                          [0, 1.0, 2.0, 3.0, 12.0, 20.0, 28.0],
                          [0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]).cuda()
    r1, r2 = torch.randn((6, 2), generator=gen).cuda(), torch.randn((6, 12), generator=gen).cuda()
    g64 = BH._head_fp64(head, feat, rois7, r1, r2, 1.0 / stride, 2)
    compat.uninstall_conv3d(), compat.uninstall_linear()
    e_torch = BH._err(BH._grads(head, feat, rois7, r1, r2), g64)          # torch's own conv3d / linear on the device
    compat.install()
    off = BH._grads(head, feat, rois7, r1, r2)
    compat.set_conv_train_narrow(True, min_units=0)
    rec = BH.Record(ops.lib())
    monkeypatch.setattr(ops, "lib", lambda: rec)
    on = BH._grads(head, feat, rois7, r1, r2)
    monkeypatch.undo()
    # two forwards and two dgrads (the first conv's input, RoIAlign's output, needs its gradient too); ops.conv3d_gy_reduce asks the
    # library twice per call (the workspace size, then the pass); no conv of the head is left on the direct kernel
    assert rec.calls.count("m3d_conv3d_zn_forward") == 4 and rec.calls.count("m3d_conv3d_gy_reduce") == 2 * 2
    assert "m3d_conv3d_forward" not in rec.calls and "m3d_conv3d_bias_grad" not in rec.calls
    e_off, e_on = BH._err(off, g64), BH._err(on, g64)
    print("ConvBoxHead gradients: e_torch %.3g e_m3d %.3g (narrow f16x2 off) %.3g (on)" % (e_torch, e_off, e_on))
    assert e_on <= 4 * e_torch, (e_on, e_torch)
    assert any(not torch.equal(on[k], off[k]) for k in on)


def _detector(monkeypatch, on):
    from m3d.model import DetectorM3D
    if on:
        monkeypatch.setenv("M3D_HEAD_CONV_F16", "1")
    else:
        monkeypatch.delenv("M3D_HEAD_CONV_F16", raising=False)
    return DetectorM3D(BH._params(), BH._cfg())


def test_detector_head_on_the_narrow_kernel(monkeypatch):
    """synth.make_params(box_head="roi_Xconv1fc_head", conv_head_dim=32): head convs 256 -> 32 -> 32 (the body's 256 channels are what
    RoIAlign reads; 32 is the smallest head width with cin % 16 == 0 the fixtures of test_gpu_conv_box_head.py build).  The fp64 chain is
    built here from the RoIAlign output, as test_gpu_conv_box_head.py::test_box_head_outputs_of_the_detector builds it."""
    from m3d import ops, conv_plan as cp
    P, cfg = BH._params(), BH._cfg()
    off, on = _detector(monkeypatch, False), _detector(monkeypatch, True)
    assert not off.head_conv_f16 and on.head_conv_f16
    gen = torch.Generator().manual_seed(6)
    feat = torch.randn((2, 256, 4, 8, 8), generator=gen).cuda()
    R = 70                                                                 # 140 launch units: above conv_plan.ZN_MIN_UNITS
    rois = BH._rois(R, gen)
    assert [c.plan((R, 7, 7, 7)).kind for c in on.head_convs] == [cp.ZN, cp.ZN]
    assert [c.plan((R, 7, 7, 7)).kind for c in off.head_convs] == [cp.DIRECT, cp.DIRECT] and all(c.zn is None for c in off.head_convs)
    x = ops.roi_align3d_forward(feat, rois, 7, 7, 7, 1.0 / 8, 2)
    c64, b64, p64 = BH._compose(P, x, rois, cfg, torch.float64, "cpu")
    c32, b32, p32 = BH._compose(P, x, rois, cfg, torch.float32, "cuda")
    base = off.box_head_outputs(feat, rois)
    for carried in (False, True):
        f = feat.clone()
        if carried:                                                        # the bound a producing conv leaves: here 2 max|feat|, a loose one
            bound = ops.ZwConv3d.bound_of(f) * 2
            f._m3d_bound = (bound, f._version)
        cls, bbox, pred = on.box_head_outputs(f, rois)
        for name, got, t32, ref in (("cls", cls, c32, c64), ("pred_boxes", pred, p32, p64)):
            e = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
            e_torch = float((t32.double().cpu() - ref).abs().max() / ref.abs().max())
            print("carried %d %-10s e %.3g e_torch %.3g" % (carried, name, e, e_torch))
            assert e <= 4 * e_torch, (name, e, e_torch)
        assert not torch.equal(cls, base[0]) or not torch.equal(pred, base[2])
    # a few RoIs stay below the threshold: today's kernels, today's bits
    few = rois[:7].contiguous()
    assert [c.plan((7, 7, 7, 7)).kind for c in on.head_convs] == [cp.DIRECT, cp.DIRECT]
    assert all(torch.equal(p, q) for p, q in zip(on.box_head_outputs(feat, few), off.box_head_outputs(feat, few)))
    # unset: bit-equal to a detector built without the new argument
    again = _detector(monkeypatch, False)
    assert all(torch.equal(p, q) for p, q in zip(again.box_head_outputs(feat, rois), base))
    assert on.box_head_outputs(feat, rois[:0])[0].shape == (0, 2)
