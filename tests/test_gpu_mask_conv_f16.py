"""GPU: the dilation-2 narrow-map f16x2 kernel through the host layers.

Training: m3d.compat.set_conv_dilated_f16 under set_conv_dilated("m3d") on one intercepted Conv3d(32, 32, 3, 1, padding=2, dilation=2)
on a [4, 32, 7, 7, 7] input: off, y / gx / gw / gb are today's bits; on, y and gx are within the contract's E of fp64
(tests/conv_f16_narrow_dilated_cases.py), gb within the gy_reduce bound of tests/test_gpu_conv_narrow_train.py, gw the bits it has off.

Detection: mask_head.MaskHeadM3D(conv_f16=True) on the synthetic parameters of tests/test_gpu_mask_head.py (32 channels, two conv_fcn
layers, a 16^3 feature map, 5 RoIs) at dilation 1 and 2: the trunk launches the narrow kernel (the launch trace of
tests/test_gpu_conv_box_head.py), the mask probabilities satisfy e <= 4 e_torch (e = max |error against a torch fp64 run| / max |ref|,
e_torch the same for torch's own fp32 ops on the device: the rule and the margin of tests/test_gpu_conv_narrow_train.py), and
conv_f16=False is bit-equal to a head built without the argument."""
import pytest
import torch
import torch.nn.functional as F

import conv_f16_narrow_dilated_cases as T
import conv_train_cases as TC
import oracle as O
import test_gpu_conv_box_head as BH
import test_gpu_mask_head as MH

pytestmark = pytest.mark.gpu


@pytest.fixture
def compat():
    import m3d.compat as c
    was = (c._orig_conv3d is not None, c._orig_linear is not None)
    c.install()
    yield c
    c.set_conv_dilated_f16(False)
    c.set_conv_dilated("torch")
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


# ----------------------------------------------------------------------------- training
def test_conv3d_forward_and_dgrad_on_the_dilated_f16_kernel(compat, monkeypatch):
    from m3d import ops, conv_plan as cp
    torch.manual_seed(4)
    conv = torch.nn.Conv3d(32, 32, 3, 1, padding=2, dilation=2).cuda()
    x = torch.relu(torch.randn(4, 32, 7, 7, 7, device="cuda")) * 3
    r = torch.randn(4, 32, 7, 7, 7, device="cuda")
    w, b = conv.weight.detach(), conv.bias.detach()
    compat.set_conv_dilated("m3d")
    assert compat.get_conv_dilated_f16() is False
    base = _step(conv, x, r)                                               # before the switch was ever set in this test: today's path
    fp32 = (ops.PackedConv3d(w, ops.W_PLAIN)(x, shift=b, dilation=2), ops.PackedConv3d(w, ops.W_DGRAD)(r, dilation=2),
            ops.conv3d_wgrad(x, r, 3, dilation=2), ops.conv3d_bias_grad(r))
    assert all(torch.equal(p, q) for p, q in zip(base, fp32))
    # 8 launch units: below conv_plan.ZN_DILATED_MIN_UNITS, so the default threshold keeps the layer where it is ...
    assert cp.ZN_DILATED_MIN_UNITS > 8
    assert compat.set_conv_dilated_f16(True) is False
    assert all(torch.equal(p, q) for p, q in zip(_step(conv, x, r), base))
    # ... and min_units = 0 routes it
    assert compat.set_conv_dilated_f16(True, min_units=0) is True
    rec = BH.Record(ops.lib())
    with monkeypatch.context() as mp:
        mp.setattr(ops, "lib", lambda: rec)
        y, gx, gw, gb = _step(conv, x, r)
    assert rec.calls.count("m3d_conv3d_zn_dilated_forward") == 2 and "m3d_conv3d_forward_dilated" not in rec.calls
    assert rec.calls.count("m3d_conv3d_wgrad_dilated") == 1 and "m3d_conv3d_bias_grad" not in rec.calls
    Z = ops.ZnConv3d
    assert torch.equal(y, Z(w)(x, Z.bound_of(x), shift=b, out_max=False, dilation=2)[0]) and not torch.equal(y, base[0])
    gb_want, gy_max = ops.conv3d_gy_reduce(r)
    assert torch.equal(gx, Z.dgrad_of(w)(r, gy_max, out_max=False, dilation=2)[0]) and not torch.equal(gx, base[1])
    assert torch.equal(gb, gb_want)                                        # one pass over gy: the bound and the bias gradient
    assert torch.equal(gw, base[2])                                        # the weight gradient: the bits it has with the switch off
    # against fp64 autograd, element by element
    c64 = torch.nn.Conv3d(32, 32, 3, 1, padding=2, dilation=2).double()
    c64.load_state_dict({k: v.detach().cpu().double() for k, v in conv.state_dict().items()})
    y64, gx64, gw64, gb64 = _step(c64, x.cpu().double(), r.cpu().double())
    yr, Ey, _ = T.contract("forward", x.cpu(), w.cpu(), None, b.cpu())
    assert bool(((yr - y64).abs() <= 1e-12 * y64.abs().max()).all())
    err_y = (y.cpu().double() - y64).abs()
    gxr, Eg, _ = T.contract("dgrad", r.cpu(), T.dgrad_weight(w.cpu()))
    assert bool(((gxr - gx64).abs() <= 1e-12 * gx64.abs().max()).all())
    err_g = (gx.cpu().double() - gx64).abs()
    print("dilated f16x2 training conv: worst |error| / E  y %.4f  gx %.4f" % (float((err_y / Ey).max()), float((err_g / Eg).max())))
    assert bool((err_y <= Ey).all()) and bool((err_g <= Eg).all())
    S, Eb = TC.gb_bound(r.cpu())                                           # the bound of tests/test_gpu_conv_train.py::test_gy_reduce
    assert bool(((S - gb64).abs() <= 1e-12 * gb64.abs().max()).all()) and bool(((gb.cpu().double() - S).abs() <= Eb).all())
    # without set_conv_dilated("m3d") the switch has no effect: torch's own conv runs, the library is not asked
    compat.set_conv_dilated("torch")
    rec = BH.Record(ops.lib())
    with monkeypatch.context() as mp:
        mp.setattr(ops, "lib", lambda: rec)
        _step(conv, x, r)
    assert not rec.calls
    compat.set_conv_dilated("m3d")
    # the switch off again: the bits from before it was set
    assert compat.set_conv_dilated_f16(False) is True
    assert all(torch.equal(p, q) for p, q in zip(_step(conv, x, r), base))


# ----------------------------------------------------------------------------- detection
CIN, DIM, NC, CONVS, R = 32, 32, 2, 2, 5
ROIS = [[0, 3, 2, 1, 60, 50, 40], [0, 0, 0, 0, 79, 71, 63], [0, 10, 10, 10, 14, 13, 12], [0, 30.5, 20.25, 8, 70, 69, 50],
        [0, 5, 40, 30, 25, 60, 62]]


def _torch_chain(P, pooled, dil, dtype, device):
    """the mask branch from the RoIAlign output in torch's own ops -> probabilities"""
    Q = {k: v.to(device=device, dtype=dtype) for k, v in P.items()}
    x = pooled.to(device=device, dtype=dtype)
    for i in range(CONVS):
        x = F.relu(F.conv3d(x, Q["Mask_Head.conv_fcn.%d.weight" % (2 * i)], Q["Mask_Head.conv_fcn.%d.bias" % (2 * i)], padding=dil, dilation=dil))
    x = F.relu(F.conv_transpose3d(x, Q["Mask_Head.upconv.weight"], Q["Mask_Head.upconv.bias"], stride=2))
    return torch.sigmoid(F.conv3d(x, Q["Mask_Outs.classify.weight"], Q["Mask_Outs.classify.bias"]))


@pytest.mark.parametrize("dil", [1, 2])
def test_mask_head_trunk_on_the_narrow_kernel(dil, monkeypatch):
    import m3d
    from m3d import ops
    from m3d.mask_head import MaskHeadM3D
    monkeypatch.delenv("M3D_MASK_CONV_F16", raising=False)
    monkeypatch.delenv("M3D_CONV_F16", raising=False)
    P = MH._mask_params(CIN, DIM, NC, CONVS, seed=70 + dil)
    G = {k: v.cuda() for k, v in P.items()}
    kw = dict(roi_res=7, dilation=dil, resolution=14)
    plain = MaskHeadM3D(G, O.Cfg(mlp_dim=64), **kw)
    off = MaskHeadM3D(G, O.Cfg(mlp_dim=64), conv_f16=False, **kw)
    on = MaskHeadM3D(G, O.Cfg(mlp_dim=64), conv_f16=True, conv_f16_min_units=0, **kw)
    assert not plain.conv_f16 and not off.conv_f16 and on.conv_f16 and all(z is None for z in off.zn) and all(z is not None for z in on.zn)
    feat = torch.randn((1, CIN, 16, 16, 16), generator=torch.Generator().manual_seed(3)).cuda()
    rois = torch.tensor(ROIS, dtype=torch.float32).cuda()
    pooled = m3d.roi_align3d_forward(feat, rois, 7, 7, 7, 1.0 / 8, 0)
    ref = _torch_chain(P, pooled.cpu(), dil, torch.float64, "cpu")
    e_torch = float((_torch_chain(P, pooled, dil, torch.float32, "cuda").double().cpu() - ref).abs().max() / ref.abs().max())
    base = plain.mask_net(feat, rois)
    assert torch.equal(off.mask_net(feat, rois), base)                     # conv_f16=False: today's bits
    new, old = ("m3d_conv3d_zn_forward", "m3d_conv3d_forward") if dil == 1 else ("m3d_conv3d_zn_dilated_forward", "m3d_conv3d_forward_dilated")
    for carried in (False, True):
        fmax = ops.ZwConv3d.bound_of(feat) * 2 if carried else None        # what a producing conv may leave: here a loose bound
        rec = BH.Record(ops.lib())
        with monkeypatch.context() as mp:
            mp.setattr(ops, "lib", lambda: rec)
            x = on.trunk(feat, rois, feat_max=fmax)
        assert rec.calls.count(new) == CONVS and old not in rec.calls      # both convs on the narrow kernel
        assert rec.calls.count("m3d_conv3d_zw_bound_of") == (0 if carried else 1)      # one sweep of the RoIAlign output, none with a carried bound
        prob = on.outputs(on.up(x))
        e = float((prob.double().cpu() - ref).abs().max() / ref.abs().max())
        print("dilation %d carried %d: e %.3g e_torch %.3g" % (dil, carried, e, e_torch))
        assert e <= 4 * e_torch, (e, e_torch)
        assert tuple(prob.shape) == (R, NC, 14, 14, 14) and not torch.equal(prob, base)
    assert torch.equal(on.mask_net(feat, rois), on.outputs(on.up(on.trunk(feat, rois))))
    # the default threshold: 5 RoIs are 10 units, below it - today's kernels, today's bits
    few = MaskHeadM3D(G, O.Cfg(mlp_dim=64), conv_f16=True, **kw)
    assert few.conv_f16_min_units > 10 and torch.equal(few.mask_net(feat, rois), base)
    # the environment: M3D_MASK_CONV_F16 switches it on, M3D_CONV_F16=0 keeps it off
    monkeypatch.setenv("M3D_MASK_CONV_F16", "1")
    assert MaskHeadM3D(G, O.Cfg(mlp_dim=64), **kw).conv_f16
    monkeypatch.setenv("M3D_CONV_F16", "0")
    assert not MaskHeadM3D(G, O.Cfg(mlp_dim=64), **kw).conv_f16
