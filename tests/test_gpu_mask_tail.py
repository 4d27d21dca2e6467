"""GPU: the mask head with its tail fused (mask_head.MaskHeadM3D(tail_f16=True): trunk -> ops.UpConvF16.tail, one launch for up-conv + ReLU +
classifier + sigmoid) against the same head with the tail off, and the training forward under compat.set_upconv_f16.

Detection: the synthetic parameters of tests/test_gpu_mask_head.py at 32 channels, 5 RoIs on a 16^3 feature map.  Every probability lies
within E_l / 4 + 2^-24 of the fp64 sigmoid of the fp64 logits computed from the off-head's trunk output (the sigmoid is 1/4-Lipschitz; E_l:
tests/upconv_f16_cases.py), bits are identical across two runs, the switch off is bit for bit `up` + `outputs`, and with the trunk on the
narrow f16x2 kernel the tail sweeps nothing: the last conv hands its bound on.
Training: m3d.train.upconv3d_2x under set_upconv_f16(True) is within E_u, its gradients are what m3d_upconv3d_2x_dgrad / _wgrad give on
that forward's y bit for bit; off, forward and backward are today's bits."""
import pytest
import torch

import oracle as O
import test_gpu_mask_head as MH
import upconv_f16_cases as T

pytestmark = pytest.mark.gpu

CIN, DIM, NC, CONVS = 32, 32, 2, 2
ROIS = [[0, 3, 2, 1, 60, 50, 40], [0, 0, 0, 0, 79, 71, 63], [0, 10, 10, 10, 14, 13, 12], [0, 30.5, 20.25, 8, 70, 69, 50],
        [0, 5, 40, 30, 25, 60, 62]]


def _setup(monkeypatch, dil):
    for k in ("M3D_MASK_TAIL_F16", "M3D_MASK_CONV_F16", "M3D_CONV_F16"):
        monkeypatch.delenv(k, raising=False)
    P = MH._mask_params(CIN, DIM, NC, CONVS, seed=90 + dil)
    G = {k: v.cuda() for k, v in P.items()}
    feat = torch.randn((1, CIN, 16, 16, 16), generator=torch.Generator().manual_seed(3)).cuda()
    rois = torch.tensor(ROIS, dtype=torch.float32).cuda()
    return P, G, feat, rois, dict(roi_res=7, dilation=dil, resolution=14)


@pytest.mark.parametrize("dil", [1, 2])
def test_mask_net_with_the_fused_tail(dil, monkeypatch):
    from m3d.mask_head import MaskHeadM3D
    P, G, feat, rois, kw = _setup(monkeypatch, dil)
    plain = MaskHeadM3D(G, O.Cfg(mlp_dim=64), **kw)
    off = MaskHeadM3D(G, O.Cfg(mlp_dim=64), tail_f16=False, **kw)
    on = MaskHeadM3D(G, O.Cfg(mlp_dim=64), tail_f16=True, tail_f16_min_rois=0, **kw)
    assert not plain.tail_f16 and not off.tail_f16 and on.tail_f16 and off.up_f16 is None
    # off: bit for bit what up + outputs give today
    base = plain.outputs(plain.up(plain.trunk(feat, rois)))
    assert torch.equal(plain.mask_net(feat, rois), base) and torch.equal(off.mask_net(feat, rois), base)
    # on: within E_l / 4 + 2^-24 of the fp64 sigmoid of the fp64 logits from the off-head's trunk output
    x = off.trunk(feat, rois).cpu()
    wu, bu = P["Mask_Head.upconv.weight"], P["Mask_Head.upconv.bias"]
    wc, bc = P["Mask_Outs.classify.weight"].reshape(NC, DIM), P["Mask_Outs.classify.bias"]
    l64, El = T.contract_fused(x, wu, bu, wc, bc)
    got = on.mask_net(feat, rois)
    assert tuple(got.shape) == (len(ROIS), NC, 14, 14, 14)
    r = T.worst(got.cpu(), torch.sigmoid(l64), El / 4 + 2.0 ** -24)
    print("dilation %d: worst |p - p64| / (E_l / 4 + 2^-24) = %.3f" % (dil, r))
    assert r <= 1.0, r
    assert torch.equal(on.mask_net(feat, rois), got) and not torch.equal(got, base)
    assert torch.equal(on.mask_net(feat, {"mask_rois": rois.cpu().numpy()}), got)
    # up and outputs stay what they are for callers that use them directly
    assert torch.equal(on.outputs(on.up(on.trunk(feat, rois))), base)
    # the default threshold: 5 RoIs are below it - today's launches, today's bits
    few = MaskHeadM3D(G, O.Cfg(mlp_dim=64), tail_f16=True, **kw)
    assert few.tail_f16_min_rois > len(ROIS) and torch.equal(few.mask_net(feat, rois), base)
    # the environment: M3D_MASK_TAIL_F16 switches it on, M3D_CONV_F16=0 keeps it off
    monkeypatch.setenv("M3D_MASK_TAIL_F16", "1")
    assert MaskHeadM3D(G, O.Cfg(mlp_dim=64), **kw).tail_f16
    monkeypatch.setenv("M3D_CONV_F16", "0")
    assert not MaskHeadM3D(G, O.Cfg(mlp_dim=64), **kw).tail_f16


@pytest.mark.parametrize("dil", [1, 2])
def test_the_tail_takes_the_trunks_bound_and_sweeps_nothing(dil, monkeypatch):
    from m3d import ops
    from m3d.mask_head import MaskHeadM3D
    P, G, feat, rois, kw = _setup(monkeypatch, dil)
    on = MaskHeadM3D(G, O.Cfg(mlp_dim=64), conv_f16=True, conv_f16_min_units=0, tail_f16=True, tail_f16_min_rois=0, **kw)
    swept_tail = MaskHeadM3D(G, O.Cfg(mlp_dim=64), tail_f16=True, tail_f16_min_rois=0, **kw)            # fp32 trunk: the tail sweeps
    calls = []
    real = ops._F16x2Conv3d.bound_of

    def counting(x):
        calls.append(tuple(x.shape))
        return real(x)
    monkeypatch.setattr(ops._F16x2Conv3d, "bound_of", staticmethod(counting))
    x, bound = on.trunk(feat, rois, want_bound=True)
    assert len(calls) == 1 and bound is not None                            # the trunk's one sweep of the RoIAlign output
    assert float(bound.max()) == float(x.abs().max())                       # the last conv's bound is max |x| bit for bit
    del calls[:]
    got = on.mask_net(feat, rois)
    assert len(calls) == 1, calls                                           # the trunk's again: none for the tail
    # the handed-on bound is the sweep's, so the tail's bits are those of a swept call on the same x
    assert torch.equal(got, on.up_f16.tail(x, real(x), on.up_bias_raw, on.classify_weight, on.classify_bias))
    del calls[:]
    swept_tail.mask_net(feat, rois)
    assert calls == [(len(ROIS), DIM, 7, 7, 7)]                             # fp32 trunk: exactly the tail's own sweep


@pytest.mark.parametrize("case", ("ragged", "roi_grid"))
def test_training_forward_on_the_f16_kernel(case):
    from m3d import compat, ops
    from m3d.train import upconv3d_2x
    x, w, bu, _, _, y64, Eu, _, _, _ = T.reference(case, "benign")
    xg = x.cuda().requires_grad_(True)
    W = torch.nn.Parameter(w.cuda())
    b = torch.nn.Parameter(bu.cuda())
    gy = torch.randn(y64.shape, generator=torch.Generator().manual_seed(11)).cuda()

    def step():
        for t in (xg, W, b):
            t.grad = None
        y = upconv3d_2x(xg, W, b, relu=True)
        y.backward(gy)
        return y.detach(), xg.grad.clone(), W.grad.clone(), b.grad.clone()
    prev_up, prev_f16 = compat.set_upconv("m3d"), compat.set_upconv_f16(False)
    try:
        assert prev_f16 is False                                            # off unless asked for
        base = step()
        y32 = ops.upconv3d_2x_forward(xg.detach(), W.detach(), b.detach(), relu=True)
        assert torch.equal(base[0], y32)
        compat.set_upconv_f16(True)
        y, gx, gw, gb = step()
        r = T.worst(y.cpu(), y64, Eu)
        assert r <= 1.0 and not torch.equal(y, y32), r
        assert torch.equal(y, ops.UpConvF16(W.detach())(xg.detach(), None, bias=b.detach(), relu=True))
        assert torch.equal(gx, ops.upconv3d_2x_dgrad(gy, W.detach(), y=y))
        rw, rb = ops.upconv3d_2x_wgrad(gy, xg.detach(), y=y)
        assert torch.equal(gw, rw) and torch.equal(gb, rb)
        # an updated parameter is re-packed
        with torch.no_grad():
            W.mul_(0.5)
        y2 = step()[0]
        assert torch.equal(y2, ops.UpConvF16(W.detach())(xg.detach(), None, bias=b.detach(), relu=True))
        with torch.no_grad():
            W.mul_(2.0)
        # no effect without set_upconv("m3d")
        compat.set_upconv("torch")
        assert torch.equal(upconv3d_2x(xg, W, b, relu=True).detach(), y32)
        # off again: today's bits, forward and backward
        compat.set_upconv("m3d")
        assert compat.set_upconv_f16(False) is True
        assert all(torch.equal(p, q) for p, q in zip(step(), base))
    finally:
        compat.set_upconv(prev_up)
        compat.set_upconv_f16(prev_f16)
