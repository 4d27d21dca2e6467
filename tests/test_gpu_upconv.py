"""GPU: the mask-head up-conv (csrc/upconv3d.hip: ConvTranspose3d(2, 2) + bias + ReLU, its dgrad, wgrad and bias gradient) against the
fp64 restatement of tests/upconv_reference.py - exactly on integer data, element by element within the derived bound on random data -
and through every layer above it: ops, m3d.upconv3d_2x under autograd, compat.conv_transpose3d, MaskHead and MaskHeadM3D under
compat.set_upconv("m3d").  The bound: |out - out64| <= gamma_n A_e + 2^-24 |out64| with n = reduction length + partials added (the
forward: + 1 for the bias), reduction lengths Cin / 8 Cout / R D H W, and 8 R D H W for the bias gradient (the number of terms it adds).

Largest err / bound measured on an MI355X over the shapes of the table (random data; informative, the pass criterion is the derived
bound): forward 0.48, dgrad 0.083, wgrad 0.26 (the one-voxel case; 0.018 and below elsewhere), bias gradient 0.025.  Each test prints its own."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import upconv_reference as UR

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def default_mode():
    import m3d.compat as compat
    compat.set_upconv("torch")
    yield
    compat.set_upconv("torch")
    compat.uninstall_conv_transpose3d()


def dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


@functools.lru_cache(maxsize=None)
def results(shape, kind, relu):
    """one device run of the three entry points on case(shape, kind) and the fp64 restatement of each (the backward's mask: the device's
    y); computed once, shared, never modified"""
    from m3d import ops
    x, w, b, gy = UR.case(shape, kind)
    dx, dw, db, dgy = dev(x, w, b, gy)
    y = ops.upconv3d_2x_forward(dx, dw, db, relu=relu)
    mask = y if relu else None
    gx = ops.upconv3d_2x_dgrad(dgy, dw, y=mask)
    gw, gb = ops.upconv3d_2x_wgrad(dgy, dx, y=mask)
    got = {"forward": y.cpu().numpy(), "dgrad": gx.cpu().numpy(), "wgrad": gw.cpu().numpy(), "gb": gb.cpu().numpy()}
    m = got["forward"] if relu else None
    gw64, Aw, gb64, Ab = UR.wgrad(gy, x, m)
    want = {"forward": UR.forward(x, w, b, relu), "dgrad": UR.dgrad(gy, w, m), "wgrad": (gw64, Aw), "gb": (gb64, Ab)}
    for v in list(got.values()) + [t for pair in want.values() for t in pair]:
        v.setflags(write=False)
    return got, want


def terms(shape):
    """n of the bound per output: reduction length + partials (+ 1 for the forward's bias)"""
    from m3d import ops
    L = UR.lengths(*shape)
    sd, sw = ops.upconv3d_2x_slices("dgrad", *shape), ops.upconv3d_2x_slices("wgrad", *shape)
    assert 1 <= sd <= 64 and 1 <= sw <= 64
    return {"forward": L["forward"] + 1, "dgrad": L["dgrad"] + sd, "wgrad": L["wgrad"] + sw, "gb": L["gb"] + sw}


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("shape", UR.SHAPES)
def test_exact_on_integer_data(shape, relu):
    """|v| <= 4 integers: every sum is exact in fp32, so all four outputs equal the fp64 restatement exactly"""
    got, want = results(shape, "int", relu)
    for k in ("forward", "dgrad", "wgrad", "gb"):
        assert got[k].shape == want[k][0].shape, k
        bad = np.flatnonzero(got[k].astype(np.float64).ravel() != want[k][0].ravel())
        assert bad.size == 0, (k, shape, relu, bad[:8], got[k].ravel()[bad[:8]], want[k][0].ravel()[bad[:8]])
    if relu:
        assert (got["forward"] >= 0).all()


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("shape", UR.SHAPES)
def test_random_data_within_the_bound(shape, relu):
    got, want = results(shape, "randn", relu)
    n = terms(shape)
    ratios = {k: UR.worst_ratio(got[k], want[k][0], want[k][1], n[k]) for k in ("forward", "dgrad", "wgrad", "gb")}
    print("upconv %s relu=%d n=%s: largest err / bound %s" % (shape, relu, n, {k: round(v, 4) for k, v in ratios.items()}))
    assert max(ratios.values()) <= 1.0, ratios


def test_masked_elements_contribute_exactly_nothing():
    """where y <= 0 the value of gy does not matter at all: huge values there change no bit of any gradient"""
    from m3d import ops
    shape = UR.SHAPES[3]
    x, w, b, gy = dev(*UR.case(shape, "randn"))
    y = ops.upconv3d_2x_forward(x, w, b, relu=True)
    off = y <= 0
    assert bool(off.any()) and bool((~off).any())
    clean, loud = torch.where(off, torch.zeros_like(gy), gy), torch.where(off, torch.full_like(gy, 3e38), gy)
    for a, c in zip((ops.upconv3d_2x_dgrad(loud, w, y=y),) + ops.upconv3d_2x_wgrad(loud, x, y=y),
                    (ops.upconv3d_2x_dgrad(clean, w),) + ops.upconv3d_2x_wgrad(clean, x)):
        assert torch.equal(a, c)


@pytest.mark.parametrize("shape", UR.SHAPES[3:])
def test_reruns_are_bit_identical(shape):
    from m3d import ops
    x, w, b, gy = dev(*UR.case(shape, "randn", seed=1))
    y = ops.upconv3d_2x_forward(x, w, b, relu=True)
    assert torch.equal(y, ops.upconv3d_2x_forward(x, w, b, relu=True))
    assert torch.equal(ops.upconv3d_2x_dgrad(gy, w, y=y), ops.upconv3d_2x_dgrad(gy, w, y=y))
    first, again = ops.upconv3d_2x_wgrad(gy, x, y=y), ops.upconv3d_2x_wgrad(gy, x, y=y)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])


def guarded(n, lead):
    """(whole, view of n floats starting `lead` floats in): NaN everywhere"""
    whole = torch.full((n + lead + 64,), float("nan"), dtype=torch.float32, device="cuda")
    assert whole.data_ptr() % 64 == 0
    return whole, whole[lead:lead + n]


@pytest.mark.parametrize("lead", (64, 68))          # 68 floats: a base that is 16-byte aligned but not 32- or 64-byte aligned
@pytest.mark.parametrize("shape", UR.SHAPES[:4])
def test_outputs_written_whole_and_only_there(shape, lead):
    from m3d._lib import lib, check
    L = lib()
    R, Cin, Cout, D, H, W = shape
    x, w, b, gy = dev(*UR.case(shape, "randn", seed=2))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def p(t):
        return C.c_void_p(t.data_ptr() if t is not None else 0)
    ny, nx, nw = gy.numel(), x.numel(), w.numel()
    wy, y = guarded(ny, lead)
    wgx, gx = guarded(nx, lead)
    wgw, gw = guarded(nw, lead)
    wgb, gb = guarded(Cout, lead + 1)                 # the bias gradient needs 4-byte alignment only
    nd, nwb = L.m3d_upconv3d_2x_dgrad_workspace_bytes(*shape), L.m3d_upconv3d_2x_wgrad_workspace_bytes(*shape)
    ws = torch.empty((max(nd, nwb, 16),), dtype=torch.uint8, device="cuda")
    check(L.m3d_upconv3d_2x_forward(p(x), p(w), p(b), p(y), *shape, 1, st), "forward")
    check(L.m3d_upconv3d_2x_dgrad(p(gy), p(y), p(w), p(gx), *shape, p(ws), C.c_size_t(nd), st), "dgrad")
    check(L.m3d_upconv3d_2x_wgrad(p(gy), p(y), p(x), p(gw), p(gb), *shape, p(ws), C.c_size_t(nwb), st), "wgrad")
    torch.cuda.synchronize()
    for whole, view, skip in ((wy, y, lead), (wgx, gx, lead), (wgw, gw, lead), (wgb, gb, lead + 1)):
        assert not bool(torch.isnan(view).any())
        assert bool(torch.isnan(whole[:skip]).all()) and bool(torch.isnan(whole[skip + view.numel():]).all())
    # and they are the values of the ordinary call
    from m3d import ops
    y2 = ops.upconv3d_2x_forward(x, w, b, relu=True)
    assert torch.equal(y.view_as(y2), y2) and torch.equal(gx.view_as(x), ops.upconv3d_2x_dgrad(gy, w, y=y2))
    gw2, gb2 = ops.upconv3d_2x_wgrad(gy, x, y=y2)
    assert torch.equal(gw.view_as(gw2), gw2) and torch.equal(gb, gb2)


def test_empty_batch():
    from m3d import ops
    x, w, b = torch.zeros((0, 5, 2, 3, 4), device="cuda"), torch.randn((5, 3, 2, 2, 2), device="cuda"), torch.randn((3,), device="cuda")
    y = ops.upconv3d_2x_forward(x, w, b, relu=True)
    assert tuple(y.shape) == (0, 3, 4, 6, 8)
    assert tuple(ops.upconv3d_2x_dgrad(y, w, y=y).shape) == (0, 5, 2, 3, 4)
    gw = torch.full((5, 3, 2, 2, 2), float("nan"), device="cuda")
    out, gb = ops.upconv3d_2x_wgrad(y, x, y=y, out=gw)
    assert out is gw and not bool(gw.any()) and not bool(gb.any()) and tuple(gb.shape) == (3,)
    assert ops.upconv3d_2x_wgrad(y, x, bias=False)[1] is None


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("shape", UR.SHAPES[1:4])
def test_autograd_function(shape, relu, monkeypatch):
    """m3d.upconv3d_2x: the gradients of x, weight and bias against a torch fp64 CPU run (with ReLU: on the device's mask, as the kernels
    take it), within the bounds of the raw entry points; only the requested gradients are computed"""
    import m3d
    from m3d import ops
    x, w, b, gy = UR.case(shape, "randn", seed=3)
    dx, dw, db = (t.requires_grad_(True) for t in dev(x, w, b))
    dgy, = dev(gy)
    y = m3d.upconv3d_2x(dx, dw, db, relu=relu)
    y.backward(dgy)
    tx, tw, tb = (torch.from_numpy(t).double().requires_grad_(True) for t in (x, w, b))
    ty = F.conv_transpose3d(tx, tw, tb, stride=2)
    mask = y.detach().cpu().numpy()
    if relu:
        ty = ty * torch.from_numpy(mask > 0)
    ty.backward(torch.from_numpy(gy).double())
    n = terms(shape)
    m = mask if relu else None
    A = {"forward": UR.forward(x, w, b, relu)[1], "dgrad": UR.dgrad(gy, w, m)[1]}
    _, A["wgrad"], _, A["gb"] = UR.wgrad(gy, x, m)
    ty64 = np.maximum(ty.detach().numpy(), 0.0) if relu else ty.detach().numpy()
    for k, got, want in (("forward", y.detach(), ty64), ("dgrad", dx.grad, tx.grad.numpy()), ("wgrad", dw.grad, tw.grad.numpy()),
                         ("gb", db.grad, tb.grad.numpy())):
        r = UR.worst_ratio(got.cpu().numpy(), want, A[k], n[k])
        print("autograd %s relu=%d %s: err / bound %.4f" % (shape, relu, k, r))
        assert r <= 1.0, (k, r)
    gx0, gb0 = dx.grad.clone(), db.grad.clone()
    calls = []
    real_d, real_w = ops.upconv3d_2x_dgrad, ops.upconv3d_2x_wgrad
    monkeypatch.setattr(ops, "upconv3d_2x_dgrad", lambda *a, **k: calls.append("dgrad") or real_d(*a, **k))
    monkeypatch.setattr(ops, "upconv3d_2x_wgrad", lambda *a, **k: calls.append(("wgrad", k.get("bias"))) or real_w(*a, **k))
    fx, fw, fb = dx.detach(), dw.detach(), db.detach()
    m3d.upconv3d_2x(fx, dw, db, relu=relu).backward(dgy)                       # x needs no gradient
    assert calls == [("wgrad", True)]
    del calls[:]
    gxo = torch.autograd.grad(m3d.upconv3d_2x(dx, fw, fb, relu=relu), dx, dgy)[0]   # the parameters need none
    assert calls == ["dgrad"] and torch.equal(gxo, gx0)
    del calls[:]
    wg = fw.clone().requires_grad_(True)
    m3d.upconv3d_2x(fx, wg, None, relu=relu).backward(dgy)                      # no bias at all
    assert calls == [("wgrad", False)] and wg.grad is not None
    del calls[:]
    bg = fb.clone().requires_grad_(True)
    m3d.upconv3d_2x(fx, fw, bg, relu=relu).backward(dgy)                        # the bias gradient alone comes out of the wgrad launch
    assert calls == [("wgrad", True)] and torch.equal(bg.grad, gb0)
    with pytest.raises(m3d.M3DError):
        m3d.upconv3d_2x(fx.cpu(), fw.cpu(), None)


def test_compat_conv_transpose3d():
    import m3d
    import m3d.compat as compat
    orig = F.conv_transpose3d
    g = torch.Generator().manual_seed(4)
    x = torch.randn((2, 4, 3, 4, 5), generator=g).cuda()
    w, b = torch.randn((4, 6, 2, 2, 2), generator=g).cuda(), torch.randn((6,), generator=g).cuda()
    assert torch.equal(compat.conv_transpose3d(x, w, b, stride=2), m3d.upconv3d_2x(x, w, b))
    assert torch.equal(compat.conv_transpose3d(x, w, None, (2, 2, 2), (0, 0, 0), 0, 1, 1), m3d.upconv3d_2x(x, w))
    w3, wg = torch.randn((4, 6, 3, 3, 3), generator=g).cuda(), torch.randn((4, 3, 2, 2, 2), generator=g).cuda()
    xt = x.transpose(3, 4)
    assert not xt.is_contiguous()
    for args, kw in (((x, w, b), dict(stride=1)), ((x, w3, b), dict(stride=2)), ((x, w, b), dict(stride=2, output_padding=1)),
                     ((x, wg, b), dict(stride=2, groups=2)), ((x.half(), w.half(), b.half()), dict(stride=2)), ((xt, w, b), dict(stride=2))):
        want = orig(*args, **kw)
        got = compat.conv_transpose3d(*args, **kw)
        assert got.dtype == want.dtype and torch.equal(got, want), kw
    compat.install(conv3d=False, linear=False)                   # install() does not patch it
    assert F.conv_transpose3d is orig
    compat.install_conv_transpose3d()
    assert F.conv_transpose3d is compat.conv_transpose3d
    mod = torch.nn.ConvTranspose3d(4, 6, 2, 2).cuda()
    assert torch.equal(mod(x), m3d.upconv3d_2x(x, mod.weight, mod.bias))
    compat.install_conv_transpose3d()                            # twice: the original is kept
    compat.uninstall_conv_transpose3d()
    assert F.conv_transpose3d is orig
    compat.uninstall_conv_transpose3d()
    assert F.conv_transpose3d is orig


def test_mask_head_under_set_upconv(monkeypatch):
    """the set-up of test_gpu_mask_train.test_mask_head_gradients_and_training with the up-conv on the library's kernels"""
    import m3d
    import m3d.compat as compat
    from test_mask_train_host import GOLD, case_inputs
    from test_gpu_mask_train import head_fp64, manual_box_targets
    g = dict(np.load(GOLD))
    d = case_inputs(g, "spot_small")
    T = manual_box_targets(d["gt"][:6], batch=16, fg_fraction=0.5)
    cfg = m3d.MaskTrainCfg.soma(in_size=d["tile"], dim_reduced=16, num_convs=2)
    MT = m3d.mask_targets(T, cfg, spots=[d["spots"]], gt_crowd=[d["crowd"]])
    torch.manual_seed(5)
    head = m3d.MaskHead(16, cfg, stride=4).cuda()
    with torch.no_grad():
        head.classify.weight.normal_(0, 0.05)
    feat = torch.randn((1, 16, 8, 16, 12), generator=torch.Generator().manual_seed(6)).cuda()
    rois7 = MT.rois7
    names = [k for k, _ in head.named_parameters()]
    keys = list(head.state_dict().keys())
    # the default mode: exactly the composition with torch's own conv_transpose3d
    assert compat.get_upconv() == "torch"
    x = compat.RoIAlignFunction_3d(7, 7, 7, 0.25, int(cfg.sampling_ratio))(feat, rois7)
    for m in head.conv_fcn:
        x = compat.conv3d(x, m.weight, m.bias, 1, 1) if isinstance(m, torch.nn.Conv3d) else torch.relu(x)
    x = torch.relu(F.conv_transpose3d(x, head.upconv.weight, head.upconv.bias, stride=2))
    assert torch.equal(head(feat, rois7), compat.conv3d(x, head.classify.weight, head.classify.bias, 1, 0))
    # "m3d": torch's conv_transpose3d is not reachable
    assert compat.set_upconv("m3d") == "torch"

    def refuse(*a, **k):
        raise AssertionError("F.conv_transpose3d called under set_upconv('m3d')")
    monkeypatch.setattr(F, "conv_transpose3d", refuse)
    logits = head(feat, rois7)
    assert tuple(logits.shape) == (8, 1, 14, 14, 14)
    loss = m3d.mask_losses(logits, MT)
    loss.backward()
    pooled = m3d.roi_align3d_forward(feat, rois7, 7, 7, 7, 0.25, 2)
    monkeypatch.undo()
    l64, g64, y64, terms_ = head_fp64(dict(head.named_parameters()), pooled, MT.masks, cfg.weight_loss_mask)
    monkeypatch.setattr(F, "conv_transpose3d", refuse)
    assert abs(float(loss) - l64) <= 1e-4 * abs(l64)
    for k, p in head.named_parameters():
        got, want = p.grad.double().cpu(), g64[k]
        err, allowed = (got - want).abs(), 1e-4 * want.abs() + 16 * 2.0 ** -24 * terms_[k]
        print(k, "max |grad|", float(want.abs().max()), "max err", float(err.max()), "largest err / allowed", float((err / allowed).max()))
        assert float(want.abs().max()) > 0 and bool((err <= allowed).all()), k
    assert [k for k, _ in head.named_parameters()] == names and list(head.state_dict().keys()) == keys
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


def test_mask_head_m3d_up():
    """MaskHeadM3D.up in both forms on the same x against fp64 within the forward bound; mask_net under "m3d" within the tolerance of
    tests/test_gpu_mask_head.py"""
    import m3d
    import m3d.compat as compat
    import oracle as O
    from m3d.mask_head import MaskHeadM3D
    from test_gpu_mask_head import _mask_params, _ref_from_pooled
    cin, dim, nc, res, convs, dil = 48, 40, 2, 7, 2, 2
    P = _mask_params(cin, dim, nc, convs, seed=9)
    head = MaskHeadM3D({k: v.cuda() for k, v in P.items()}, O.Cfg(mlp_dim=64), roi_res=res, dilation=dil, resolution=2 * res)
    feat = torch.randn((1, cin, 8, 9, 10), generator=torch.Generator().manual_seed(3)).cuda()
    rois = torch.tensor([[0, 3, 2, 1, 60, 50, 40], [0, 0, 0, 0, 79, 71, 63], [0, 10, 10, 10, 14, 13, 12],
                         [0, 30.5, 20.25, 8, 70, 69, 50], [0, 5, 40, 30, 25, 60, 62]], dtype=torch.float32).cuda()
    x = head.trunk(feat, rois)
    assert tuple(x.shape) == (5, dim, res, res, res)
    y64, A = UR.forward(x.cpu().numpy(), P["Mask_Head.upconv.weight"].numpy(), P["Mask_Head.upconv.bias"].numpy(), relu=True)
    outs = {}
    for mode in ("torch", "m3d"):
        compat.set_upconv(mode)
        outs[mode] = head.up(x)
        assert tuple(outs[mode].shape) == (5, dim, 2 * res, 2 * res, 2 * res)
        r = UR.worst_ratio(outs[mode].cpu().numpy(), y64, A, dim + 1)
        print("MaskHeadM3D.up %s: err / bound %.4f" % (mode, r))
        assert r <= 1.0, mode
    assert torch.equal(head.head(feat, rois), outs["m3d"])
    pooled = m3d.roi_align3d_forward(feat, rois, res, res, res, 1.0 / 8, 0)
    up_ref, prob_ref = _ref_from_pooled(P, pooled.cpu(), convs, dil)
    prob = head.mask_net(feat, {"mask_rois": rois.cpu().numpy()})
    assert np.allclose(outs["m3d"].cpu().numpy(), up_ref.numpy(), rtol=1e-4, atol=1e-4 * float(up_ref.abs().max()))
    assert np.allclose(prob.cpu().numpy(), prob_ref.numpy(), rtol=1e-4, atol=1e-5)
