"""GPU: the dilation-2 narrow-map f16x2 conv weight gradient (m3d_conv3d_wgrad_narrow_dilated_f16x2) against fp64, element by element, on
the cases of tests/wgrad_dilated_f16_cases.py under the contract of tests/wgrad_f16x2_contract.py: integer data bit-exact (index, halo,
shift and zero-column errors), every element within the bound, exact zeros and whole zero taps, handed-over bounds, sentinels around
everything it may write, determinism, dilation 1 through the new entry, the routing through m3d.compat.set_conv_wgrad_dilated_f16, and
m3d.train.MaskHead's gradients at dilation 2 with the switch on.

The worst |error| / bound per case is printed with pytest -s."""
import ctypes as C

import pytest
import torch

import wgrad_f16x2_contract as K
import wgrad_dilated_f16_cases as N

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                    # a quiet NaN with a payload
GUARD = 1024                             # floats before and after each buffer
CASE_NAMES = sorted(N.cases(2))          # the names do not depend on tile_z


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as o
    return o


def case_of(name):
    from m3d import ops as o
    return N.cases(o.conv3d_wgrad_narrow_f16x2_plan(1, 32, 32, 1, 1, 1, dilation=2)["tile_z"])[name]


def n_acc(case):
    from m3d import ops as o
    p = o.conv3d_wgrad_narrow_f16x2_plan(*case, dilation=2)
    return p["chain"] + p["folds"]


def contract(gy, x, n):
    """K.contract with the dilation-2 op: (fp64 reference, E, C)"""
    A, B = float(gy.abs().max()), float(x.abs().max())
    y = N.wgrad_op_d2(gy, x)
    Cm, Sa, Sb, cnt = K.terms(N.wgrad_op_d2, gy, x)
    return y, K.bound(n, Cm, Sa, Sb, cnt, A, B, y), Cm


_ref = {}


def reference(name):
    """(gy, x, fp64 dW, E, C) of a case on random data, computed once and shared (never modified)"""
    if name not in _ref:
        case = case_of(name)
        gy, x = K.make_inputs("benign", case, 11, relu_x=True)
        _ref[name] = (gy, x) + contract(gy, x, n_acc(case))
    return _ref[name]


def d2(ops, x, gy, *bounds):
    return ops.conv3d_wgrad_narrow_f16x2(x, gy, *bounds, dilation=2)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_integer_data_is_bit_exact(ops, name):
    gy, x = K.integer_inputs(case_of(name), 3)
    want = N.wgrad_op_d2(gy, x)
    got = d2(ops, x.cuda(), gy.cuda()).cpu()
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.double(), want)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_every_element_within_the_bound_and_exact_zeros(ops, name):
    gy, x, y, E, Cm = reference(name)
    got = d2(ops, x.cuda(), gy.cuda()).cpu().double()
    assert bool(torch.isfinite(got).all())
    err = (got - y).abs()
    ratio = float((err / E.clamp_min(1e-300)).max())
    print("%s: worst |error| / bound %.4f, worst |error| / max |dW| %.3g" % (name, ratio, float(err.max() / y.abs().max())))
    assert bool((err <= E).all())
    assert bool((got[Cm == 0] == 0).all())
    zero = N.zero_taps(case_of(name))
    for axis, t in zero:
        assert bool((got.select(axis, t) == 0).all()), (name, axis, t)                       # a whole tap reads the padding only
    if name in ("one_tile", "d1_co64", "w2", "h2"):
        assert len(zero) == 2, name


@pytest.mark.parametrize("family", ["heavy", "outlier8", "quiet", "at_bound_pow2", "at_bound_below", "zero"])
def test_input_families_within_the_bound(ops, family):
    case = case_of(N.FAMILY_CASE)
    for relu_x in (False, True):
        gy, x = K.make_inputs(family, case, 17, relu_x)
        y, E, Cm = contract(gy, x, n_acc(case))
        got = d2(ops, x.cuda(), gy.cuda()).cpu().double()
        err = (got - y).abs()
        print("%s relu_x=%d: worst |error| / bound %.4f" % (family, relu_x, float((err / E.clamp_min(1e-300)).max())))
        assert bool(torch.isfinite(got).all()) and bool((err <= E).all())
        assert bool((got[Cm == 0] == 0).all())
        if family == "zero":
            assert bool((got == 0).all())                                                    # x = 0
            assert bool((d2(ops, gy.cuda().new_ones(x.shape), torch.zeros_like(gy).cuda()) == 0).all())      # gy = 0


def test_a_loose_bound_changes_nothing_beyond_the_contract(ops):
    """bounds handed over by a producer (2^3 above the maximum, in an arbitrary slot) instead of a sweep: the contract with those bounds"""
    name = "d1_co64"
    gy, x, y, _, _ = reference(name)
    A, B = float(gy.abs().max()) * 8, float(x.abs().max()) * 8
    Cm, Sa, Sb, n = K.terms(N.wgrad_op_d2, gy, x)
    E = K.bound(n_acc(case_of(name)), Cm, Sa, Sb, n, A, B, y)
    slots = lambda v, at: torch.tensor([0.0] * at + [v] + [0.0] * (31 - at), device="cuda")     # the largest slot counts, wherever it is
    got = d2(ops, x.cuda(), gy.cuda(), slots(B, 7), slots(A, 29)).cpu().double()
    assert bool(torch.isfinite(got).all()) and bool(((got - y).abs() <= E).all())


@pytest.mark.parametrize("name", N.SENTINEL_CASES)
def test_sentinels_around_output_and_workspace(ops, name):
    from m3d._lib import lib, check
    case = case_of(name)
    B, cin, cout, D, H, W = case
    gy, x, y, E, _ = reference(name)
    xg, gg = x.cuda(), gy.cuda()
    n = cout * cin * 27
    wsb = int(lib().m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(*case, 2))
    assert wsb % 4 == 0 and wsb == ops.conv3d_wgrad_narrow_f16x2_plan(*case, dilation=2)["slots"] * n * 4
    bufs = [torch.full((GUARD + m + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for m in (n, wsb // 4)]
    dw, ws = (b[GUARD:-GUARD] for b in bufs)
    xm, gm = ops.ZwConv3d.bound_of(xg), ops.ZwConv3d.bound_of(gg)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    check(lib().m3d_conv3d_wgrad_narrow_dilated_f16x2(ptr(xg), ptr(gg), ptr(dw), B, cin, cout, D, H, W, 2, ptr(xm), ptr(gm), ptr(ws),
                                                      C.c_size_t(wsb), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "conv3d_wgrad_narrow_dilated_f16x2")
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())
    assert not bool((dw == SENTINEL).any()) and not bool((ws == SENTINEL).any())           # every element of both was written
    got = dw.view(torch.float32).reshape(cout, cin, 3, 3, 3).cpu().double()
    assert bool(((got - y).abs() <= E).all())
    assert torch.equal(dw.view(torch.float32).reshape(cout, cin, 3, 3, 3), d2(ops, xg, gg))
    assert torch.equal(x.cuda(), xg) and torch.equal(gy.cuda(), gg)                        # the operands are read only


@pytest.mark.parametrize("name", ["roi7_b3", "slot16"])
def test_bit_identical_run_to_run_and_on_a_side_stream(ops, name):
    gy, x, _, _, _ = reference(name)
    xg, gg = x.cuda(), gy.cuda()
    first = d2(ops, xg, gg)
    for _ in range(3):
        assert torch.equal(d2(ops, xg, gg), first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = d2(ops, xg, gg)
    side.synchronize()
    assert torch.equal(other, first)


def test_unsupported_shape_or_dilation_is_an_error(ops):
    from m3d import M3DError
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(M3DError):
        d2(ops, z(1, 32, 2, 4, 9), z(1, 32, 2, 4, 9))                                      # W = 9
    with pytest.raises(M3DError):
        d2(ops, z(1, 16, 2, 4, 8), z(1, 32, 2, 4, 8))                                      # cin = 16
    with pytest.raises(M3DError):
        ops.conv3d_wgrad_narrow_f16x2(z(1, 32, 2, 4, 8), z(1, 32, 2, 4, 8), dilation=3)    # dilation 3


@pytest.mark.parametrize("name", ["roi7_b3", "short", "ci96"])
def test_dilation_1_through_the_new_entry_is_the_old_launch(ops, name):
    from m3d._lib import lib, check
    case = case_of(name)
    B, cin, cout, D, H, W = case
    gy, x, _, _, _ = reference(name)
    xg, gg = x.cuda(), gy.cuda()
    want = ops.conv3d_wgrad_narrow_f16x2(xg, gg)
    xm, gm = ops.ZwConv3d.bound_of(xg), ops.ZwConv3d.bound_of(gg)
    wsb = int(lib().m3d_conv3d_wgrad_narrow_dilated_f16x2_workspace_bytes(*case, 1))
    assert wsb == int(lib().m3d_conv3d_wgrad_narrow_f16x2_workspace_bytes(*case))
    dw, ws = torch.empty_like(want), torch.empty((wsb,), dtype=torch.uint8, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    check(lib().m3d_conv3d_wgrad_narrow_dilated_f16x2(ptr(xg), ptr(gg), ptr(dw), B, cin, cout, D, H, W, 1, ptr(xm), ptr(gm), ptr(ws),
                                                      C.c_size_t(wsb), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "conv3d_wgrad_narrow_dilated_f16x2")
    assert torch.equal(dw, want)
    assert torch.equal(ops.conv3d_wgrad_narrow_f16x2(xg, gg, dilation=1), want)
    assert not torch.equal(d2(ops, xg, gg), want)                                          # and dilation 2 is another gradient


@pytest.fixture
def compat():
    import m3d.compat as c
    was = (c._orig_conv3d is not None, c._orig_linear is not None)
    prev = c.get_conv_dilated()
    c.install()
    yield c
    c.set_conv_wgrad_dilated_f16(False)
    c.set_conv_dilated_f16(False)
    c.set_conv_dilated(prev)
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


def test_routing_through_compat(ops, compat):
    from m3d import conv_plan as cp
    torch.manual_seed(4)
    conv = torch.nn.Conv3d(32, 64, 3, 1, padding=2, dilation=2).cuda()
    x = torch.relu(torch.randn(4, 32, 7, 7, 7, device="cuda")) * 3
    r = torch.randn(4, 64, 7, 7, 7, device="cuda")
    compat.set_conv_dilated("m3d")
    assert compat.get_conv_wgrad_dilated_f16() is False                                     # the default, install() or not
    y0, gx0, gw0, gb0 = _step(conv, x, r)
    assert torch.equal(gw0, ops.conv3d_wgrad(x, r, 3, dilation=2))
    assert compat.set_conv_wgrad_dilated_f16(True, min_work=0) is False
    s = cp.TrainSetting(dilated="m3d")
    assert cp.plan_train_conv(s._replace(wgrad_dilated_f16=0), x.shape, conv.weight.shape, 2, (True, True, True)).wgrad == cp.WGRAD_DILATED_F16X2
    y1, gx1, gw1, gb1 = _step(conv, x, r)
    assert torch.equal(gw1, d2(ops, x, r))                                                  # this kernel's dW bit for bit
    assert float((gw1 - gw0).abs().max()) <= 1e-5 * float(gw0.abs().max())
    assert torch.equal(y1, y0) and torch.equal(gx1, gx0) and torch.equal(gb1, gb0)
    # with the dilated f16x2 forward / dgrad as well: the bounds the step already holds are the ones the kernel takes
    compat.set_conv_dilated_f16(True, 0)
    y2, gx2, gw2, gb2 = _step(conv, x, r)
    gb_want, gy_max = ops.conv3d_gy_reduce(r)
    assert torch.equal(gw2, d2(ops, x, r, ops.ZwConv3d.bound_of(x), gy_max))
    assert torch.equal(gb2, gb_want)
    compat.set_conv_wgrad_dilated_f16(False)
    y3, gx3, gw3, gb3 = _step(conv, x, r)                                                   # the new switch off: only gw moves
    assert torch.equal(y3, y2) and torch.equal(gx3, gx2) and torch.equal(gb3, gb2) and torch.equal(gw3, gw0)
    compat.set_conv_dilated_f16(False)
    # the default threshold is the constant
    compat.set_conv_wgrad_dilated_f16(True)
    want = cp.plan_train_conv(s._replace(wgrad_dilated_f16=cp.WGRAD_DILATED_F16X2_MIN_WORK), x.shape, conv.weight.shape, 2, (True, True, True)).wgrad
    assert torch.equal(_step(conv, x, r)[2], gw1 if want == cp.WGRAD_DILATED_F16X2 else gw0)
    compat.set_conv_wgrad_dilated_f16(True, 0)
    # a W = 12 dilation-2 layer and every dilation-1 layer are unchanged
    x12 = torch.randn(2, 32, 4, 6, 12, device="cuda")
    r12 = torch.randn(2, 64, 4, 6, 12, device="cuda")
    assert torch.equal(_step(conv, x12, r12)[2], ops.conv3d_wgrad(x12, r12, 3, dilation=2))
    conv1 = torch.nn.Conv3d(32, 64, 3, 1, 1).cuda()
    assert torch.equal(_step(conv1, x, r)[2], ops.conv3d_wgrad(x, r, 3))
    assert torch.equal(_step(conv1, x12, r12)[2], ops.conv3d_wgrad(x12, r12, 3))
    c1 = torch.nn.Conv3d(32, 64, 1, 1, 0).cuda()
    assert torch.equal(_step(c1, x, r)[2], ops.conv3d_wgrad(x, r, 1))
    # without set_conv_dilated("m3d") the switch has no effect: torch's own conv runs the layer
    compat.set_conv_dilated("torch")
    gw_t = _step(conv, x, r)[2]
    compat.set_conv_wgrad_dilated_f16(False)
    assert torch.equal(_step(conv, x, r)[2], gw_t)


def _head_grads(head, feat, rois7, r):
    for p in head.parameters():
        p.grad = None
    f = feat.clone().requires_grad_(True)
    (head(f, rois7) * r).sum().backward()
    got = {k: p.grad.clone() for k, p in head.named_parameters()}
    got["feat"] = f.grad
    return got


def test_mask_head_at_dilation_2_gradients(compat):
    """the construction of tests/test_gpu_conv_dilated.py::test_mask_head_at_dilation_2 with 32 input channels, so that both convs route:
    the error against the fp64 module within 4 x torch's own fp32 error on the same device"""
    import m3d
    import oracle as O
    import test_gpu_conv_dilated as CD
    ocfg = O.Cfg(mlp_dim=64)
    stride = int(ocfg.stride)
    cfg = m3d.MaskTrainCfg(dim_reduced=32, num_convs=2, dilation=2)
    torch.manual_seed(7)
    head = m3d.MaskHead(32, cfg, stride=stride).cuda()
    with torch.no_grad():
        head.classify.weight.normal_(0, 0.05)
        for p in head.parameters():
            if p.dim() == 1:
                p.normal_(0, 0.1)
    gen = torch.Generator().manual_seed(8)
    feat = torch.randn((1, 32, 8, 16, 16), generator=gen).cuda()
    ext = torch.tensor([16.0, 16.0, 8.0]) * stride
    lo = torch.rand((5, 3), generator=gen) * ext * 0.5
    hi = lo + (0.1 + 0.4 * torch.rand((5, 3), generator=gen)) * ext
    rois7 = torch.cat([torch.zeros(5, 1), lo, hi], 1).cuda()
    r = torch.randn((5, 1, 14, 14, 14), generator=gen).cuda()
    _, g64 = CD._head_fp64(head, feat, rois7, r, 1.0 / stride, int(cfg.sampling_ratio))
    err = lambda got: max(float((got[k].double().cpu() - g64[k]).abs().max() / g64[k].abs().max()) for k in g64)
    assert all(float(g64[k].abs().max()) > 0 for k in g64)
    compat.set_conv_dilated("torch")
    e_torch = err(_head_grads(head, feat, rois7, r))                       # torch's own dilated conv3d on the device
    compat.set_conv_dilated("m3d")
    off = _head_grads(head, feat, rois7, r)
    compat.set_conv_wgrad_dilated_f16(True, 0)
    on = _head_grads(head, feat, rois7, r)
    compat.set_conv_dilated_f16(True, 0)
    both = _head_grads(head, feat, rois7, r)                               # with the carried bounds
    assert set(on) == set(g64)
    e_off, e_on, e_both = err(off), err(on), err(both)
    print("MaskHead at dilation 2: e_torch %.3g e_m3d %.3g (f16x2 dilated wgrad off) %.3g (on) %.3g (on, f16x2 forward / dgrad too)"
          % (e_torch, e_off, e_on, e_both))
    assert e_on <= 4 * e_torch, (e_on, e_torch)
    assert e_both <= 4 * e_torch, (e_both, e_torch)
    # only the conv weights' gradients moved ("feat" comes out of RoIAlign's default backward, whose atomic adds meet in any order)
    moved = [k for k in on if k != "feat" and not torch.equal(on[k], off[k])]
    assert moved and all(on[k].dim() == 5 for k in moved), moved
    assert len([k for k in moved if tuple(on[k].shape[2:]) == (3, 3, 3)]) == 2             # both 3^3 convs routed
