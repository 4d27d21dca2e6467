"""GPU: the f16x2 conv weight gradient (m3d_conv3d_wgrad_f16x2) against fp64, element by element, on the cases of
tests/wgrad_f16x2_contract.py: integer data bit-exact (index and halo errors), every element within the contract's bound, exact zeros,
sentinels around everything it may write, determinism, and the routing through m3d.compat.

Measured worst |error| / bound per case (printed with pytest -s) stays below 0.1: the bound's n_acc term is a worst case over signs."""
import ctypes as C

import pytest
import torch

import wgrad_f16x2_contract as K

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                    # a quiet NaN with a payload
GUARD = 1024                             # floats before and after each buffer


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as o
    return o


_ref = {}


def reference(name):
    """(gy, x, fp64 dW, E, C) of a case on random data, computed once and shared (never modified)"""
    if name not in _ref:
        from m3d import ops as o
        case = K.CASES[name]
        p = o.conv3d_wgrad_f16x2_plan(*case)
        gy, x = K.make_inputs("benign", case, 11, relu_x=True)
        y, E, Cm, _, _ = K.contract(gy, x, p["chain"] + p["folds"])
        _ref[name] = (gy, x, y, E, Cm)
    return _ref[name]


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_integer_data_is_bit_exact(ops, name):
    gy, x = K.integer_inputs(K.CASES[name], 3)
    want = K.wgrad_op(gy, x)
    got = ops.conv3d_wgrad_f16x2(x.cuda(), gy.cuda()).cpu()
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert torch.equal(got.double(), want)


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_every_element_within_the_bound_and_exact_zeros(ops, name):
    gy, x, y, E, Cm = reference(name)
    got = ops.conv3d_wgrad_f16x2(x.cuda(), gy.cuda()).cpu().double()
    assert bool(torch.isfinite(got).all())
    err = (got - y).abs()
    ratio = float((err / E.clamp_min(1e-300)).max())
    print("%s: worst |error| / bound %.4f, worst |error| / max |dW| %.3g" % (name, ratio, float(err.max() / y.abs().max())))
    assert bool((err <= E).all())
    assert bool((got[Cm == 0] == 0).all())


@pytest.mark.parametrize("family", ["heavy", "outlier8", "quiet", "at_bound_pow2", "at_bound_below", "zero"])
def test_input_families_within_the_bound(ops, family):
    case = K.CASES["ragged3"]
    p = ops.conv3d_wgrad_f16x2_plan(*case)
    for relu_x in (False, True):
        gy, x = K.make_inputs(family, case, 17, relu_x)
        y, E, Cm, _, _ = K.contract(gy, x, p["chain"] + p["folds"])
        got = ops.conv3d_wgrad_f16x2(x.cuda(), gy.cuda()).cpu().double()
        err = (got - y).abs()
        print("%s relu_x=%d: worst |error| / bound %.4f" % (family, relu_x, float((err / E.clamp_min(1e-300)).max())))
        assert bool(torch.isfinite(got).all()) and bool((err <= E).all())
        assert bool((got[Cm == 0] == 0).all())
        if family == "zero":
            assert bool((got == 0).all())
            assert bool((ops.conv3d_wgrad_f16x2(gy.cuda().new_ones(x.shape), torch.zeros_like(gy).cuda()) == 0).all())     # gy = 0


def test_a_loose_bound_changes_nothing_beyond_the_contract(ops):
    """a bound handed over by a producer (2^3 above the maximum) instead of a sweep: the contract with that bound"""
    name = "co64"
    gy, x, y, _, _ = reference(name)
    case = K.CASES[name]
    p = ops.conv3d_wgrad_f16x2_plan(*case)
    A, B = float(gy.abs().max()) * 8, float(x.abs().max()) * 8
    Cm, Sa, Sb, n = K.terms(K.wgrad_op, gy, x)
    E = K.bound(p["chain"] + p["folds"], Cm, Sa, Sb, n, A, B, y)
    slots = lambda v: torch.tensor([0.0] * 7 + [v] + [0.0] * 24, device="cuda")         # the largest slot counts, wherever it is
    got = ops.conv3d_wgrad_f16x2(x.cuda(), gy.cuda(), x_max=slots(B), gy_max=slots(A)).cpu().double()
    assert bool(((got - y).abs() <= E).all())


@pytest.mark.parametrize("name", ["ragged3", "co96_ci64", "slot2", "roi7_b5"])
def test_sentinels_around_output_and_workspace(ops, name):
    from m3d._lib import lib, check
    case = K.CASES[name]
    B, cin, cout, D, H, W = case
    gy, x, y, E, _ = reference(name)
    xg, gg = x.cuda(), gy.cuda()
    n = cout * cin * 27
    wsb = int(lib().m3d_conv3d_wgrad_f16x2_workspace_bytes(*case))
    assert wsb % 4 == 0 and wsb == ops.conv3d_wgrad_f16x2_plan(*case)["slots"] * n * 4
    bufs = [torch.full((GUARD + m + GUARD,), SENTINEL, dtype=torch.int32, device="cuda") for m in (n, wsb // 4)]
    dw, ws = (b[GUARD:-GUARD] for b in bufs)
    xm, gm = ops.ZwConv3d.bound_of(xg), ops.ZwConv3d.bound_of(gg)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    check(lib().m3d_conv3d_wgrad_f16x2(ptr(xg), ptr(gg), ptr(dw), B, cin, cout, D, H, W, ptr(xm), ptr(gm), ptr(ws), C.c_size_t(wsb),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "conv3d_wgrad_f16x2")
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[-GUARD:] == SENTINEL).all())
    got = dw.view(torch.float32).reshape(cout, cin, 3, 3, 3).cpu().double()
    assert bool(((got - y).abs() <= E).all())                                              # every output element was written
    assert torch.equal(dw.view(torch.float32).reshape(cout, cin, 3, 3, 3), ops.conv3d_wgrad_f16x2(xg, gg))
    assert torch.equal(x.cuda(), xg) and torch.equal(gy.cuda(), gg)                        # the operands are read only


@pytest.mark.parametrize("name", ["ragged3", "slot16"])
def test_bit_identical_run_to_run_and_on_a_side_stream(ops, name):
    gy, x, _, _, _ = reference(name)
    xg, gg = x.cuda(), gy.cuda()
    first = ops.conv3d_wgrad_f16x2(xg, gg)
    for _ in range(3):
        assert torch.equal(ops.conv3d_wgrad_f16x2(xg, gg), first)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = ops.conv3d_wgrad_f16x2(xg, gg)
    side.synchronize()
    assert torch.equal(other, first)


def test_unsupported_shape_is_an_error(ops):
    from m3d import M3DError
    with pytest.raises(M3DError):
        ops.conv3d_wgrad_f16x2(torch.zeros(1, 16, 2, 4, 16, device="cuda"), torch.zeros(1, 32, 2, 4, 16, device="cuda"))


@pytest.fixture
def conv_compat():
    import m3d.compat as c
    c.install_conv3d()
    yield c
    c.set_conv_wgrad("fp32")
    c.uninstall_conv3d()


def _step(conv, x, r):
    conv.zero_grad()
    xr = x.clone().requires_grad_(True)
    y = conv(xr)
    (y * r).sum().backward()
    return y.detach(), xr.grad, conv.weight.grad.clone(), conv.bias.grad.clone()


def test_routing_through_compat(ops, conv_compat):
    from m3d import conv_plan as cp
    torch.manual_seed(0)
    conv = torch.nn.Conv3d(32, 64, 3, 1, 1).cuda()
    shape = (2, 17, 33, 63)                                                                 # odd extents, 2^27 products per tap and more
    x = torch.relu(torch.randn(shape[0], 32, *shape[1:], device="cuda"))
    r = torch.randn(shape[0], 64, *shape[1:], device="cuda")
    assert conv_compat.get_conv_wgrad() == "fp32"                                           # the default, install() or not
    y0, gx0, gw0, gb0 = _step(conv, x, r)
    assert torch.equal(gw0, ops.conv3d_wgrad(x, r, 3))
    conv_compat.set_conv_wgrad("f16x2")
    assert cp.wgrad_kernel(shape[0], 32, 64, *shape[1:], "f16x2") == cp.WGRAD_F16X2
    y1, gx1, gw1, gb1 = _step(conv, x, r)
    assert torch.equal(gw1, ops.conv3d_wgrad_f16x2(x, r))                                   # this kernel's dW bit for bit
    assert not torch.equal(gw1, gw0)
    assert torch.equal(y1, y0) and torch.equal(gx1, gx0) and torch.equal(gb1, gb0)
    assert float((gw1 - gw0).abs().max()) <= 1e-5 * float(gw0.abs().max())
    # a layer the kernel takes but the rule does not route (one voxel tile of work) stays on the fp32 kernel
    xs, rs = x[:1, :, :2, :4, :16].contiguous(), r[:1, :, :2, :4, :16].contiguous()
    assert ops.conv3d_wgrad_f16x2_supported(1, 32, 64, 2, 4, 16)
    assert cp.wgrad_kernel(1, 32, 64, 2, 4, 16, "f16x2") == cp.WGRAD_FP32
    assert torch.equal(_step(conv, xs, rs)[2], ops.conv3d_wgrad(xs, rs, 3))
    # unsupported layers stay on the fp32 kernel: cin 16, k = 1, the 5^3 stem
    for cin, cout, k in ((16, 32, 3), (32, 32, 1), (1, 32, 5)):
        c2 = torch.nn.Conv3d(cin, cout, k, 1, k // 2).cuda()
        x2 = torch.randn(1, cin, 4, 8, 24, device="cuda")
        r2 = torch.randn(1, cout, 4, 8, 24, device="cuda")
        assert cp.wgrad_kernel(1, cin, cout, 4, 8, 24, "f16x2", k=k) == cp.WGRAD_FP32
        assert torch.equal(_step(c2, x2, r2)[2], ops.conv3d_wgrad(x2, r2, k))
