"""GPU: the training convs on the f16x2 kernel (m3d.compat.set_conv_train("f16x2")): m3d_conv3d_zw_pack_dgrad byte for byte against the
pack of the flipped, transposed copy; m3d_conv3d_gy_reduce against fp64 sums and ops.absmax; forward and backward-data through m3d.ops on
the cases of tests/conv_train_cases.py, every element against the f16x2 contract's bound; the routing through m3d.compat (the default
unchanged bit for bit); and the gradients of m3d.train.DsnBody against an fp64 CPU run of the same modules.

Measured on an MI355X (pytest -s prints them): the worst |error| / bound is 0.13 over every case and direction of the families
benign, heavy, outlier8, zero and at_bound (the bound's n_acc term is a worst case over signs) and 0.85 in the forward `quiet` family, where
the rounding of the bias add, 2^-24 |y|, is nearly all of the bound; gy_reduce's worst |gb - S| / bound is 0.59; DsnBody(stride=4, width=16) gradients, largest error / largest fp64 gradient: see
test_body_gradients' docstring."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv_train_cases as T

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                    # a quiet NaN with a payload
GUARD = 1024                             # floats before and after each buffer


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as o
    return o


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded(n):
    """(whole buffer, the n-element middle) of SENTINEL words"""
    buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    return buf, buf[GUARD:GUARD + n]


def intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


# ------------------------------------------------------------------ 1. pack_dgrad
@pytest.mark.parametrize("cout,cin", [(64, 32), (48, 20), (16, 1), (96, 16)])
def test_pack_dgrad_bytes(ops, cout, cin):
    from m3d._lib import lib, check
    w = (torch.randn(cout, cin, 3, 3, 3, generator=torch.Generator().manual_seed(cout)) * 0.2).cuda()
    want = ops.ZwConv3d(T.dgrad_weight(w)).packed
    nbytes = int(lib().m3d_conv3d_zw_packed_bytes(cout, cin))
    assert nbytes == want.numel() and nbytes % 4 == 0
    got = ops.ZwConv3d.dgrad_of(w)
    assert (got.cin, got.cout) == (cout, cin)
    # the bytes the kernels write: the fragments and the scale float behind them (the rest of the 256-byte tail is never written)
    written = nbytes - 256 + 4
    assert torch.equal(got.packed[:written], want[:written])
    buf, mid = guarded(nbytes // 4)
    check(lib().m3d_conv3d_zw_pack_dgrad(_ptr(w), cin, cout, _ptr(mid), _stream()), "conv3d_zw_pack_dgrad")
    torch.cuda.synchronize()
    assert intact(buf)
    assert torch.equal(mid.view(torch.uint8)[:written], want[:written])
    assert bool((mid[written // 4:] == SENTINEL).all())                   # nothing behind the scale float is touched
    assert float(mid[written // 4 - 1:written // 4].view(torch.float32)) == float(w.abs().max())


# ------------------------------------------------------------------ 2. gy_reduce
GY_SHAPES = [(2, 5, 3, 5, 13), (2, 3, 17, 33, 63), (1, 1, 1, 1, 1)]


def _gy(shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))) * 3


@pytest.mark.parametrize("shape", GY_SHAPES)
def test_gy_reduce(ops, shape):
    from m3d._lib import lib, check
    g = _gy(shape)
    S, bound = T.gb_bound(g)
    gg = g.cuda()
    gb, gmax = ops.conv3d_gy_reduce(gg)
    assert gb.dtype == torch.float32 and tuple(gb.shape) == (shape[1],) and tuple(gmax.shape) == (ops.ZwConv3d.SLOTS,)
    err = (gb.cpu().double() - S).abs()
    print("gy_reduce %s: worst |gb - S| / bound %.3f" % (shape, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all())
    amax = ops.absmax(gg)
    assert torch.equal(gmax.max().reshape(1), amax.reshape(1)) and float(amax) == float(g.abs().max())
    assert bool((gmax >= 0).all())
    none, gmax2 = ops.conv3d_gy_reduce(gg, bias=False)                     # d_grad_bias = NULL: the same bound
    assert none is None and torch.equal(gmax2, gmax)
    # sentinels around gb, the slots and the workspace
    n = C.c_size_t(0)
    check(lib().m3d_conv3d_gy_reduce(None, *shape, None, None, None, C.byref(n), None), "size")
    assert n.value % 8 == 0 and n.value > 0
    bufs = [guarded(m) for m in (shape[1], ops.ZwConv3d.SLOTS, n.value // 4)]
    (b_gb, m_gb), (b_sl, m_sl), (b_ws, m_ws) = bufs
    cap = C.c_size_t(n.value)
    check(lib().m3d_conv3d_gy_reduce(_ptr(gg), *shape, _ptr(m_gb), _ptr(m_sl), _ptr(m_ws), C.byref(cap), _stream()), "conv3d_gy_reduce")
    torch.cuda.synchronize()
    assert all(intact(b) for b, _ in bufs) and cap.value == n.value
    assert torch.equal(m_gb.view(torch.float32), gb) and torch.equal(m_sl.view(torch.float32), gmax)
    assert torch.equal(g.cuda(), gg)                                        # the operand is read only
    # bit-identical run to run and on a side stream
    for _ in range(3):
        gb2, gm2 = ops.conv3d_gy_reduce(gg)
        assert torch.equal(gb2, gb) and torch.equal(gm2, gmax)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        gb3, gm3 = ops.conv3d_gy_reduce(gg)
    side.synchronize()
    assert torch.equal(gb3, gb) and torch.equal(gm3, gmax)


def test_gy_reduce_misaligned_base_and_zero(ops):
    """a tensor that starts 4 bytes off a 16-byte boundary (every slab's head is scalar), and an all-zero gradient"""
    shape = GY_SHAPES[1]
    g = _gy(shape)
    base = torch.zeros(g.numel() + 1, device="cuda")
    gg = base[1:].view(shape)
    gg.copy_(g)
    assert gg.data_ptr() % 16 == 4
    gb, gmax = ops.conv3d_gy_reduce(gg)
    gb0, gmax0 = ops.conv3d_gy_reduce(g.cuda())
    S, bound = T.gb_bound(g)
    assert bool(((gb.cpu().double() - S).abs() <= bound).all()) and float(gmax.max()) == float(g.abs().max())
    assert torch.equal(gmax.max(), gmax0.max())
    z, zmax = ops.conv3d_gy_reduce(torch.zeros(shape, device="cuda"))
    assert bool((z == 0).all()) and bool((zmax == 0).all())


# ------------------------------------------------------------------ 3. forward and dgrad through ops, swept bounds
def _run(ops, direction, a, w, bias, out=None):
    ag, wg = a.cuda(), w.cuda()
    if direction == "forward":
        return ops.ZwConv3d(wg)(ag, ops.ZwConv3d.bound_of(ag), shift=bias.cuda(), out_max=False, out=out)[0]
    gb, gmax = ops.conv3d_gy_reduce(ag, bias=False)
    return ops.ZwConv3d.dgrad_of(wg)(ag, gmax, out_max=False, out=out)[0]


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("case", sorted(T.CASES))
@pytest.mark.parametrize("direction", T.DIRECTIONS)
def test_every_element_within_the_bound(ops, direction, case, family):
    a, w, bias, y, E, Cm = T.reference(case, direction, family)
    got = _run(ops, direction, a, w, bias).cpu().double()
    assert got.shape == y.shape and bool(torch.isfinite(got).all())
    err = (got - y).abs()
    print("%s %s %s: worst |error| / bound %.4f" % (direction, case, family, float((err / E.clamp_min(1e-300)).max())))
    assert bool((err <= E).all())
    exact = y if direction == "forward" else torch.zeros_like(y)          # where C == 0: exactly the bias / exactly 0
    assert torch.equal(got[Cm == 0], exact[Cm == 0].float().double())
    if family == "zero":
        assert bool((Cm == 0).all())


@pytest.mark.parametrize("case", sorted(T.CASES))
@pytest.mark.parametrize("direction", T.DIRECTIONS)
def test_integer_data_sentinels_and_determinism(ops, direction, case):
    a, w, bias = T.integer_inputs(case, direction)
    want = T.reference_op(direction, a, w, bias)
    got = _run(ops, direction, a, w, bias)
    assert got.dtype == torch.float32 and torch.equal(got.cpu().double(), want)            # bit-exact: index and halo errors show
    # sentinels around the output, on the random data of the contract test
    a, w, bias, y, E, _ = T.reference(case, direction, "benign")
    buf, mid = guarded(y.numel())
    out = mid.view(torch.float32).view(y.shape)
    first = _run(ops, direction, a, w, bias, out=out)
    torch.cuda.synchronize()
    assert intact(buf)
    assert bool(((first.cpu().double() - y).abs() <= E).all())                              # every element was written
    for _ in range(2):
        assert torch.equal(_run(ops, direction, a, w, bias), first)


# ------------------------------------------------------------------ 4 / 5. through m3d.compat
@pytest.fixture
def conv_compat():
    import m3d.compat as c
    c.install_conv3d()
    yield c
    c.set_conv_train("fp32")
    c.set_conv_wgrad("fp32")
    c.uninstall_conv3d()


def _step(conv, x, r):
    conv.zero_grad()
    xr = x.clone().requires_grad_(True)
    y = conv(xr)
    (y * r).sum().backward()
    return y.detach(), xr.grad, conv.weight.grad.clone(), None if conv.bias is None else conv.bias.grad.clone()


SHAPE = (2, 17, 33, 63)                  # tests/test_gpu_wgrad_f16x2.py::test_routing_through_compat: 324 zw units at 32 -> 64


def _layer(cin, cout, k=3, seed=0):
    torch.manual_seed(seed)
    conv = torch.nn.Conv3d(cin, cout, k, 1, k // 2).cuda()
    x = torch.relu(torch.randn(SHAPE[0], cin, *SHAPE[1:], device="cuda"))
    r = torch.randn(SHAPE[0], cout, *SHAPE[1:], device="cuda")
    return conv, x, r


def _fp32_path(ops, conv, x, r):
    w, b, k = conv.weight.detach(), conv.bias.detach(), conv.weight.shape[2]
    return (ops.PackedConv3d(w, ops.W_PLAIN)(x, shift=b), ops.PackedConv3d(w, ops.W_DGRAD)(r) if k != 5 else None,
            ops.conv3d_wgrad(x, r, k), ops.conv3d_bias_grad(r))


def test_the_default_changes_nothing(ops, conv_compat):
    conv, x, r = _layer(32, 64)
    assert conv_compat.get_conv_train() == "fp32" and conv_compat.get_conv_wgrad() == "fp32"
    y, gx, gw, gb = _step(conv, x, r)
    y0, gx0, gw0, gb0 = _fp32_path(ops, conv, x, r)
    assert torch.equal(y, y0) and torch.equal(gx, gx0) and torch.equal(gw, gw0) and torch.equal(gb, gb0)


def test_routing_through_compat(ops, conv_compat):
    from m3d import conv_plan as cp
    Z = ops.ZwConv3d
    for cin in (32, 64):
        conv, x, r = _layer(cin, 64)
        w, b = conv.weight.detach(), conv.bias.detach()
        y0, gx0, gw0, gb0 = _step(conv, x, r)
        assert conv_compat.set_conv_train("f16x2") == "fp32"
        assert cp.train_conv_kernel("forward", SHAPE[0], cin, 64, *SHAPE[1:], "f16x2") == "f16x2"
        y1, gx1, gw1, gb1 = _step(conv, x, r)
        x_max = Z.bound_of(x)
        assert torch.equal(y1, Z(w)(x, x_max, shift=b, out_max=False)[0]) and not torch.equal(y1, y0)
        gb_want, gy_max = ops.conv3d_gy_reduce(r)
        assert torch.equal(gb1, gb_want)
        route = cp.train_conv_kernel("dgrad", SHAPE[0], cin, 64, *SHAPE[1:], "f16x2")
        assert cin != 64 or route == "f16x2"                                # the layer the issue names for the f16x2 dgrad
        if route == "f16x2":
            assert torch.equal(gx1, Z.dgrad_of(w)(r, gy_max, out_max=False)[0]) and not torch.equal(gx1, gx0)
            assert float((gx1 - gx0).abs().max()) <= 1e-5 * float(gx0.abs().max())
        else:
            assert torch.equal(gx1, gx0)
        assert torch.equal(gw1, gw0)                                        # the wgrad setting is its own
        assert float((y1 - y0).abs().max()) <= 1e-5 * float(y0.abs().max())
        # with the f16x2 wgrad as well: the saved x bound and the shared gy bound, no further sweep
        conv_compat.set_conv_wgrad("f16x2")
        assert cp.wgrad_kernel(SHAPE[0], cin, 64, *SHAPE[1:], "f16x2") == cp.WGRAD_F16X2
        _, _, gw2, gb2 = _step(conv, x, r)
        assert torch.equal(gw2, ops.conv3d_wgrad_f16x2(x, r, x_max, gy_max)) and torch.equal(gb2, gb_want)
        conv_compat.set_conv_wgrad("fp32")
        conv_compat.set_conv_train("fp32")
        assert all(torch.equal(p, q) for p, q in zip(_step(conv, x, r), (y0, gx0, gw0, gb0)))      # and back


def test_layers_that_stay_on_fp32(ops, conv_compat):
    from m3d import conv_plan as cp
    conv_compat.set_conv_train("f16x2")
    conv_compat.set_conv_wgrad("f16x2")
    # below ZW_MIN_UNITS
    conv, x, r = _layer(32, 64)
    xs, rs = x[:1, :, :2, :4, :16].contiguous(), r[:1, :, :2, :4, :16].contiguous()
    assert cp.train_conv_kernel("forward", 1, 32, 64, 2, 4, 16, "f16x2") == "fp32"
    assert cp.train_conv_kernel("forward", 1, 32, 64, 2, 4, 16, "f16x2", min_units=0) == "f16x2"
    y, gx, gw, gb = _step(conv, xs, rs)
    y0, gx0, gw0, _ = _fp32_path(ops, conv, xs, rs)
    assert torch.equal(y, y0) and torch.equal(gx, gx0) and torch.equal(gw, gw0)
    assert torch.equal(gb, ops.conv3d_gy_reduce(rs)[0])                    # f16x2 mode: gb from gy_reduce whatever the route
    # ... and with min_units = 0 the small supported layer moves
    conv_compat.set_conv_train("f16x2", min_units=0)
    y2, gx2, _, gb2 = _step(conv, xs, rs)
    assert torch.equal(y2, ops.ZwConv3d(conv.weight.detach())(xs, ops.ZwConv3d.bound_of(xs), shift=conv.bias.detach(), out_max=False)[0])
    assert not torch.equal(y2, y0) and torch.equal(gb2, gb)
    if cp.train_conv_kernel("dgrad", 1, 32, 64, 2, 4, 16, "f16x2", min_units=0) == "f16x2":
        assert torch.equal(gx2, ops.ZwConv3d.dgrad_of(conv.weight.detach())(rs, ops.conv3d_gy_reduce(rs)[1], out_max=False)[0])
        assert not torch.equal(gx2, gx0)
    else:
        assert torch.equal(gx2, gx0)
    # cin = 24, k = 1, the 5^3 stem: unsupported, whatever min_units says
    for cin, cout, k in ((24, 32, 3), (32, 32, 1), (1, 32, 5)):
        torch.manual_seed(cin)
        c2 = torch.nn.Conv3d(cin, cout, k, 1, k // 2).cuda()
        x2 = torch.randn(1, cin, 4, 8, 24, device="cuda")
        r2 = torch.randn(1, cout, 4, 8, 24, device="cuda")
        for d in T.DIRECTIONS:
            assert cp.train_conv_kernel(d, 1, cin, cout, 4, 8, 24, "f16x2", min_units=0, k=k) == "fp32"
        y, gx, gw, gb = _step(c2, x2, r2)
        y0, gx0, gw0, _ = _fp32_path(ops, c2, x2, r2)
        assert torch.equal(y, y0) and torch.equal(gw, gw0) and (k == 5 or torch.equal(gx, gx0))
        if k == 5:
            assert torch.equal(gx, ops.conv3d_stem5_dgrad(r2, ops.conv3d_stem5_dgrad_weights(c2.weight.detach())))


def test_a_weight_update_repacks(ops, conv_compat):
    conv_compat.set_conv_train("f16x2")
    conv, x, r = _layer(64, 64, seed=2)
    Z = ops.ZwConv3d
    _step(conv, x, r)
    _step(conv, x, r)                                                       # the same version: served from the cache
    with torch.no_grad():
        conv.weight.mul_(0.5).add_(0.01 * torch.randn_like(conv.weight))
    w, b = conv.weight.detach(), conv.bias.detach()
    y, gx, _, _ = _step(conv, x, r)
    assert torch.equal(y, Z(w)(x, Z.bound_of(x), shift=b, out_max=False)[0])
    assert torch.equal(gx, Z.dgrad_of(w)(r, ops.conv3d_gy_reduce(r, bias=False)[1], out_max=False)[0])
    conv_compat.invalidate_packs()
    assert torch.equal(_step(conv, x, r)[0], y)


# ------------------------------------------------------------------ 6. the body
class PlainBody4(torch.nn.Module):
    """m3d.train.DsnBody(stride=4) as plain torch.nn modules (lib/modeling/DSN.py up to pool2 / conv3b)"""
    PLAN = (("1a", 5, True), ("2a", 3, False), ("2b", 3, True), ("3a", 3, False), ("3b", 3, False))

    def __init__(self, w):
        super().__init__()
        ch = {"1a": (1, w), "2a": (w, 2 * w), "2b": (2 * w, 2 * w), "3a": (2 * w, 4 * w), "3b": (4 * w, 4 * w)}
        for n, k, _ in self.PLAN:
            setattr(self, "conv" + n, torch.nn.Conv3d(ch[n][0], ch[n][1], k, 1, k // 2))
            setattr(self, "bn" + n, torch.nn.BatchNorm3d(ch[n][1], momentum=0.001))

    def forward(self, x):
        for n, _, pool in self.PLAN:
            x = F.relu(getattr(self, "bn" + n)(getattr(self, "conv" + n)(x)))
            if pool:
                x = F.max_pool3d(x, 2, 2)
        return x


def test_body_gradients(conv_compat):
    """DsnBody(stride=4, width=16) in train() on [2, 1, 16, 32, 48]: its 3^3 layers run at W = 24 (the 32-wide tile) and W = 12 (the
    16-wide tile).  Parameter and input gradients of (out * r).sum() against an fp64 CPU run of the same modules; the largest error
    relative to the largest fp64 gradient in mode "f16x2" (min_units = 0, wgrad f16x2 on) may be at most 8 x the same figure in mode
    "fp32" (short-K layers: the fp32 kernel was measured 5 - 7 x better there, equal at long K).
    Measured on an MI355X: fp32 1.55e-06, f16x2 9.7e-07 (ratio 0.62)."""
    import m3d
    torch.manual_seed(11)
    body = m3d.train.DsnBody(stride=4, width=16)
    with torch.no_grad():
        for n, p in body.named_parameters():      # weights large enough for every layer to matter, gamma / beta off their defaults
            if n.startswith("conv") and n.endswith("weight"):
                p.normal_(0, (2.0 / p[0].numel()) ** 0.5)
            elif n.startswith("bn"):
                p.add_(0.2 * torch.randn_like(p))
    sd = {k: v.clone() for k, v in body.state_dict().items()}
    x = torch.randn(2, 1, 16, 32, 48)
    r = torch.randn(2, 64, 4, 8, 12)

    def grads(model, inp, rr):
        model.train()
        model.zero_grad()
        inp = inp.clone().requires_grad_(True)
        (model(inp) * rr).sum().backward()
        g = {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}
        g["input"] = inp.grad.detach().double().cpu()
        return g
    ref = PlainBody4(16).double()
    ref.load_state_dict(sd)
    g64 = grads(ref, x.double(), r.double())
    scale = max(v.abs().max().item() for v in g64.values())
    body = body.cuda()
    errs = {}
    for mode in ("fp32", "f16x2"):
        body.load_state_dict(sd)
        conv_compat.set_conv_train(mode, min_units=0)
        conv_compat.set_conv_wgrad(mode)
        g = grads(body, x.cuda(), r.cuda())
        assert set(g) == set(g64)
        errs[mode] = max((g[n] - g64[n]).abs().max().item() for n in g64) / scale
    print("DsnBody(stride=4, width=16) gradients, largest error / largest fp64 gradient: fp32 %.3e, f16x2 %.3e (ratio %.2f)"
          % (errs["fp32"], errs["f16x2"], errs["f16x2"] / errs["fp32"]))
    assert errs["f16x2"] <= 8 * errs["fp32"]
