"""GPU: every production instantiation of the direct fp32 conv (csrc/conv3d.hip) against fp64, element by element, over the case table of
tests/direct_conv_cases.py (which instantiation a case runs, and that the table covers all of them at ragged tiles, partial chunks and
half-empty cout tiles, is proved on the CPU by tests/test_direct_conv_cases_host.py).

 (a) exact on integers: with integer-valued inputs and sum |w| |x| < 2^24 every fp32 summation order is exact, so the result must EQUAL the
     fp64 reference - one wrong tap, one dropped voxel at a ragged edge, one stale channel of a partial chunk, K-split halves joined
     wrongly or a batch item read from its neighbour all show, at any channel count;
 (b) bounded on random data: the per-element bound of direct_conv_cases.bound (guards the arithmetic; the worst ratio per variant is
     printed, pytest -s);
 (c) conv3d_wgrad / conv3d_bias_grad / conv3d_stem5_dgrad exact on integers against fp64 autograd, and bit-identical when repeated;
 (d) nn.Conv3d through m3d.compat's autograd function: y and all three gradients exact, nothing falling through to torch's conv."""
import pytest
import torch
import torch.nn.functional as F

import direct_conv_cases as T

pytestmark = pytest.mark.gpu

F64 = T.F64
LIMIT = 2.0 ** 24
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from m3d import ops as _ops
    assert torch.cuda.is_available()
    yield _ops
    for (variant, what), r in sorted(WORST.items()):
        print("direct conv: worst |got - y| / bound  variant %2d %-6s %.4f" % (variant, what, r))
    torch.cuda.empty_cache()


def gen_of(c, salt=0):
    return torch.Generator().manual_seed(1000 * T.CASES.index(c) + salt)


def runs_variant(ops, c):
    p = ops.conv3d_direct_plan(c.batch, c.cin, c.cout, c.D, c.H, c.W, c.k, c.pool)
    assert p is not None and p["variant"] == c.variant, (c, p)


def same(got, ref, what):
    """bit-equal to the fp64 reference cast to fp32; on a mismatch, where the wrong elements are (tile, row and channel block name the path)"""
    got, ref = got.cpu(), ref.to(torch.float32)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        raise AssertionError("%s: %d of %d elements differ; first (b, c, z, y, x) %s got %r want %r; last %s; channels %s"
                             % (what, bad.shape[0], ref.numel(), bad[0].tolist(), float(got[tuple(bad[0])]), float(ref[tuple(bad[0])]),
                                bad[-1].tolist(), sorted(set(bad[:, 1].tolist()))[:40]))


def epilogue_operands(c, gen):
    """integer in_offset, power-of-two scale, integer shift and mul: every step of the epilogue is exact"""
    off = torch.tensor([-2.0])
    scale = 2.0 ** torch.randint(-1, 3, (c.cout,), generator=gen).to(torch.float32)
    shift = T.integers((c.cout,), -8, 8, gen)
    return off, scale, shift


def epilogue64(conv, scale, shift, mul=None):
    v = torch.relu(conv * scale.to(F64).view(1, -1, 1, 1, 1) + shift.to(F64).view(1, -1, 1, 1, 1))
    return v if mul is None else v * mul.to(F64)


@pytest.mark.parametrize("c", [c for c in T.CASES if not c.pool], ids=T.case_id)
def test_exact_on_integers(ops, c):
    runs_variant(ops, c)
    gen = gen_of(c)
    shape = (c.batch, c.cin, c.D, c.H, c.W)
    x = T.integers(shape, -4, 4, gen)
    w = T.integers((c.cout, c.cin) + (c.k,) * 3, -2, 2, gen)
    taps = c.k ** 3 * c.cin
    assert taps * 2 * 4 < LIMIT                       # sum |w| |x| of any output, at most
    xd = x.cuda()
    same(ops.PackedConv3d(w.cuda())(xd), T.conv64(x, w, c.k), "plain")

    # relu(W) pack, input offset (padding stays 0, not -offset), scale, shift, ReLU, mul
    off, scale, shift = epilogue_operands(c, gen)
    mul = T.integers((c.batch, c.cout, c.D, c.H, c.W), -2, 2, gen)
    assert (taps * 2 * 6 * 4 + 8) * 2 < LIMIT
    ref = epilogue64(T.conv64(x - off, torch.relu(w), c.k), scale, shift, mul)
    got = ops.PackedConv3d(w.cuda(), ops.W_RELU)(xd, scale=scale.cuda(), shift=shift.cuda(), relu=True, in_offset=off.cuda(), mul=mul.cuda())
    same(got, ref, "relu(W), in_offset, scale, shift, relu, mul")
    if c.k == 5:                                      # the stem has no backward-data pack (conv3d_stem5_dgrad, below)
        return
    # backward-data packs of a weight whose conv maps cout -> cin channels: the same logical shape, hence the same instantiation
    wd = T.integers((c.cin, c.cout) + (c.k,) * 3, -2, 2, gen)
    for mode, wref in ((ops.W_DGRAD, wd), (ops.W_DGRAD_RELU, torch.relu(wd))):
        pack = ops.PackedConv3d(wd.cuda(), mode)
        assert (pack.cin, pack.cout) == (c.cin, c.cout)
        same(pack(xd), T.dgrad64(x, wref, c.k), "dgrad pack, mode %d" % mode)


@pytest.mark.parametrize("c", [c for c in T.CASES if c.pool], ids=T.case_id)
def test_fused_pool_exact_on_integers(ops, c):
    """pooled values bit-equal to max_pool3d of the exact conv; the arg-max by value (integer data tie): the un-pooled exact result,
    gathered at it, is the pooled value"""
    runs_variant(ops, c)
    gen = gen_of(c)
    x = T.integers((c.batch, c.cin, c.D, c.H, c.W), -4, 4, gen)
    w = T.integers((c.cout, c.cin) + (c.k,) * 3, -2, 2, gen)
    taps = c.k ** 3 * c.cin
    assert (taps * 2 * 6 * 4 + 8) < LIMIT
    off, scale, shift = epilogue_operands(c, gen)
    plain = T.conv64(x, w, c.k)
    full = epilogue64(T.conv64(x - off, torch.relu(w), c.k), scale, shift)
    runs = ((ops.PackedConv3d(w.cuda()), {}, plain, "plain"),
            (ops.PackedConv3d(w.cuda(), ops.W_RELU), dict(scale=scale.cuda(), shift=shift.cuda(), relu=True, in_offset=off.cuda()), full, "epilogue"))
    for pack, kw, ref, what in runs:
        got, am = pack.pooled(x.cuda(), return_argmax=True, **kw)
        want = F.max_pool3d(ref, 2)
        assert tuple(want.shape[2:]) == (c.D // 2, c.H // 2, c.W // 2)
        same(got, want, "pooled " + what)
        am = am.cpu()
        assert int(am.max()) < 8
        same(T.pool_gather(ref, am), want, "arg-max " + what)
        same(pack.pooled(x.cuda(), **kw), want, "pooled without arg-max " + what)


def within(c, what, got, y, cabs):
    got = got.cpu().to(F64)
    assert got.shape == y.shape and bool(torch.isfinite(got).all())
    bound = T.bound(c, y, cabs)
    ratio = float(((got - y).abs() / bound.clamp_min(1e-300)).max())
    WORST[(c.variant, what)] = max(WORST.get((c.variant, what), 0.0), ratio)
    print("direct conv ratio: %s %s %.4f" % (T.case_id(c), what, ratio))
    assert ratio <= 1.0, (T.case_id(c), what, ratio)


@pytest.mark.parametrize("c", T.CASES, ids=T.case_id)
def test_bounded_on_random_data(ops, c):
    """N(0,1) inputs, He-scaled weights; forward and (k = 1, 3) backward-data.  The fused pool: |max a - max b| <= max |a - b|, so the pooled
    result is held to the pooled bound."""
    runs_variant(ops, c)
    gen = gen_of(c, salt=1)
    taps = c.k ** 3 * c.cin
    x = torch.randn((c.batch, c.cin, c.D, c.H, c.W), generator=gen)
    w = torch.randn((c.cout, c.cin) + (c.k,) * 3, generator=gen) * (2.0 / taps) ** 0.5
    y, cabs = T.conv64(x, w, c.k), T.conv64(x.abs(), w.abs(), c.k)
    pack = ops.PackedConv3d(w.cuda())
    if c.pool:
        got = pack.pooled(x.cuda()).cpu().to(F64)
        want, bound = F.max_pool3d(y, 2), F.max_pool3d(T.bound(c, y, cabs), 2)
        ratio = float(((got - want).abs() / bound).max())
        WORST[(c.variant, "fwd")] = max(WORST.get((c.variant, "fwd"), 0.0), ratio)
        print("direct conv ratio: %s pooled %.4f" % (T.case_id(c), ratio))
        assert ratio <= 1.0, (T.case_id(c), ratio)
        return
    within(c, "fwd", pack(x.cuda()), y, cabs)
    if c.k == 5:
        return
    wd = torch.randn((c.cin, c.cout) + (c.k,) * 3, generator=gen) * (2.0 / taps) ** 0.5
    within(c, "dgrad", ops.PackedConv3d(wd.cuda(), ops.W_DGRAD)(x.cuda()), T.dgrad64(x, wd, c.k), T.dgrad64(x.abs(), wd.abs(), c.k))


# ------------------------------------------------------------------ (c) gradients
def autograd64(x, w, b, gy, k):
    xr, wr, br = (t.to(F64).requires_grad_() for t in (x, w, b))
    y = F.conv3d(xr, wr, br, padding=k // 2)
    y.backward(gy.to(F64))
    return y.detach(), xr.grad, wr.grad, br.grad


@pytest.mark.parametrize("shape", T.WGRAD_CASES, ids=lambda s: "b%d-%dto%d-%dx%dx%d-k%d" % s)
def test_wgrad_and_bias_grad_exact_on_integers(ops, shape):
    B, cin, cout, D, H, W, k = shape
    gen = torch.Generator().manual_seed(T.WGRAD_CASES.index(shape))
    x = T.integers((B, cin, D, H, W), -3, 3, gen)
    gy = T.integers((B, cout, D, H, W), -3, 3, gen)
    assert 3 * 3 * B * D * H * W < LIMIT             # sum |x| |gy| of any weight, at most; the bias gradient's sum is smaller
    _, _, gw, gb = autograd64(x, torch.zeros((cout, cin) + (k,) * 3), torch.zeros(cout), gy, k)
    xd, gyd = x.cuda(), gy.cuda()
    got_w, got_b = ops.conv3d_wgrad(xd, gyd, k), ops.conv3d_bias_grad(gyd)
    same(got_w, gw, "wgrad")
    same(got_b, gb, "bias grad")
    assert torch.equal(ops.conv3d_wgrad(xd, gyd, k), got_w) and torch.equal(ops.conv3d_bias_grad(gyd), got_b)


@pytest.mark.parametrize("shape", T.STEM_DGRAD_CASES, ids=lambda s: "b%d-c%d-%dx%dx%d" % s)
def test_stem5_dgrad_exact_on_integers(ops, shape):
    B, ch, D, H, W = shape
    gen = torch.Generator().manual_seed(77 + ch)
    gy = T.integers((B, ch, D, H, W), -3, 3, gen)
    w = T.integers((ch, 1, 5, 5, 5), -2, 2, gen)
    assert 125 * ch * 2 * 3 < LIMIT
    wf = ops.conv3d_stem5_dgrad_weights(w.cuda())
    got = ops.conv3d_stem5_dgrad(gy.cuda(), wf)
    same(got, T.dgrad64(gy, w, 5), "stem dgrad")
    assert torch.equal(ops.conv3d_stem5_dgrad(gy.cuda(), wf), got)


# ------------------------------------------------------------------ (d) through autograd
@pytest.fixture(scope="module")
def compat():
    import m3d.compat as c
    c.install()
    yield c
    c.uninstall_conv3d()
    c.uninstall_linear()


@pytest.mark.parametrize("cin,cout,k,shape,fwd_variant,dgrad_variant", [
    (17, 70, 3, (2, 18, 15, 61), 4, 0),              # forward: the K-split 32x2x4 tile; backward-data 70 -> 17 channels: 32x4x4, one cout block
    (1, 48, 5, (2, 9, 10, 45), 19, None),            # the two-block stem; backward-data by conv3d_stem5_dgrad
], ids=["17to70-k3", "stem-1to48-k5"])
def test_conv3d_module_exact_through_autograd(ops, compat, cin, cout, k, shape, fwd_variant, dgrad_variant):
    import torch.nn as nn
    B, D, H, W = shape
    assert ops.conv3d_direct_plan(B, cin, cout, D, H, W, k)["variant"] == fwd_variant
    if dgrad_variant is not None:
        assert ops.conv3d_direct_plan(B, cout, cin, D, H, W, k)["variant"] == dgrad_variant
    gen = torch.Generator().manual_seed(5 + k)
    conv = nn.Conv3d(cin, cout, k, padding=k // 2).cuda()
    w, b = T.integers(tuple(conv.weight.shape), -2, 2, gen), T.integers((cout,), -8, 8, gen)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    x = T.integers((B, cin, D, H, W), -3, 3, gen)
    gy = T.integers((B, cout, D, H, W), -3, 3, gen)
    assert k ** 3 * cin * 2 * 3 + 8 < LIMIT and k ** 3 * cout * 2 * 3 < LIMIT and 3 * 3 * B * D * H * W < LIMIT
    xd = x.cuda().requires_grad_()
    calls = []
    orig = compat._orig_conv3d
    compat._orig_conv3d = lambda *a, **kw: (calls.append(1), orig(*a, **kw))[1]
    try:
        assert F.conv3d is compat.conv3d
        y = conv(xd)
        y.backward(gy.cuda())
    finally:
        compat._orig_conv3d = orig
    assert not calls, "fell through to torch's conv"
    ry, rgx, rgw, rgb = autograd64(x, w, b, gy, k)
    same(y.detach(), ry, "y")
    same(xd.grad, rgx, "x.grad")
    same(conv.weight.grad, rgw, "weight.grad")
    same(conv.bias.grad, rgb, "bias.grad")
