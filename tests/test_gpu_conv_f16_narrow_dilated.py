"""GPU: the narrow-map f16x2 conv at dilation 2 (csrc/conv3d_zn.hip, conv3d_zn_kernel<2>), forward and backward-data, through
ops.ZnConv3d(..., dilation=2) and through m3d_conv3d_zn_dilated_forward itself, on the cases of tests/conv_f16_narrow_dilated_cases.py:
small integers bit-equal to fp64 at every element (NaN-filled output between guard rows), two runs and a side stream bit-identical, every
random family within the contract's bound E at every element with the shift returned exactly where C == 0, the output bound equal to
max|out| bit for bit, dilation 1 through the new entry point bit-equal to m3d_conv3d_zn_forward.

Measured on an MI355X (pytest -s prints them), worst |got - y| / E per case over the six families, forward / dgrad: see DESIGN.md
"Dilated per-RoI convs on the f16 pipe"."""
import ctypes as C

import pytest
import torch

import conv_f16_narrow_cases as T1
import conv_f16_narrow_dilated_cases as T

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


def _dev(t):
    return None if t is None else t.cuda()


def _pack(ops, direction, wl):
    wg = wl.cuda()
    return ops.ZnConv3d(wg) if direction == "forward" else ops.ZnConv3d.dgrad_of(T.forward_weight("dgrad", wg))


def _bound(ops, direction, ag):
    return ops.ZnConv3d.bound_of(ag) if direction == "forward" else ops.conv3d_gy_reduce(ag, bias=False)[1]


def _run(ops, direction, a, wl, scale=None, shift=None, relu=False, out=None, out_max=False, via_c=False, dilation=2):
    """the launched conv through ops.ZnConv3d(dilation=) (forward: the plain pack and a swept bound; dgrad: the dgrad_of pack of the
    forward parameter and gy_reduce's bound), or with via_c through m3d_conv3d_zn_dilated_forward itself"""
    ag = a.cuda()
    conv = _pack(ops, direction, wl)
    im = _bound(ops, direction, ag)
    if not via_c:
        return conv(ag, im, scale=_dev(scale), shift=_dev(shift), relu=relu, out=out, out_max=out_max, dilation=dilation)[0]
    from m3d._lib import lib, check
    B, cin, D, H, W = a.shape
    sc, sh = _dev(scale), _dev(shift)
    if out is None:
        out = torch.empty((B, conv.cout, D, H, W), dtype=torch.float32, device="cuda")
    check(lib().m3d_conv3d_zn_dilated_forward(_ptr(ag), _ptr(conv.packed), _ptr(out), B, cin, conv.cout, D, H, W, dilation, _ptr(sc), _ptr(sh),
                                              int(relu), _ptr(im), None, _stream()), "conv3d_zn_dilated_forward")
    return out


# ------------------------------------------------------------------ 1. integers: bit-exact, guards, determinism, a side stream
@pytest.mark.parametrize("via_c", [False, True], ids=["ops", "c_abi"])
@pytest.mark.parametrize("case", T.CASE_NAMES)
@pytest.mark.parametrize("direction", T.DIRECTIONS)
def test_integer_data_sentinels_and_determinism(ops, direction, case, via_c):
    a, wl, shift = T.integer_inputs(case, direction)
    want = T.reference_op(direction, a, wl, None, shift, False)
    buf, mid = guarded(want.numel())
    out = mid.view(torch.float32).view(want.shape)
    got = _run(ops, direction, a, wl, shift=shift, out=out, via_c=via_c)
    torch.cuda.synchronize()
    assert intact(buf)
    assert got.dtype == torch.float32 and not bool(torch.isnan(got).any())                  # every element was written
    assert torch.equal(got.cpu().double(), want)                                            # bit-exact: index and halo errors show
    first = got.clone()
    buf2, mid2 = guarded(want.numel())
    again = _run(ops, direction, a, wl, shift=shift, out=mid2.view(torch.float32).view(want.shape), via_c=via_c)
    assert torch.equal(again, first) and intact(buf2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        buf3, mid3 = guarded(want.numel())
        third = _run(ops, direction, a, wl, shift=shift, out=mid3.view(torch.float32).view(want.shape), via_c=via_c)
    side.synchronize()
    assert torch.equal(third, first) and intact(buf3)


# ------------------------------------------------------------------ 2. random families: every element within E
_worst = {}


@pytest.mark.parametrize("family", T.FAMILIES)
@pytest.mark.parametrize("case", T.CASE_NAMES)
@pytest.mark.parametrize("direction", T.DIRECTIONS)
def test_every_element_within_the_bound(ops, direction, case, family):
    a, wl, scale, shift, relu, y, E, Cm = T.reference(case, direction, family)
    buf, mid = guarded(y.numel())
    out = mid.view(torch.float32).view(y.shape)
    got = _run(ops, direction, a, wl, scale, shift, relu, out=out, via_c=(family == "benign")).cpu().double()
    assert intact(buf)
    assert got.shape == y.shape and bool(torch.isfinite(got).all())
    err = (got - y).abs()
    worst = float((err / E.clamp_min(1e-300)).max())
    _worst[(direction, case)] = max(_worst.get((direction, case), 0.0), worst)
    print("%s %s %s: worst |got - y| / E %.4f (per case so far %.4f)" % (direction, case, family, worst, _worst[(direction, case)]))
    assert bool((err <= E).all())
    assert torch.equal(got[Cm == 0], y[Cm == 0].float().double())              # where C == 0: exactly the shift (ReLU'd) / exactly 0
    again = _run(ops, direction, a, wl, scale, shift, relu).cpu().double()
    assert torch.equal(again, got)                                             # bit-identical run to run, through ops


def test_a_loose_bound_still_meets_its_own_E(ops):
    """an operand bound 4 max|x| (what a carried bound may be): E computed from that A"""
    a, wl, scale, shift, relu = T.make("roi_grid", "forward", "benign")
    A = 4.0 * float(a.abs().max())
    y, E, _ = T.contract("forward", a, wl, scale, shift, relu, in_bound=A)
    im = torch.zeros(ops.ZnConv3d.SLOTS, device="cuda")
    im[7] = A
    got = ops.ZnConv3d(wl.cuda())(a.cuda(), im, scale=scale.cuda(), shift=shift.cuda(), relu=relu, out_max=False, dilation=2)[0].cpu().double()
    assert bool(((got - y).abs() <= E).all())


# ------------------------------------------------------------------ 3. the output's bound
@pytest.mark.parametrize("case", ["roi_grid", "short", "ragged_walk"])
def test_out_max_is_the_largest_output_bit_for_bit(ops, case):
    a, wl, scale, shift, relu, y, E, _ = T.reference(case, "forward", "benign")
    conv, ag = ops.ZnConv3d(wl.cuda()), a.cuda()
    im = ops.ZnConv3d.bound_of(ag)
    out, om = conv(ag, im, scale=scale.cuda(), shift=shift.cuda(), relu=relu, dilation=2)
    assert tuple(om.shape) == (ops.ZnConv3d.SLOTS,) and bool((om >= 0).all())
    assert torch.equal(om.max().reshape(1), out.abs().max().reshape(1))
    out2, om2 = conv(ag, im, shift=shift.cuda(), dilation=2)                   # signed outputs: the magnitude
    assert torch.equal(om2.max().reshape(1), out2.abs().max().reshape(1))
    # out_max=False: nothing beyond out is written
    buf, mid = guarded(y.numel())
    o3, none = conv(ag, im, scale=scale.cuda(), shift=shift.cuda(), relu=relu, out=mid.view(torch.float32).view(y.shape), out_max=False,
                    dilation=2)
    torch.cuda.synchronize()
    assert none is None and intact(buf) and torch.equal(o3, out)
    # a chain: the second conv on the first's bound, no sweep
    w2 = (torch.randn(16, conv.cout, 3, 3, 3, generator=torch.Generator().manual_seed(2)) * 0.1)
    if conv.cout % 16 == 0:
        y2, E2, _ = T.contract("forward", out.cpu(), w2, in_bound=float(om.max()))
        z = ops.ZnConv3d(w2.cuda())(out, om, out_max=False, dilation=2)[0].cpu().double()
        assert bool(((z - y2).abs() <= E2).all())


# ------------------------------------------------------------------ 4. dilation 1 through the new entry point
@pytest.mark.parametrize("case", ["roi_grid", "short", "tiles"])
@pytest.mark.parametrize("direction", T.DIRECTIONS)
def test_dilation_1_through_the_new_entry_point_is_the_old_launch(ops, direction, case):
    from m3d._lib import lib, check
    a, wl, scale, shift, relu = T1.make(case, direction, "benign")
    ag, conv = a.cuda(), _pack(ops, direction, wl)
    im = _bound(ops, direction, ag)
    B, cin, D, H, W = a.shape
    sc, sh = _dev(scale), _dev(shift)
    outs, maxes = [], []
    for new in (False, True):
        out = torch.empty((B, conv.cout, D, H, W), dtype=torch.float32, device="cuda")
        om = torch.zeros(ops.ZnConv3d.SLOTS, device="cuda")
        head = (_ptr(ag), _ptr(conv.packed), _ptr(out), B, cin, conv.cout, D, H, W)
        tail = (_ptr(sc), _ptr(sh), int(relu), _ptr(im), _ptr(om), _stream())
        if new:
            check(lib().m3d_conv3d_zn_dilated_forward(*head, 1, *tail), "conv3d_zn_dilated_forward")
        else:
            check(lib().m3d_conv3d_zn_forward(*head, *tail), "conv3d_zn_forward")
        outs.append(out)
        maxes.append(om)
    assert torch.equal(outs[0], outs[1]) and torch.equal(maxes[0], maxes[1])
    assert torch.equal(conv(ag, im, scale=sc, shift=sh, relu=relu, out_max=False, dilation=1)[0], outs[0])
    y, E, _ = T1.contract(direction, a, wl, scale, shift, relu)
    assert bool(((outs[1].cpu().double() - y).abs() <= E).all())
