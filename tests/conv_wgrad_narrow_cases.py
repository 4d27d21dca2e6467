"""The table and the fp64 reference of the narrow-map (k = 3, dilation 1, W <= 8) conv weight-gradient tests: test_conv_box_head_host.py
(CPU) and test_gpu_conv_wgrad_narrow.py.  Reference: autograd of F.conv3d(x64, w64, padding=1) on the CPU in fp64 - what the nn.Conv3d
layers of lib/modeling/fast_rcnn_heads.py:128-136 (roi_Xconv1fc_head) compute in training.  Every reference is computed once per process
(lru_cache) and never written to."""
import functools

import torch
import torch.nn.functional as F

F64 = torch.float64
EPS = 2.0 ** -24

# (batch, cin, cout, D, H, W) and why the 2 x 8 x 8 tile kernel can go wrong on it
CASES = [
    (3, 32, 32, 7, 7, 7),      # the RoI grid: 7 of 8 along y and x, an odd z tile (the last tile's second plane is outside)
    (2, 32, 32, 8, 8, 8),      # full tiles
    (1, 4, 5, 2, 8, 8),        # channel counts below a block, exactly one tile
    (2, 33, 31, 3, 5, 7),      # ragged channels (one past / one short of a 32-block) and all three extents short
    (5, 32, 64, 1, 7, 7),      # D = 1: every dz != 1 tap is exactly 0
    (1, 64, 32, 14, 14, 8),    # several y and z tiles
    (17, 32, 32, 7, 7, 7),     # many split slots, an uneven number of tiles per slot
    (2, 20, 40, 7, 7, 3),      # a very narrow row: one quad of x, a halo quad that begins before the tensor
]
D1_CASE = CASES[4]


def case_id(c):
    return "b%d_ci%d_co%d_%dx%dx%d" % c


def operands(case, kind):
    """fp32 CPU tensors x [B,cin,D,H,W], gy [B,cout,D,H,W]; kind 'int': integers in [-3, 3] (every sum of absolute products of the table
    stays below 2^24, so any fp32 evaluation order is exact), 'randn': standard normal"""
    B, cin, cout, D, H, W = case
    g = torch.Generator().manual_seed(sum(v * 31 ** i for i, v in enumerate(case)) % (1 << 31) + (0 if kind == "int" else 1))
    shapes = ((B, cin, D, H, W), (B, cout, D, H, W))
    if kind == "int":
        assert 9 * B * D * H * W < 2 ** 24
        return tuple(torch.randint(-3, 4, s, generator=g).to(torch.float32) for s in shapes)
    return tuple(torch.randn(s, generator=g) for s in shapes)


def wgrad64(x, gy):
    """dW [cout,cin,3,3,3] in fp64: autograd of F.conv3d (linear in w, so w's value does not matter)"""
    w = torch.zeros((gy.shape[1], x.shape[1], 3, 3, 3), dtype=F64, requires_grad=True)
    F.conv3d(x.to(F64), w, padding=1).backward(gy.to(F64))
    return w.grad


@functools.lru_cache(maxsize=None)
def reference(case, kind):
    """dict(x, gy: fp32 operands; gw: fp64; A: the fp64 sum of |gy| |x| over the terms of every gw element)"""
    x, gy = operands(case, kind)
    return dict(x=x, gy=gy, gw=wgrad64(x, gy), A=wgrad64(x.abs(), gy.abs()))


def terms(case):
    """n of the bound below without the slots: the number of products behind one gw element, at most"""
    B, _, _, D, H, W = case
    return B * D * H * W


def bound(ref64, A, n):
    """|got - ref64| <= n 2^-24 A_e + 2^-24 |ref64|: the summation bound of n rounded operations in any order, plus the rounding of the
    result itself (the bound of tests/conv_dilated_cases.py).  Nothing measured sets it."""
    return n * EPS * A + EPS * ref64.abs()


def worst_ratio(got, ref64, A, n):
    err, b = (got.to(F64) - ref64).abs(), bound(ref64, A, n)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)        # 0 / 0 (an exactly zero tap) is no error; x / 0 is inf
    return float(ratio.max())
