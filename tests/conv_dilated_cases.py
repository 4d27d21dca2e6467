"""The table and the fp64 reference of the dilated (k = 3, dilation 2, padding 2) conv backward tests: test_conv_dilated_host.py (CPU) and
test_gpu_conv_dilated.py.  Reference: F.conv3d(x64, w64, padding=2, dilation=2) and its autograd on the CPU in fp64 - what the nn.Conv3d
layers of lib/modeling/mask_rcnn_heads.py:141-151 compute in training with MRCNN.DILATION = 2.  Every reference is computed once per
process (lru_cache) and never written to."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
EPS = 2.0 ** -24

# (batch, cin, cout, D, H, W): the weight-gradient cases and what each is for.  The kernel has two voxel tiles, 2 x 4 x 16 and 2 x 8 x 8
# (the library takes the second for W <= 8); the GPU tests run every case on the library's choice and on each tile asked for by name.
CASES = [
    (1, 4, 5, 2, 4, 16),       # exactly one 2 x 4 x 16 tile: the split is capped at 1
    (3, 33, 70, 1, 3, 3),      # D = 1: every dz != 1 tap is exactly 0; H = W = 3: a +-2 tap joins only voxels 0 and 2; channels one past a 32-block
    (2, 7, 33, 3, 5, 6),       # W % 4 = 2
    (1, 33, 7, 2, 2, 9),       # W % 4 = 1, H < 4; W = 9 is the first width on the 2 x 4 x 16 tile
    (2, 5, 6, 5, 9, 19),       # W % 4 = 3, two x tiles; the first halo row of channel 0 lies before the tensor's first element
    (1, 70, 33, 3, 4, 8),      # W = 8: the last width on the 2 x 8 x 8 tile; three cin blocks
    (3, 32, 32, 7, 7, 7),      # the 7^3 RoI grid
    (2, 33, 32, 14, 14, 14),   # the 14^3 RoI grid
    (2, 3, 40, 11, 22, 40),    # 216 tiles of 2 x 4 x 16, several split slots
    (1, 4, 5, 2, 8, 8),        # exactly one 2 x 8 x 8 tile
    (2, 5, 6, 3, 9, 7),        # 2 x 8 x 8 with two y tiles (H = 9), W % 4 = 3
]
TILES = (0, 16, 8)             # 0: the library's choice
D1_CASE = CASES[1]
COMPAT_CASES = (CASES[2], CASES[6])


def case_id(c):
    return "b%d_ci%d_co%d_%dx%dx%d" % c


def operands(case, kind):
    """fp32 CPU tensors x [B,cin,D,H,W], gy [B,cout,D,H,W], w [cout,cin,3,3,3], bias [cout]; kind 'int': integers in [-3, 3] (every sum
    of absolute products of the table stays below 2^24, so any fp32 evaluation order is exact), 'randn': standard normal"""
    B, cin, cout, D, H, W = case
    g = torch.Generator().manual_seed(hash(case) % (1 << 31) + (0 if kind == "int" else 1))
    shapes = ((B, cin, D, H, W), (B, cout, D, H, W), (cout, cin, 3, 3, 3), (cout,))
    if kind == "int":
        assert 9 * B * D * H * W < 2 ** 24 and 9 * 27 * max(cin, cout) + 3 < 2 ** 24
        return tuple(torch.randint(-3, 4, s, generator=g).to(torch.float32) for s in shapes)
    return tuple(torch.randn(s, generator=g) for s in shapes)


def wgrad64(x, gy, dilation=2):
    """dW [cout,cin,3,3,3] in fp64: autograd of F.conv3d (linear in w, so w's value does not matter)"""
    w = torch.zeros((gy.shape[1], x.shape[1], 3, 3, 3), dtype=F64, requires_grad=True)
    F.conv3d(x.to(F64), w, padding=dilation, dilation=dilation).backward(gy.to(F64))
    return w.grad


def dgrad64(gy, w, dilation=2):
    x = torch.zeros((gy.shape[0], w.shape[1]) + tuple(gy.shape[2:]), dtype=F64, requires_grad=True)
    F.conv3d(x, w.to(F64), padding=dilation, dilation=dilation).backward(gy.to(F64))
    return x.grad


@functools.lru_cache(maxsize=None)
def reference(case, kind):
    """dict(x, gy, w, bias: fp32 operands; y, gx, gw, gb: fp64; A: the fp64 sum of |gy| |x| over the terms of every gw element)"""
    x, gy, w, bias = operands(case, kind)
    r = dict(x=x, gy=gy, w=w, bias=bias)
    r["y"] = F.conv3d(x.to(F64), w.to(F64), bias.to(F64), padding=2, dilation=2)
    r["gw"] = wgrad64(x, gy)
    r["gx"] = dgrad64(gy, w)
    r["gb"] = gy.to(F64).sum((0, 2, 3, 4))
    r["A"] = wgrad64(x.abs(), gy.abs())
    return r


def terms(case):
    """n of the bound below without the slots: the number of products behind one gw element, at most"""
    B, _, _, D, H, W = case
    return B * D * H * W


def bound(ref64, A, n):
    """|got - ref64| <= n 2^-24 A_e + 2^-24 |ref64|: the summation bound of n rounded operations in any order, plus the rounding of the
    result itself.  Nothing measured sets it."""
    return n * EPS * A + EPS * ref64.abs()


def worst_ratio(got, ref64, A, n):
    err, b = (got.to(F64) - ref64).abs(), bound(ref64, A, n)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b)        # 0 / 0 (an exactly zero tap) is no error; x / 0 is inf
    return float(ratio.max())
