"""The cases of the training convs on the f16x2 kernel (m3d.compat.set_conv_train("f16x2")): forward and backward-data of a 3^3 layer on
m3d_conv3d_zw_forward, with fp64 references and the per-element bound of tests/f16x2_contract.py (zw_contract).  No GPU needed.

  forward   y = conv3d(x, w) + bias                          bound: zw_contract(x, w, max|x|, shift=bias)
  dgrad     gx = conv_transpose3d(gy, w)                     bound: zw_contract(gy, w.flip(2, 3, 4).transpose(0, 1), max|gy|)

The cases are the smallest at which each form of the kernel can go wrong, as (B, cin, cout, D, H, W) of the FORWARD layer."""
import torch

import f16x2_contract as K

F64 = torch.float64

CASES = {
    "xb16_ragged": (2, 16, 96, 3, 5, 13),     # the 16-wide tile, ragged on every axis, a partial second 64-channel group
    "xb32_ragged": (1, 32, 64, 5, 9, 37),     # the 32-wide tile, two x tiles, ragged
    "cout32": (2, 64, 32, 4, 8, 24),          # 32 output channels (forward); the dgrad has 64
    "min_map": (2, 32, 64, 2, 4, 12),         # the smallest map the kernel takes
}
FAMILIES = ("benign", "heavy", "outlier8", "quiet", "zero", "at_bound_pow2", "at_bound_below")
DIRECTIONS = ("forward", "dgrad")

# the six 3^3 body layers (cin, cout, map divisor) of m3d.train.DsnBody(width=32): conv2a / 2b, 3a / 3b, 4a / 4b
BODY_LAYERS = ((32, 64, 2), (64, 64, 2), (64, 128, 4), (128, 128, 4), (128, 256, 8), (256, 256, 8))
SOMA_TILE, NUCLEI_TILE = (64, 256, 256), (128, 128, 128)          # TRAIN.IN_SIZE of the two configurations


def shapes(case, direction):
    """(operand shape, weight shape [cout, cin, 3, 3, 3]) of a case: x for forward, gy for dgrad"""
    B, cin, cout, D, H, W = CASES[case]
    return (B, cin if direction == "forward" else cout, D, H, W), (cout, cin, 3, 3, 3)


def dgrad_weight(w):
    """the weight of the backward-data conv as a forward conv: taps flipped, channel roles swapped"""
    return w.flip(2, 3, 4).transpose(0, 1).contiguous()


def make(case, direction, family, seed=5):
    """(a, w, bias): the operand (x ReLU'd / gy signed), the FORWARD layer's weight and its bias (None for dgrad)"""
    ashape, wshape = shapes(case, direction)
    a, w = K.inputs(family, ashape, wshape, seed, signed=(direction == "dgrad"))
    bias = None
    if direction == "forward":
        bias = torch.randn(wshape[0], generator=torch.Generator().manual_seed(seed + 1))
    return a, w, bias


def integer_inputs(case, direction, seed=3):
    """small integers: every product, every Winograd combination and every sum is exact in fp16 x 2 / fp32, so the result is bit-exact"""
    ashape, wshape = shapes(case, direction)
    g = torch.Generator().manual_seed(seed)
    lo = 0 if direction == "forward" else -7
    a = torch.randint(lo, 8, ashape, generator=g).float()
    w = torch.randint(-3, 4, wshape, generator=g).float()
    bias = torch.randint(-5, 6, (wshape[0],), generator=g).float() if direction == "forward" else None
    return a, w, bias


def reference_op(direction, a, w, bias=None):
    """fp64: the forward conv + bias, or the transposed conv (what autograd's backward-data is)"""
    if direction == "forward":
        y = K.conv3d_op(a.to(F64), w.to(F64))
        return y if bias is None else y + bias.to(F64).view(1, -1, 1, 1, 1)
    return K.dgrad_op(a.to(F64), w.to(F64))


def contract(direction, a, w, bias=None):
    """(fp64 reference, E, C) of one direction with the swept bound max|a|"""
    amax = float(a.abs().max())
    if direction == "forward":
        return K.zw_contract(a, w, amax, shift=bias)
    y, E, C = K.zw_contract(a, dgrad_weight(w), amax)
    return reference_op("dgrad", a, w), E, C        # (the reference the issue names; equal to y up to fp64 rounding, checked on the host)


_cache = {}


def reference(case, direction, family):
    """(a, w, bias, y, E, C), computed once and shared (never modified)"""
    key = (case, direction, family)
    if key not in _cache:
        a, w, bias = make(case, direction, family)
        _cache[key] = (a, w, bias) + tuple(contract(direction, a, w, bias))
    return _cache[key]


def pack_dgrad_index(cin, cout):
    """NumPy-style restatement of the role swap and tap flip (index arithmetic only): for the backward-data conv's weight wd [cin, cout, 3,
    3, 3] of a forward parameter w [cout, cin, 3, 3, 3], the flat index into w of every element of wd: wd.flat = w.flat[index]"""
    import numpy as np
    o, i, z, y, x = np.meshgrid(np.arange(cin), np.arange(cout), np.arange(3), np.arange(3), np.arange(3), indexing="ij")
    # wd[o, i, z, y, x] = w[i, o, 2 - z, 2 - y, 2 - x]; one tap index t = 9 z + 3 y + x flips to 26 - t
    return ((i * cin + o) * 27 + (26 - (9 * z + 3 * y + x))).reshape(-1)


def gb_bound(g):
    """the contract of m3d_conv3d_gy_reduce's d_grad_bias for g [B, cout, D, H, W]: (S fp64 [cout], bound [cout]) with
    |gb - S| <= 2^-24 |S| + n 2^-53 sum |g|"""
    g64 = g.to(F64)
    S = g64.sum(dim=(0, 2, 3, 4))
    n = g.numel() // g.shape[1]
    return S, 2.0 ** -24 * S.abs() + n * 2.0 ** -53 * g64.abs().sum(dim=(0, 2, 3, 4))
