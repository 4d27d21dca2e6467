"""The fp64 reference of the dilation-2 narrow-map f16x2 weight-gradient tests (tests/wgrad_dilated_f16_cases.py::wgrad_op_d2) is the
weight gradient of conv3d(dilation 2, padding 2): against autograd in fp64, and against an explicit loop.  A check of the tests' own
yardstick: it needs neither the library nor a GPU."""
import itertools

import torch

import wgrad_dilated_f16_cases as N


def test_the_reference_is_the_dilated_conv_weight_gradient():
    """wgrad_op_d2 against autograd's fp64 gradient of conv3d(dilation 2, padding 2), and against an explicit loop on a tiny shape"""
    g = torch.Generator().manual_seed(1)
    for shape in ((2, 3, 4, 5, 6, 7), (1, 2, 3, 2, 2, 2), (1, 1, 2, 3, 1, 8)):
        B, cin, cout, D, H, W = shape
        x = torch.randn((B, cin, D, H, W), generator=g, dtype=torch.float64)
        gy = torch.randn((B, cout, D, H, W), generator=g, dtype=torch.float64)
        w = torch.zeros((cout, cin, 3, 3, 3), dtype=torch.float64, requires_grad=True)
        torch.nn.functional.conv3d(x, w, None, 1, 2, 2).backward(gy)
        got = N.wgrad_op_d2(gy, x)
        assert float((got - w.grad).abs().max()) <= 1e-12 * max(1.0, float(w.grad.abs().max())), shape
    x = torch.randn((1, 1, 3, 4, 5), generator=g, dtype=torch.float64)
    gy = torch.randn((1, 1, 3, 4, 5), generator=g, dtype=torch.float64)
    want = torch.zeros(3, 3, 3, dtype=torch.float64)
    for dz, dy, dx, z, y, a in itertools.product(range(3), range(3), range(3), range(3), range(4), range(5)):
        zz, yy, aa = z + 2 * (dz - 1), y + 2 * (dy - 1), a + 2 * (dx - 1)
        if 0 <= zz < 3 and 0 <= yy < 4 and 0 <= aa < 5:
            want[dz, dy, dx] += gy[0, 0, z, y, a] * x[0, 0, zz, yy, aa]
    assert float((N.wgrad_op_d2(gy, x)[0, 0] - want).abs().max()) <= 1e-13
