"""CPU: the host side of the training convs on the f16x2 kernel: the routing rule (conv_plan.train_conv_kernel), the setting
(m3d.compat.set_conv_train), the refusals of the two new entry points before any pointer is followed, and the NumPy restatements of
what they compute (the role swap / tap flip of m3d_conv3d_zw_pack_dgrad, the error bound of m3d_conv3d_gy_reduce's bias gradient)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import conv_train_cases as T


@pytest.fixture(scope="module")
def cp():
    from m3d import conv_plan
    return conv_plan


@pytest.fixture(scope="module")
def L():
    from m3d._lib import lib
    return lib()


def _codes():
    import os
    import re
    from conftest import ROOT
    txt = open(os.path.join(ROOT, "include", "m3d.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (M3D_E\w+) \((-?\d+)\)", txt)}


# ------------------------------------------------------------------ the rule
def test_rule_is_fp32_where_the_issue_says(cp):
    big = (2, 32, 64, 17, 33, 63)                                        # 324 units: routes
    assert cp.train_conv_kernel("forward", *big, "f16x2") == "f16x2"
    for d in T.DIRECTIONS:
        assert cp.train_conv_kernel(d, 2, 64, 64, 17, 33, 63, "f16x2") == "f16x2"
        assert cp.train_conv_kernel(d, 2, 64, 64, 17, 33, 63, "fp32") == "fp32"                    # the mode
        for k in (1, 5):
            assert cp.train_conv_kernel(d, 2, 64, 64, 17, 33, 63, "f16x2", k=k) == "fp32"
        assert cp.train_conv_kernel(d, 2, 64, 64, 17, 33, 8, "f16x2", min_units=0) == "fp32"       # a map 8 wide
        assert cp.train_conv_kernel(d, 1, 64, 64, 2, 4, 16, "f16x2") == "fp32"                     # below min_units
    assert cp.train_conv_kernel("forward", 2, 24, 64, 17, 33, 63, "f16x2") == "fp32"               # forward cin 24
    assert cp.train_conv_kernel("dgrad", 2, 64, 24, 17, 33, 63, "f16x2") == "fp32"                 # dgrad: its input channels are cout
    assert cp.train_conv_kernel("dgrad", 2, 16, 64, 17, 33, 63, "f16x2") == "fp32"                 # dgrad with 16 output channels
    assert cp.train_conv_kernel("forward", 2, 64, 16, 17, 33, 63, "f16x2") == "fp32"               # forward with 16 output channels
    # a batch item at ITEM_LIMIT: 16 channels x 2^25 voxels x 4 bytes = 2^31
    for d in T.DIRECTIONS:
        assert 16 * 128 * 512 * 512 * 4 >= cp.ITEM_LIMIT
        assert cp.train_conv_kernel(d, 1, 16, 16, 128, 512, 512, "f16x2", min_units=0) == "fp32"
    assert 16 * 128 * 512 * 512 * 4 >= cp.ITEM_LIMIT > 16 * 64 * 512 * 512 * 4
    assert cp.train_conv_kernel("forward", 1, 16, 32, 128, 512, 512, "f16x2", min_units=0) == "fp32"
    assert cp.train_conv_kernel("forward", 1, 16, 32, 64, 512, 512, "f16x2", min_units=0) == "f16x2"
    assert cp.train_conv_kernel("dgrad", 1, 32, 16, 128, 512, 512, "f16x2", min_units=0) == "fp32"
    assert cp.train_conv_kernel("dgrad", 1, 32, 16, 64, 512, 512, "f16x2", min_units=0) == "f16x2"
    for bad in ("f16", None):
        with pytest.raises(ValueError):
            cp.train_conv_kernel("forward", *big, bad)
    with pytest.raises(ValueError):
        cp.train_conv_kernel("wgrad", *big, "f16x2")


def test_rule_is_a_pure_function_of_its_arguments(cp):
    src = inspect.getsource(cp.train_conv_kernel)
    assert "environ" not in src and "global" not in src
    args = ("dgrad", 4, 64, 128, 32, 32, 32, "f16x2")
    assert len({cp.train_conv_kernel(*args) for _ in range(3)}) == 1
    assert inspect.signature(cp.train_conv_kernel).parameters["min_units"].default == cp.ZW_MIN_UNITS


def test_rule_on_the_body_layers(cp):
    """the four 3^3 layers of the stride-4 soma body on its 64 x 256 x 256 tile, the six of the stride-8 nuclei body on four 128^3 volumes:
    forward everywhere; dgrad where the launched conv (output channels: the forward cin, at least 32) fills the chip"""
    for tile, B, layers in ((T.SOMA_TILE, 1, T.BODY_LAYERS[:4]), (T.NUCLEI_TILE, 4, T.BODY_LAYERS)):
        for cin, cout, div in layers:
            D, H, W = (t // div for t in tile)
            assert cp.train_conv_kernel("forward", B, cin, cout, D, H, W, "f16x2") == "f16x2", (tile, cin, cout)
            units = T_units(B, cout, cin, D, H, W)
            want = "f16x2" if (cin >= cp.TRAIN_F16X2_MIN_COUT["dgrad"] and units >= cp.ZW_MIN_UNITS) else "fp32"
            assert cp.train_conv_kernel("dgrad", B, cin, cout, D, H, W, "f16x2") == want, (tile, cin, cout)
    assert cp.train_conv_kernel("dgrad", 1, 64, 64, 32, 128, 128, "f16x2") == "f16x2"
    assert cp.train_conv_kernel("dgrad", 1, 32, 64, 32, 128, 128, "f16x2") == "f16x2"               # measured to win: 3.8 x
    assert cp.train_conv_kernel("dgrad", 1, 64, 128, 32, 32, 32, "f16x2") == "fp32"                  # 128 units: below ZW_MIN_UNITS
    assert cp.TRAIN_F16X2_MIN_COUT == {"forward": 32, "dgrad": 32}


def T_units(B, cin, cout, D, H, W):
    from m3d._lib import lib
    return int(lib().m3d_conv3d_zw_launch_units(B, cin, cout, D, H, W))


def test_min_units_zero_routes_the_small_cases(cp):
    for name, (B, cin, cout, D, H, W) in T.CASES.items():
        assert cp.train_conv_kernel("forward", B, cin, cout, D, H, W, "f16x2") == "fp32", name          # all below ZW_MIN_UNITS
        assert cp.train_conv_kernel("forward", B, cin, cout, D, H, W, "f16x2", min_units=0) == "f16x2", name
        want = "f16x2" if cin >= 32 else "fp32"                                                          # xb16_ragged: 16 output channels
        assert cp.train_conv_kernel("dgrad", B, cin, cout, D, H, W, "f16x2", min_units=0) == want, name


# ------------------------------------------------------------------ the setting
def test_set_conv_train():
    import m3d.compat as c
    assert c.get_conv_train() == "fp32"                                    # the default
    try:
        assert c.set_conv_train("f16x2") == "fp32"
        assert c.get_conv_train() == "f16x2"
        assert c.set_conv_train("f16x2", min_units=0) == "f16x2"
        for bad in ("f16", "FP32", None, 1):
            with pytest.raises(ValueError):
                c.set_conv_train(bad)
        with pytest.raises(ValueError):
            c.set_conv_train("f16x2", min_units=-1)
        assert c.get_conv_train() == "f16x2"                               # a refused call changes nothing
        assert c.set_conv_train("fp32") == "f16x2"
    finally:
        c.set_conv_train("fp32")
    assert c.get_conv_train() == "fp32" and c.get_conv_wgrad() == "fp32"


def test_exports():
    import m3d
    assert callable(m3d.conv3d_gy_reduce) and callable(m3d.ZwConv3d.dgrad_of)
    from m3d._lib import SYMBOLS
    assert "m3d_conv3d_zw_pack_dgrad" in SYMBOLS and "m3d_conv3d_gy_reduce" in SYMBOLS


# ------------------------------------------------------------------ refusals before any pointer is followed
BAD = C.c_void_p(64)          # a non-NULL, aligned address nobody may follow: a call that dereferenced it would crash this process


def test_pack_dgrad_refusals(L):
    E = _codes()["M3D_EINVAL"]
    assert L.m3d_conv3d_zw_pack_dgrad(None, 32, 64, BAD, None) == E
    assert L.m3d_conv3d_zw_pack_dgrad(BAD, 32, 64, None, None) == E
    for cin, cout in ((32, 24), (32, 8), (0, 64), (32, 0), (-16, 64), (32, -16)):
        assert L.m3d_conv3d_zw_pack_dgrad(BAD, cin, cout, BAD, None) == E, (cin, cout)


def test_gy_reduce_refusals_and_size_query(L):
    codes = _codes()
    E, EW = codes["M3D_EINVAL"], codes["M3D_EWORKSPACE"]
    n = C.c_size_t(12345)
    shape = (2, 3, 17, 33, 63)
    # the size query: no pointer is given at all, nothing can be launched; one fp64 partial per (channel, image, span of 16384)
    assert L.m3d_conv3d_gy_reduce(None, *shape, None, None, None, C.byref(n), None) == 0
    spans = -(-17 * 33 * 63 // 16384)
    assert spans == 3 and n.value == 8 * 3 * 2 * spans
    assert L.m3d_conv3d_gy_reduce(None, *shape, None, None, None, None, None) == E                     # nowhere to store the size
    for bad in ((0, 3, 17, 33, 63), (2, 0, 17, 33, 63), (2, 3, 0, 33, 63), (2, 3, 17, -1, 63), (2, 3, 17, 33, 0)):
        assert L.m3d_conv3d_gy_reduce(BAD, *bad, BAD, BAD, BAD, C.byref(n), None) == E, bad
    need = n.value
    ok = C.c_size_t(need)
    assert L.m3d_conv3d_gy_reduce(None, *shape, BAD, BAD, BAD, C.byref(ok), None) == E                 # d_gy NULL
    assert L.m3d_conv3d_gy_reduce(BAD, *shape, BAD, None, BAD, C.byref(ok), None) == E                 # d_gy_max NULL
    assert L.m3d_conv3d_gy_reduce(BAD, *shape, BAD, BAD, BAD, None, None) == E                         # ws_bytes NULL
    assert L.m3d_conv3d_gy_reduce(C.c_void_p(66), *shape, BAD, BAD, BAD, C.byref(ok), None) == E       # misaligned floats
    assert L.m3d_conv3d_gy_reduce(BAD, *shape, BAD, BAD, C.c_void_p(68), C.byref(ok), None) == E       # workspace not 8-byte aligned
    short = C.c_size_t(need - 1)
    assert L.m3d_conv3d_gy_reduce(BAD, *shape, BAD, BAD, BAD, C.byref(short), None) == EW
    assert L.m3d_conv3d_gy_reduce(BAD, *shape, None, BAD, BAD, C.byref(short), None) == EW             # (without a bias gradient too)


# ------------------------------------------------------------------ restatements
@pytest.mark.parametrize("cout,cin", [(64, 32), (48, 20), (16, 1), (96, 16)])
def test_pack_dgrad_index_restatement(cout, cin):
    w = torch.randn(cout, cin, 3, 3, 3, generator=torch.Generator().manual_seed(cout + cin))
    wd = T.dgrad_weight(w)
    assert tuple(wd.shape) == (cin, cout, 3, 3, 3)
    idx = T.pack_dgrad_index(cin, cout)
    assert np.array_equal(wd.numpy().reshape(-1), w.numpy().reshape(-1)[idx])
    assert float(wd.abs().max()) == float(w.abs().max())                   # the scale float behind the fragments: the same set's maximum


def test_dgrad_as_a_forward_conv_is_the_transposed_conv():
    a, w, _ = T.make("xb16_ragged", "dgrad", "benign")
    y1 = T.reference_op("dgrad", a, w)
    y2 = T.reference_op("forward", a, T.dgrad_weight(w))
    assert tuple(y1.shape) == (2, 16, 3, 5, 13)
    assert float((y1 - y2).abs().max()) <= 1e-12 * float(y1.abs().max())


@pytest.mark.parametrize("shape", [(2, 5, 3, 5, 13), (2, 3, 17, 33, 63), (1, 1, 1, 1, 1)])
def test_gy_reduce_bound_holds_for_an_fp64_then_fp32_sum(shape):
    """NumPy: sums in fp64 in another order than the kernel's (pairwise), rounded once to fp32, stay within the contract's bound of the
    fp64 sum taken as math.fsum takes it (exactly rounded)"""
    import math
    g = (torch.randn(shape, generator=torch.Generator().manual_seed(9)) * 3).numpy()
    S, bound = T.gb_bound(torch.from_numpy(g))
    for c in range(shape[1]):
        col = g[:, c].astype(np.float64).reshape(-1)
        exact = math.fsum(col.tolist())
        got = np.float32(np.add.reduce(col))
        got_seq = np.float32(np.cumsum(col)[-1])                                 # a plain ascending loop
        b = 2.0 ** -24 * abs(exact) + col.size * 2.0 ** -53 * np.abs(col).sum()
        assert abs(float(got) - exact) <= b and abs(float(got_seq) - exact) <= b
        assert abs(float(S[c]) - exact) <= col.size * 2.0 ** -53 * np.abs(col).sum()
        assert abs(float(bound[c]) - b) <= 1e-12 * b + 2.0 ** -24 * abs(float(S[c]) - exact)


def test_integer_inputs_are_exact_in_fp32():
    for case in T.CASES:
        for d in T.DIRECTIONS:
            a, w, bias = T.integer_inputs(case, d)
            y = T.reference_op(d, a, w, bias)
            assert float(y.abs().max()) < 2 ** 22 and bool((y == y.round()).all())
