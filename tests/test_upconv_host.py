"""CPU: the fp64 restatement of the mask-head up-conv (tests/upconv_reference.py) is torch's ConvTranspose3d(2, 2) and its autograd; the C
ABI of m3d_upconv3d_2x_* refuses what it must before any device pointer is followed or anything is launched, so every call below is
safe with made-up pointers (none of them passes the checks with R > 0); the compat switch and the CPU fall-through."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import upconv_reference as UR


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


@pytest.mark.parametrize("relu", (False, True))
@pytest.mark.parametrize("shape", UR.SHAPES[:4])
def test_restatement_is_torchs_conv_transpose3d(shape, relu):
    """pins the weight layout [Cin,Cout,a,b,c] and the parity order; fp64 both sides, 1e-12 relative"""
    x, w, b, gy = (torch.from_numpy(t).double() for t in UR.case(shape, "randn"))
    x.requires_grad_(True), w.requires_grad_(True), b.requires_grad_(True)
    y = F.conv_transpose3d(x, w, b, stride=2)
    y = torch.relu(y) if relu else y
    y.backward(gy)
    mask = y.detach().numpy() if relu else None
    y64, A = UR.forward(x.detach().numpy(), w.detach().numpy(), b.detach().numpy(), relu)
    gx64, _ = UR.dgrad(gy.numpy(), w.detach().numpy(), mask)
    gw64, _, gb64, Ab = UR.wgrad(gy.numpy(), x.detach().numpy(), mask)
    for got, want in ((y64, y), (gx64, x.grad), (gw64, w.grad), (gb64, b.grad)):
        want = want.detach().numpy()
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
    assert (A >= np.abs(y64) * (1 - 1e-12)).all() and (Ab >= np.abs(gb64) * (1 - 1e-12)).all()


def test_the_bound_holds_for_an_fp32_evaluation_and_has_teeth():
    shape = UR.SHAPES[3]
    x, w, b, gy = UR.case(shape, "randn")
    R, Cin, Cout, D, H, W = shape
    y64, A = UR.forward(x, w, b)
    y32 = F.conv_transpose3d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=2).numpy()
    r = UR.worst_ratio(y32, y64, A, Cin + 1)
    print("torch fp32 forward: err / bound", r)
    assert r <= 1.0
    xb = torch.from_numpy(x).bfloat16().float()                   # one operand rounded to bf16
    yb = F.conv_transpose3d(xb, torch.from_numpy(w), torch.from_numpy(b), stride=2).numpy()
    assert UR.worst_ratio(yb, y64, A, Cin + 1) > 1.0
    swapped = np.ascontiguousarray(w.transpose(0, 1, 4, 3, 2))    # parities (a,b,c) read as (c,b,a)
    ys = F.conv_transpose3d(torch.from_numpy(x), torch.from_numpy(swapped), torch.from_numpy(b), stride=2).numpy()
    assert UR.worst_ratio(ys, y64, A, Cin + 1) > 1.0


X, WT, Y, GX, WS, B = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600004   # bias / gb only 4-byte aligned: legal
EINVAL, EUNSUPPORTED = -1, -4
DIMS = dict(R=2, Cin=8, Cout=64, D=3, H=3, W=3)


def p(v):
    return C.c_void_p(v)


def fwd(L, x=X, w=WT, b=B, y=Y, relu=1, **kw):
    d = dict(DIMS, **kw)
    return L.m3d_upconv3d_2x_forward(p(x), p(w), p(b), p(y), d["R"], d["Cin"], d["Cout"], d["D"], d["H"], d["W"], relu, None)


def dgrad(L, gy=Y, ym=Y + 0x80000, w=WT, gx=GX, ws=None, wsb=0, **kw):
    d = dict(DIMS, **kw)
    return L.m3d_upconv3d_2x_dgrad(p(gy), p(ym), p(w), p(gx), d["R"], d["Cin"], d["Cout"], d["D"], d["H"], d["W"], p(ws), C.c_size_t(wsb), None)


def wgrad(L, gy=Y, ym=Y + 0x80000, x=X, gw=GX, gb=B, ws=None, wsb=0, **kw):
    d = dict(DIMS, **kw)
    return L.m3d_upconv3d_2x_wgrad(p(gy), p(ym), p(x), p(gw), p(gb), d["R"], d["Cin"], d["Cout"], d["D"], d["H"], d["W"], p(ws),
                                   C.c_size_t(wsb), None)


def test_abi_limits_without_a_gpu(L):
    from m3d._lib import SYMBOLS
    for s in ("m3d_upconv3d_2x_forward", "m3d_upconv3d_2x_dgrad", "m3d_upconv3d_2x_wgrad", "m3d_upconv3d_2x_dgrad_workspace_bytes",
              "m3d_upconv3d_2x_wgrad_workspace_bytes", "m3d_upconv3d_2x_slices"):
        assert s in SYMBOLS and hasattr(L, s), s
    # few output tiles and a reduction of more than four chunks (dgrad: 8 Cout = 512; wgrad at R = 40: 40 chunks): a workspace is needed
    need_d = L.m3d_upconv3d_2x_dgrad_workspace_bytes(*DIMS.values())
    need_w = L.m3d_upconv3d_2x_wgrad_workspace_bytes(*[dict(DIMS, R=40)[k] for k in DIMS])
    assert need_d > 0 and need_w > 0
    required = {fwd: ("x", "w", "y"), dgrad: ("gy", "w", "gx"), wgrad: ("gy", "x", "gw")}
    every = {fwd: ("x", "w", "b", "y"), dgrad: ("gy", "ym", "w", "gx"), wgrad: ("gy", "ym", "x", "gw", "gb")}
    big = {fwd: ("x", "w", "y"), dgrad: ("gy", "ym", "w", "gx"), wgrad: ("gy", "ym", "x", "gw")}
    defaults = dict(x=X, w=WT, y=Y, gy=Y, ym=Y + 0x80000, gx=GX, gw=GX, b=B, gb=B)
    for call in (fwd, dgrad, wgrad):
        # M3D_EINVAL
        for k in required[call]:
            assert call(L, **{k: None}) == EINVAL, (call.__name__, k)
        for k in every[call]:
            assert call(L, **{k: defaults[k] + 2}) == EINVAL and call(L, **{k: defaults[k] + 1}) == EINVAL, (call.__name__, k)
        for k in ("Cin", "Cout", "D", "H", "W"):
            assert call(L, **{k: 0}) == EINVAL and call(L, **{k: -3}) == EINVAL, (call.__name__, k)
        assert call(L, R=-1) == EINVAL
        # M3D_EUNSUPPORTED
        for k in big[call]:
            for off in (4, 8, 12):
                assert call(L, **{k: defaults[k] + off}) == EUNSUPPORTED, (call.__name__, k, off)
        assert call(L, R=1 << 16, Cin=1 << 15, Cout=1, D=1, H=1, W=1) == EUNSUPPORTED          # x / gx: 2^31 elements
        assert call(L, R=1 << 14, Cin=1, Cout=1 << 14, D=1, H=1, W=1) == EUNSUPPORTED          # y / gy: 8 * 2^28
        assert call(L, R=1, Cin=1 << 14, Cout=1 << 14, D=1, H=1, W=1) == EUNSUPPORTED          # weight / gw
        assert call(L, R=1, Cin=1, Cout=1, D=1 << 11, H=1 << 11, W=1 << 9) == EUNSUPPORTED      # one RoI of 2^31 voxels
    # the workspace
    assert dgrad(L, ws=None, wsb=need_d) == EINVAL and dgrad(L, ws=WS, wsb=need_d - 16) == EINVAL and dgrad(L, ws=WS, wsb=0) == EINVAL
    assert dgrad(L, ws=WS + 2, wsb=need_d) == EINVAL and dgrad(L, ws=WS + 4, wsb=need_d) == EUNSUPPORTED
    assert wgrad(L, R=40, ws=None, wsb=need_w) == EINVAL and wgrad(L, R=40, ws=WS, wsb=need_w - 16) == EINVAL
    assert wgrad(L, R=40, ws=WS + 2, wsb=need_w) == EINVAL and wgrad(L, R=40, ws=WS + 8, wsb=need_w) == EUNSUPPORTED
    # an empty batch: forward and dgrad have nothing to write and look at no pointer (wgrad zero-fills its outputs: tested on the GPU)
    assert fwd(L, R=0) == 0 and fwd(L, x=None, w=None, y=None, R=0) == 0
    assert dgrad(L, R=0) == 0 and dgrad(L, gy=None, w=None, gx=None, R=0) == 0
    assert wgrad(L, gw=None, R=0) == EINVAL


def test_workspace_sizes_and_slices(L):
    for Cin, Cout, D, H, W in ((1, 1, 1, 1, 1), (5, 3, 2, 3, 5), (16, 16, 7, 7, 7), (40, 72, 3, 4, 33), (256, 256, 7, 7, 7), (64, 8, 14, 14, 14)):
        V = D * H * W
        for f, kind, cap in ((L.m3d_upconv3d_2x_dgrad_workspace_bytes, 1, lambda R: 64 * R * Cin * V * 4),
                             (L.m3d_upconv3d_2x_wgrad_workspace_bytes, 2, lambda R: 64 * (Cin * Cout * 8 + Cout) * 4)):
            prev = 0
            for R in list(range(1, 130)) + [300, 511, 512, 513, 1000]:
                b = f(R, Cin, Cout, D, H, W)
                assert b % 16 == 0 and b >= prev, (Cin, Cout, V, R, b, prev)
                assert b <= cap(R) + 16                                                      # at most 64 slices
                s = L.m3d_upconv3d_2x_slices(kind, R, Cin, Cout, D, H, W)
                assert 1 <= s <= 64
                unit = (R * Cin * V if kind == 1 else Cin * Cout * 8 + Cout) * 4
                assert b >= (s * unit if s > 1 else 0)                                       # this call's partials fit
                prev = b
            assert f(0, Cin, Cout, D, H, W) == 0
        assert L.m3d_upconv3d_2x_slices(0, 7, Cin, Cout, D, H, W) == 1
    assert L.m3d_upconv3d_2x_slices(1, 0, 8, 8, 3, 3, 3) == 0 and L.m3d_upconv3d_2x_slices(3, 1, 8, 8, 3, 3, 3) == 0
    # a function of the shape only
    assert L.m3d_upconv3d_2x_wgrad_workspace_bytes(64, 256, 256, 7, 7, 7) == L.m3d_upconv3d_2x_wgrad_workspace_bytes(64, 256, 256, 7, 7, 7)


def test_set_upconv():
    import m3d.compat as compat
    assert compat.get_upconv() == "torch"
    assert compat.set_upconv("m3d") == "torch" and compat.get_upconv() == "m3d"
    assert compat.set_upconv("torch") == "m3d" and compat.get_upconv() == "torch"
    for bad in ("M3D", "", None, 1, "fp32"):
        with pytest.raises(ValueError):
            compat.set_upconv(bad)
        assert compat.get_upconv() == "torch"


def test_compat_conv_transpose3d_on_cpu_tensors_is_torchs():
    import m3d
    import m3d.compat as compat
    orig = F.conv_transpose3d
    g = torch.Generator().manual_seed(1)
    x, w, b = torch.randn((2, 4, 3, 3, 3), generator=g), torch.randn((4, 6, 2, 2, 2), generator=g), torch.randn((6,), generator=g)
    assert torch.equal(compat.conv_transpose3d(x, w, b, stride=2), orig(x, w, b, stride=2))         # would qualify on the GPU
    w3 = torch.randn((4, 6, 3, 3, 3), generator=g)
    assert torch.equal(compat.conv_transpose3d(x, w3, None, 2, 1, 1), orig(x, w3, None, 2, 1, 1))
    assert F.conv_transpose3d is not compat.conv_transpose3d                                         # opt-in: nothing is patched by the import
    compat.install_conv_transpose3d()
    try:
        assert F.conv_transpose3d is compat.conv_transpose3d
        assert torch.equal(F.conv_transpose3d(x, w, b, stride=2), orig(x, w, b, stride=2))
    finally:
        compat.uninstall_conv_transpose3d()
    assert F.conv_transpose3d is orig
    with pytest.raises(m3d.M3DError):                                                                # there is no CPU path
        m3d.upconv3d_2x(x, w, b)
