"""CPU: the table of tests/conv_dilated_cases.py has teeth; its bound holds for an fp32 evaluation and catches a displaced tap; the C ABI
of m3d_conv3d_wgrad_dilated* refuses what it must before any pointer is followed or anything is launched, so every call below is safe
with made-up pointers on a machine without a GPU; the compat switch, the CPU fall-through, MaskTrainCfg(dilation) and MaskHead."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_dilated_cases as T


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from m3d._lib import lib
    return lib()


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_the_table_has_teeth(case):
    """a kernel that ignores the dilation cannot pass: the dilation-2 gradient differs from the dilation-1 gradient of the same operands"""
    for kind in ("int", "randn"):
        r = T.reference(case, kind)
        gw1 = T.wgrad64(r["x"], r["gy"], dilation=1)
        assert r["gw"].shape == gw1.shape == (case[2], case[1], 3, 3, 3)
        assert (r["gw"] != gw1).any()
        assert (T.dgrad64(r["gy"], r["w"], 1) != r["gx"]).any()
        assert (r["A"] >= r["gw"].abs() * (1 - 1e-12)).all()
    r = T.reference(case, "int")
    assert torch.equal(r["gw"], r["gw"].round()) and float(r["A"].max()) < 2 ** 24          # exact in any fp32 order


def test_depth_one_leaves_only_the_middle_plane_of_taps():
    for kind in ("int", "randn"):
        gw = T.reference(T.D1_CASE, kind)["gw"]
        assert (gw[:, :, 0] == 0).all() and (gw[:, :, 2] == 0).all() and (gw[:, :, 1] != 0).any()
        # H = W = 3: a +-2 tap joins only voxels 0 and 2
        x, gy = T.reference(T.D1_CASE, kind)["x"].double(), T.reference(T.D1_CASE, kind)["gy"].double()
        want = torch.einsum("bo,bi->oi", gy[:, :, 0, 0, 0], x[:, :, 0, 2, 2])
        assert torch.allclose(gw[:, :, 1, 2, 2], want, rtol=1e-12, atol=1e-12)


def _terms32(x, gy):
    """every product behind every gw element, fp32: [cout, cin, 27, B D H W] (zero where the tap leaves the volume)"""
    B, cin, D, H, W = x.shape
    xp = np.zeros((B, cin, D + 4, H + 4, W + 4), np.float32)
    xp[:, :, 2:-2, 2:-2, 2:-2] = x
    out = np.empty((gy.shape[1], cin, 27, B * D * H * W), np.float32)
    g = gy.transpose(1, 0, 2, 3, 4).reshape(gy.shape[1], 1, -1)
    for t in range(27):
        dz, dy, dx = t // 9, (t // 3) % 3, t % 3
        xs = xp[:, :, 2 * dz:2 * dz + D, 2 * dy:2 * dy + H, 2 * dx:2 * dx + W].transpose(1, 0, 2, 3, 4).reshape(1, cin, -1)
        out[:, :, t] = g * xs
    return out


def test_the_bound_holds_for_an_fp32_evaluation_and_has_teeth():
    case = T.CASES[2]
    r = T.reference(case, "randn")
    n = T.terms(case) + 1
    tm = _terms32(r["x"].numpy(), r["gy"].numpy())
    tm = tm[..., np.random.default_rng(5).permutation(tm.shape[-1])]                     # a shuffled order
    acc = np.zeros(tm.shape[:3], np.float32)
    for i in range(tm.shape[-1]):                                                        # one fp32 rounding per term
        acc += tm[..., i]
    got = torch.from_numpy(acc.reshape(r["gw"].shape))
    ratio = T.worst_ratio(got, r["gw"], r["A"], n)
    print("fp32 NumPy, shuffled order: err / bound", ratio)
    assert 0 < ratio <= 1.0
    # pairwise fp32 summation is another order of the same n operations
    pair = torch.from_numpy(tm.sum(-1, dtype=np.float32).reshape(r["gw"].shape))
    assert T.worst_ratio(pair, r["gw"], r["A"], n) <= 1.0
    # one tap displaced: (dz, dy, dx) = (1, 1, 0) holds what belongs to (1, 1, 2)
    moved = got.clone()
    moved[:, :, 1, 1, 0] = got[:, :, 1, 1, 2]
    assert T.worst_ratio(moved, r["gw"], r["A"], n) > 1.0
    # the dilation-1 gradient is far outside
    assert T.worst_ratio(T.wgrad64(r["x"], r["gy"], 1).float(), r["gw"], r["A"], n) > 1.0
    # one operand rounded to bf16
    xb = r["x"].bfloat16().float()
    assert T.worst_ratio(T.wgrad64(xb, r["gy"]).float(), r["gw"], r["A"], n) > 1.0


X, GY, GW, WS = 0x100000, 0x200000, 0x300000, 0x400000
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4
DIMS = dict(batch=3, cin=32, cout=32, D=7, H=7, W=7, k=3, dilation=2)


def p(v):
    return C.c_void_p(v)


def need(L, **kw):
    d = dict(DIMS, **kw)
    return L.m3d_conv3d_wgrad_dilated_workspace_bytes(*[d[k] for k in DIMS])


def wgrad(L, x=X, gy=GY, gw=GW, ws=WS, wsb=None, tile_x=None, **kw):
    d = dict(DIMS, **kw)
    wsb = need(L, **kw) if wsb is None else wsb
    shape = [d[k] for k in DIMS]
    if tile_x is None:
        return L.m3d_conv3d_wgrad_dilated(p(x), p(gy), p(gw), *shape, p(ws), C.c_size_t(wsb), None)
    return L.m3d_conv3d_wgrad_dilated_tile(p(x), p(gy), p(gw), *shape, tile_x, p(ws), C.c_size_t(wsb), None)


def test_abi_limits_without_a_gpu(L):
    from m3d._lib import SYMBOLS
    for s in ("m3d_conv3d_wgrad_dilated_workspace_bytes", "m3d_conv3d_wgrad_dilated", "m3d_conv3d_wgrad_dilated_tile",
              "m3d_conv3d_wgrad_dilated_plan"):
        assert s in SYMBOLS and hasattr(L, s), s
    assert need(L) > 0
    for tile in (None, 0, 8, 16):
        # M3D_EINVAL: NULL pointers, non-positive extents, at either dilation
        for dil in (1, 2):
            for k in ("x", "gy", "gw", "ws"):
                assert wgrad(L, tile_x=tile, dilation=dil, **{k: None}) == EINVAL, (tile, dil, k)
            for k in ("batch", "cin", "cout", "D", "H", "W"):
                assert wgrad(L, tile_x=tile, dilation=dil, wsb=1 << 20, **{k: 0}) == EINVAL, (tile, dil, k)
                assert wgrad(L, tile_x=tile, dilation=dil, wsb=1 << 20, **{k: -3}) == EINVAL, (tile, dil, k)
        # M3D_EWORKSPACE: a short workspace
        assert wgrad(L, tile_x=tile, wsb=need(L) - 1) == EWORKSPACE and wgrad(L, tile_x=tile, wsb=0) == EWORKSPACE
        # M3D_EUNSUPPORTED: k != 3 at dilation 2, dilations 0 and 3, one image of x or gy beyond the 32-bit offsets
        for kw in (dict(k=1), dict(k=5), dict(k=5, cin=1), dict(k=2), dict(dilation=0), dict(dilation=3), dict(dilation=-1),
                   dict(batch=1, cin=1, cout=1, D=1 << 10, H=1 << 10, W=1 << 9), dict(batch=1, cin=1 << 9, cout=1, D=1 << 7, H=1 << 7, W=1 << 6),
                   dict(batch=1, cin=1, cout=1 << 9, D=1 << 7, H=1 << 7, W=1 << 6)):
            assert wgrad(L, tile_x=tile, wsb=1 << 20, **kw) == EUNSUPPORTED, (tile, kw)
            assert need(L, **kw) == 0, kw
    assert wgrad(L, wsb=need(L, dilation=1) - 1, dilation=1) == EWORKSPACE
    for tile in (1, 4, 12, 32, -8):                                      # a tile the kernel does not have
        assert wgrad(L, tile_x=tile) == EUNSUPPORTED
    for k in ("batch", "cin", "cout", "D", "H", "W"):
        assert need(L, **{k: 0}) == 0 and need(L, dilation=1, **{k: 0}) == 0


def test_workspace_and_plan(L):
    for case in T.CASES + [(64, 256, 256, 7, 7, 7), (300, 256, 256, 7, 7, 7), (16, 256, 256, 14, 14, 14)]:
        B, cin, cout, D, H, W = case
        # dilation 1 is m3d_conv3d_wgrad's own need, for every k it takes
        for k in (1, 3):
            assert L.m3d_conv3d_wgrad_dilated_workspace_bytes(B, cin, cout, D, H, W, k, 1) == L.m3d_conv3d_wgrad_workspace_bytes(B, cin, cout, D, H, W, k)
        assert L.m3d_conv3d_wgrad_dilated_workspace_bytes(B, 1, cout, D, H, W, 5, 1) == L.m3d_conv3d_wgrad_workspace_bytes(B, 1, cout, D, H, W, 5)
        wsb = L.m3d_conv3d_wgrad_dilated_workspace_bytes(B, cin, cout, D, H, W, 3, 2)
        for tile in (0, 8, 16):
            tx, ty, slots = C.c_int(), C.c_int(), C.c_int()
            assert L.m3d_conv3d_wgrad_dilated_plan(B, cin, cout, D, H, W, 3, 2, tile, C.byref(tx), C.byref(ty), C.byref(slots)) == 0
            assert tx.value == (tile or (8 if W <= 8 else 16)) and tx.value * ty.value * 2 == 128
            tiles = B * -(-D // 2) * -(-H // ty.value) * -(-W // tx.value)
            assert 1 <= slots.value <= tiles                                                # no slot without a tile
            assert wsb >= slots.value * cout * cin * 27 * 4                                  # one workspace serves both tiles
            assert L.m3d_conv3d_wgrad_dilated_plan(B, cin, cout, D, H, W, 3, 2, tile, None, None, None) == 0
    assert L.m3d_conv3d_wgrad_dilated_plan(1, 4, 5, 2, 4, 16, 3, 2, 16, None, None, C.byref(slots)) == 0 and slots.value == 1
    assert L.m3d_conv3d_wgrad_dilated_plan(1, 4, 5, 2, 8, 8, 3, 2, 8, None, None, C.byref(slots)) == 0 and slots.value == 1
    assert L.m3d_conv3d_wgrad_dilated_plan(1, 4, 5, 2, 8, 8, 3, 1, 0, None, None, None) == EUNSUPPORTED
    assert L.m3d_conv3d_wgrad_dilated_plan(1, 4, 5, 2, 8, 8, 3, 2, 4, None, None, None) == EUNSUPPORTED
    assert L.m3d_conv3d_wgrad_dilated_plan(0, 4, 5, 2, 8, 8, 3, 2, 0, None, None, None) == EINVAL


def test_set_conv_dilated():
    import m3d.compat as compat
    assert compat.get_conv_dilated() == "torch"
    assert compat.set_conv_dilated("m3d") == "torch" and compat.get_conv_dilated() == "m3d"
    assert compat.set_conv_dilated("torch") == "m3d" and compat.get_conv_dilated() == "torch"
    for bad in ("M3D", "", None, 2, "fp32", "f16x2"):
        with pytest.raises(ValueError):
            compat.set_conv_dilated(bad)
        assert compat.get_conv_dilated() == "torch"


def test_compat_conv3d_on_cpu_tensors_is_torchs_under_both_modes():
    import m3d.compat as compat
    orig = F.conv3d
    g = torch.Generator().manual_seed(2)
    x, w, b = torch.randn((2, 4, 5, 6, 7), generator=g), torch.randn((6, 4, 3, 3, 3), generator=g), torch.randn((6,), generator=g)
    want = orig(x, w, b, 1, 2, 2)
    for mode in ("torch", "m3d"):
        prev = compat.set_conv_dilated(mode)
        try:
            assert torch.equal(compat.conv3d(x, w, b, 1, 2, 2), want)                        # would qualify on the GPU under "m3d"
            assert torch.equal(compat.conv3d(x, w, b, 1, (2, 2, 2), (2, 2, 2)), want)
            assert torch.equal(compat.conv3d(x, w, None, 1, 3, 3), orig(x, w, None, 1, 3, 3))
            assert F.conv3d is orig                                                         # the setter patches nothing
            compat.install_conv3d()
            try:
                assert F.conv3d is compat.conv3d and torch.equal(F.conv3d(x, w, b, 1, 2, 2), want)
            finally:
                compat.uninstall_conv3d()
        finally:
            compat.set_conv_dilated(prev)
    assert F.conv3d is orig and compat.get_conv_dilated() == "torch"


def test_mask_train_cfg_dilation_and_mask_head_state():
    from m3d.train import MaskHead, MaskTrainCfg
    assert MaskTrainCfg().dilation == 1 and MaskTrainCfg.nuclei().dilation == 1 and MaskTrainCfg.soma().dilation == 1
    assert MaskTrainCfg(dilation=2).dilation == 2 and MaskTrainCfg.soma(dilation=2).dilation == 2
    for bad in (3, 0, -1, 4):
        with pytest.raises(ValueError):
            MaskTrainCfg(dilation=bad)
    heads = [MaskHead(16, MaskTrainCfg(dim_reduced=32, num_convs=2, dilation=d), 4) for d in (1, 2)]
    s1, s2 = (h.state_dict() for h in heads)
    assert list(s1) == list(s2) and all(s1[k].shape == s2[k].shape for k in s1)
    assert list(heads[0].detector_state()) == list(heads[1].detector_state())
    convs = [m for m in heads[1].conv_fcn if isinstance(m, torch.nn.Conv3d)]
    assert len(convs) == 2 and all(m.dilation == (2, 2, 2) and m.padding == (2, 2, 2) and m.kernel_size == (3, 3, 3) for m in convs)
    assert all(m.dilation == (1, 1, 1) and m.padding == (1, 1, 1) for m in heads[0].conv_fcn if isinstance(m, torch.nn.Conv3d))
    heads[0].load_detector_state(heads[1].detector_state())                                # one checkpoint format at either dilation
    # on the CPU the dilated stack is torch's conv3d: the module's own layers applied in order
    x = torch.randn((2, 16, 5, 5, 5), generator=torch.Generator().manual_seed(4))
    import m3d.compat as compat
    y = x
    for m in heads[1].conv_fcn:
        y = compat.conv3d(y, m.weight, m.bias, 1, m.padding, m.dilation) if isinstance(m, torch.nn.Conv3d) else torch.relu(y)
    assert torch.equal(y, heads[1].conv_fcn(x)) and y.shape == (2, 32, 5, 5, 5)
